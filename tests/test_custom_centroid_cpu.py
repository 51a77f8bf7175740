"""CPU: system.CustomCentroidBondForce -- the class, the compiler's centroid kind (openmmtools_amd/custom_expr.py: the compound
programs under the names g1 ...), the descriptor with its groups, the refusals, and the independent f64 helper
tests/centroid_expr_oracle.py against central differences of its own energy and against the closed form of HarmonicRestraintForce."""
import copy

import numpy as np
import pytest

import centroid_expr_oracle as oracle
import compound_expr_oracle as compound
from custom_expr_oracle import Expression
from openmmtools_amd import alchemy, custom_expr as cx, forces, states, testsystems
from openmmtools_amd.system import System, system_to_desc, CustomCompoundBondForce, CustomCentroidBondForce

MASSES = [12.0, 1.0, 16.0, 14.0, 1.0, 12.0, 32.0, 1.0, 12.0, 16.0]


def _system(masses=MASSES):
    s = System()
    for m in masses:
        s.addParticle(m)
    return s


def _harmonic(lam=1.0, K=300.0):
    f = CustomCentroidBondForce(2, 'lambda*(K/2)*distance(g1,g2)^2')
    f.addGlobalParameter('lambda', lam)
    f.addPerBondParameter('K')
    f.addGroup([0, 1, 2])
    f.addGroup([5, 6], [1.0, 3.0])
    f.addBond([0, 1], [K])
    return f


def test_the_class_mirrors_openmm():
    f = CustomCentroidBondForce(3, 'angle(g1,g2,g3)')
    assert (f.getNumGroupsPerBond(), f.getNumGroups(), f.getNumBonds()) == (3, 0, 0)
    assert f.addGroup([0, 1, 2]) == 0 and f.addGroup((3, 4), (1.0, 2.0)) == 1 and f.addGroup([5], []) == 2 and f.getNumGroups() == 3
    assert f.getGroupParameters(0) == ([0, 1, 2], []) and f.getGroupParameters(1) == ([3, 4], [1.0, 2.0]) and f.getGroupParameters(2) == ([5], [])
    f.setGroupParameters(0, [2, 1], [0.5, 0.5]); f.setGroupParameters(1, [7])
    assert f.getGroupParameters(0) == ([2, 1], [0.5, 0.5]) and f.getGroupParameters(1) == ([7], [])
    assert f.addPerBondParameter('k') == 0 and f.getNumPerBondParameters() == 1 and f.getPerBondParameterName(0) == 'k'
    assert f.addBond([0, 1, 2], [4.0]) == 0 and f.addBond((2, 1, 0), (5.0,)) == 1 and f.getNumBonds() == 2
    assert f.getBondParameters(1) == ([2, 1, 0], [5.0])
    f.setBondParameters(0, [1, 0, 2], [6.0])
    assert f.getBondParameters(0) == ([1, 0, 2], [6.0])
    assert f.addGlobalParameter('lam', 0.5) == 0 and (f.getGlobalParameterName(0), f.getGlobalParameterDefaultValue(0)) == ('lam', 0.5)
    f.setUsesPeriodicBoundaryConditions(True); f.setForceGroup(3); f.setEnergyFunction('k*angle(g1,g2,g3)')
    assert f.usesPeriodicBoundaryConditions() and f.getForceGroup() == 3 and f.getEnergyFunction() == 'k*angle(g1,g2,g3)'
    assert f.addTabulatedFunction('tab', object()) == 0 and (f.getNumTabulatedFunctions(), f.getTabulatedFunctionName(0)) == (1, 'tab')
    with pytest.raises(ValueError, match='a bond of 2 groups, the force declares 3'):
        f.addBond([0, 1])
    with pytest.raises(ValueError, match='a bond of 4 groups, the force declares 3'):
        f.setBondParameters(0, [0, 1, 2, 0], [1.0])
    with pytest.raises(ValueError, match='a group of 3 particles with 2 weights'):
        f.addGroup([0, 1, 2], [1.0, 2.0])
    atoms, params = f._term_arrays()
    assert atoms.dtype == np.int32 and np.array_equal(atoms, [[1, 0, 2], [2, 1, 0]]) and np.array_equal(params, [[6.0], [5.0]])
    # routing is by class identity: this class goes down the expression path, the restraints' base class is another one
    assert cx.is_custom_term_force(f) and cx.KIND_OF_CLASS['CustomCentroidBondForce'] == cx.KIND_CENTROID == 5
    assert not issubclass(CustomCentroidBondForce, forces.CustomCentroidBondForce) and not issubclass(forces.CustomCentroidBondForce, CustomCentroidBondForce)
    assert not cx.is_custom_term_force(forces.CustomCentroidBondForce(2, 'distance(g1,g2)^4'))
    assert not cx.is_custom_term_force(forces.HarmonicRestraintForce(100.0, [0, 1], [2, 3]))


@pytest.mark.parametrize('function, n', [('distance', 2), ('angle', 3), ('dihedral', 4)])
def test_programs_are_the_compound_forces(function, n):
    """the names g1 ... compile to what p1 ... compile to: programs, constants and stack depth"""
    def text(prefix):
        return 'k*(%s(%s)-a0)^2 + x%d*pointdistance(x1,y1,z1,x%d,y%d,z%d)' % (function, ','.join('%s%d' % (prefix, i + 1) for i in range(n)), n, n, n, n)
    got = cx.compile_expression(text('g'), cx.compound_variables(n), ['k', 'a0'], {}, n_particles=n, particle_prefix='g')
    want = cx.compile_expression(text('p'), cx.compound_variables(n), ['k', 'a0'], {}, n_particles=n)
    assert np.array_equal(got['program'], want['program']) and np.array_equal(got['consts'], want['consts'])
    assert got['stack_depth'] == want['stack_depth']
    packed = sum(i << (4 * i) for i in range(n))
    assert ({'distance': cx.DISTANCE, 'angle': cx.ANGLE, 'dihedral': cx.DIHEDRAL}[function], packed) in [tuple(p) for p in got['program']]


def test_descriptor_carries_the_groups():
    s = _system()
    f = _harmonic(lam=0.5)
    f.addGroup([9, 3, 4, 3])                                          # (named by no bond; an atom twice is two entries)
    f.setForceGroup(2); f.setUsesPeriodicBoundaryConditions(True)
    s.addForce(f)
    d = system_to_desc(s)
    t = d['custom_terms']['000']
    assert (t['kind'], t['n_particles'], t['periodic'], t['force_group'], t['global_names']) == (cx.KIND_CENTROID, 2, 1, 2, ['lambda'])
    assert np.array_equal(t['atoms'], [[0, 1]]) and t['atoms'].dtype == np.int32 and np.array_equal(t['params'], [[300.0]])
    assert np.array_equal(t['group_offsets'], [0, 3, 5, 9]) and t['group_offsets'].dtype == np.int32
    assert np.array_equal(t['group_atoms'], [0, 1, 2, 5, 6, 9, 3, 4, 3]) and t['group_atoms'].dtype == np.int32
    w = t['group_weights']
    assert w.dtype == np.float64
    assert np.array_equal(w[:3], np.array([12.0, 1.0, 16.0]) / 29.0)                   # masses where the group gives no weights
    assert np.array_equal(w[3:5], [0.25, 0.75])                                        # the group's own, normalised
    assert np.array_equal(w[5:], np.array([16.0, 14.0, 1.0, 14.0]) / 45.0)
    for g in range(3):
        assert abs(w[t['group_offsets'][g]:t['group_offsets'][g + 1]].sum() - 1.0) <= 1e-15
    assert d['custom_globals']['names'] == ['lambda'] and np.array_equal(d['custom_globals']['defaults'], [0.5])
    # the program is the compound force's
    c = CustomCompoundBondForce(2, 'lambda*(K/2)*distance(p1,p2)^2'); c.addGlobalParameter('lambda', 0.5); c.addPerBondParameter('K')
    c.addBond([0, 1], [300.0])
    s2 = _system(); s2.addForce(c)
    u = system_to_desc(s2)['custom_terms']['000']
    assert np.array_equal(t['program'], u['program']) and np.array_equal(t['consts'], u['consts']) and 'group_offsets' not in u
    # the fingerprint sees the groups, the weights and the masses behind default weights
    prints = {s.fingerprint()}
    for change in (lambda f: f.setGroupParameters(0, [0, 1, 3]), lambda f: f.setGroupParameters(1, [5, 6], [1.0, 2.0]),
                   lambda f: f.setBondParameters(0, [0, 2], [300.0]), lambda f: f.setBondParameters(0, [0, 1], [301.0])):
        s3 = copy.deepcopy(s); change(s3.getForce(0))
        prints.add(s3.fingerprint())
    assert len(prints) == 5


def _one(P, energy, groups=None, bond=None):
    f = CustomCentroidBondForce(P, energy)
    for g in (groups if groups is not None else [[i] for i in range(P)]):
        f.addGroup(*g) if isinstance(g, tuple) else f.addGroup(g)
    f.addBond(list(range(P)) if bond is None else bond)
    return f


def _desc(*fs):
    s = _system()
    for f in fs:
        s.addForce(f)
    return system_to_desc(s)


def test_refusals_name_the_force_and_the_item():
    with pytest.raises(ValueError, match='CustomCentroidBondForce: group 1 is empty'):
        _desc(_one(2, 'distance(g1,g2)', groups=[[0], []]))
    with pytest.raises(ValueError, match='CustomCentroidBondForce: the weights of group 0 sum to zero'):
        _desc(_one(2, 'distance(g1,g2)', groups=[([0, 1], [0.0, 0.0]), [2]]))
    f = _one(2, 'distance(g1,g2)')
    f._groups[1] = ([3, 4], [1.0])                                     # (past the class's own check, as a foreign object could be)
    with pytest.raises(ValueError, match='CustomCentroidBondForce: group 1 has 2 particles and 1 weights'):
        _desc(f)
    with pytest.raises(ValueError, match=r'CustomCentroidBondForce: group 0 names particle 10 \(the System has 10\)'):
        _desc(_one(2, 'distance(g1,g2)', groups=[[0, 10], [1]]))
    with pytest.raises(ValueError, match='CustomCentroidBondForce: group 1 names particle -1'):
        _desc(_one(2, 'distance(g1,g2)', groups=[[0], [-1]]))
    with pytest.raises(ValueError, match=r'CustomCentroidBondForce: a bond names group 2 \(the force has 2\)'):
        _desc(_one(2, 'distance(g1,g2)', bond=[0, 2]))
    with pytest.raises(ValueError, match='a bond of 3 groups, the force declares 2'):
        _one(2, 'distance(g1,g2)', bond=[0, 1, 1])
    with pytest.raises(NotImplementedError, match=r'CustomCentroidBondForce: bonds of 9 groups \(the engine takes 1 ... 8\)'):
        _desc(_one(9, 'distance(g1,g9)'))
    with pytest.raises(NotImplementedError, match="CustomCentroidBondForce.*particle name 'p1' \\(the groups of this force are g1 ... g2\\)"):
        _desc(_one(2, 'distance(p1,g2)'))
    c = CustomCompoundBondForce(2, 'distance(g1,p2)'); c.addBond([0, 1])
    with pytest.raises(NotImplementedError, match="CustomCompoundBondForce.*group name 'g1' \\(the particles of this force are p1 ... p2\\)"):
        _desc(c)
    with pytest.raises(NotImplementedError, match="CustomCentroidBondForce.*group name 'g2' outside"):
        _desc(_one(2, 'distance(g1,g2) + g2'))
    with pytest.raises(NotImplementedError, match="CustomCentroidBondForce.*group 'g3' in a bond of 2 groups"):
        _desc(_one(2, 'distance(g1,g3)'))
    with pytest.raises(NotImplementedError, match="CustomCentroidBondForce.*'angle' takes 3 groups, not 2"):
        _desc(_one(3, 'angle(g1,g2)'))
    with pytest.raises(NotImplementedError, match="CustomCentroidBondForce.*arguments of 'dihedral' are group names g1 ... g4"):
        _desc(_one(4, 'dihedral(g1,g2,g3,x4)'))
    for name in ('pointangle', 'pointdihedral'):
        with pytest.raises(NotImplementedError, match="CustomCentroidBondForce.*function '%s'" % name):
            _desc(_one(4, '%s(%s)' % (name, ','.join(['x1'] * (9 if name == 'pointangle' else 12)))))
    f = _one(2, 'tab(distance(g1,g2))'); f.addTabulatedFunction('tab', object())
    with pytest.raises(NotImplementedError, match="CustomCentroidBondForce.*tabulated function 'tab'"):
        _desc(f)
    f, g = _one(2, 'distance(g1,g2)'), _one(2, 'distance(g1,g2)'); g.setForceGroup(3)
    with pytest.raises(NotImplementedError, match=r'several force groups \(0, 3\).*CustomCentroidBondForce in 3'):
        _desc(f, g)
    with pytest.raises(NotImplementedError, match='%d custom forces' % (cx.MAX_FORCES + 1)):                # it counts among the 8
        _desc(*[_one(2, 'distance(g1,g2)') for _ in range(cx.MAX_FORCES + 1)])
    many = [_one(2, 'a%d*distance(g1,g2)' % k) for k in range(2)]
    for k, f in enumerate(many):
        for i in range(9):
            f.addGlobalParameter('a%d' % k if i == 0 else 'b%d_%d' % (k, i), 1.0)
    with pytest.raises(NotImplementedError, match='18 global parameters'):                                  # the same 16 columns
        _desc(*many)
    assert len(_desc(_one(8, 'dihedral(g5,g6,g7,g8) + x8'))['custom_terms']) == 1                           # (the most groups the engine takes)


def test_stores_and_pools_refuse_by_name():
    from openmmtools_amd import system_xml
    from openmmtools_amd.multistate._reference_store import ReferenceStoreWriter
    from openmmtools_amd.multistate._engine_pool import EnginePool
    s = _system(); s.addForce(_harmonic())
    with pytest.raises(NotImplementedError, match='CustomCentroidBondForce with the energy'):
        system_xml.to_xml(s)
    assert 'CustomCentroidBondForce' in ReferenceStoreWriter.can_store([states.ThermodynamicState(s, 300.0)], [], [])

    class Stub:
        def spawn(self): return Stub()
    d = system_to_desc(s)
    with pytest.raises(NotImplementedError, match='centroid-bond forces.*more than one compatibility group'):
        EnginePool(Stub(), [[0], [1]]).set_system([d, d])


def test_global_table_and_alchemical_factory_take_the_force():
    class LambdaState(states.GlobalParameterState):
        lambda_com = states.GlobalParameterState.GlobalParameter('lambda_com', standard_value=1.0)
    f = CustomCentroidBondForce(2, 'lambda_com*50*distance(g1,g2)^4'); f.addGlobalParameter('lambda_com', 0.5)
    f.addGroup([0, 1, 2]); f.addGroup([5, 6]); f.addBond([0, 1])
    s = _system(); s.addForce(f)
    assert LambdaState.from_system(s).lambda_com == 0.5
    ts = states.ThermodynamicState(s, 300.0)
    compound_states = [states.CompoundThermodynamicState(copy.deepcopy(ts), [LambdaState(lambda_com=l)]) for l in (1.0, 0.25)]
    assert np.array_equal(cx.custom_globals(s, ['lambda_com'], compound_states + [ts]), [[1.0], [0.25], [0.5]])
    al = testsystems.AlanineDipeptideVacuum()
    al.system.addForce(f)
    system = alchemy.AbsoluteAlchemicalFactory().create_alchemical_system(al.system, alchemy.AlchemicalRegion(alchemical_atoms=list(range(0, 6))))
    kept = [g for g in system.getForces() if isinstance(g, CustomCentroidBondForce)]
    assert len(kept) == 1 and kept[0].getEnergyFunction() == f.getEnergyFunction() and kept[0].getGroupParameters(1) == f.getGroupParameters(1)
    assert [t['kind'] for t in system_to_desc(system)['custom_terms'].values()] == [cx.KIND_CENTROID]


def test_the_cpu_port_refuses_the_force():
    import os
    from openmmtools_amd import _engine
    here = os.path.dirname(os.path.abspath(__file__))
    cpu_lib = os.path.join(os.path.dirname(here), 'oracle', '_build', 'libremd_cpu.so')
    if not os.path.exists(cpu_lib):
        import __graft_entry__
        __graft_entry__.build()
    eng = _engine.HipEngine(lib_path=cpu_lib)
    hg = testsystems.HostGuestVacuum()
    f = _harmonic()
    hg.system.addForce(f)
    with pytest.raises(NotImplementedError, match='remd_set_custom_terms.*centroid-bond forces.*remd_hip_custom.h'):
        eng.set_system(system_to_desc(hg.system))


# ---- the helper itself ---------------------------------------------------------------------------------------------------------------
RNG = np.random.default_rng(7)
X = RNG.uniform(0.0, 1.2, (10, 3))
BOX = np.array([1.3, 1.4, 1.5])


@pytest.mark.parametrize('periodic', [False, True])
def test_helper_against_central_differences_of_its_own_energy(periodic):
    """the spread forces are minus the gradient of the helper's total energy with respect to the ATOMS (not the centroids): the chain
    rule through the centroids, an atom in two groups and a group in two bonds included"""
    energy = 'k*(distance(g1,g2)-0.2)^2 + 3*cos(angle(g1,g2,g3)) + 2*sin(dihedral(g1,g2,g3,g4)) + z1*x4'
    groups = [([0, 1, 2], [1.0, 2.0, 3.0]), ([3, 4], [2.0, 1.0]), ([5, 2, 6], [1.0, 1.0, 5.0]), ([7, 8, 9], [3.0, 1.0, 1.0]), ([1], [4.0])]
    bonds, params = [[0, 1, 2, 3], [3, 4, 0, 2]], [[40.0], [25.0]]
    x = X.copy()
    if periodic:
        x[1] += [BOX[0], 0.0, -BOX[2]]                               # (an atom of group 0 wrapped away from the group's first atom)

    expression = Expression(oracle.as_particles(energy))

    def total(y):
        c = oracle.centroids([(a, oracle.normalised(w)) for a, w in groups], y, BOX, periodic)
        return sum(compound.bond_energy(expression, c[idx], ['k'], p, {}, BOX, periodic) for idx, p in zip(bonds, params))
    E, F = oracle.evaluate(4, energy, bonds, ['k'], params, {}, groups, x, BOX, periodic)
    assert E.sum() == pytest.approx(total(x), rel=1e-14)
    G = compound.gradient(total, x, 1e-4)
    print('helper: max |F + dE/dx| / max|F| = %.3g' % (np.abs(F + G).max() / np.abs(F).max()))
    assert np.abs(F + G).max() <= 1e-7 * np.abs(F).max()
    if periodic:                                                     # the wrapped atom is seen where it was
        E0, F0 = oracle.evaluate(4, energy, bonds, ['k'], params, {}, groups, X, BOX, periodic)
        assert np.allclose(E, E0, rtol=1e-10, atol=0.0) and np.abs(F - F0).max() <= 1e-9 * np.abs(F0).max()


def test_helper_against_the_closed_form_of_the_harmonic_restraint():
    """E = lambda (K/2) |c2 - c1|^2, F_i = -/+ lambda K w_i (c2 - c1): the mass-weighted HarmonicRestraintForce written out"""
    masses = np.array(MASSES)
    K, lam = 700.0, 0.6
    g1, g2 = [0, 1, 2, 3], [6, 7, 8]
    restraint = forces.HarmonicRestraintForce(K, g1, g2)
    f = CustomCentroidBondForce(2, restraint.getEnergyFunction())
    f.addGlobalParameter('lambda_restraints', lam); f.addPerBondParameter('K')
    f.addGroup(g1); f.addGroup(g2); f.addBond([0, 1], [K])
    E, F = oracle.evaluate_force(f, masses, X)
    w1, w2 = masses[g1] / masses[g1].sum(), masses[g2] / masses[g2].sum()
    d = w2 @ X[g2] - w1 @ X[g1]
    assert E.shape == (1,) and E[0] == pytest.approx(lam * 0.5 * K * d @ d, rel=1e-13)
    want = np.zeros_like(X)
    want[g1] = lam * K * w1[:, None] * d
    want[g2] = -lam * K * w2[:, None] * d
    assert np.abs(F - want).max() <= 1e-8 * np.abs(want).max()
