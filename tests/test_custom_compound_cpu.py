"""CPU: CustomCompoundBondForce -- the compiler's compound kind (openmmtools_amd/custom_expr.py) against the independent f64 helper
(tests/compound_expr_oracle.py) through a small Python mirror of the device's machine with its seeded passes, and the host plumbing:
the class, the descriptor, the fingerprint, the refusals."""
import copy
import math

import numpy as np
import pytest

import compound_expr_oracle as oracle
from custom_expr_oracle import Expression
from custom_opcode_cases import run_pass
from openmmtools_amd import alchemy, custom_expr as cx, states, testsystems
from openmmtools_amd.system import System, system_to_desc, CustomBondForce, CustomCompoundBondForce


# (the mirror of the machine for a compound program, run_pass with its seeded passes, lives in tests/custom_opcode_cases.py)


# six particles of a bent chain: no three in a line, no four in a plane
X6 = np.array([[0.00, 0.00, 0.00], [0.15, 0.02, -0.03], [0.21, 0.14, 0.04], [0.35, 0.17, -0.05], [0.40, 0.31, 0.02], [0.55, 0.30, 0.13]])


def boresch_parameters(x, offsets=(0.03, 0.4, -0.35, 0.45, -0.3, 0.5)):
    """the twelve per-bond parameters with every reference value `offsets` off the geometry of x, so that every term pulls"""
    v = oracle.boresch_values(x)
    K = (4000.0, 80.0, 90.0, 70.0, 60.0, 50.0)
    return [p for k, ref in zip(K, (a - o for a, o in zip(v, offsets))) for p in (k, ref)]


# (energy, particles, parameter names, parameter values, global names -> values, positions)
CASES = [
    (oracle.BORESCH, 6, oracle.BORESCH_PARAMETERS, boresch_parameters(X6), dict(lambda_restraints=0.7), X6),
    ('k*(x1-x0)^2 + kd*distance(p2,p1)^2*z2 + pointdistance(x1,y1,z1,x2,y2+0.1,z3)^3 + sin(y3)*angle(p1,p3,p2)', 3, ('k', 'x0', 'kd'),
     [30.0, 0.1, 12.0], {}, X6[:3]),
    ('k*(1+cos(n*dihedral(p1,p2,p3,p4)-phase)) + exp(-distance(p1,p4))', 4, ('k', 'n', 'phase'), [4.6, 3.0, 0.4], {}, X6[:4]),
    ('k*(1+cos(n*dihedral(p1,p2,p3,p4)-phase)) + exp(-distance(p1,p4))', 4, ('k', 'n', 'phase'), [4.6, 3.0, 0.4], {},
     X6[:4] * np.array([1.0, 1.0, -1.0])),                       # (the mirror image: the dihedral of the other sign)
]


def _compile(energy, P, names, global_values):
    return cx.compile_expression(energy, cx.compound_variables(P), list(names), {n: i for i, n in enumerate(global_values)}, n_particles=P)


def test_the_boresch_expression_fits_the_engines_limits():
    prog = _compile(oracle.BORESCH, 6, oracle.BORESCH_PARAMETERS, dict(lambda_restraints=1.0))
    print('Boresch: %d instructions, %d stack slots, %d constants' % (len(prog['program']), prog['stack_depth'], len(prog['consts'])))
    assert len(prog['program']) <= cx.MAX_PROGRAM and prog['stack_depth'] <= cx.MAX_STACK and len(oracle.BORESCH_PARAMETERS) <= cx.MAX_PARAMS
    ops = [tuple(p) for p in prog['program']]
    assert (cx.DISTANCE, 2 | 3 << 4) in ops and (cx.ANGLE, 1 | 2 << 4 | 3 << 8) in ops and (cx.DIHEDRAL, 0 | 1 << 4 | 2 << 8 | 3 << 12) in ops
    assert (cx.DIHEDRAL, 2 | 3 << 4 | 4 << 8 | 5 << 12) in ops


def test_both_signs_of_the_dihedral_are_covered():
    a, b = (oracle.geometry(CASES[k][5])['dihedral'](0, 1, 2, 3) for k in (2, 3))
    assert a == -b and abs(a) > 0.3
    # no dihedral difference of the Boresch case within 0.1 rad of its wrap: the helper's differences never straddle the floor
    v, p = oracle.boresch_values(X6), CASES[0][3]
    for phi, ref in zip(v[3:], (p[7], p[9], p[11])):
        assert abs(abs(oracle.wrap(phi - ref)) - math.pi) > 0.1


@pytest.mark.parametrize('case', range(len(CASES)))
def test_compiled_program_against_the_helper(case):
    energy, P, names, params, global_values, x = CASES[case]
    prog = _compile(energy, P, names, global_values)
    expression = Expression(energy)

    def f(y):
        return oracle.bond_energy(expression, y, names, params, global_values)
    want = f(x)
    for seed in range(P):
        E, dE, deepest = run_pass(prog, x, params, list(global_values.values()), seed)
        assert deepest == prog['stack_depth'] <= cx.MAX_STACK
        assert E == pytest.approx(want, rel=1e-12)
        for k in range(3):
            # five-point differences at h and h / 2 and their Richardson combination: the helper's derivative, with the error the
            # halving shows; the analytic partial must sit within it (never looser than 1e-7, never tighter than 1e-12, relative)
            d = []
            for h in (1e-3, 5e-4):
                e = []
                for m in (-2, -1, 1, 2):
                    y = x.copy(); y[seed, k] += m * h
                    e.append(f(y))
                d.append((e[0] - 8.0 * e[1] + 8.0 * e[2] - e[3]) / (12.0 * h))
            best = (16.0 * d[1] - d[0]) / 15.0
            scale = max(abs(best), abs(want))
            err = abs(best - d[1])
            assert err <= 1e-7 * scale
            assert abs(dE[k] - best) <= max(4.0 * err, 1e-12 * scale), (energy, seed, k, dE[k], best, err)
    E, dE, _ = run_pass(prog, x, params, list(global_values.values()), -1)          # unseeded (the u_kl kernel): the value alone
    assert E == pytest.approx(want, rel=1e-12) and not dE.any()


# ---- host plumbing -------------------------------------------------------------------------------------------------------------------
def _system(n=10):
    s = System()
    for _ in range(n):
        s.addParticle(12.0)
    return s


def _boresch(lam=1.0, group=0, params=None):
    f = CustomCompoundBondForce(6, oracle.BORESCH)
    f.addGlobalParameter('lambda_restraints', lam)
    for name in oracle.BORESCH_PARAMETERS:
        f.addPerBondParameter(name)
    f.addBond([0, 1, 2, 3, 4, 5], boresch_parameters(X6) if params is None else params)
    f.setForceGroup(group)
    return f


def test_the_class_mirrors_openmm():
    f = _boresch(lam=0.5, group=3)
    assert (f.getNumParticlesPerBond(), f.getNumBonds(), f.getNumPerBondParameters(), f.getPerBondParameterName(1)) == (6, 1, 12, 'r_aA0')
    assert (f.getNumGlobalParameters(), f.getGlobalParameterName(0), f.getGlobalParameterDefaultValue(0)) == (1, 'lambda_restraints', 0.5)
    particles, parameters = f.getBondParameters(0)
    assert particles == [0, 1, 2, 3, 4, 5] and parameters == boresch_parameters(X6)
    f.setBondParameters(0, [5, 4, 3, 2, 1, 0], [1.0] * 12)
    assert f.getBondParameters(0) == ([5, 4, 3, 2, 1, 0], [1.0] * 12)
    assert f.addBond((1, 2, 3, 4, 5, 6), [2.0] * 12) == 1 and f.getNumBonds() == 2
    f.setGlobalParameterDefaultValue(0, 0.25); f.setUsesPeriodicBoundaryConditions(True); f.setEnergyFunction(oracle.BORESCH + '; unused = 1')
    assert f.getGlobalParameterDefaultValue(0) == 0.25 and f.usesPeriodicBoundaryConditions() and f.getForceGroup() == 3
    assert f.getEnergyFunction().endswith('unused = 1')
    assert f.addTabulatedFunction('tab', object()) == 0 and (f.getNumTabulatedFunctions(), f.getTabulatedFunctionName(0)) == (1, 'tab')
    with pytest.raises(ValueError, match='a bond of 5 particles, the force declares 6'):
        f.addBond([0, 1, 2, 3, 4], [0.0] * 12)
    atoms, params = f._term_arrays()
    assert atoms.shape == (2, 6) and atoms.dtype == np.int32 and params.shape == (2, 12)
    assert cx.is_custom_term_force(f) and cx.KIND_OF_CLASS['CustomCompoundBondForce'] == cx.KIND_COMPOUND == 4
    assert (cx.DISTANCE, cx.ANGLE, cx.DIHEDRAL, cx.MAX_PARTICLES) == (35, 36, 37, 8)


def test_descriptor_and_fingerprint():
    s = _system(); s.addForce(_boresch(lam=0.5, group=2))
    b = CustomBondForce('0.5*K*r^2'); b.addPerBondParameter('K'); b.addBond(0, 1, [3.0]); b.setForceGroup(2)
    s.addForce(b)
    d = system_to_desc(s)
    t, u = d['custom_terms']['000'], d['custom_terms']['001']
    assert (t['kind'], t['n_particles'], t['periodic'], t['force_group'], t['global_names']) == (cx.KIND_COMPOUND, 6, 0, 2, ['lambda_restraints'])
    assert np.array_equal(t['atoms'], [[0, 1, 2, 3, 4, 5]]) and t['atoms'].dtype == np.int32 and t['params'].shape == (1, 12)
    assert t['program'].dtype == np.int32 and t['program'].shape[1] == 2 and t['consts'].dtype == np.float64 and 2 <= t['stack_depth'] <= cx.MAX_STACK
    assert u['kind'] == cx.KIND_BOND and 'n_particles' not in u                    # (the siblings' dicts are what they were)
    assert d['custom_globals']['names'] == ['lambda_restraints'] and np.array_equal(d['custom_globals']['defaults'], [0.5])
    prints = {s.fingerprint()}
    for change in (lambda f: f.setBondParameters(0, [0, 1, 2, 3, 4, 5], [1.0] + boresch_parameters(X6)[1:]),
                   lambda f: f.setBondParameters(0, [0, 1, 2, 3, 4, 6], boresch_parameters(X6)),
                   lambda f: f.setEnergyFunction(oracle.BORESCH.replace('K_r/2', 'K_r/3')),
                   lambda f: f.setGlobalParameterDefaultValue(0, 0.75)):
        s2 = copy.deepcopy(s); change(s2.getForce(0))
        prints.add(s2.fingerprint())
    assert len(prints) == 5


def test_global_table_and_alchemical_factory_take_the_force():
    class RestraintState(states.GlobalParameterState):
        lambda_restraints = states.GlobalParameterState.GlobalParameter('lambda_restraints', standard_value=1.0)
    s = _system(); s.addForce(_boresch(lam=0.5))
    assert RestraintState.from_system(s).lambda_restraints == 0.5
    ts = states.ThermodynamicState(s, 300.0)
    compound = [states.CompoundThermodynamicState(copy.deepcopy(ts), [RestraintState(lambda_restraints=l)]) for l in (1.0, 0.25, 0.0)]
    assert np.array_equal(cx.custom_globals(s, ['lambda_restraints'], compound + [ts]), [[1.0], [0.25], [0.0], [0.5]])
    al = testsystems.AlanineDipeptideVacuum()
    f = _boresch()
    al.system.addForce(f)
    system = alchemy.AbsoluteAlchemicalFactory().create_alchemical_system(al.system, alchemy.AlchemicalRegion(alchemical_atoms=list(range(0, 6))))
    kept = [g for g in system.getForces() if isinstance(g, CustomCompoundBondForce)]
    assert len(kept) == 1 and kept[0].getEnergyFunction() == f.getEnergyFunction() and kept[0].getBondParameters(0) == f.getBondParameters(0)
    assert [t['kind'] for t in system_to_desc(system)['custom_terms'].values()] == [cx.KIND_COMPOUND]


def _compound(P, energy, group=0):
    f = CustomCompoundBondForce(P, energy)
    f.addBond(list(range(P)))
    f.setForceGroup(group)
    return f


def test_refusals_name_the_force_and_the_item():
    def desc(*forces):
        s = _system()
        for f in forces:
            s.addForce(f)
        return system_to_desc(s)
    with pytest.raises(NotImplementedError, match="CustomCompoundBondForce.*particle name 'p2' outside"):
        desc(_compound(3, 'distance(p1,p2) + p2'))
    with pytest.raises(NotImplementedError, match="CustomCompoundBondForce.*arguments of 'angle' are particle names"):
        desc(_compound(3, 'angle(p1,p2,x3)'))
    with pytest.raises(NotImplementedError, match="CustomCompoundBondForce.*particle 'p4' in a bond of 3 particles"):
        desc(_compound(3, 'distance(p1,p4)'))
    with pytest.raises(NotImplementedError, match="CustomCompoundBondForce.*unknown variable 'x4'"):
        desc(_compound(3, 'x4^2'))
    with pytest.raises(NotImplementedError, match="CustomCompoundBondForce.*'dihedral' takes 4 particles, not 3"):
        desc(_compound(4, 'dihedral(p1,p2,p3)'))
    with pytest.raises(NotImplementedError, match="CustomCompoundBondForce.*'pointdistance' takes 6 arguments, not 5"):
        desc(_compound(2, 'pointdistance(x1,y1,z1,x2,y2)'))
    for name in ('pointangle', 'pointdihedral'):
        with pytest.raises(NotImplementedError, match="CustomCompoundBondForce.*function '%s'" % name):
            desc(_compound(4, '%s(%s)' % (name, ','.join(['x1'] * (9 if name == 'pointangle' else 12)))))
    f = _compound(2, 'tab(distance(p1,p2))'); f.addTabulatedFunction('tab', object())
    with pytest.raises(NotImplementedError, match="CustomCompoundBondForce.*tabulated function 'tab'"):
        desc(f)
    with pytest.raises(NotImplementedError, match=r'CustomCompoundBondForce: bonds of 9 particles \(the engine takes 1 ... 8\)'):
        desc(_compound(9, 'distance(p1,p9)'))
    with pytest.raises(NotImplementedError, match="unknown function 'distance'"):          # the particles' functions: only in a compound force
        b = CustomBondForce('distance(p1,p2)'); b.addBond(0, 1); desc(b)
    with pytest.raises(NotImplementedError, match=r'several force groups \(0, 3\).*CustomCompoundBondForce in 3'):
        desc(_compound(2, 'distance(p1,p2)', group=0), _compound(2, 'distance(p1,p2)', group=3))
    with pytest.raises(NotImplementedError, match='%d custom forces' % (cx.MAX_FORCES + 1)):
        desc(*[_compound(2, 'distance(p1,p2)') for _ in range(cx.MAX_FORCES + 1)])
    assert len(desc(_compound(8, 'dihedral(p5,p6,p7,p8) + x8'))['custom_terms']) == 1       # (the most particles the engine takes)


def test_stores_and_pools_refuse_by_name():
    from openmmtools_amd import system_xml
    from openmmtools_amd.multistate._reference_store import ReferenceStoreWriter
    from openmmtools_amd.multistate._engine_pool import EnginePool
    s = _system(); s.addForce(_boresch())
    with pytest.raises(NotImplementedError, match='CustomCompoundBondForce with the energy'):
        system_xml.to_xml(s)
    assert 'CustomCompoundBondForce' in ReferenceStoreWriter.can_store([states.ThermodynamicState(s, 300.0)], [], [])

    class Stub:
        def spawn(self): return Stub()
    d = system_to_desc(s)
    with pytest.raises(NotImplementedError, match='compound-bond forces.*more than one compatibility group'):
        EnginePool(Stub(), [[0], [1]]).set_system([d, d])


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
    hg.system.addForce(_boresch())
    with pytest.raises(NotImplementedError, match='remd_set_custom_terms.*compound-bond forces.*remd_hip_custom.h'):
        eng.set_system(system_to_desc(hg.system))
