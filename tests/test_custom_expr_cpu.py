"""CPU: the expression compiler (openmmtools_amd/custom_expr.py) against the independent f64 helper (tests/custom_expr_oracle.py), and
the host plumbing of the custom bond / angle / torsion / external forces: the four classes, the refusals, the descriptors of the two
forms that keep their own paths, GlobalParameterState over the forces' globals and the [K][n_globals] table the sampler builds."""
import copy
import math

import numpy as np
import pytest

import custom_expr_oracle as oracle
from custom_opcode_cases import run_program
from openmmtools_amd import alchemy, custom_expr as cx, forces, states, testsystems
from openmmtools_amd.system import (System, system_to_desc, CustomBondForce, CustomAngleForce, CustomTorsionForce, CustomExternalForce)


# (the small stack machine for the postfix program, run_program, lives in tests/custom_opcode_cases.py)


# (energy, variables, parameter names -> values, global names -> values); between them every operator and every function
CASES = [
    ('0.5*K*(r-r0)^2', dict(r=0.17), dict(K=2.5e5, r0=0.153), {}),
    ('lambda_bonds^gamma * 0.5*K*(r-r0)^2', dict(r=0.17), dict(K=2.5e5, r0=0.153), dict(lambda_bonds=0.7, gamma=1.5)),
    ('D*(1-exp(-a*(r-r0)))^2; a = sqrt(K/(2*D)); D = 4.2e2', dict(r=0.21), dict(K=3.1e5, r0=0.15), {}),
    ('e2 + e1; e1 = k*(1+cos(n*theta-phase)); e2 = 1.5E-1*sin(theta)^2', dict(theta=-2.1), dict(k=4.6, n=3.0, phase=0.4), {}),
    ('select(step(theta-t0), k*(theta-t0)^2, -k2*(theta-t0)^3)', dict(theta=1.2), dict(k=30.0, k2=8.0, t0=1.9), {}),
    ('((k/2)*((x-x0)^2+(y-y0)^2)) + k4*(z-z0)^4', dict(x=0.3, y=-1.1, z=0.8), dict(k=900.0, k4=120.0, x0=0.25, y0=-1.0, z0=0.6), {}),
    ('a^2 + a^-1 + a^0.5 + (-a)^3 - -a^2; a = r/s', dict(r=0.37), dict(s=0.5), {}),
    ('tan(r) + asin(r) + acos(r) + atan(r/2) + atan2(r, 0.3) + log(1+r)', dict(r=0.41), {}, {}),
    ('sinh(r) + cosh(2*r) - tanh(r/3) + erf(r) + erfc(2*r) + abs(r-1) + abs(1-r)', dict(r=0.83), {}, {}),
    ('min(r, c)^2 + max(r, c)*3 + floor(r*10) + ceil(r*10) + delta(r-r) + delta(r) + step(-r)', dict(r=0.52), dict(c=0.7), {}),
    ('k*(min(theta, c)-1)^2 / (1 + max(theta, c))', dict(theta=2.3), dict(k=3.0, c=1.1), {}),
    ('k*periodicdistance(x, y, z, x0, y0, z0)^2', dict(x=0.2, y=2.9, z=1.4), dict(k=500.0, x0=2.8, y0=0.1, z0=1.5), {}),
    ('g^lam * 2.0e+1 * r^(1/2) * (3 - 1)', dict(r=0.9), {}, dict(g=2.0, lam=0.3)),
]
BOX = np.array([3.0, 3.1, 3.2])


def _compile(energy, variables, params, global_values):
    return cx.compile_expression(energy, list(variables), list(params), {n: i for i, n in enumerate(global_values)},
                                 periodic_distance='periodicdistance' in energy)


@pytest.mark.parametrize('case', range(len(CASES)))
def test_compiled_program_against_the_helper(case):
    energy, variables, params, global_values = CASES[case]
    prog = _compile(energy, variables, params, global_values)
    E, dE, deepest = run_program(prog, list(variables.values()), list(params.values()), list(global_values.values()), BOX)
    assert deepest == prog['stack_depth'] <= cx.MAX_STACK
    expression = oracle.Expression(energy)

    def f(v):
        return expression(dict(zip(variables, v), **params, **global_values), BOX)
    x = np.array(list(variables.values()))
    want = f(x)
    assert E == pytest.approx(want, rel=1e-12)
    for k in range(len(x)):
        # five-point differences at h and h / 2 and their Richardson combination: the helper's derivative, with the error the
        # halving shows; the analytic partial must sit within it (never looser than 1e-7, never tighter than 1e-12, relative)
        d = []
        for h in (1e-3, 5e-4):
            e = [f(x + m * h * np.eye(len(x))[k]) for m in (-2, -1, 1, 2)]
            d.append((e[0] - 8.0 * e[1] + 8.0 * e[2] - e[3]) / (12.0 * h))
        best = (16.0 * d[1] - d[0]) / 15.0
        scale = max(abs(best), abs(want))
        err = abs(best - d[1])
        assert err <= 1e-7 * scale
        assert abs(dE[k] - best) <= max(4.0 * err, 1e-12 * scale), (energy, k, dE[k], best, err)


def test_small_integer_powers_are_multiplications():
    prog = _compile('a^2 + a^-1 + a^0.5', dict(a=1.0), {}, {})
    ops = [tuple(p) for p in prog['program']]
    assert (cx.POWI, 2) in ops and (cx.POWI, -1) in ops and [o for o, _ in ops].count(cx.POW) == 1
    E, dE, _ = run_program(_compile('a^3', dict(a=1.0), {}, {}), [-2.0], [], [])
    assert (E, dE[0]) == (-8.0, 12.0)


def test_definitions_in_any_order_and_scientific_notation():
    a = _compile('u*v; u = 2.5e-1*w; w = r+1E1; v = .5', dict(r=1.0), {}, {})
    assert run_program(a, [1.0], [], [])[0] == 0.25 * 11.0 * 0.5


# ---- host plumbing -------------------------------------------------------------------------------------------------------------------
def _two_particles():
    s = System()
    for _ in range(4):
        s.addParticle(12.0)
    return s


def _bond(energy='lambda_bonds^gamma * 0.5*K*(r-r0)^2', group=0, lam=1.0):
    f = CustomBondForce(energy)
    f.addGlobalParameter('lambda_bonds', lam); f.addGlobalParameter('gamma', 1.0)
    f.addPerBondParameter('K'); f.addPerBondParameter('r0')
    f.addBond(0, 1, [1000.0, 0.15])
    f.setForceGroup(group)
    return f


def test_the_four_classes_mirror_openmm():
    b = _bond()
    assert forces.CustomBondForce is CustomBondForce
    assert (b.getNumGlobalParameters(), b.getGlobalParameterName(1), b.getGlobalParameterDefaultValue(0)) == (2, 'gamma', 1.0)
    assert (b.getNumPerBondParameters(), b.getPerBondParameterName(1), b.getNumBonds()) == (2, 'r0', 1)
    b.setBondParameters(0, 1, 2, [5.0, 0.2]); assert b.getBondParameters(0) == (1, 2, [5.0, 0.2])
    a = CustomAngleForce('k*(theta-t0)^2'); a.addPerAngleParameter('k'); a.addPerAngleParameter('t0'); a.addAngle(0, 1, 2, [3.0, 1.9])
    assert (a.getNumPerAngleParameters(), a.getPerAngleParameterName(0), a.getNumAngles(), a.getAngleParameters(0)) == (2, 'k', 1, (0, 1, 2, [3.0, 1.9]))
    t = CustomTorsionForce('k*cos(theta)'); t.addPerTorsionParameter('k'); t.addTorsion(0, 1, 2, 3, [2.0])
    t.setTorsionParameters(0, 3, 2, 1, 0, [4.0])
    assert (t.getNumPerTorsionParameters(), t.getNumTorsions(), t.getTorsionParameters(0)) == (1, 1, (3, 2, 1, 0, [4.0]))
    e = CustomExternalForce('k*x^2'); e.addPerParticleParameter('k'); e.addParticle(2, [7.0])
    assert (e.getNumPerParticleParameters(), e.getNumParticles(), e.getParticleParameters(0)) == (1, 1, (2, [7.0]))
    for f in (a, t, e):
        f.setEnergyFunction(f.getEnergyFunction() + '+0'); f.setUsesPeriodicBoundaryConditions(True); f.setForceGroup(3)
        assert f.getEnergyFunction().endswith('+0') and f.usesPeriodicBoundaryConditions() and f.getForceGroup() == 3


def test_descriptor_of_a_custom_bond_force():
    s = _two_particles(); s.addForce(_bond(group=2, lam=0.5))
    d = system_to_desc(s)
    t = d['custom_terms']['000']
    assert (t['kind'], t['periodic'], t['force_group'], t['global_names']) == (cx.KIND_BOND, 0, 2, ['lambda_bonds', 'gamma'])
    assert np.array_equal(t['atoms'], [[0, 1]]) and np.array_equal(t['params'], [[1000.0, 0.15]]) and np.array_equal(t['global_defaults'], [0.5, 1.0])
    assert t['program'].dtype == np.int32 and t['program'].shape[1] == 2 and t['consts'].dtype == np.float64 and t['stack_depth'] >= 2
    assert 'restraints' not in d and d['n_ext'] == 0
    assert d['custom_globals']['names'] == ['lambda_bonds', 'gamma'] and np.array_equal(d['custom_globals']['defaults'], [0.5, 1.0])
    s2 = _two_particles(); s2.addForce(_bond(group=2, lam=0.25))
    assert s.fingerprint() != s2.fingerprint()


def test_refusals_name_the_force_and_the_item():
    def desc(force, *more):
        s = _two_particles(); s.addForce(force)
        for f in more:
            s.addForce(f)
        return system_to_desc(s)
    with pytest.raises(NotImplementedError, match="CustomBondForce.*unknown variable 'q'"):
        desc(_bond('K*(r-r0)^2 + q'))
    with pytest.raises(NotImplementedError, match="CustomBondForce.*unknown function 'besselj'"):
        desc(_bond('K*besselj(r-r0)'))
    with pytest.raises(NotImplementedError, match="CustomAngleForce.*unknown variable 'r'"):
        a = CustomAngleForce('r^2'); a.addAngle(0, 1, 2); desc(a)
    with pytest.raises(NotImplementedError, match="unknown function 'periodicdistance'"):      # only in a periodic external force
        e = CustomExternalForce('periodicdistance(x,y,z,0,0,0)'); e.addParticle(0); desc(e)
    f = _bond('K*tab(r)'); f.addTabulatedFunction('tab', object())
    with pytest.raises(NotImplementedError, match="CustomBondForce.*tabulated function 'tab'"):
        desc(f)
    with pytest.raises(NotImplementedError, match='CustomBondForce.*%d instructions' % (2 * cx.MAX_PROGRAM + 1)):
        desc(_bond('+'.join(['r'] * (cx.MAX_PROGRAM + 1))))
    deep = 'r'
    for _ in range(cx.MAX_STACK):
        deep = 'r+(%s)' % deep                                  # right-nested: one more slot per level
    with pytest.raises(NotImplementedError, match='CustomBondForce.*%d stack slots' % (cx.MAX_STACK + 1)):
        desc(_bond(deep))
    f = CustomBondForce('r')
    for k in range(cx.MAX_PARAMS + 1):
        f.addPerBondParameter('p%d' % k)
    f.addBond(0, 1, [0.0] * (cx.MAX_PARAMS + 1))
    with pytest.raises(NotImplementedError, match='CustomBondForce.*%d per-term parameters' % (cx.MAX_PARAMS + 1)):
        desc(f)
    f = CustomBondForce('r'); f.addBond(0, 1)
    for k in range(cx.MAX_GLOBALS + 1):
        f.addGlobalParameter('g%d' % k, 0.0)
    with pytest.raises(NotImplementedError, match='%d global parameters.*g0' % (cx.MAX_GLOBALS + 1)):
        desc(f)
    with pytest.raises(NotImplementedError, match=r'several force groups \(0, 3\).*CustomBondForce in 3'):
        desc(_bond(group=0), _bond(group=3))
    with pytest.raises(ValueError, match="global parameter 'lambda_bonds' has the default value 0.5"):
        desc(_bond(lam=1.0), _bond(lam=0.5))
    with pytest.raises(NotImplementedError):
        c = forces.CustomCentroidBondForce(2, 'K*distance(g1,g2)^3'); c.addGroup([0]); c.addGroup([1]); c.addPerBondParameter('K'); c.addBond([0, 1], [1.0])
        desc(c)


def test_the_two_existing_forms_keep_their_descriptors():
    ho = testsystems.HarmonicOscillator()
    d = system_to_desc(ho.system)
    f = ho.system.getForce(0)
    assert 'custom_terms' not in d and d['n_ext'] == 1 and d['ext_K'] == f.getGlobalParameter('testsystems_HarmonicOscillator_K')
    assert d['ext_x0'] == f.getGlobalParameter('testsystems_HarmonicOscillator_x0') and np.array_equal(d['ext_atoms'], [0])
    for make in (lambda: forces.HarmonicRestraintForce(100.0, [0, 1], [2, 3]), lambda: forces.HarmonicRestraintBondForce(100.0, 0, 3),
                 lambda: forces.FlatBottomRestraintForce(100.0, 0.5, [0, 1], [2, 3]), lambda: forces.FlatBottomRestraintBondForce(100.0, 0.5, 0, 3)):
        s = _two_particles(); s.addForce(make())
        d = system_to_desc(s)
        assert 'custom_terms' not in d and len(d['restraints']) == 1
        r = d['restraints']['000']
        assert (r['K'], r['parameter'], r['kind']) == (100.0, 'lambda_restraints', int('FlatBottom' in type(s.getForce(0)).__name__))


class BondState(states.GlobalParameterState):
    """the example of the reference's GlobalParameterState docstring: lambda_bonds and gamma of a CustomBondForce"""
    lambda_bonds = states.GlobalParameterState.GlobalParameter('lambda_bonds', standard_value=1.0)
    gamma = states.GlobalParameterState.GlobalParameter('gamma', standard_value=1.0)


def test_global_parameter_state_over_a_custom_bond_force():
    s = _two_particles(); s.addForce(_bond(lam=0.5))
    e = CustomExternalForce('k*gamma*x^2'); e.addGlobalParameter('gamma', 1.0); e.addPerParticleParameter('k'); e.addParticle(0, [3.0])
    s.addForce(e)                                                     # gamma: one column shared by two forces
    st = BondState.from_system(s)
    assert (st.lambda_bonds, st.gamma) == (0.5, 1.0)
    st.lambda_bonds, st.gamma = 0.2, 2.0
    st.apply_to_system(s)
    assert s.getForce(0).getGlobalParameterDefaultValue(0) == 0.2 and s.getForce(0).getGlobalParameterDefaultValue(1) == 2.0
    assert s.getForce(1).getGlobalParameterDefaultValue(0) == 2.0
    names = system_to_desc(s)['custom_terms']['000']['global_names']
    assert names == ['lambda_bonds', 'gamma'] and system_to_desc(s)['custom_terms']['001']['global_names'] == names
    ts = states.ThermodynamicState(s, 300.0)
    compound = [states.CompoundThermodynamicState(copy.deepcopy(ts), [BondState(lambda_bonds=l, gamma=g)]) for l, g in ((1.0, 1.0), (0.5, 2.0), (0.0, 3.0))]
    table = cx.custom_globals(s, names, compound + [ts])
    assert np.array_equal(table, [[1.0, 1.0], [0.5, 2.0], [0.0, 3.0], [0.2, 2.0]])        # the plain state: the forces' defaults


def test_the_alchemical_factory_passes_a_custom_force_through():
    al = testsystems.AlanineDipeptideVacuum()
    f = _bond()
    al.system.addForce(f)
    system = alchemy.AbsoluteAlchemicalFactory().create_alchemical_system(al.system, alchemy.AlchemicalRegion(alchemical_atoms=list(range(0, 6))))
    kept = [g for g in system.getForces() if isinstance(g, CustomBondForce)]
    assert len(kept) == 1 and kept[0].getEnergyFunction() == f.getEnergyFunction() and kept[0].getBondParameters(0) == f.getBondParameters(0)
    assert len(system_to_desc(system)['custom_terms']) == 1


def test_stores_and_pools_refuse_by_name():
    from openmmtools_amd import system_xml
    from openmmtools_amd.multistate._reference_store import ReferenceStoreWriter
    from openmmtools_amd.multistate._engine_pool import EnginePool
    s = _two_particles(); s.addForce(_bond())
    with pytest.raises(NotImplementedError, match='CustomBondForce with the energy'):
        system_xml.to_xml(s)
    what = ReferenceStoreWriter.can_store([states.ThermodynamicState(s, 300.0)], [], [])
    assert 'CustomBondForce' in what

    class Stub:
        def spawn(self): return Stub()
    d = system_to_desc(s)
    with pytest.raises(NotImplementedError, match='custom bond / angle / torsion / external forces'):
        EnginePool(Stub(), [[0], [1]]).set_system([d, d])


def test_the_cpu_port_refuses_custom_terms():
    import os
    from openmmtools_amd import _engine
    here = os.path.dirname(os.path.abspath(__file__))
    cpu_lib = os.path.join(os.path.dirname(here), 'oracle', '_build', 'libremd_cpu.so')
    if not os.path.exists(cpu_lib):
        import __graft_entry__
        __graft_entry__.build()
    eng = _engine.HipEngine(lib_path=cpu_lib)
    hg = testsystems.HostGuestVacuum()
    hg.system.addForce(_bond())
    with pytest.raises(NotImplementedError, match='remd_set_custom_terms.*remd_hip_custom.h'):
        eng.set_system(system_to_desc(hg.system))
