"""CPU: system.CustomNonbondedForce, the sixth kind of openmmtools_amd/custom_expr.py (the variable r, p1 / p2 operands), its descriptor,
the host's long-range correction, the refusals, and the four test systems built on it."""
import math

import numpy as np
import pytest

import custom_dual_oracle as dual
import custom_nonbonded_oracle as oracle
import custom_opcode_cases as machine
from openmmtools_amd import alchemy, custom_expr as cx, system_xml, testsystems, unit
from openmmtools_amd.constants import kB
from openmmtools_amd.system import System, system_to_desc, CustomNonbondedForce

WCA = '4.0*epsilon*((sigma/r)^12 - (sigma/r)^6) + epsilon;sigma = 0.340000;epsilon = 0.997740;'
MIXTURE = '4*epsilon*((sigma/r)^12 - (sigma/r)^6);sigma = 0.340000;epsilon = 0.995792;'
LJ_MIXED = '4*epsilon*((sigma/r)^12 - (sigma/r)^6); sigma = 0.5*(sigma1 + sigma2); epsilon = sqrt(epsilon1*epsilon2)'


def _system(n, forces, box=(3.0, 3.0, 3.0)):
    s = System()
    for _ in range(n):
        s.addParticle(39.9)
    s.setDefaultPeriodicBoxVectors([box[0], 0, 0], [0, box[1], 0], [0, 0, box[2]])
    for f in forces:
        s.addForce(f)
    return s


def _two_class_lj(n_a=30, n_b=50, switch=None, lrc=True):
    f = CustomNonbondedForce(LJ_MIXED)
    f.addPerParticleParameter('sigma')
    f.addPerParticleParameter('epsilon')
    for k in range(n_a + n_b):
        f.addParticle([0.30, 1.1] if k < n_a else [0.36, 0.4])
    f.setNonbondedMethod(CustomNonbondedForce.CutoffPeriodic)
    f.setCutoffDistance(1.0)
    if switch is not None:
        f.setUseSwitchingFunction(True)
        f.setSwitchingDistance(switch)
    f.setUseLongRangeCorrection(lrc)
    return f


# ---- the class -----------------------------------------------------------------------------------------------------------------------------
def test_accessors():
    f = CustomNonbondedForce('a*r')
    assert (f.NoCutoff, f.CutoffNonPeriodic, f.CutoffPeriodic) == (0, 1, 2)
    assert f.getEnergyFunction() == 'a*r' and f.getNonbondedMethod() == f.NoCutoff and not f.usesPeriodicBoundaryConditions()
    assert f.addPerParticleParameter('q') == 0 and f.addPerParticleParameter('s') == 1
    assert f.getNumPerParticleParameters() == 2 and f.getPerParticleParameterName(1) == 's'
    assert f.addGlobalParameter('a', 2.0) == 0 and f.getGlobalParameterName(0) == 'a' and f.getGlobalParameterDefaultValue(0) == 2.0
    assert f.addParticle([1.0, 2.0]) == 0 and f.addParticle([3.0, 4.0]) == 1 and f.getNumParticles() == 2
    f.setParticleParameters(1, [5.0, 6.0])
    assert f.getParticleParameters(1) == [5.0, 6.0]
    assert f.addExclusion(0, 1) == 0 and f.getNumExclusions() == 1 and f.getExclusionParticles(0) == (0, 1)
    f.setNonbondedMethod(f.CutoffPeriodic)
    f.setCutoffDistance(0.9)
    f.setUseSwitchingFunction(True)
    f.setSwitchingDistance(0.7)
    f.setUseLongRangeCorrection(True)
    f.setForceGroup(3)
    assert f.usesPeriodicBoundaryConditions() and f.getCutoffDistance() == 0.9 and f.getUseSwitchingFunction()
    assert f.getSwitchingDistance() == 0.7 and f.getUseLongRangeCorrection() and f.getForceGroup() == 3
    f.setNonbondedMethod(f.CutoffNonPeriodic)
    assert not f.usesPeriodicBoundaryConditions()


@pytest.mark.parametrize('cutoff, want', [
    (1, [(0, 1), (1, 2), (2, 3), (3, 4)]),
    (2, [(0, 1), (0, 2), (1, 2), (1, 3), (2, 3), (2, 4), (3, 4)]),
    (3, [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (1, 4), (2, 3), (2, 4), (3, 4)])])
def test_create_exclusions_from_bonds_on_a_chain_of_five(cutoff, want):
    f = CustomNonbondedForce('r')
    for _ in range(5):
        f.addParticle([])
    f.createExclusionsFromBonds([(0, 1), (1, 2), (2, 3), (3, 4)], cutoff)
    got = sorted(tuple(sorted(f.getExclusionParticles(k))) for k in range(f.getNumExclusions()))
    assert got == want and len(set(got)) == len(got)


# ---- the compiler --------------------------------------------------------------------------------------------------------------------------
def _compile(energy, per_particle=(), global_columns=None):
    return cx.compile_expression(energy, ('r',), (), global_columns or {}, where='CustomNonbondedForce', pair_parameters=tuple(per_particle))


@pytest.mark.parametrize('energy, names, p1, p2', [(WCA, (), (), ()), (MIXTURE, ('charge', 'sigma', 'epsilon'), (0.0, 0.34, 0.9), (0.0, 0.34, 0.0)),
                                                   (LJ_MIXED, ('sigma', 'epsilon'), (0.30, 1.1), (0.36, 0.4))])
def test_compiled_programs_against_the_dual_oracle(energy, names, p1, p2):
    """the programs run through the Python interpreter of the machine (value and dE/dr) within 1e-13 of the dual numbers, the bound of
    tests/test_custom_dual_oracle_cpu.py"""
    prog = _compile(energy, names)
    expression = dual.Expression(energy)
    for r in (0.31, 0.3816, 0.5, 0.97, 1.7):
        v, g, _ = machine.run_program(prog, [r, 0.0, 0.0], list(p1) + list(p2), [])
        values = {'r': dual.Dual(r, np.ones(1))}
        for k, n in enumerate(names):
            values[n + '1'], values[n + '2'] = p1[k], p2[k]
        e = expression(values)
        scale = max(abs(e.v), abs(e.g[0]), 1.0)
        assert abs(v - e.v) <= 1e-13 * scale and abs(g[0] - e.g[0]) <= 1e-13 * scale
        assert cx.run_values(prog, np.array([r]), list(p1) + list(p2), [])[0] == pytest.approx(e.v, rel=1e-13, abs=1e-13)


def test_operand_mapping_of_particle_one_and_two():
    prog = _compile('a1*b2 - b1*a2 + g*r', ('a', 'b'), {'g': 3})
    ops = [tuple(p) for p in prog['program'].tolist()]
    assert [arg for op, arg in ops if op == cx.PARAM] == [0, 3, 1, 2]          # a1, b2, b1, a2: k and n_params + k
    assert (cx.GLOBAL, 3) in ops and (cx.VAR, 0) in ops
    # the definitions come first: a definition may shadow a per-particle name (the mixture string does)
    assert all(op != cx.PARAM for op, _ in _compile(MIXTURE, ('charge', 'sigma', 'epsilon'))['program'].tolist())


@pytest.mark.parametrize('energy, message', [('sigma*r', "per-particle parameter 'sigma' without a particle suffix"),
                                             ('sigma3*r', "per-particle parameter 'sigma3'"),
                                             ('sigma1*x', "variable 'x'"), ('sigma1*y', "variable 'y'"), ('sigma1*z', "variable 'z'"),
                                             ('theta*sigma1', "unknown variable 'theta'")])
def test_names_refused(energy, message):
    with pytest.raises(NotImplementedError, match=message):
        _compile(energy, ('sigma',))


# ---- the descriptor ------------------------------------------------------------------------------------------------------------------------
def test_descriptor_arrays():
    f = _two_class_lj(3, 4, switch=0.8)
    f.addGlobalParameter('unused', 1.5)
    f.addExclusion(5, 1)
    f.addExclusion(1, 0)
    f.setForceGroup(2)
    d = system_to_desc(_system(7, [f]))
    assert d['nb_method'] == 0 and set(d['custom_terms']) == {'000'}          # (no NonbondedForce: the built-in path stays off)
    t = d['custom_terms']['000']
    assert t['kind'] == cx.KIND_NONBONDED == 6 and t['nb_method'] == 2 and t['periodic'] == 1 and t['force_group'] == 2
    assert t['cutoff'] == 1.0 and t['switch_distance'] == 0.8 and t['long_range_correction'] == 1
    assert t['atoms'].shape == (0, 0) and t['params'].shape == (7, 2) and t['params'][3].tolist() == [0.36, 0.4]
    assert t['excl_offsets'].tolist() == [0, 1, 3, 3, 3, 3, 4, 4] and t['excl_atoms'].tolist() == [1, 0, 5, 1]
    assert t['global_names'] == ['unused'] and d['custom_globals']['names'] == ['unused']
    assert t['program'][:, 0].max() < cx.DISTANCE and t['program'][t['program'][:, 0] == cx.PARAM, 1].max() == 3
    g = CustomNonbondedForce('r')
    for _ in range(7):
        g.addParticle([])
    g.setUseSwitchingFunction(True)                                         # NoCutoff: cutoff, switch and correction are ignored
    g.setUseLongRangeCorrection(True)
    t = system_to_desc(_system(7, [g]))['custom_terms']['000']
    assert (t['nb_method'], t['cutoff'], t['switch_distance'], t['long_range_correction'], t['periodic']) == (0, 0.0, -1.0, 0, 0)


# ---- the refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    f = _two_class_lj(3, 4)
    with pytest.raises(NotImplementedError, match='interaction groups'):
        f.addInteractionGroup([0], [1])
    with pytest.raises(NotImplementedError, match='energy parameter derivatives'):
        f.addEnergyParameterDerivative('a')
    s = _system(7, [f])
    with pytest.raises(NotImplementedError, match='CustomNonbondedForce'):
        alchemy.AbsoluteAlchemicalFactory().create_alchemical_system(s, alchemy.AlchemicalRegion(alchemical_atoms=[0]))
    with pytest.raises(NotImplementedError, match='CustomNonbondedForce'):
        system_xml.to_xml(s)
    g = _two_class_lj(3, 4)
    g.addTabulatedFunction('tab', object())
    g.setEnergyFunction('tab(r)')
    with pytest.raises(NotImplementedError, match="tabulated function 'tab'"):
        system_to_desc(_system(7, [g]))
    g = CustomNonbondedForce('r')
    for k in range(9):
        g.addPerParticleParameter('p%d' % k)
    for _ in range(7):
        g.addParticle([0.0] * 9)
    with pytest.raises(NotImplementedError, match='9 per-particle parameters'):
        system_to_desc(_system(7, [g]))
    with pytest.raises(ValueError, match='has 7 particles, the System has 8'):
        system_to_desc(_system(8, [_two_class_lj(3, 4)]))
    tri = _system(7, [_two_class_lj(3, 4)])
    tri.setDefaultPeriodicBoxVectors([3.0, 0, 0], [0.5, 3.0, 0], [0, 0, 3.0])
    with pytest.raises(NotImplementedError, match='triclinic'):
        system_to_desc(tri)
    with pytest.raises(ValueError, match='half the smallest box edge'):
        system_to_desc(_system(7, [_two_class_lj(3, 4)], box=(1.9, 3.0, 3.0)))
    from openmmtools_amd.multistate import _reference_store
    from openmmtools_amd import states
    st = states.ThermodynamicState(s, 300.0 * unit.kelvin)
    assert 'CustomNonbondedForce' in _reference_store.ReferenceStoreWriter.can_store([st], [], [])     # (layout='auto' falls back to records)


def test_several_compatibility_groups_are_refused():
    from openmmtools_amd.multistate._engine_pool import EnginePool

    class Stub:
        def spawn(self): return Stub()
    d = system_to_desc(_system(7, [_two_class_lj(3, 4)]))
    with pytest.raises(NotImplementedError, match='nonbonded custom forces.*more than one compatibility group'):
        EnginePool(Stub(), [[0], [1]]).set_system([d, d])


def test_a_library_without_the_custom_entry_points_refuses_the_force():
    """the CPU port of the ABI exports none of include/remd_hip_custom.h: an engine on such a library names the header and the kinds"""
    import types
    from openmmtools_amd import _engine
    d = system_to_desc(_system(7, [_two_class_lj(3, 4)]))
    eng = object.__new__(_engine.HipEngine)
    eng.lib, eng.h = types.SimpleNamespace(), None                          # (a library that binds nothing of the header)
    for call in (lambda: eng.set_custom_terms([d['custom_terms']['000']]), lambda: eng.set_custom_globals(np.zeros((1, 0))),
                 lambda: eng.custom_energies()):
        with pytest.raises(NotImplementedError, match='nonbonded custom forces.*remd_hip_custom.h is GPU-only'):
            call()


# ---- the long-range correction -------------------------------------------------------------------------------------------------------------
def _coefficients(force, n, table=None):
    t = system_to_desc(_system(n, [force]))['custom_terms']['000']
    return cx.long_range_coefficients([t], np.zeros((1, len(t['global_defaults']))) + t['global_defaults'] if table is None else table)


def _mixed(pa, pb):
    return 0.5 * (pa[0] + pb[0]), math.sqrt(pa[1] * pb[1])


def test_long_range_correction_of_a_two_class_mixture_against_the_closed_form():
    """1e-9 relative: the quadrature in rc / r is exact for the polynomial the Lennard-Jones tail becomes"""
    f = _two_class_lj(30, 50)
    got = _coefficients(f, 80)[0, 0]
    classes = oracle.class_counts([f.getParticleParameters(k) for k in range(80)])
    assert [c for _, c in classes] == [30, 50]
    want = oracle.long_range_coefficient(80, classes, lambda a, b: oracle.lj_tail(*_mixed(a, b), 1.0))
    assert abs(got - want) <= 1e-9 * abs(want)
    # one class: 8 pi N^2 eps (s^12 / (9 rc^9) - s^6 / (3 rc^3))
    g = _two_class_lj(80, 0)
    assert _coefficients(g, 80)[0, 0] == pytest.approx(8.0 * math.pi * 6400 * 1.1 * (0.3 ** 12 / 9.0 - 0.3 ** 6 / 3.0), rel=1e-9)
    assert _coefficients(_two_class_lj(30, 50, lrc=False), 80)[0, 0] == 0.0


def test_long_range_correction_with_a_switch_against_the_trapezoid():
    """the bound is the trapezoid's own: the difference between its values on n and 2 n steps (its error falls by four per doubling, so
    that difference exceeds the finer grid's error), plus 1e-9 relative for the tail"""
    f = _two_class_lj(30, 50, switch=0.75)
    got = _coefficients(f, 80)[0, 0]
    classes = oracle.class_counts([f.getParticleParameters(k) for k in range(80)])

    def lj(a, b):
        s, e = _mixed(a, b)
        return lambda r: 4.0 * e * ((s / r) ** 12 - (s / r) ** 6)
    want, coarse = [oracle.long_range_coefficient(80, classes, lambda a, b: oracle.lj_tail(*_mixed(a, b), 1.0) +
                                                  oracle.switched_part(lj(a, b), 0.75, 1.0, n)) for n in (200000, 100000)]
    bound = abs(want - coarse) + 1e-9 * abs(want)
    print('switched correction: got %.12g, trapezoid %.12g, bound %.3g' % (got, want, bound))
    assert abs(want - coarse) < 1e-8 * abs(want)
    assert abs(got - want) <= bound
    assert abs(got - _coefficients(_two_class_lj(30, 50), 80)[0, 0]) > 1e-3 * abs(got)      # (the switched part is not small)


def test_long_range_correction_follows_a_global_per_state():
    f = CustomNonbondedForce('lambda*4*epsilon*((sigma/r)^12 - (sigma/r)^6); sigma = 0.34; epsilon = 0.997740')
    f.addGlobalParameter('lambda', 1.0)
    for _ in range(70):
        f.addParticle([])
    f.setNonbondedMethod(CustomNonbondedForce.CutoffPeriodic)
    f.setCutoffDistance(1.0)
    f.setUseLongRangeCorrection(True)
    got = _coefficients(f, 70, np.array([[1.0], [0.5], [0.0]]))
    one = 8.0 * math.pi * 4900 * 0.997740 * (0.34 ** 12 / 9.0 - 0.34 ** 6 / 3.0)
    assert got.shape == (3, 1) and np.allclose(got[:, 0], [one, 0.5 * one, 0.0], rtol=1e-9, atol=0.0)


def test_a_correction_that_does_not_converge_names_the_force():
    f = CustomNonbondedForce(WCA)                                           # tends to epsilon, not to zero
    for _ in range(70):
        f.addParticle([])
    f.setNonbondedMethod(CustomNonbondedForce.CutoffPeriodic)
    f.setCutoffDistance(0.38)
    f.setUseLongRangeCorrection(True)
    with pytest.raises(ValueError, match='CustomNonbondedForce.*does not converge'):
        _coefficients(f, 70)


# ---- the test systems (values of the reference's constructors, openmmtools/testsystems.py:2169-2623) -------------------------------------
def _forces(system):
    return [type(f).__name__ for f in system.getForces()]


def test_wca_fluid():
    t = testsystems.WCAFluid()
    f = t.system.getForces()[0]
    assert t.system.getNumParticles() == 216 == f.getNumParticles() and _forces(t.system) == ['CustomNonbondedForce']
    assert np.allclose(np.diag(t.system.getDefaultPeriodicBoxVectors()), float(np.float32((216 / 0.96) ** (1.0 / 3.0))), rtol=0, atol=0)
    assert f.getEnergyFunction() == WCA.replace('0.997740', '%f' % (120.0 * kB))
    assert f.getNonbondedMethod() == CustomNonbondedForce.CutoffPeriodic and f.getCutoffDistance() == 2.0 ** (1.0 / 6.0) * 0.34
    assert not f.getUseSwitchingFunction() and not f.getUseLongRangeCorrection() and f.getNumExclusions() == 0
    assert t.positions.shape == (216, 3) and system_to_desc(t.system)['nb_method'] == 0


def test_double_well_dimer_and_chain():
    d = testsystems.DoubleWellDimer_WCAFluid(ndimers=2, nparticles=70)
    assert _forces(d.system) == ['CustomNonbondedForce', 'CustomBondForce'] and d.system.getNumParticles() == 70
    b = d.system.getForces()[1]
    assert b.getEnergyFunction() == 'h*(1 - ((r-r0-w)/w)^2)^2' and b.getNumBonds() == 2
    assert [b.getBondParameters(k)[:2] for k in range(2)] == [(0, 1), (2, 3)]
    assert np.allclose(b.getBondParameters(0)[2], [6.0 * 0.824 * 120 * kB, 2.0 ** (1.0 / 6.0) * 0.34, 0.3 * 0.34], rtol=1e-15)
    assert d.system.getForces()[0].getNumExclusions() == 0                   # (the reference adds none)
    assert set(system_to_desc(d.system)['custom_terms']) == {'000', '001'}
    with pytest.raises(ValueError, match="Can't create 36 bonds with 70 particles"):
        testsystems.DoubleWellDimer_WCAFluid(ndimers=36, nparticles=70)
    c = testsystems.DoubleWellChain_WCAFluid()
    b = c.system.getForces()[1]
    assert c.system.getNumParticles() == 216 and [b.getBondParameters(k)[:2] for k in range(b.getNumBonds())] == [(0, 1), (1, 2)]
    assert b.getBondParameters(0)[2][0] == pytest.approx(6.0 * 0.824 * kB, rel=1e-15)          # (the reference's default here)
    assert _forces(testsystems.DoubleWellChain_WCAFluid(nchained=0).system) == ['CustomNonbondedForce', 'CustomBondForce']
    assert testsystems.DoubleWellChain_WCAFluid(nchained=1).system.getForces()[1].getNumBonds() == 0
    assert set(system_to_desc(testsystems.DoubleWellChain_WCAFluid(nchained=1).system)['custom_terms']) == {'000'}


def test_custom_lennard_jones_fluid_mixture():
    t = testsystems.CustomLennardJonesFluidMixture()
    nb, c = t.system.getForces()
    assert _forces(t.system) == ['NonbondedForce', 'CustomNonbondedForce'] and t.system.getNumParticles() == 1000
    edge = (1000 / (0.05 / 0.34 ** 3)) ** (1.0 / 3.0)
    assert np.allclose(np.diag(t.system.getDefaultPeriodicBoxVectors()), edge, rtol=1e-15)
    assert c.getEnergyFunction() == MIXTURE and c.getCutoffDistance() == nb.getCutoffDistance() == pytest.approx(1.02, rel=1e-15)
    assert c.getUseLongRangeCorrection() and nb.getUseDispersionCorrection() and not c.getUseSwitchingFunction()
    assert [c.getPerParticleParameterName(k) for k in range(3)] == ['charge', 'sigma', 'epsilon']
    assert c.getParticleParameters(499) == pytest.approx([0.0, 0.34, 0.238 * 4.184]) and c.getParticleParameters(500) == pytest.approx([0.0, 0.34, 0.0])
    assert nb.getParticleParameters(499) == pytest.approx((0.0, 0.34, 0.0)) and nb.getParticleParameters(500) == pytest.approx((0.0, 0.34, 0.238 * 4.184))
    s = testsystems.CustomLennardJonesFluidMixture(nparticles=100, switch_width=0.2, dispersion_correction=False)
    nb, c = s.system.getForces()
    assert c.getUseSwitchingFunction() and c.getSwitchingDistance() == pytest.approx(0.82) and not c.getUseLongRangeCorrection()
    d = system_to_desc(t.system)
    assert d['nb_method'] == 1 and d['custom_terms']['000']['long_range_correction'] == 1
    # every pair of the custom force interacts with the string's own sigma and epsilon: two classes, one integral
    got = cx.long_range_coefficients([d['custom_terms']['000']], np.zeros((1, 0)))[0, 0]
    assert got == pytest.approx(8.0 * math.pi * 1e6 * 0.995792 * (0.34 ** 12 / (9.0 * 1.02 ** 9) - 0.34 ** 6 / (3.0 * 1.02 ** 3)), rel=1e-9)
