"""GPU: CustomManyParticleForce (openmmtools_amd/custom_expr.py kind 11, csrc/custom_manyparticle.hip, include/remd_hip_custom.h) against
the independent f64 helper tests/custom_manyparticle_oracle.py, which goes over all N^3 ordered candidates.

Bounds, derived from the formats (DESIGN sections 12, 16, 23 and 24): the energy within 1e-11 sum|E_set| (an f64 sum of f64 set energies);
the force on an atom, per component, within n (2^-23 max|contribution| + 2^-31) with n the atom's contributions (one per set and named
particle slot: each is rounded to f32 once, then added in fixed point); the u_kl rows within the bound of tests/test_custom_nonbonded_gpu.py
(rtol 1e-5, atol 1e-5 max|want|).  Positions are rounded to f32 before they go to either side, and every test with a cutoff asserts on the
CPU that no non-excluded pair's distance lies within 1e-6 nm of the cutoff, so that both sides sum the same sets."""
import copy
import math

import numpy as np
import pytest

import custom_manyparticle_oracle as oracle
import tabulated_oracle
import tabulated2d_oracle
from openmmtools_amd import custom_expr as cx, states, testsystems, unit
from openmmtools_amd.system import (System, system_to_desc, CustomManyParticleForce, CustomBondForce, CustomNonbondedForce, CustomHbondForce,
                                    Continuous1DFunction, Discrete2DFunction)

pytestmark = pytest.mark.gpu

KB = 0.008314462618153242
BETA = 1.0 / (KB * 300.0)
SP, UCP = CustomManyParticleForce.SinglePermutation, CustomManyParticleForce.UniqueCentralParticle
# Stillinger-Weber's three-body form around the central particle p1, without its cutoff factor
THREE_BODY = 'eps*exp(-3*(distance(p1,p2)+distance(p1,p3)))*(cos(angle(p2,p1,p3))+1/3)^2'
# the same with Stillinger-Weber's cutoff factors: it vanishes with all its derivatives where a neighbour reaches rc (a minimiser then has
# no discontinuity to settle on)
SMOOTH = 'eps*exp(g/(distance(p1,p2)-rc))*exp(g/(distance(p1,p3)-rc))*(cos(angle(p2,p1,p3))+1/3)^2; g=0.4; rc=0.6'
AXILROD_TELLER = 'c1*c2*c3*(1+3*cos(angle(p2,p1,p3))*cos(angle(p1,p2,p3))*cos(angle(p1,p3,p2)))/(distance(p1,p2)*distance(p2,p3)*distance(p1,p3))^3'
_CACHE = {}


def _f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def _system(n, forces, box=None):
    s = System()
    for _ in range(n):
        s.addParticle(12.0)
    if box is not None:
        s.setDefaultPeriodicBoxVectors([box[0], 0, 0], [0, box[1], 0], [0, 0, box[2]])
    for f in forces:
        s.addForce(f)
    return s


def _setup(engine, system, xs, boxes=None, global_table=None, labels=None):
    desc = system_to_desc(system, box=None if boxes is None else boxes[0])
    engine.set_system(desc)
    custom = desc.get('custom_terms')
    K = 1 if global_table is None else len(global_table)
    engine.set_states(np.full(K, BETA))
    if custom:
        engine.set_custom_globals(np.tile(custom['000']['global_defaults'], (K, 1)) if global_table is None else global_table)
    R = len(xs)
    engine.set_replicas(R, 0, xs, None, np.zeros((R, 3)) if boxes is None else boxes, np.zeros(R, dtype=np.int64) if labels is None else labels)
    return desc


def _device(engine, system, xs, boxes=None, global_table=None, labels=None):
    """forces [R][N][3], potentials [R], per-force energies [R][n]"""
    _setup(engine, system, xs, boxes, global_table, labels)
    f = engine.get_forces()
    u = engine.get_replicas(positions=False, velocities=False, potential=True)[2]
    return f, u, engine.custom_energies()


def _reference(force, x, box=None, global_values=None, functions=None):
    g = {force.getGlobalParameterName(i): force.getGlobalParameterDefaultValue(i) for i in range(force.getNumGlobalParameters())}
    g.update(global_values or {})
    rows = [force.getParticleParameters(k) for k in range(force.getNumParticles())]
    ref = oracle.evaluate(force.getEnergyFunction(), [force.getPerParticleParameterName(k) for k in range(force.getNumPerParticleParameters())],
                          [r[0] for r in rows], [r[1] for r in rows], [force.getTypeFilter(s) for s in range(3)], g, x, box,
                          force.getNonbondedMethod(), force.getCutoffDistance(),
                          [force.getExclusionParticles(k) for k in range(force.getNumExclusions())], force.getPermutationMode(), functions)
    if force.getNonbondedMethod():                  # the membership condition: a condition on the inputs, not a tolerance
        assert oracle.clear_of_cutoff(ref, force.getCutoffDistance(), 1e-6)
    return ref


def _assert_matches(tag, f, e, ref):
    worst = np.abs(f - ref['F']) / oracle.force_bound(ref).clip(min=1e-300)
    print('%s: %d sets, |dE| / (1e-11 sum|E|) = %.3g, worst |dF| / bound = %.3g, max|F| = %.3g' % (
        tag, len(ref['E']), abs(e - ref['E'].sum()) / max(oracle.energy_bound(ref), 1e-300), worst.max(), np.abs(ref['F']).max()))
    assert abs(e - ref['E'].sum()) <= oracle.energy_bound(ref)
    assert np.all(np.abs(f - ref['F']) <= oracle.force_bound(ref))


def _force(energy, n, mode, params=(), values=None, types=None, method=0, cutoff=1.0):
    f = CustomManyParticleForce(3, energy)
    for name in params:
        f.addPerParticleParameter(name)
    for k in range(n):
        f.addParticle([] if values is None else values[k], 0 if types is None else int(types[k]))
    f.setPermutationMode(mode)
    f.setNonbondedMethod(method)
    f.setCutoffDistance(cutoff)
    return f


# ---- 1. three particles, one set -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', [SP, UCP])
def test_three_particles_with_distance_and_angle(hip_engine_factory, mode):
    f = _force('k*(distance(p1,p2)-0.3)^2 + cos(angle(p2,p1,p3)) + 0.4*distance(p1,p3)', 3, mode)
    f.addGlobalParameter('k', 40.0)
    rng = np.random.default_rng(1101)
    base = np.array([[0.0, 0.0, 0.0], [0.31, 0.02, 0.0], [-0.1, 0.27, 0.05]])
    xs = _f32([base + rng.normal(0.0, 0.01, base.shape) for _ in range(3)])
    fd, u, e = _device(hip_engine_factory(), _system(3, [f]), xs)
    for r in range(3):
        ref = _reference(f, xs[r])
        assert len(ref['E']) == (1 if mode == SP else 3)
        _assert_matches('replica %d' % r, fd[r], e[r, 0], ref)
        assert u[r] == e[r, 0]


# ---- 2. NoCutoff, 13 particles: 66 pairs per central particle, one full batch and a rest of 2 ---------------------------------------------------
def _case2(mode):
    if ('case2', mode) not in _CACHE:
        rng = np.random.default_rng(1102)
        f = _force(AXILROD_TELLER, 13, mode, ['c'], rng.uniform(0.05, 0.1, (13, 1)))
        grid = np.array([[a, b, c] for a in range(3) for b in range(3) for c in range(2)], dtype=np.float64)[:13] * 0.35
        xs = _f32([grid + rng.uniform(-0.05, 0.05, grid.shape) for _ in range(2)])
        _CACHE[('case2', mode)] = (f, xs, [_reference(f, x) for x in xs])
    return _CACHE[('case2', mode)]


@pytest.mark.parametrize('mode', [SP, UCP])
def test_nocutoff_13_particles_a_full_batch_and_a_rest_of_two(hip_engine_factory, mode):
    force, xs, refs = _case2(mode)
    fd, u, e = _device(hip_engine_factory(), _system(13, [force]), xs)
    for r, ref in enumerate(refs):
        assert len(ref['E']) == (286 if mode == SP else 3 * 286)
        if mode == UCP:
            assert np.all(np.bincount(ref['sets'][:, 0], minlength=13) == 66)
        _assert_matches('replica %d' % r, fd[r], e[r, 0], ref)


# ---- 11a. bit-reproducibility -------------------------------------------------------------------------------------------------------------------
def test_two_evaluations_are_bitwise_equal(hip_engine_factory):
    force, xs, _ = _case2(UCP)
    a = _device(hip_engine_factory(), _system(13, [force]), xs)
    b = _device(hip_engine_factory(), _system(13, [force]), xs)
    for p, q in zip(a, b):
        assert np.array_equal(p, q)


# ---- 3. CutoffNonPeriodic, 70 particles: two blocks of central particles, two column blocks --------------------------------------------------------
def _case3_positions(rng):
    """66 particles scattered in a cube of 1.6 nm; a line of three far from them -- particle 0 in the middle, 65 and 69 at +-0.4 nm, 0.8 nm
    from one another (cutoff 0.5) -- and particle 64 alone"""
    x = rng.uniform(0.0, 1.6, (70, 3))
    x[0] = [5.0, 0.0, 0.0]; x[65] = [5.4, 0.01, 0.0]; x[69] = [4.6, 0.0, 0.02]
    x[64] = [0.0, 7.0, 0.0]
    return x


@pytest.mark.parametrize('mode', [SP, UCP])
def test_cutoff_nonperiodic_70_particles_sparse_rows_and_a_set_of_one_mode_only(hip_engine_factory, mode):
    rng = np.random.default_rng(1103)
    f = _force(THREE_BODY, 70, mode, method=1, cutoff=0.5)
    f.addGlobalParameter('eps', 30.0)
    xs = _f32([_case3_positions(rng) for _ in range(2)])
    refs = [_reference(f, x) for x in xs]
    for x, ref in zip(xs, refs):                                          # asserted on the CPU before the device is asked
        r = oracle.distances(x)
        near = (r < 0.5) & ~np.eye(70, dtype=bool)
        assert near[0].sum() == 2 and near[65].sum() == 1 and near[64].sum() == 0 and not near[65, 69]
        assert near.sum(axis=1).max() < 128
        line = [s for s in ref['sets'].tolist() if set(s) == {0, 65, 69}]
        assert line == ([] if mode == SP else [[0, 65, 69]])             # i-j and i-k inside, j-k outside: UniqueCentralParticle only
        assert len(ref['E']) > 100
    fd, u, e = _device(hip_engine_factory(), _system(70, [f]), xs)
    for r, ref in enumerate(refs):
        _assert_matches('replica %d' % r, fd[r], e[r, 0], ref)
        assert np.all(fd[r][64] == 0.0)


# ---- 4. a full row, and one neighbour too many --------------------------------------------------------------------------------------------------
def test_a_row_of_exactly_128_is_correct_and_129_gives_nan_for_that_replica_only(hip_engine_factory):
    """particle 70 (type 1, the only admitted central particle) with particles 0 ... 69 and 71 ... 128 on a sphere of 0.45 nm around it
    (cutoff 0.5): 128 neighbours, C(128, 2) sets.  Particle 129 sits 0.7 nm away (outside) or 0.3 nm away (the 129th neighbour);
    particle 130 is far from everything."""
    rng = np.random.default_rng(1104)
    N = 131
    types = np.zeros(N, dtype=int); types[70] = 1
    f = _force('0.01*distance(p1,p2)*distance(p1,p3)*(1+cos(angle(p2,p1,p3)))', N, UCP, types=types, method=1, cutoff=0.5)
    f.setTypeFilter(0, [1])
    u = rng.normal(size=(N, 3))
    x = 0.45 * u / np.linalg.norm(u, axis=1, keepdims=True) + [2.0, 2.0, 2.0]
    x[70] = [2.0, 2.0, 2.0]
    x[130] = [9.0, 9.0, 9.0]
    full, over = x.copy(), x.copy()
    full[129] = [2.7, 2.0, 2.0]
    over[129] = [2.3, 2.0, 2.0]
    full, over = _f32(full), _f32(over)
    ref = _reference(f, full)
    assert len(ref['E']) == 128 * 127 // 2 and np.all(ref['sets'][:, 0] == 70)
    assert ((oracle.distances(over)[70] < 0.5).sum() - 1) == 129
    eng = hip_engine_factory()
    fd, _, e = _device(eng, _system(N, [f]), np.array([full]))
    _assert_matches('128 neighbours', fd[0], e[0, 0], ref)
    eng.set_replicas(2, 0, np.array([over, full]), None, np.zeros((2, 3)), np.zeros(2, dtype=np.int64))
    fd, e = eng.get_forces(), eng.custom_energies()
    assert np.isnan(e[0, 0]) and np.all(fd[0] == 0.0)                     # the row overflowed: NaN, nothing evaluated
    _assert_matches('beside the overflowing replica', fd[1], e[1, 0], ref)
    eng.set_replicas(2, 0, np.array([full, full]), None, np.zeros((2, 3)), np.zeros(2, dtype=np.int64))
    fd, e = eng.get_forces(), eng.custom_energies()
    for r in range(2):
        _assert_matches('after the overflow, replica %d' % r, fd[r], e[r, 0], ref)


# ---- 5. CutoffPeriodic in boxes barely above twice the cutoff -----------------------------------------------------------------------------------------
def _case5(mode, energy=THREE_BODY):
    """30 particles in boxes of about 1.25 ... 1.4 nm, cutoff 0.6: particle 0 in a corner with neighbours 1, 2, 3 through an x face, a y face
    and the opposite corner"""
    f = _force(energy, 30, mode, method=2, cutoff=0.6)
    f.addGlobalParameter('eps', 30.0)
    boxes = _f32([[1.25, 1.3, 1.35], [1.3, 1.25, 1.4]])
    rng = np.random.default_rng(1105)
    xs = []
    for L in boxes:
        x = rng.uniform(0.0, 1.0, (30, 3)) * L
        x[0] = [0.05, 0.06, 0.04]
        x[1] = [L[0] - 0.2, 0.1, 0.1]
        x[2] = [0.1, L[1] - 0.25, 0.05]
        x[3] = [L[0] - 0.1, L[1] - 0.12, L[2] - 0.15]
        xs.append(x)
    return f, _f32(xs), boxes


@pytest.mark.parametrize('mode', [SP, UCP])
def test_cutoff_periodic_sets_through_faces_and_a_corner_in_two_boxes(hip_engine_factory, mode):
    force, xs, boxes = _case5(mode)
    fd, u, e = _device(hip_engine_factory(), _system(30, [force], boxes[0]), xs, boxes)
    for r in range(2):
        ref = _reference(force, xs[r], boxes[r])
        sets = {frozenset(s) for s in ref['sets'].tolist()}
        assert any({0, 1, 3} <= s or {0, 2, 3} <= s or {0, 1, 2} <= s for s in sets)
        raw = oracle.distances(xs[r])
        assert raw[0, 1] > 0.6 and raw[0, 2] > 0.6 and raw[0, 3] > 1.5    # in range through the boundary only
        assert any(0 in s and 3 in s for s in sets)                      # a set through the corner
        assert len(ref['E']) > 50
        _assert_matches('replica %d' % r, fd[r], e[r, 0], ref)


# ---- 6. exclusions ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', [SP, UCP])
def test_exclusions_of_a_central_pair_of_two_neighbours_and_of_a_whole_particle(hip_engine_factory, mode):
    rng = np.random.default_rng(1106)
    f = _force(AXILROD_TELLER, 12, mode, ['c'], rng.uniform(0.05, 0.1, (12, 1)))
    f.addExclusion(0, 1)
    f.addExclusion(7, 3)
    for j in range(12):
        if j != 5:
            f.addExclusion(5, j)
    grid = np.array([[a, b, c] for a in range(3) for b in range(2) for c in range(2)], dtype=np.float64) * 0.4
    xs = _f32([grid + rng.uniform(-0.05, 0.05, grid.shape) for _ in range(2)])
    fd, u, e = _device(hip_engine_factory(), _system(12, [f]), xs)
    for r in range(2):
        ref = _reference(f, xs[r])
        n_sets = 165 - 2 * 9 + 0                                          # C(11, 3) without particle 5, less the sets that hold {0, 1} or {3, 7}
        assert len(ref['E']) == (n_sets if mode == SP else 3 * n_sets)
        assert ref['count'][5] == 0 and np.all(fd[r][5] == 0.0)
        _assert_matches('replica %d' % r, fd[r], e[r, 0], ref)


# ---- 7. types and filters ---------------------------------------------------------------------------------------------------------------------------
ASYMMETRIC = 'exp(-2*distance(p1,p2)-0.5*distance(p1,p3))*(1.2+cos(angle(p2,p1,p3)))+0.1*distance(p2,p3)'


def test_a_water_like_filter_of_one_oxygen_and_two_hydrogens(hip_engine_factory):
    types = np.tile([0, 1, 1], 4)
    f = _force(THREE_BODY, 12, UCP, types=types)
    f.addGlobalParameter('eps', 30.0)
    f.setTypeFilter(0, [0]); f.setTypeFilter(1, [1]); f.setTypeFilter(2, [1])
    rng = np.random.default_rng(1107)
    xs = _f32(rng.uniform(0.0, 1.0, (2, 12, 3)))
    fd, u, e = _device(hip_engine_factory(), _system(12, [f]), xs)
    for r in range(2):
        ref = _reference(f, xs[r])
        assert len(ref['E']) == 4 * 28 and np.all(types[ref['sets'][:, 0]] == 0) and np.all(types[ref['sets'][:, 1:]] == 1)
        _assert_matches('replica %d' % r, fd[r], e[r, 0], ref)


def test_a_filter_that_forces_the_second_assignment(hip_engine_factory):
    """UniqueCentralParticle, slot 2 takes type 1 and slot 3 type 2: where the lower neighbour has type 2 only (p1, k, j) passes"""
    types = np.array([0, 2, 1, 2, 1, 1, 2, 0, 1, 2])
    f = _force(ASYMMETRIC, 10, UCP, types=types)
    f.setTypeFilter(1, [1]); f.setTypeFilter(2, [2])
    rng = np.random.default_rng(1108)
    xs = _f32(rng.uniform(0.0, 1.0, (2, 10, 3)))
    fd, u, e = _device(hip_engine_factory(), _system(10, [f]), xs)
    for r in range(2):
        ref = _reference(f, xs[r])
        s = ref['sets']
        assert (s[:, 1] > s[:, 2]).sum() > 10 and (s[:, 1] < s[:, 2]).sum() > 10      # both assignments occur
        _assert_matches('replica %d' % r, fd[r], e[r, 0], ref)


def test_single_permutation_where_only_the_fourth_of_six_assignments_passes(hip_engine_factory):
    """types 0 0 0 1 1 1 2 2 2 by index and the filters (1, 2, 0): a set with one particle of each type i < j < k passes as (j, k, i) alone,
    the fourth of (i,j,k) (i,k,j) (j,i,k) (j,k,i) (k,i,j) (k,j,i)"""
    types = np.repeat([0, 1, 2], 3)
    f = _force(ASYMMETRIC, 9, SP, types=types)
    f.setTypeFilter(0, [1]); f.setTypeFilter(1, [2]); f.setTypeFilter(2, [0])
    rng = np.random.default_rng(1109)
    xs = _f32(rng.uniform(0.0, 1.0, (2, 9, 3)))
    fd, u, e = _device(hip_engine_factory(), _system(9, [f]), xs)
    for r in range(2):
        ref = _reference(f, xs[r])
        s = ref['sets']
        assert len(s) == 27 and np.all(s[:, 2] < s[:, 0]) and np.all(s[:, 0] < s[:, 1])
        _assert_matches('replica %d' % r, fd[r], e[r, 0], ref)


# ---- 8. five parameters per particle, a global, u_kl ---------------------------------------------------------------------------------------------------
LAMBDAS = np.array([[1.0], [0.5], [0.0]])


def test_five_parameters_and_the_ukl_rows_of_a_global(hip_engine_factory):
    names = ['a', 'b', 'c', 'd', 'e']
    rng = np.random.default_rng(1110)
    f = _force('(0.2+lam)*(a1+b2+c3+d1*e2)*exp(-distance(p1,p2)*(a2+b3+c1))*(1+e3*cos(angle(p2,p1,p3))+d2*d3)', 10, SP, names, rng.uniform(0.1, 1.0, (10, 5)))
    f.addGlobalParameter('lam', 1.0)
    system = _system(10, [f])
    x = rng.uniform(0.0, 1.0, (10, 3))
    xs = _f32([x, x, x])                                                  # one geometry at every state: custom_energies() gives E(g_l)
    LamState = type('LamState', (states.GlobalParameterState,), {'lam': states.GlobalParameterState.GlobalParameter('lam', standard_value=1.0)})
    sts = [states.CompoundThermodynamicState(states.ThermodynamicState(system, 300.0 * unit.kelvin), [LamState(lam=float(v))]) for v in LAMBDAS[:, 0]]
    table = cx.custom_globals(system, ['lam'], sts)
    assert np.array_equal(table, LAMBDAS)
    eng = hip_engine_factory()
    labels = np.array([0, 1, 2])
    _setup(eng, system, xs, None, table, labels)
    u = eng.compute_energies()
    per_state = eng.custom_energies()[:, 0]                               # replica l sits at state l
    fd = eng.get_forces()
    want = np.zeros((3, 3))
    for l in range(3):
        ref = _reference(f, xs[0], None, {'lam': LAMBDAS[l, 0]})
        assert len(ref['E']) == 120
        want[:, l] = BETA * ref['E'].sum()
        _assert_matches('state %d' % l, fd[l], per_state[l], ref)
    print('u_kl: max |got - want| / max|want| = %.3g' % (np.abs(u - want).max() / np.abs(want).max()))
    assert np.allclose(u, want, rtol=1e-5, atol=1e-5 * np.abs(want).max())
    assert np.allclose(u[np.arange(3), labels], BETA * per_state, rtol=1e-14, atol=0.0)   # (the own column is beta U)


# ---- 9. tabulated functions -------------------------------------------------------------------------------------------------------------------------
def test_a_periodic_spline_of_an_angle_and_a_lookup_of_two_types(hip_engine_factory):
    phi = np.linspace(-math.pi, math.pi, 25)
    values = 1.0 + 0.6 * np.cos(2.0 * phi) + 0.3 * np.sin(phi)
    values[-1] = values[0]
    scale = np.array([1.0, 0.5, 2.0, 0.5, 0.25, 1.5])                     # [3 types of p1][2 types of p2], p1's fastest
    rng = np.random.default_rng(1111)
    f = _force('tab(angle(p2,p1,p3))*scale(t1,u2)*exp(-distance(p1,p3))', 9, UCP, ['t', 'u'], [[k % 3, k % 2] for k in range(9)])
    f.addTabulatedFunction('tab', Continuous1DFunction(values, -math.pi, math.pi, True))
    f.addTabulatedFunction('scale', Discrete2DFunction(3, 2, scale))
    xs = _f32(rng.uniform(0.0, 1.0, (2, 9, 3)))
    functions = dict(tab=tabulated_oracle.Spline(values, -math.pi, math.pi, True), scale=tabulated2d_oracle.Lookup2D(3, 2, scale))
    fd, u, e = _device(hip_engine_factory(), _system(9, [f]), xs)
    for r in range(2):
        ref = _reference(f, xs[r], functions=functions)
        assert len(ref['E']) == 9 * 28
        _assert_matches('replica %d' % r, fd[r], e[r, 0], ref)


# ---- 10. beside a CustomBondForce, a CustomNonbondedForce and a CustomHbondForce ------------------------------------------------------------------------
def test_coexistence_leaves_the_other_custom_forces_bitwise_unchanged(hip_engine_factory):
    rng = np.random.default_rng(1112)
    N = 40
    bond = CustomBondForce('0.5*kb*(r-b0)^2')
    bond.addPerBondParameter('kb'); bond.addPerBondParameter('b0')
    for k in range(0, 20, 2):
        bond.addBond(k, k + 1, [300.0, 0.12])
    nb = CustomNonbondedForce('4*e*((s/r)^12-(s/r)^6); s=0.2; e=0.3')
    for _ in range(N):
        nb.addParticle([])
    for k in range(0, 20, 2):
        nb.addExclusion(k, k + 1)
    hb = CustomHbondForce('k*(distance(d1,a1)-r0)^2*(1+cos(angle(d2,d1,a1)))^2*step(0.6-distance(d1,a1))')
    hb.addPerDonorParameter('k'); hb.addPerAcceptorParameter('r0')
    for k in range(0, 20, 2):
        hb.addDonor(k, k + 1, -1, [rng.uniform(20.0, 40.0)])
    for k in range(20, N):
        hb.addAcceptor(k, -1, -1, [rng.uniform(0.2, 0.3)])
    mp = _force(THREE_BODY, N, UCP, method=1, cutoff=0.55)
    mp.addGlobalParameter('eps', 30.0)
    for k in range(0, 20, 2):
        mp.addExclusion(k, k + 1)
    for f in (bond, nb, hb, mp):
        f.setForceGroup(3)
    grid = np.array([[a, b, c] for a in range(4) for b in range(4) for c in range(3)], dtype=np.float64)[:N] * 0.3
    x = grid + rng.uniform(-0.03, 0.03, grid.shape)
    x[1:20:2] = x[0:20:2] + [0.11, 0.02, 0.0]
    xs = _f32([x, x + rng.normal(0.0, 0.005, x.shape)])
    f_all, u_all, e_all = _device(hip_engine_factory(), _system(N, [bond, mp, nb, hb]), xs)
    f_old, u_old, e_old = _device(hip_engine_factory(), _system(N, [bond, nb, hb]), xs)
    eng = hip_engine_factory()
    f_mp, u_mp, e_mp = _device(eng, _system(N, [copy.deepcopy(mp)]), xs)
    assert np.array_equal(eng.get_forces(groups=1 << 3), f_mp) and np.all(eng.get_forces(groups=1 << 2) == 0.0)
    assert e_all.shape == (2, 4) and np.abs(e_all[:, 1]).min() > 0.0
    assert np.array_equal(e_all[:, [0, 2, 3]], e_old)                     # the other forces' energies, bit for bit
    assert np.array_equal(e_all[:, 1], e_mp[:, 0])
    assert np.array_equal(f_all, f_old + f_mp)                            # fixed-point sums: the others' forces are unchanged to the bit
    for r in range(2):
        ref = _reference(mp, xs[r])
        assert abs(e_all[r, 1] - ref['E'].sum()) <= oracle.energy_bound(ref)
        assert np.all(np.abs(f_all[r] - f_old[r] - ref['F']) <= oracle.force_bound(ref))


# ---- 11b. phased propagation ------------------------------------------------------------------------------------------------------------------------
def test_phased_propagation_with_a_many_particle_force_is_the_one_block_run(hip_engine_factory):
    """AlanineDipeptideExplicit with a three-body term among every seventh atom (type 1, all three filters; cutoff 0.45 nm, so that a row
    of 128 holds every atom in range), a global that differs between the states, 6 replicas: two blocks equal one block bit for bit"""
    al = testsystems.AlanineDipeptideExplicit()
    N = al.system.getNumParticles()
    f = _force('scale*' + THREE_BODY, N, UCP, types=[1 if i % 7 == 0 else 0 for i in range(N)], method=2, cutoff=0.45)
    f.addGlobalParameter('scale', 1.0)
    f.addGlobalParameter('eps', 30.0)
    for s in range(3):
        f.setTypeFilter(s, [1])
    al.system.addForce(f)
    desc = system_to_desc(al.system, ewald_split='auto')
    box = np.diag(al.system.getDefaultPeriodicBoxVectors())
    R = 6
    table = np.column_stack([np.linspace(1.0, 0.5, R), np.full(R, 30.0)])
    out = []
    for phases in (1, 2):
        eng = hip_engine_factory()
        eng.set_phases(phases)
        eng.set_system(desc)
        eng.set_states(1.0 / (KB * np.linspace(300.0, 320.0, R)))
        eng.set_custom_globals(table)
        eng.set_integrator('V R R O R R V', 0.002, 1.0, 20, True, 1e-8)
        eng.seed(9)
        eng.set_replicas(R, 0, np.tile(al.positions, (R, 1, 1)), None, np.tile(box, (R, 1)), np.arange(R))
        for it in range(2):
            assert not eng.propagate(it).any()
            u = eng.compute_energies()
        x, v = eng.get_replicas()[:2]
        out.append((x.copy(), v.copy(), u.copy(), eng.custom_energies(), eng.phases_active()))
    (xa, va, ua, ea, pa), (xb, vb, ub, eb, pb) = out
    assert (pa, pb) == (1, 2)
    assert np.all(np.isfinite(ea)) and np.all(ea != 0.0) and np.any(ua != ua[:, :1])
    assert np.array_equal(xa, xb) and np.array_equal(va, vb) and np.array_equal(ua, ub) and np.array_equal(ea, eb)


# ---- 12. dynamics, minimisation, the barostat -----------------------------------------------------------------------------------------------------------
def test_md_steps_minimisation_and_barostat_trials_on_the_periodic_case(hip_engine_factory):
    force, xs, boxes = _case5(UCP, SMOOTH)
    system = _system(30, [force], boxes[0])
    eng = hip_engine_factory()
    _setup(eng, system, xs, boxes)
    eng.set_integrator('V R O R V', 0.001, 1.0, 5, True, 1e-8)
    eng.seed(12)
    u0 = eng.compute_energies(want_potential=True)[1]
    assert not eng.propagate(0).any()
    x1 = eng.get_replicas()[0]
    u1 = eng.compute_energies(want_potential=True)[1]
    assert np.abs(x1 - xs).max() > 1e-4
    for r in range(2):                                                    # the potential the steps left is the oracle's at the positions they left
        ref = _reference(force, _f32(x1[r]), boxes[r])
        assert abs(u1[r] - ref['E'].sum()) <= oracle.energy_bound(ref)
    converged, n_fire = eng.minimize(1.0, 100)
    u2 = eng.compute_energies(want_potential=True)[1]
    print('potential: start %s, after 5 BAOAB steps %s, after %d FIRE steps %s' % (u0, u1, n_fire, u2))
    assert n_fire > 0 and np.all(u2 < u1)
    # isotropic barostat trials: after every attempt the potential is the oracle's at the replica's positions and box, and no box
    # edge has fallen below twice the cutoff
    eng.set_barostat(np.full(1, 500.0 * unit.bar), 25)
    box_before = eng.get_boxes().copy()
    moved = 0
    for attempt in range(4):
        eng.barostat_attempts(1)
        box_now = eng.get_boxes()
        x, _, pot, _ = eng.get_replicas(potential=True)
        for r in range(2):
            ref = _reference(force, _f32(x[r]), _f32(box_now[r]))
            assert abs(pot[r] - ref['E'].sum()) <= oracle.energy_bound(ref), (attempt, r, pot[r], ref['E'].sum())
        moved += int(np.any(box_now != box_before))
        box_before = box_now.copy()
    assert moved >= 1
    assert np.all(eng.get_boxes() >= 1.2)


def test_per_axis_barostat_trials_on_the_periodic_case(hip_engine_factory):
    """MonteCarloAnisotropicBarostat over x, y and z (one axis per trial): after every attempt the potential is the oracle's at the
    replica's positions and box, and the edges change one at a time"""
    force, xs, boxes = _case5(UCP, SMOOTH)
    eng = hip_engine_factory()
    _setup(eng, _system(30, [force], boxes[0]), xs, boxes)
    eng.set_barostat_axes(np.full(1, 500.0 * unit.bar), None, 1, 0b111, 0, 25)
    eng.seed(13)
    eng.compute_energies()
    box_before = eng.get_boxes().copy()
    moved = np.zeros(3, dtype=int)
    for attempt in range(6):
        eng.barostat_attempts(1)
        box_now = eng.get_boxes()
        x, _, pot, _ = eng.get_replicas(potential=True)
        for r in range(2):
            changed = box_now[r] != box_before[r]
            assert changed.sum() <= 1                                     # a per-axis trial scales one edge
            moved += changed
            ref = _reference(force, _f32(x[r]), _f32(box_now[r]))
            assert abs(pot[r] - ref['E'].sum()) <= oracle.energy_bound(ref), (attempt, r, pot[r], ref['E'].sum())
        box_before = box_now.copy()
    print('per-axis barostat: accepted moves per axis %s' % moved)
    assert moved.sum() >= 1
    assert np.all(eng.get_boxes() >= 1.2)


@pytest.mark.parametrize('per_axis', [False, True])
def test_a_barostat_trial_below_twice_the_cutoff_is_refused_as_for_the_nonbonded_kind(hip_engine_factory, per_axis):
    """a weak force (eps = 0.01) under 20 000 bar, so that Metropolis accepts every compression.  With room (edges of 1.4 nm, cutoff 0.6)
    the boxes shrink and nothing is refused; a replica whose x edge starts 0.0005 nm above twice the cutoff makes the engine refuse the
    trial that would take it below, with the sentence of the built-in cutoff (the force's cutoff is this handle's only one)"""
    force = _force(SMOOTH, 30, UCP, method=2, cutoff=0.6)
    force.addGlobalParameter('eps', 0.01)
    rng = np.random.default_rng(1113)
    pressure = np.full(1, 20000.0 * unit.bar)

    def handle(boxes):
        xs = _f32([rng.uniform(0.0, 1.0, (30, 3)) * L for L in boxes])
        eng = hip_engine_factory()
        _setup(eng, _system(30, [force], boxes[0]), xs, boxes)
        if per_axis:
            eng.set_barostat_axes(pressure, None, 1, 0b111, 0, 25)
        else:
            eng.set_barostat(pressure, 25)
        eng.seed(14)
        eng.compute_energies()
        return eng
    roomy = _f32([[1.4, 1.4, 1.4], [1.45, 1.4, 1.5]])
    eng = handle(roomy)
    eng.barostat_attempts(12)
    box = eng.get_boxes()
    print('with room (%s): boxes %s -> %s' % ('per axis' if per_axis else 'isotropic', roomy.tolist(), box.tolist()))
    assert np.all(np.prod(box, axis=1) < 0.99 * np.prod(roomy, axis=1)) and np.all(box >= np.float32(1.2))
    assert np.all(np.isfinite(eng.get_replicas(potential=True)[2]))
    eng = handle(_f32([[1.2005, 1.3, 1.35], [1.4, 1.4, 1.4]]))
    with pytest.raises(RuntimeError, match='proposed a periodic box smaller than twice the nonbonded cutoff'):
        eng.barostat_attempts(40)


def test_twenty_steps_of_the_64_particle_stillinger_weber_fluid(hip_engine_factory):
    ts = testsystems.StillingerWeberFluid(nparticles=64)
    box = np.diag(ts.system.getDefaultPeriodicBoxVectors())
    eng = hip_engine_factory()
    xs = _f32([ts.positions, ts.positions])
    _setup(eng, ts.system, xs, _f32([box, box]))
    eng.set_integrator('V R O R V', 0.002, 1.0, 20, True, 1e-8)
    eng.seed(3)
    e0 = eng.custom_energies()
    assert not eng.propagate(0).any()
    x = eng.get_replicas()[0]
    e1 = eng.custom_energies()
    print('StillingerWeberFluid(64): two-body, three-body energies at the lattice %s, after 20 steps %s' % (e0[0], e1[0]))
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(e1)) and np.abs(x - xs).max() > 1e-4
    assert np.all(e0[:, 0] < 0.0) and np.all(e1[:, 1] >= 0.0)            # the pair term binds, the three-body term is a penalty
