"""GPU: CustomHbondForce (openmmtools_amd/custom_expr.py kind 10, csrc/custom_hbond.hip, include/remd_hip_custom.h) against the independent
f64 helper tests/custom_hbond_oracle.py.

Bounds, derived from the formats (DESIGN sections 12, 16 and 23): the energy within 1e-11 sum|E_pair| (an f64 sum of f64 pair energies);
the force on an atom, per component, within n (2^-23 max|contribution| + 2^-31) with n the atom's contributions (one per pair and named
particle slot: each is rounded to f32 once, then added in fixed point); the u_kl rows within the bound of tests/test_custom_nonbonded_gpu.py
(rtol 1e-5, atol 1e-5 max|want|).  Positions are rounded to f32 before they go to either side, and every test with a cutoff asserts on the
CPU that no non-excluded pair's d1-a1 distance lies within 1e-6 nm of the cutoff, so that both sides sum the same pairs."""
import copy
import math

import numpy as np
import pytest

import custom_hbond_oracle as oracle
import custom_dual_oracle as dual
import tabulated_oracle
import tabulated2d_oracle
from openmmtools_amd import custom_expr as cx, states, unit
from openmmtools_amd.system import (System, system_to_desc, CustomHbondForce, CustomBondForce, CustomNonbondedForce,
                                    Continuous1DFunction, Discrete2DFunction)

pytestmark = pytest.mark.gpu

KB = 0.008314462618153242
BETA = 1.0 / (KB * 300.0)
REFERENCE = 'k*(distance(d1,a1)-r0)^2*(1+cos(angle(d2,d1,a1)))^2*step(rc-distance(d1,a1)); rc=0.6'
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
    donors = [force.getDonorParameters(k) for k in range(force.getNumDonors())]
    acceptors = [force.getAcceptorParameters(k) for k in range(force.getNumAcceptors())]
    ref = oracle.evaluate(force.getEnergyFunction(), [force.getPerDonorParameterName(k) for k in range(force.getNumPerDonorParameters())],
                          [force.getPerAcceptorParameterName(k) for k in range(force.getNumPerAcceptorParameters())],
                          [d[:3] for d in donors], [a[:3] for a in acceptors], [d[3] for d in donors], [a[3] for a in acceptors], g, x, box,
                          force.getNonbondedMethod(), force.getCutoffDistance(),
                          [force.getExclusionParticles(k) for k in range(force.getNumExclusions())], functions)
    if force.getNonbondedMethod():                  # the membership condition: a condition on the inputs, not a tolerance
        assert oracle.clear_of_cutoff(ref, force.getCutoffDistance(), 1e-6)
    return ref


def _assert_matches(tag, f, e, ref):
    worst = np.abs(f - ref['F']) / oracle.force_bound(ref).clip(min=1e-300)
    print('%s: %d pairs, |dE| / (1e-11 sum|E|) = %.3g, worst |dF| / bound = %.3g, max|F| = %.3g' % (
        tag, len(ref['E']), abs(e - ref['E'].sum()) / max(oracle.energy_bound(ref), 1e-300), worst.max(), np.abs(ref['F']).max()))
    assert abs(e - ref['E'].sum()) <= oracle.energy_bound(ref)
    assert np.all(np.abs(f - ref['F']) <= oracle.force_bound(ref))


def _tile_counts(ref, nD, nA):
    """{(donor block, acceptor block): surviving pairs} over every tile"""
    counts = {(a, b): 0 for a in range((nD + 63) // 64) for b in range((nA + 63) // 64)}
    for i, j in zip(ref['i'].tolist(), ref['j'].tolist()):
        counts[(i // 64, j // 64)] += 1
    return counts


# ---- 1. one donor, one acceptor, three particles each: distance + angle + dihedral ------------------------------------------------------------
def test_one_pair_of_three_particle_groups_with_distance_angle_and_dihedral(hip_engine_factory):
    f = CustomHbondForce('k*(distance(d1,a1)-0.3)^2 + cos(angle(d2,d1,a1)) + 0.7*sin(dihedral(d3,d2,d1,a1)) + 0.5*cos(dihedral(d1,a1,a2,a3)) + 0.2*angle(a1,a2,a3)^2')
    f.addGlobalParameter('k', 40.0)
    f.addDonor(0, 1, 2)
    f.addAcceptor(3, 4, 5)
    rng = np.random.default_rng(901)
    base = np.array([[0.0, 0.0, 0.0], [-0.1, 0.02, 0.0], [-0.13, 0.11, 0.03], [0.29, 0.05, 0.02], [0.38, -0.04, 0.06], [0.41, -0.02, 0.17]])
    xs = _f32([base + rng.normal(0.0, 0.01, base.shape) for _ in range(3)])
    fd, u, e = _device(hip_engine_factory(), _system(6, [f]), xs)
    for r in range(3):
        ref = _reference(f, xs[r])
        assert len(ref['E']) == 1 and np.all(ref['count'] == 1)
        _assert_matches('replica %d' % r, fd[r], e[r, 0], ref)
        assert u[r] == e[r, 0]


# ---- 2. 70 donors x 130 acceptors without a cutoff: 2 x 3 tiles, overflowing queues, partial batches ------------------------------------------
def _case2():
    f = CustomHbondForce('eps*exp(-(distance(d1,a1)-r0)^2/0.08)*(1+cos(angle(d2,d1,a1)))')
    f.addPerDonorParameter('eps')
    f.addPerAcceptorParameter('r0')
    rng = np.random.default_rng(902)
    for k in range(70):
        f.addDonor(2 * k, 2 * k + 1, -1, [rng.uniform(0.5, 2.0)])
    for k in range(130):
        f.addAcceptor(140 + k, -1, -1, [rng.uniform(0.25, 0.4)])
    # no tile's pair count a multiple of 64: every tile ends on a partial batch
    for i, j in ((0, 0), (5, 70), (9, 128), (64, 3), (65, 66)):
        f.addExclusion(i, j)
    xs = []
    for _ in range(2):
        x = rng.uniform(0.0, 2.5, (270, 3))
        u = rng.normal(size=(70, 3))
        x[1:140:2] = x[0:140:2] + 0.1 * u / np.linalg.norm(u, axis=1, keepdims=True)
        xs.append(x)
    return f, _f32(xs)


def _case2_reference():
    if 'case2' not in _CACHE:
        f, xs = _case2()
        _CACHE['case2'] = (f, xs, [_reference(f, x) for x in xs])
    return _CACHE['case2']


def test_nocutoff_70_donors_by_130_acceptors_over_six_tiles(hip_engine_factory):
    force, xs, refs = _case2_reference()
    fd, u, e = _device(hip_engine_factory(), _system(270, [force]), xs)
    for r, ref in enumerate(refs):
        counts = _tile_counts(ref, 70, 130)
        assert len(counts) == 6 and sum(counts.values()) == 70 * 130 - 5
        assert all(n % 64 != 0 for n in counts.values())                 # every tile ends on a partial batch
        assert sum(n > 128 for n in counts.values()) >= 4                # and most flush a full queue several times first
        _assert_matches('replica %d' % r, fd[r], e[r, 0], ref)


# ---- 11. bit-reproducibility ------------------------------------------------------------------------------------------------------------------
def test_two_evaluations_are_bitwise_equal(hip_engine_factory):
    force, xs, _ = _case2_reference()
    a = _device(hip_engine_factory(), _system(270, [force]), xs)
    b = _device(hip_engine_factory(), _system(270, [force]), xs)
    for p, q in zip(a, b):
        assert np.array_equal(p, q)


# ---- 3. CutoffNonPeriodic: a tile of exactly 64 survivors, an empty tile, a tile of 65 ... 127 -------------------------------------------------
def test_cutoff_nonperiodic_tiles_of_exactly_64_of_none_and_of_94_survivors(hip_engine_factory):
    """64 donors in close pairs (0.4 nm apart, the pairs 1.5 nm apart), three blocks of 64 acceptors, cutoff 0.45 nm: acceptor k sits 0.3 nm
    beside donor k (0.5 nm from its partner: outside); the second block lies far away; of the third block 30 acceptors sit 0.1 nm from
    their donor and 0.41 nm from its partner (two survivors each), 34 sit 0.3 nm away (one each): 94"""
    f = CustomHbondForce(REFERENCE)
    f.addPerDonorParameter('k')
    f.addPerAcceptorParameter('r0')
    rng = np.random.default_rng(903)
    d1 = np.array([[1.5 * (k // 2) + 0.4 * (k % 2), 0.0, 0.0] for k in range(64)])
    acc = np.zeros((192, 3))
    acc[:64] = d1 + [0.0, 0.3, 0.0]
    acc[64:128] = d1 + [0.0, 50.0, 0.0]
    acc[128:158] = d1[:30] + [0.0, -0.1, 0.0]
    acc[158:192] = d1[30:] + [0.0, 0.0, 0.3]
    N = 64 * 2 + 192 * 2
    xs = []
    for _ in range(2):
        x = np.zeros((N, 3))
        x[0:128:2] = d1 + rng.uniform(-0.005, 0.005, d1.shape)
        x[1:128:2] = x[0:128:2] + [0.03, 0.0, -0.09]
        x[128::2] = acc + rng.uniform(-0.005, 0.005, acc.shape)
        x[129::2] = x[128::2] + [0.0, 0.08, 0.05]
        xs.append(x)
    xs = _f32(xs)
    for k in range(64):
        f.addDonor(2 * k, 2 * k + 1, -1, [rng.uniform(50.0, 100.0)])
    for k in range(192):
        f.addAcceptor(128 + 2 * k, 129 + 2 * k, -1, [rng.uniform(0.15, 0.25)])
    f.setNonbondedMethod(CustomHbondForce.CutoffNonPeriodic)
    f.setCutoffDistance(0.45)
    refs = [_reference(f, x) for x in xs]
    for ref in refs:                                                      # asserted on the CPU before the device is asked
        assert _tile_counts(ref, 64, 192) == {(0, 0): 64, (0, 1): 0, (0, 2): 94}
    fd, u, e = _device(hip_engine_factory(), _system(N, [f]), xs)
    for r, ref in enumerate(refs):
        _assert_matches('replica %d' % r, fd[r], e[r, 0], ref)
        assert np.all(fd[r][128 + 128:128 + 256] == 0.0)                  # (the far block feels nothing)


# ---- 4. CutoffPeriodic in a small box -------------------------------------------------------------------------------------------------------
PERIODIC = 'k*exp(-2*(distance(d1,a1)-0.3)^2)*cos(angle(d2,d1,a1))^2*(1+0.3*cos(dihedral(d3,d2,d1,a1)))'


def _case4():
    """20 donors of three particles (atoms 3 k ... 3 k + 2) and 20 one-particle acceptors (atoms 60 ...) in boxes of 3.0 and 3.3 nm, cutoff
    1 nm; donors 0 and 1 sit at the low x and y faces with d2 wrapped to the far side, acceptors 0 and 1 beyond the same faces"""
    f = CustomHbondForce(PERIODIC)
    f.addGlobalParameter('k', 8.0)
    for k in range(20):
        f.addDonor(3 * k, 3 * k + 1, 3 * k + 2)
    for k in range(20):
        f.addAcceptor(60 + k, -1, -1)
    f.setNonbondedMethod(CustomHbondForce.CutoffPeriodic)
    f.setCutoffDistance(1.0)
    boxes = _f32([[3.0, 3.1, 3.2], [3.3, 3.2, 3.1]])
    rng = np.random.default_rng(904)
    xs = []
    for L in boxes:
        x = np.zeros((80, 3))
        x[0:60:3] = rng.uniform(0.3, L - 0.3, (20, 3))
        x[60:] = rng.uniform(0.3, L - 0.3, (20, 3))
        x[0] = [0.04, 1.5, 1.5]; x[60] = [L[0] - 0.25, 1.55, 1.45]       # neighbours through the x face only
        x[3] = [1.5, 0.05, 1.0]; x[61] = [1.45, L[1] - 0.3, 1.05]        # and through the y face
        u = rng.normal(size=(20, 3))
        x[1:60:3] = x[0:60:3] + 0.1 * u / np.linalg.norm(u, axis=1, keepdims=True)
        x[1] = x[0] + [-0.1, 0.01, 0.0]; x[4] = x[3] + [0.0, -0.1, 0.02]
        w = rng.normal(size=(20, 3))
        x[2:60:3] = x[1:60:3] + 0.1 * w / np.linalg.norm(w, axis=1, keepdims=True)
        x[1, 0] += L[0]; x[4, 1] += L[1]                                   # d2 of donors 0 and 1 wrapped into the box: the molecule straddles the face
        xs.append(x)
    return f, _f32(xs), boxes


def test_cutoff_periodic_pairs_through_the_faces_and_a_straddling_donor(hip_engine_factory):
    force, xs, boxes = _case4()
    fd, u, e = _device(hip_engine_factory(), _system(80, [force], boxes[0]), xs, boxes)
    for r in range(2):
        ref = _reference(force, xs[r], boxes[r])
        pairs = set(zip(ref['i'].tolist(), ref['j'].tolist()))
        assert (0, 0) in pairs and (1, 1) in pairs                        # in range through the boundary only:
        assert np.linalg.norm(xs[r][60] - xs[r][0]) > 2.0 and np.linalg.norm(xs[r][61] - xs[r][3]) > 2.0
        assert np.linalg.norm(xs[r][1] - xs[r][0]) > 2.0                  # d1 - d2 is imaged
        assert 10 < len(ref['E']) < 400
        _assert_matches('replica %d' % r, fd[r], e[r, 0], ref)


# ---- 5. donors of one particle, acceptors of two ----------------------------------------------------------------------------------------------
def test_one_particle_donors_and_two_particle_acceptors(hip_engine_factory):
    f = CustomHbondForce('c*exp(-distance(d1,a1)/w)*(1.5+cos(angle(d1,a1,a2)))')
    f.addGlobalParameter('c', 3.0)
    f.addPerAcceptorParameter('w')
    rng = np.random.default_rng(905)
    for k in range(7):
        f.addDonor(k, -1, -1)
    for k in range(5):
        f.addAcceptor(7 + 2 * k, 8 + 2 * k, -1, [rng.uniform(0.2, 0.5)])
    assert cx.custom_terms_desc([f], np.ones(17))['000']['particle_mask'] == 0b011001
    xs = _f32(rng.uniform(0.0, 1.2, (3, 17, 3)))
    fd, u, e = _device(hip_engine_factory(), _system(17, [f]), xs)
    for r in range(3):
        ref = _reference(f, xs[r])
        assert len(ref['E']) == 35
        _assert_matches('replica %d' % r, fd[r], e[r, 0], ref)


# ---- 6. exclusions --------------------------------------------------------------------------------------------------------------------------
def test_exclusion_rows_across_column_blocks_and_an_acceptor_nobody_sees(hip_engine_factory):
    f = CustomHbondForce('q*exp(-distance(d1,a1)^2)')
    f.addPerDonorParameter('q')
    rng = np.random.default_rng(906)
    for k in range(10):
        f.addDonor(k, -1, -1, [rng.uniform(1.0, 2.0)])
    for k in range(130):
        f.addAcceptor(10 + k, -1, -1)
    f.addExclusion(0, 3); f.addExclusion(0, 70)                           # one donor, two column blocks
    for j in (1, 2, 64, 65, 128, 129):                                    # more than four, over all three blocks
        f.addExclusion(1, j)
    for i in range(10):                                                   # an acceptor excluded by every donor
        f.addExclusion(i, 5)
    xs = _f32(rng.uniform(0.0, 2.0, (2, 140, 3)))
    fd, u, e = _device(hip_engine_factory(), _system(140, [f]), xs)
    for r in range(2):
        ref = _reference(f, xs[r])
        assert len(ref['E']) == 1300 - 2 - 6 - 10
        assert ref['count'][15] == 0 and np.all(fd[r][15] == 0.0)
        _assert_matches('replica %d' % r, fd[r], e[r, 0], ref)


# ---- 7. one atom in three roles -----------------------------------------------------------------------------------------------------------------
def test_an_atom_that_is_d1_d2_and_a1_gets_forces_from_all_roles(hip_engine_factory):
    """six waters O H1 H2 (atoms 3 w ...): donor (O, H1) has O as d1, donor (H2, O) has O as d2, acceptor (O) has it as a1; the pairs of
    one water share O and are excluded"""
    f = CustomHbondForce('k*exp(-distance(d1,a1))*(1+cos(angle(d2,d1,a1)))')
    f.addGlobalParameter('k', 5.0)
    for w in range(6):
        f.addDonor(3 * w, 3 * w + 1, -1)
        f.addDonor(3 * w + 2, 3 * w, -1)
        f.addAcceptor(3 * w, -1, -1)
        f.addExclusion(2 * w, w); f.addExclusion(2 * w + 1, w)
    rng = np.random.default_rng(907)
    o = np.array([[0.35 * a, 0.33 * b, 0.3 * c] for a in range(3) for b in range(2) for c in range(1)], dtype=np.float64)
    xs = []
    for _ in range(2):
        x = np.zeros((18, 3))
        x[0::3] = o + rng.uniform(-0.03, 0.03, o.shape)
        x[1::3] = x[0::3] + rng.normal(0.0, 0.06, o.shape)
        x[2::3] = x[0::3] + rng.normal(0.0, 0.06, o.shape)
        xs.append(x)
    xs = _f32(xs)
    fd, u, e = _device(hip_engine_factory(), _system(18, [f]), xs)
    for r in range(2):
        ref = _reference(f, xs[r])
        assert len(ref['E']) == 12 * 6 - 12
        assert np.all(ref['count'][0::3] == 5 + 5 + 10) and np.all(ref['count'][1::3] == 5)     # O: as d1, as d2 and as a1 of ten donors
        _assert_matches('replica %d' % r, fd[r], e[r, 0], ref)


# ---- 8. sixteen parameters, a global, u_kl -------------------------------------------------------------------------------------------------------
LAMBDAS = np.array([[1.0], [0.5], [0.0]])


def test_sixteen_parameters_and_the_ukl_rows_of_a_global(hip_engine_factory):
    donor_names, acceptor_names = ['p%d' % k for k in range(10)], ['q%d' % k for k in range(6)]
    f = CustomHbondForce('lam*(%s)*exp(-distance(d1,a1)*(%s))' % ('+'.join(donor_names), '+'.join(acceptor_names)))
    f.addGlobalParameter('lam', 1.0)
    for n in donor_names:
        f.addPerDonorParameter(n)
    for n in acceptor_names:
        f.addPerAcceptorParameter(n)
    rng = np.random.default_rng(908)
    for k in range(9):
        f.addDonor(k, -1, -1, rng.uniform(0.1, 1.0, 10))
    for k in range(11):
        f.addAcceptor(9 + k, -1, -1, rng.uniform(0.1, 0.5, 6))
    system = _system(20, [f])
    x = rng.uniform(0.0, 1.0, (20, 3))
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
        want[:, l] = BETA * ref['E'].sum()
        _assert_matches('state %d' % l, fd[l], per_state[l], ref)
    print('u_kl: max |got - want| / max|want| = %.3g' % (np.abs(u - want).max() / np.abs(want).max()))
    assert np.allclose(u, want, rtol=1e-5, atol=1e-5 * np.abs(want).max())
    # against the device's own energies at each state's globals: f64 sums of f64 per-pair differences
    assert np.allclose(u, BETA * np.tile(per_state, (3, 1)), rtol=1e-9, atol=1e-11 * np.abs(want).max())
    assert np.allclose(u[np.arange(3), labels], BETA * per_state, rtol=1e-14, atol=0.0)   # (the own column is beta U)


# ---- 9. tabulated functions ---------------------------------------------------------------------------------------------------------------------
def test_a_periodic_spline_of_a_dihedral_and_a_lookup_of_two_types(hip_engine_factory):
    phi = np.linspace(-math.pi, math.pi, 25)
    values = 1.0 + 0.6 * np.cos(2.0 * phi) + 0.3 * np.sin(phi)
    values[-1] = values[0]
    scale = np.array([1.0, 0.5, 2.0, 0.5, 0.25, 1.5])                     # [3 donor types][2 acceptor types], the donor type fastest
    f = CustomHbondForce('tab(dihedral(d2,d1,a1,a2))*scale(td,ta)*exp(-distance(d1,a1))')
    f.addTabulatedFunction('tab', Continuous1DFunction(values, -math.pi, math.pi, True))
    f.addTabulatedFunction('scale', Discrete2DFunction(3, 2, scale))
    f.addPerDonorParameter('td')
    f.addPerAcceptorParameter('ta')
    for k in range(6):
        f.addDonor(2 * k, 2 * k + 1, -1, [k % 3])
    for k in range(5):
        f.addAcceptor(12 + 2 * k, 13 + 2 * k, -1, [k % 2])
    rng = np.random.default_rng(909)
    xs = _f32(rng.uniform(0.0, 1.0, (2, 22, 3)))
    functions = dict(tab=tabulated_oracle.Spline(values, -math.pi, math.pi, True), scale=tabulated2d_oracle.Lookup2D(3, 2, scale))
    fd, u, e = _device(hip_engine_factory(), _system(22, [f]), xs)
    for r in range(2):
        ref = _reference(f, xs[r], functions=functions)
        assert len(ref['E']) == 30
        _assert_matches('replica %d' % r, fd[r], e[r, 0], ref)


# ---- 10. beside a CustomBondForce and a CustomNonbondedForce ----------------------------------------------------------------------------------
def test_coexistence_leaves_the_other_custom_forces_bitwise_unchanged(hip_engine_factory):
    rng = np.random.default_rng(910)
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
    hb = CustomHbondForce(REFERENCE)
    hb.addPerDonorParameter('k'); hb.addPerAcceptorParameter('r0')
    for k in range(0, 20, 2):
        hb.addDonor(k, k + 1, -1, [rng.uniform(20.0, 40.0)])
    for k in range(20, N):
        hb.addAcceptor(k, -1, -1, [rng.uniform(0.2, 0.3)])
    for f in (bond, nb, hb):
        f.setForceGroup(3)
    grid = np.array([[a, b, c] for a in range(4) for b in range(4) for c in range(3)], dtype=np.float64)[:N] * 0.3
    x = grid + rng.uniform(-0.03, 0.03, grid.shape)
    x[1:20:2] = x[0:20:2] + [0.11, 0.02, 0.0]
    xs = _f32([x, x + rng.normal(0.0, 0.005, x.shape)])
    f_all, u_all, e_all = _device(hip_engine_factory(), _system(N, [bond, hb, nb]), xs)
    f_two, u_two, e_two = _device(hip_engine_factory(), _system(N, [bond, nb]), xs)
    eng = hip_engine_factory()
    f_hb, u_hb, e_hb = _device(eng, _system(N, [copy.deepcopy(hb)]), xs)
    assert np.array_equal(eng.get_forces(groups=1 << 3), f_hb) and np.all(eng.get_forces(groups=1 << 2) == 0.0)
    assert e_all.shape == (2, 3) and np.abs(e_all[:, 1]).min() > 0.0
    assert np.array_equal(e_all[:, [0, 2]], e_two)                        # the bond's and the nonbonded force's energies, bit for bit
    assert np.array_equal(e_all[:, 1], e_hb[:, 0])
    assert np.array_equal(f_all, f_two + f_hb)                            # fixed-point sums: the others' forces are unchanged to the bit
    for r in range(2):
        ref = _reference(hb, xs[r])
        assert abs(e_all[r, 1] - ref['E'].sum()) <= oracle.energy_bound(ref)
        assert np.all(np.abs(f_all[r] - f_two[r] - ref['F']) <= oracle.force_bound(ref))


# ---- 12. dynamics, minimisation, the barostat ---------------------------------------------------------------------------------------------------
def test_md_steps_minimisation_and_barostat_trials_on_the_periodic_case(hip_engine_factory):
    force, xs, boxes = _case4()
    system = _system(80, [force], boxes[0])
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
    # isotropic barostat trials: after every attempt the potential is the oracle's at the replica's positions and box
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
