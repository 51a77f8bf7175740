"""GPU: CustomNonbondedForce (openmmtools_amd/custom_expr.py kind 6, csrc/custom_nonbonded.hip, include/remd_hip_custom.h) against the
independent f64 helper tests/custom_nonbonded_oracle.py.

Bounds, derived from the formats: the energy within 1e-11 sum|E_pair| (an f64 sum of f64 pair energies), the
force on an atom, per component, within n (2^-23 max|contribution| + 2^-31) with n the atom's partners (every pair's force is rounded to
f32 once, then added in fixed point).  Positions are rounded to f32 before they go to either side, and every test asserts on the CPU that
no pair lies within 1e-9 nm of the cutoff or the switching distance, so that a borderline pair cannot decide a result."""
import numpy as np
import pytest

import custom_nonbonded_oracle as oracle
from openmmtools_amd import custom_expr as cx, states, testsystems, unit
from openmmtools_amd.system import System, system_to_desc, CustomNonbondedForce, NonbondedForce

pytestmark = pytest.mark.gpu

KB = 0.008314462618153242
BETA = 1.0 / (KB * 300.0)
WCA = '4.0*epsilon*((sigma/r)^12 - (sigma/r)^6) + epsilon; sigma = 0.34; epsilon = 0.997740'
LJ_MIXED = '4*epsilon*((sigma/r)^12 - (sigma/r)^6); sigma = 0.5*(sigma1 + sigma2); epsilon = sqrt(epsilon1*epsilon2)'


def _f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def _system(n, forces, box=None):
    s = System()
    for _ in range(n):
        s.addParticle(39.9)
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


def _reference(force, x, box=None, global_values=None):
    g = {force.getGlobalParameterName(i): force.getGlobalParameterDefaultValue(i) for i in range(force.getNumGlobalParameters())}
    g.update(global_values or {})
    n = force.getNumParticles()
    ref = oracle.evaluate(force.getEnergyFunction(), [force.getPerParticleParameterName(k) for k in range(force.getNumPerParticleParameters())],
                          [force.getParticleParameters(k) for k in range(n)], g, x, box, force.getNonbondedMethod(), force.getCutoffDistance(),
                          force.getSwitchingDistance() if (force.getUseSwitchingFunction() and force.getNonbondedMethod()) else -1.0,
                          [force.getExclusionParticles(k) for k in range(force.getNumExclusions())])
    # no pair within 1e-9 nm of the cutoff or the switching distance
    if force.getNonbondedMethod():
        assert np.abs(ref['r_all'] - force.getCutoffDistance()).min() > 1e-9
        if force.getUseSwitchingFunction():
            assert np.abs(ref['r_all'] - force.getSwitchingDistance()).min() > 1e-9
    return ref


def _assert_matches(tag, f, e, ref, lrc=0.0):
    worst = np.abs(f - ref['F']) / oracle.force_bound(ref).clip(min=1e-300)
    print('%s: %d pairs, |dE| / (1e-11 sum|E|) = %.3g, worst |dF| / bound = %.3g' % (
        tag, len(ref['E']), abs(e - ref['E'].sum() - lrc) / max(oracle.energy_bound(ref), 1e-300), worst.max()))
    assert abs(e - ref['E'].sum() - lrc) <= oracle.energy_bound(ref) + 1e-11 * abs(lrc)
    assert np.all(np.abs(f - ref['F']) <= oracle.force_bound(ref))


def _spread(n, rng, lo, hi, dmin):
    """n points uniform in the box lo ... hi, no two closer than dmin (in plain distance)"""
    pts = []
    while len(pts) < n:
        p = rng.uniform(lo, hi)
        if all(np.linalg.norm(p - q) >= dmin for q in pts):
            pts.append(p)
    return np.array(pts)


def _wca(n, method=CustomNonbondedForce.CutoffPeriodic):
    f = CustomNonbondedForce(WCA)
    for _ in range(n):
        f.addParticle([])
    f.setNonbondedMethod(method)
    f.setCutoffDistance(2.0 ** (1.0 / 6.0) * 0.34)
    return f


# ---- 1. N = 70, periodic: the three tile shapes, the minimum image, the remainder flush alone ---------------------------------------------
def test_periodic_wca_of_70_atoms_across_every_face(hip_engine_factory):
    """one full and one 6-atom block: a diagonal tile, an off-diagonal tile and a padded diagonal tile; fewer than 64 pairs in all, so
    only the remainder flush runs; pairs across every face of the box, in every tile; two replicas with different boxes"""
    boxes = _f32([[3.0, 3.2, 3.4], [3.3, 3.1, 3.5]])                    # (the device holds the box in f32 as well)
    rng = np.random.default_rng(701)
    xs = []
    for L in boxes:
        x = _spread(70, rng, np.full(3, 0.45), L - 0.45, 0.45)           # the bulk: apart, and away from the faces
        # pairs through the x, y and z faces: in the diagonal tile (2, 3), across tiles (10, 66), in the padded tile (65, 69)
        for axis, (a, b) in enumerate(((2, 3), (10, 66), (65, 69))):
            x[a, axis] = 0.06 + 0.01 * axis
            x[b] = x[a]
            x[b, axis] = L[axis] - 0.27 + 0.01 * axis                   # 0.33 + 0.02 axis away through the face
        x[3, 0] += L[0]                                                   # (an atom outside the box: the image is of the difference)
        xs.append(x)
    xs = _f32(xs)
    force = _wca(70)
    system = _system(70, [force], boxes[0])
    f, u, e = _device(hip_engine_factory(), system, xs, boxes)
    for r in range(2):
        ref = _reference(force, xs[r], boxes[r])
        assert 3 <= len(ref['E']) < 64
        tiles = {(i // 64, j // 64) for i, j in zip(ref['i'], ref['j'])}
        assert tiles == {(0, 0), (0, 1), (1, 1)}
        plain = np.linalg.norm(xs[r][ref['j']] - xs[r][ref['i']], axis=1)
        assert np.sum(plain > 1.0) >= 3                                   # (pairs that are pairs through a face only)
        _assert_matches('replica %d' % r, f[r], e[r, 0], ref)
        assert u[r] == e[r, 0]                                            # (the System has no other force)


# ---- 2. N = 130 without a cutoff: overflowing queues, per-particle parameters, exclusions -------------------------------------------------
def _mixed_lj_130():
    f = CustomNonbondedForce(LJ_MIXED)
    f.addPerParticleParameter('sigma')
    f.addPerParticleParameter('epsilon')
    rng = np.random.default_rng(1302)
    for _ in range(130):
        f.addParticle([rng.uniform(0.25, 0.35), rng.uniform(0.2, 1.0)])
    f.addExclusion(3, 7)                                                  # inside a diagonal tile
    f.addExclusion(100, 10)                                               # across tiles
    f.addExclusion(129, 128)                                              # inside the padded diagonal tile
    for j in range(130):                                                  # an atom whose whole row is excluded
        if j != 65:
            f.addExclusion(65, j)
    grid = np.array([[a, b, c] for a in range(6) for b in range(5) for c in range(5)], dtype=np.float64)[:130] * 0.42
    xs = _f32([grid + rng.uniform(-0.04, 0.04, grid.shape), grid * 1.03 + rng.uniform(-0.04, 0.04, grid.shape)])
    return f, xs


_CACHE = {}


def _mixed_lj_130_reference():
    if 'lj130' not in _CACHE:
        f, xs = _mixed_lj_130()
        _CACHE['lj130'] = (f, xs, [_reference(f, x) for x in xs])
    return _CACHE['lj130']


def test_nocutoff_mixed_lj_of_130_atoms_with_exclusions(hip_engine_factory):
    force, xs, refs = _mixed_lj_130_reference()
    f, u, e = _device(hip_engine_factory(), _system(130, [force]), xs)
    for r, ref in enumerate(refs):
        assert len(ref['E']) == 130 * 129 // 2 - 3 - 129 and len(ref['E']) % 64 != 0
        assert ref['partners'][65] == 0 and np.all(f[r][65] == 0.0)      # (the excluded atom feels nothing)
        _assert_matches('replica %d' % r, f[r], e[r, 0], ref)


# ---- 9a. bit-reproducibility ------------------------------------------------------------------------------------------------------------
def test_two_evaluations_are_bitwise_equal(hip_engine_factory):
    force, xs, _ = _mixed_lj_130_reference()
    a = _device(hip_engine_factory(), _system(130, [force]), xs)
    b = _device(hip_engine_factory(), _system(130, [force]), xs)
    for p, q in zip(a, b):
        assert np.array_equal(p, q)


# ---- 3. CutoffNonPeriodic and the switch ------------------------------------------------------------------------------------------------
def test_cutoff_nonperiodic_with_switch_and_a_pair_at_zero_distance(hip_engine_factory):
    """pairs below rs, inside (rs, rc) and beyond rc; energy and force with the E S' term; two atoms at one point: a finite energy and
    no force from that pair"""
    f = CustomNonbondedForce('k*(1 + cos(3.0*r))*exp(-r/width1 - r/width2)')
    f.addGlobalParameter('k', 2.5)
    f.addPerParticleParameter('width')
    rng = np.random.default_rng(703)
    for _ in range(70):
        f.addParticle([rng.uniform(0.8, 1.6)])
    f.setNonbondedMethod(CustomNonbondedForce.CutoffNonPeriodic)
    f.setCutoffDistance(1.0)
    f.setUseSwitchingFunction(True)
    f.setSwitchingDistance(0.7)
    xs = np.array([_spread(70, rng, np.zeros(3), np.full(3, 2.4), 0.2) for _ in range(2)])
    xs[:, 66] = xs[:, 5]                                                  # r = 0, across tiles
    xs = _f32(xs)
    fd, u, e = _device(hip_engine_factory(), _system(70, [f]), xs)
    for r in range(2):
        ref = _reference(f, xs[r])
        rr = ref['r_all']
        assert np.sum(rr < 0.7) > 10 and np.sum((rr > 0.7) & (rr < 1.0)) > 10 and np.sum(rr > 1.0) > 10 and np.sum(rr == 0.0) == 1
        _assert_matches('replica %d' % r, fd[r], e[r, 0], ref)
        assert np.isfinite(fd[r]).all()


# ---- 4. an empty result -----------------------------------------------------------------------------------------------------------------
def test_a_cutoff_below_every_distance_gives_exact_zeros(hip_engine_factory):
    force, xs, _ = _mixed_lj_130_reference()
    import copy
    g = copy.deepcopy(force)
    g.setNonbondedMethod(CustomNonbondedForce.CutoffNonPeriodic)
    g.setCutoffDistance(0.05)
    ref = _reference(g, xs[0])
    assert len(ref['E']) == 0
    f, u, e = _device(hip_engine_factory(), _system(130, [g]), xs)
    assert np.all(f == 0.0) and np.all(u == 0.0) and np.all(e == 0.0)


# ---- 5. against the built-in path -------------------------------------------------------------------------------------------------------
def test_lennard_jones_fluid_as_a_custom_force_matches_the_built_in_path(hip_engine_factory):
    """LennardJonesFluid (216, the built-in NonbondedForce) against the same fluid as a CustomNonbondedForce with the LJ string, the same
    cutoff, switch and long-range correction: within the HIP leg's 1e-5 relative of each other, each within its own bound of the oracle"""
    fluid = testsystems.LennardJonesFluid(nparticles=216)
    nb = [f for f in fluid.system.getForces() if isinstance(f, NonbondedForce)][0]
    sigma, epsilon = nb.getParticleParameters(0)[1:]
    c = CustomNonbondedForce('4*epsilon*((sigma/r)^12 - (sigma/r)^6)')
    c.addPerParticleParameter('unused')
    c.addGlobalParameter('sigma', sigma)
    c.addGlobalParameter('epsilon', epsilon)
    for _ in range(216):
        c.addParticle([0.0])
    c.setNonbondedMethod(CustomNonbondedForce.CutoffPeriodic)
    c.setCutoffDistance(nb.getCutoffDistance())
    c.setUseSwitchingFunction(True)
    c.setSwitchingDistance(nb.getSwitchingDistance())
    c.setUseLongRangeCorrection(True)
    L = _f32(np.diag(fluid.system.getDefaultPeriodicBoxVectors()))
    boxes = np.array([L, L])
    rng = np.random.default_rng(705)
    xs = _f32([fluid.positions, fluid.positions + rng.normal(0.0, 0.01, fluid.positions.shape)])
    custom = _system(216, [c], L)
    f1, u1, e1 = _device(hip_engine_factory(), custom, xs, boxes)
    eng = hip_engine_factory()
    _setup(eng, fluid.system, xs, boxes)
    f0 = eng.get_forces()
    u0 = eng.get_replicas(positions=False, velocities=False, potential=True)[2]
    rc, rs = nb.getCutoffDistance(), nb.getSwitchingDistance()
    tail = oracle.lj_tail(sigma, epsilon, rc) + oracle.switched_part(
        lambda r: 4.0 * epsilon * ((sigma / r) ** 12 - (sigma / r) ** 6), rs, rc, 200000)
    lrc = oracle.long_range_coefficient(216, [((0.0,), 216)], lambda a, b: tail) / np.prod(L)
    for r in range(2):
        ref = _reference(c, xs[r], L)
        scale_f, scale_e = np.abs(ref['F']).max(), np.abs(ref['E']).sum()
        print('replica %d: custom - built-in: |dF| / max|F| = %.3g, |dU| / sum|E| = %.3g' % (
            r, np.abs(f1[r] - f0[r]).max() / scale_f, abs(u1[r] - u0[r]) / scale_e))
        assert np.abs(f1[r] - f0[r]).max() <= 1e-5 * scale_f
        assert abs(u1[r] - u0[r]) <= 1e-5 * scale_e
        # the custom path within its own bound (the correction's trapezoid: 2e-10 relative at 200000 steps, see the CPU test)
        assert np.all(np.abs(f1[r] - ref['F']) <= oracle.force_bound(ref))
        assert abs(e1[r, 0] - ref['E'].sum() - lrc) <= oracle.energy_bound(ref) + 1e-9 * abs(lrc)
        # the built-in path within the HIP leg's bound of the same oracle
        assert np.abs(f0[r] - ref['F']).max() <= 1e-5 * scale_f
        assert abs(u0[r] - ref['E'].sum() - lrc) <= 1e-5 * scale_e


# ---- 6. globals and u_kl ----------------------------------------------------------------------------------------------------------------
LAMBDAS = np.array([[1.0], [0.5], [0.0]])


def _lambda_lj(n):
    f = CustomNonbondedForce('lambda*4*epsilon*((sigma/r)^12 - (sigma/r)^6); sigma = 0.34; epsilon = 0.997740')
    f.addGlobalParameter('lambda', 1.0)
    for _ in range(n):
        f.addParticle([])
    f.setNonbondedMethod(CustomNonbondedForce.CutoffPeriodic)
    f.setCutoffDistance(1.0)
    f.setUseLongRangeCorrection(True)
    return f


def test_ukl_rows_with_a_global_and_the_long_range_share(hip_engine_factory):
    """lambda at three states through a GlobalParameterState; rows against the oracle within the u_kl bound of DESIGN section 12 (rtol
    1e-5, atol 1e-5 max|want|); the own column is exactly beta U; uniform globals launch nothing"""
    boxes = _f32([[2.4, 2.5, 2.6], [2.6, 2.4, 2.5]])
    rng = np.random.default_rng(706)
    xs = _f32([_spread(70, rng, np.zeros(3), L, 0.3) for L in boxes])
    force = _lambda_lj(70)
    system = _system(70, [force], boxes[0])
    LambdaState = type('LambdaState', (states.GlobalParameterState,),
                       {'lambda': states.GlobalParameterState.GlobalParameter('lambda', standard_value=1.0)})
    sts = [states.CompoundThermodynamicState(states.ThermodynamicState(system, 300.0 * unit.kelvin), [LambdaState(**{'lambda': float(v)})])
           for v in LAMBDAS[:, 0]]
    table = cx.custom_globals(system, ['lambda'], sts)
    assert np.array_equal(table, LAMBDAS)
    labels = np.array([1, 0])
    eng = hip_engine_factory()
    _setup(eng, system, xs, boxes, table, labels)
    u = eng.compute_energies()
    per_force = eng.custom_energies()
    tail = oracle.lj_tail(0.34, 0.997740, 1.0)
    want = np.zeros((2, 3))
    for r in range(2):
        ref = _reference(force, xs[r], boxes[r], dict({'lambda': 1.0}))
        for l in range(3):
            c = oracle.long_range_coefficient(70, [((), 70)], lambda a, b: LAMBDAS[l, 0] * tail)
            want[r, l] = BETA * (LAMBDAS[l, 0] * ref['E'].sum() + c / np.prod(boxes[r]))
        assert c == 0.0 and oracle.long_range_coefficient(70, [((), 70)], lambda a, b: tail) != 0.0
    print('u_kl: max |got - want| / max|want| = %.3g' % (np.abs(u - want).max() / np.abs(want).max()))
    assert np.allclose(u, want, rtol=1e-5, atol=1e-5 * np.abs(want).max())
    # tighter: the rows' differences from the own column are f64 sums of f64 differences (1e-11 of the summed magnitudes would do;
    # the f32 box behind V limits the long-range share to 1e-7 relative)
    assert np.allclose(u - u[np.arange(2), labels][:, None], want - want[np.arange(2), labels][:, None], rtol=1e-6,
                       atol=1e-9 * np.abs(want).max())
    assert np.allclose(per_force[:, 0], want[np.arange(2), labels] / BETA, rtol=1e-9)
    # uniform globals: custom_energies() unchanged in kind, every column equal to the own one bitwise
    eng.set_custom_globals(np.tile(LAMBDAS[1], (3, 1)))
    u2 = eng.compute_energies()
    assert np.array_equal(u2, np.tile(u2[:, :1], (1, 3)))              # (one temperature: the temperature-only rows are one column)
    assert u[0, 1] == u2[0, 1]                                            # replica 0 sits at that state: its own column carried a share of exactly 0
    assert np.allclose(eng.custom_energies()[:, 0], want[:, 1] / BETA, rtol=1e-9)
    # a fourth state that repeats lambda = 0.5 while the kernel IS launched: the column of a state with the replica's own globals carries a
    # share of exactly 0 (the kernel skips such a state), for both replicas, whichever of the two states is the own one
    table4 = np.array([[1.0], [0.5], [0.0], [0.5]])
    labels4 = np.array([1, 3])
    eng4 = hip_engine_factory()
    _setup(eng4, system, xs, boxes, table4, labels4)
    u4 = eng4.compute_energies()
    assert np.array_equal(u4[:, 1], u4[:, 3])
    assert np.array_equal(u4[0, 1], u[0, 1])                              # (and it is the column the three-state handle gave its own state)
    assert np.allclose(u4[:, :3], want, rtol=1e-5, atol=1e-5 * np.abs(want).max())


# ---- 7. mixed: beside a CustomBondForce and the built-in NonbondedForce ---------------------------------------------------------------
def test_beside_a_custom_bond_force_and_the_built_in_nonbonded_force(hip_engine_factory):
    """DoubleWellDimer_WCAFluid(ndimers=2, nparticles=70) with the NonbondedForce half of a CustomLennardJonesFluidMixture-like split added:
    custom_energies() per force, get_forces(groups=...) returns the custom forces alone"""
    dimer = testsystems.DoubleWellDimer_WCAFluid(ndimers=2, nparticles=70)
    system = dimer.system
    L = _f32(np.diag(system.getDefaultPeriodicBoxVectors()))
    nb = NonbondedForce()
    nb.setNonbondedMethod(NonbondedForce.CutoffPeriodic)
    nb.setCutoffDistance(1.02)
    nb.setUseDispersionCorrection(False)
    for k in range(70):
        nb.addParticle(0.0, 0.34, 0.0 if k < 35 else 0.996)
    nb.setForceGroup(2)
    system.addForce(nb)
    for f in system.getForces():
        if not isinstance(f, NonbondedForce):
            f.setForceGroup(1)
    rng = np.random.default_rng(707)
    x = _spread(70, rng, np.zeros(3), L, 0.33)
    x[1] = x[0] + [0.36, 0.0, 0.0]                                        # the dimers near their short state
    x[3] = x[2] + [0.0, 0.40, 0.0]
    xs = _f32([x, x + rng.normal(0.0, 0.004, x.shape)])
    boxes = np.array([L, L])
    eng = hip_engine_factory()
    _setup(eng, system, xs, boxes)
    e = eng.custom_energies()
    f_custom = eng.get_forces(groups=1 << 1)
    f_all = eng.get_forces()
    f_nb = eng.get_forces(groups=1 << 2)
    wca, bond = [f for f in system.getForces() if isinstance(f, CustomNonbondedForce)][0], dimer.dw_dimer
    import custom_dual_oracle as dual
    for r in range(2):
        ref = _reference(wca, xs[r], L)
        atoms, params = bond._term_arrays()
        eb, fb = dual.evaluate(dual.KIND_BOND, bond.getEnergyFunction(), atoms, ['h', 'r0', 'w'], params, {}, xs[r])
        assert len(ref['E']) > 0
        assert abs(e[r, 0] - ref['E'].sum()) <= oracle.energy_bound(ref)
        assert abs(e[r, 1] - eb.sum()) <= 1e-11 * np.abs(eb).sum() + 1e-12
        bound = oracle.force_bound(ref) + 2.0 * (2.0 ** -23 * np.abs(fb).max() + 2.0 ** -31)
        assert np.all(np.abs(f_custom[r] - ref['F'] - fb) <= bound)
        assert np.abs(f_nb[r]).max() > 0.0
        assert np.allclose(f_all[r], f_custom[r] + f_nb[r], rtol=0.0, atol=2.0 ** -30)


# ---- 8. dynamics, minimisation and the barostat on a System whose only pair force is the custom one -----------------------------------
def _drift(engine, fluid, n_steps=200, dt=0.0005):
    """max over 2 replicas of |E_end - E_start|, E = potential + kinetic (kJ/mol), of n_steps velocity-Verlet steps ("V R V") after
    minimize(); the kinetic energy is formed here in f64 from the device's velocities"""
    system = fluid.system
    L = _f32(np.diag(system.getDefaultPeriodicBoxVectors()))
    boxes = np.array([L, L])
    N = system.getNumParticles()
    rng = np.random.default_rng(708)
    xs = _f32([fluid.positions, fluid.positions + rng.normal(0.0, 0.002, fluid.positions.shape)])
    _setup(engine, system, xs, boxes)
    engine.set_integrator('V R V', dt, 1.0, n_steps, False, 1e-8)
    converged, n_fire = engine.minimize(10.0, 200)
    x = engine.get_replicas()[0]
    m = np.array([system.getParticleMass(i) for i in range(N)])
    v = rng.normal(0.0, 1.0, (2, N, 3)) * np.sqrt(KB * 120.0 / m)[None, :, None]
    v -= v.mean(axis=1, keepdims=True)
    engine.set_replicas(2, 0, x, v, boxes, np.zeros(2, dtype=np.int64))

    def total():
        pot = engine.compute_energies(want_potential=True)[1]
        vel = engine.get_replicas()[1]
        return pot + 0.5 * (m[None, :, None] * vel * vel).sum(axis=(1, 2)), pot
    e0, u0 = total()
    assert not engine.propagate(0).any()
    e1, u1 = total()
    return np.abs(e1 - e0).max(), n_fire, u0, u1, engine.get_replicas()[0], x


def test_wca_fluid_dynamics_conserve_energy_as_the_built_in_fluid_does(hip_engine_factory):
    """WCAFluid() (216 particles, no NonbondedForce), 2 replicas, after minimize(): 200 velocity-Verlet steps of 0.5 fs conserve the
    total energy; the drift may be twice that of the same run of LennardJonesFluid(216) on the built-in path, measured here"""
    d_lj, _, _, _, _, _ = _drift(hip_engine_factory(), testsystems.LennardJonesFluid(nparticles=216))
    wca = testsystems.WCAFluid()
    d_wca, n_fire, u0, u1, x1, x0 = _drift(hip_engine_factory(), wca)
    print('drift over 200 steps of 0.5 fs: WCAFluid %.3g kJ/mol, LennardJonesFluid %.3g kJ/mol; FIRE steps %d; WCA potential %s -> %s'
          % (d_wca, d_lj, n_fire, u0, u1))
    assert np.abs(x1 - x0).max() > 1e-3                                   # (the particles moved)
    assert np.isfinite(d_wca) and d_wca <= 2.0 * d_lj
    # the potential the propagation left is the oracle's at the final positions
    force = wca.system.getForces()[0]
    L = _f32(np.diag(wca.system.getDefaultPeriodicBoxVectors()))
    for r in range(2):
        ref = _reference(force, _f32(x1[r]), L)
        assert abs(u1[r] - ref['E'].sum()) <= oracle.energy_bound(ref)


def test_isotropic_barostat_moves_see_the_custom_energy_and_its_long_range_share(hip_engine_factory):
    """a System whose only force is a CustomNonbondedForce with a long-range correction under the isotropic Monte Carlo barostat: after
    every attempt the potential the move left (the trial box's where it was accepted, the old one where it was rejected) is the oracle's
    at the replica's positions and box, coeff / V included; at least one move is accepted and one rejected"""
    boxes = _f32([[2.5, 2.5, 2.5], [2.6, 2.6, 2.6]])
    rng = np.random.default_rng(709)
    xs = _f32([_spread(70, rng, np.zeros(3), L, 0.33) for L in boxes])
    force = _lambda_lj(70)
    system = _system(70, [force], boxes[0])
    eng = hip_engine_factory()
    desc = system_to_desc(system, box=boxes[0])
    eng.set_system(desc)
    eng.set_states(np.full(1, BETA))
    eng.set_custom_globals(np.array([[1.0]]))
    eng.set_integrator('V R O R V', 0.001, 1.0, 5, True, 1e-8)
    eng.set_barostat(np.full(1, 2000.0 * unit.bar), 25)
    eng.seed(31)
    eng.set_replicas(2, 0, xs, None, boxes, np.zeros(2, dtype=np.int64))
    eng.compute_energies()
    coeff = oracle.long_range_coefficient(70, [((), 70)], lambda a, b: oracle.lj_tail(0.34, 0.997740, 1.0))
    accepted = rejected = 0
    box_before = eng.get_boxes().copy()
    for attempt in range(10):
        n_acc_before = eng.barostat_stats()[2].copy()
        eng.barostat_attempts(1)
        box_now = eng.get_boxes()
        x, _, pot, _ = eng.get_replicas(potential=True)
        took = eng.barostat_stats()[2] - n_acc_before
        for r in range(2):
            assert (took[r] == 1) == bool(np.any(box_now[r] != box_before[r]))
            ref = _reference(force, _f32(x[r]), _f32(box_now[r]))
            want = ref['E'].sum() + coeff / np.prod(_f32(box_now[r]))
            assert abs(pot[r] - want) <= oracle.energy_bound(ref) + 1e-11 * abs(want), (attempt, r, took[r], pot[r], want)
        accepted += int(took.sum()); rejected += int(2 - took.sum())
        box_before = box_now.copy()
        if accepted and rejected and attempt >= 3:
            break
    print('barostat: %d accepted, %d rejected' % (accepted, rejected))
    assert accepted >= 1 and rejected >= 1
    assert np.all(eng.get_boxes() >= 2.0)                                 # (twice the force's cutoff: the only cutoff this handle has)


# ---- 9b. phased propagation -------------------------------------------------------------------------------------------------------------
def test_phased_propagation_with_a_custom_nonbonded_force_is_the_one_block_run(hip_engine_factory):
    """AlanineDipeptideExplicit with a small CustomNonbondedForce added (a switched, long-range-corrected r^-6 attraction between 45
    marked atoms, exclusions among them, a global that differs between the states), 6 replicas: two blocks equal one block bit for bit,
    as tests/test_phases_gpu.py compares them"""
    al = testsystems.AlanineDipeptideExplicit()
    N = al.system.getNumParticles()
    f = CustomNonbondedForce('-scale*mark1*mark2*c6/r^6')
    f.addGlobalParameter('scale', 1.0)
    f.addGlobalParameter('c6', 2.0e-3)
    f.addPerParticleParameter('mark')
    marked = set(range(22, N, 50))
    for i in range(N):
        f.addParticle([1.0 if i in marked else 0.0])
    ordered = sorted(marked)
    for a, b in zip(ordered[::2], ordered[1::2]):
        f.addExclusion(a, b)
    f.setNonbondedMethod(CustomNonbondedForce.CutoffPeriodic)
    f.setCutoffDistance(0.9)
    f.setUseSwitchingFunction(True)
    f.setSwitchingDistance(0.8)
    f.setUseLongRangeCorrection(True)
    al.system.addForce(f)
    desc = system_to_desc(al.system, ewald_split='auto')
    box = np.diag(al.system.getDefaultPeriodicBoxVectors())
    R = 6
    table = np.column_stack([np.linspace(1.0, 0.5, R), np.full(R, 2.0e-3)])
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
    assert np.all(ea != 0.0) and np.any(ua != ua[:, :1])
    assert np.array_equal(xa, xb) and np.array_equal(va, vb) and np.array_equal(ua, ub) and np.array_equal(ea, eb)
