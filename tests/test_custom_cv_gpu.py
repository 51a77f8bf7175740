"""GPU: system.RMSDForce / system.CustomCVForce (openmmtools_amd/custom_expr.py, csrc/custom_cv.hip, include/remd_hip_custom.h) against
the independent f64 helper tests/custom_cv_oracle.py (Kabsch through an SVD; the device diagonalises Horn's matrix).

Positions are rounded to f32 before they go to either side: that is what the engine stores.  The Systems hold nothing but the force
under test, so get_forces() is the force's own.  Bounds:
  forces   per component 2^-23 |contribution| + 2^-31 for every collective variable that names the atom (tests/test_custom_opcodes_gpu.py:
           one f32 rounding of what goes to add_force plus the fixed-point quantum);
  RMSD     RMSD_RTOL |V| + RMSD_ATOL through custom_cv_values(): ten times the worst figure measured over the cases of this file
           (profiles/custom_cv_cost.txt), never looser than 1e-8 relative + 1e-8 nm;
  net force and torque about the centroid: the f32 rounding of n forces, n (2^-23 max|F| + 2^-31), times the lever arm for the torque.
The superposition and spread kernels walk a variable with a stride of 256 and reduce over four wavefronts of 64: n = 3, 4, 63, 64, 65,
257 and 1000 cover fewer particles than a wavefront, the wavefront's edge, more than one trip."""
import copy

import numpy as np
import pytest

import custom_cv_oracle as oracle
from openmmtools_amd import custom_expr as cx, mcmc, states, testsystems, unit
from openmmtools_amd.system import System, system_to_desc, RMSDForce, CustomCVForce, Continuous1DFunction

pytestmark = pytest.mark.gpu

KB = 0.008314462618153242
BETA = 1.0 / (KB * 300.0)
RMSD_RTOL, RMSD_ATOL = 2.5e-12, 2e-15        # measured worst: 2.35e-13 relative, 1.51e-16 nm near zero
SIZES = [3, 4, 63, 64, 65, 257, 1000]
GEOMETRIES = ['rigid', 'perturbed_0.01', 'perturbed_0.3', 'half_turn', 'mirrored', 'far']
worst_rmsd = [0.0, 0.0]                 # relative (RMSD above 1e-6 nm), absolute (below): printed by every test that compares one


def _f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def _rotation(axis, angle):
    a = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _setup(engine, system, xs, global_table=None, labels=None):
    desc = system_to_desc(system)
    engine.set_system(desc)
    K = 1 if global_table is None else len(global_table)
    engine.set_states(np.full(K, BETA))
    engine.set_custom_globals(np.tile(desc['custom_terms']['000']['global_defaults'], (K, 1)) if global_table is None else global_table)
    R = len(xs)
    engine.set_replicas(R, 0, xs, None, np.zeros((R, 3)), np.zeros(R, dtype=np.int64) if labels is None else labels)
    return desc


def _bare_system(n_atoms, *forces):
    s = System()
    for _ in range(n_atoms):
        s.addParticle(12.0)
    for f in forces:
        s.addForce(f)
    return s


def _harmonic(reference, particles, k=800.0, v0=0.05):
    f = CustomCVForce('0.5*k*(v-v0)^2')
    f.addGlobalParameter('k', k); f.addGlobalParameter('v0', v0)
    f.addCollectiveVariable('v', RMSDForce(reference, particles))
    return f


def _check_rmsd(got, want):
    got, want = np.asarray(got), np.asarray(want)
    big = want > 1e-6
    if big.any():
        worst_rmsd[0] = max(worst_rmsd[0], float((np.abs(got - want)[big] / want[big]).max()))
    if (~big).any():
        worst_rmsd[1] = max(worst_rmsd[1], float(np.abs(got - want)[~big].max()))
    print('RMSD: worst so far %.3g relative, %.3g nm absolute (near zero)' % tuple(worst_rmsd))
    assert np.all(np.abs(got - want) <= RMSD_RTOL * np.abs(want) + RMSD_ATOL), (got, want)


def _check_forces(F_dev, parts):
    """parts [n_cvs][N][3]: the helper's contribution of every variable"""
    bound = (2.0 ** -23 * np.abs(parts) + 2.0 ** -31 * (parts != 0.0).any(axis=2, keepdims=True)).sum(axis=0)
    dF = np.abs(F_dev - parts.sum(axis=0))
    named = bound > 0.0
    print('forces: worst |dF| / bound = %.3g' % (dF[named] / bound[named]).max())
    assert np.isfinite(F_dev).all() and np.all(dF <= bound)


def _check_net(F, x, particles):
    n = len(particles)
    Fp, xp = F[particles], x[particles]
    lever = np.abs(xp - xp.mean(axis=0)).max()
    slack = n * (2.0 ** -23 * np.abs(Fp).max() + 2.0 ** -31)
    assert np.abs(Fp.sum(axis=0)).max() <= slack
    assert np.abs(np.cross(xp - xp.mean(axis=0), Fp).sum(axis=0)).max() <= 2.0 * lever * slack


def _cases(n, shape, seed):
    """reference [n + 5][3], shuffled particles [n], positions [geometries][n + 5][3] (f32-exact) for one reference shape"""
    rng = np.random.default_rng(seed)
    N = n + 5
    ref = rng.uniform(-0.8, 0.8, (N, 3))
    particles = rng.permutation(N)[:n]
    if shape == 'planar':
        ref[particles, 2] = 0.25
    if shape == 'collinear':
        ref[particles] = np.outer(rng.uniform(-0.8, 0.8, n), [0.6, -0.5, 0.62]) + [0.1, 0.2, -0.1]
    y = ref[particles]
    R = _rotation(rng.normal(size=3), rng.uniform(0.3, 2.8))
    shift = np.array([1.5, -0.7, 2.2])
    xs, names = [], []
    for g in (GEOMETRIES if shape == 'generic' else ['perturbed_0.01', 'perturbed_0.3']):
        x = rng.uniform(-1.0, 1.0, (N, 3))
        if g == 'rigid':
            x[particles] = y @ R.T + shift
        elif g.startswith('perturbed'):
            x[particles] = y @ R.T + shift + rng.normal(0.0, float(g.split('_')[1]), (n, 3))
        elif g == 'half_turn':
            x[particles] = y @ _rotation(rng.normal(size=3), np.pi - 1e-3 * rng.uniform(-1.0, 1.0)).T + rng.normal(0.0, 0.002, (n, 3))
        elif g == 'mirrored':
            x[particles] = (y * [1.0, 1.0, -1.0]) @ R.T + rng.normal(0.0, 0.01, (n, 3))
        elif g == 'far':
            x[particles] = y @ R.T + rng.normal(0.0, 0.05, (n, 3)) + 40.0
        xs.append(x); names.append(g)
    return ref, [int(p) for p in particles], _f32(np.array(xs)), names


# ---- 1. every size and geometry -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', ['generic', 'planar', 'collinear'])
@pytest.mark.parametrize('n', SIZES)
def test_rmsd_and_forces_at_every_size_and_geometry(hip_engine_factory, n, shape):
    ref, particles, xs, names = _cases(n, shape, seed=100 * n + len(shape))
    f = _harmonic(ref, particles)
    eng = hip_engine_factory()
    _setup(eng, _bare_system(n + 5, f), xs)
    V, F, E = eng.custom_cv_values(), eng.get_forces(), eng.custom_energies()
    assert V.shape == (len(xs), 1) and E.shape == (len(xs), 1)
    others = sorted(set(range(n + 5)) - set(particles))
    for r, g in enumerate(names):
        e, _, v, parts = oracle.evaluate(f, xs[r])
        print('%s %s n = %d: RMSD %.12g (helper %.12g), E %.12g' % (shape, g, n, V[r, 0], v[0], E[r, 0]))
        assert np.isfinite(V[r, 0]) and np.isfinite(E[r, 0]) and np.isfinite(F[r]).all()
        assert not F[r, others].any()                                              # particles outside the variable: exactly zero
        if g == 'rigid':
            # (f32 positions of magnitude ~3 nm: 2^-24 x 3 nm per coordinate; no comparison of forces whose direction is that rounding)
            assert V[r, 0] < 1e-6
            _check_rmsd(V[r], v)
            _check_net(F[r], xs[r], particles)                                      # (1 / (n V) is largest here)
            continue
        _check_rmsd(V[r], v)
        assert abs(E[r, 0] - e) <= 1e-11 * abs(e) + 800.0 * abs(v[0] - 0.05) * (RMSD_RTOL * v[0] + RMSD_ATOL)
        _check_forces(F[r], parts)
        _check_net(F[r], xs[r], particles)
        if g == 'mirrored':
            assert V[r, 0] > (0.05 if n > 3 else 0.0)                                # clearly above the 0.01 nm noise: no improper rotation (three points are planar: their mirror image is a rotation)


def test_positions_on_the_reference_give_zero_and_no_force(hip_engine_factory):
    """the "no force" branch: f32-exact reference positions, untransformed and translated by an f32-exact shift, leave a mean square
    deviation below 1e-20 nm^2 -> RMSD exactly 0, a finite energy, exactly zero forces (no 0 / 0 in the spread)"""
    rng = np.random.default_rng(77)
    n, N = 70, 75
    ref = np.round(rng.uniform(-0.8, 0.8, (N, 3)) * 1024.0) / 1024.0               # multiples of 2^-10 below 4 nm: ref and ref + shift are exact in f32
    particles = [int(p) for p in rng.permutation(N)[:n]]
    xs = np.array([ref, ref + [0.5, -0.25, 2.0]])
    assert np.array_equal(xs, _f32(xs))
    assert np.array_equal(xs[1] - xs[0], np.tile([0.5, -0.25, 2.0], (N, 1)))       # (the shift is exact in f32)
    f = _harmonic(ref, particles)
    eng = hip_engine_factory()
    _setup(eng, _bare_system(N, f), xs)
    V, F, E = eng.custom_cv_values(), eng.get_forces(), eng.custom_energies()
    print('on the reference: RMSD %s, E %s' % (V[:, 0], E[:, 0]))
    assert np.array_equal(V, np.zeros((2, 1))) and not F.any()
    assert np.all(np.abs(E[:, 0] - 0.5 * 800.0 * 0.05 ** 2) <= 1e-14)
    assert oracle.evaluate(f, xs[1])[2][0] == 0.0


def test_the_library_refuses_a_broken_descriptor_and_keeps_the_handle(hip_engine_factory):
    """what the host never lets through, handed to set_custom_terms directly: the library names the fault, and the forces it held
    before the refused call still act"""
    N, ref, xs, fs = _expression_system()
    eng = hip_engine_factory()
    desc = _setup(eng, _bare_system(N, *fs), xs)
    before, v_before = eng.custom_energies(), eng.custom_cv_values()
    good = desc['custom_terms']['000']

    def broken(**changes):
        t = dict(good)
        t.update(changes)
        return t
    ref0, atoms0 = good['cv_reference'], good['cv_atoms']
    dup = atoms0.copy(); dup[1] = dup[0]
    far = atoms0.copy(); far[2] = N
    nan = ref0.copy(); nan[3, 1] = np.nan
    for t, message in ((broken(cv_reference=ref0 + [0.0, 1e-6, 0.0]), 'collective variable 0: the reference must be centred'),
                       (broken(cv_reference=nan), 'collective variable 0: a reference position that is not finite'),
                       (broken(cv_atoms=dup), 'collective variable 0: particle %d named twice' % dup[0]),
                       (broken(cv_atoms=far), 'collective variable 0: particle index out of range'),
                       (broken(cv_offsets=np.array([0, 2], dtype=np.int32), cv_atoms=atoms0[:2], cv_reference=ref0[:2] - ref0[:2].mean(axis=0)),
                        'an RMSD needs at least 3 particles'),
                       (broken(cv_offsets=np.array([1, len(atoms0)], dtype=np.int32)), 'cv_offsets must start at 0'),
                       (broken(periodic=1), 'n_terms = 1, no per-term parameters and is not periodic'),
                       (broken(params=np.zeros((1, 1))), 'n_terms = 1, no per-term parameters and is not periodic'),
                       (broken(program=np.array([[cx.VAR, 1]], dtype=np.int32)), 'a variable index out of range')):
        with pytest.raises(RuntimeError, match='remd_set_custom_terms.*force 0: .*' + message):
            eng.set_custom_terms([t] + [desc['custom_terms'][k] for k in sorted(desc['custom_terms'])[1:]])
        assert np.array_equal(eng.custom_energies(), before) and np.array_equal(eng.custom_cv_values(), v_before)


# ---- 2. expressions ------------------------------------------------------------------------------------------------------------------------
def _expression_system():
    rng = np.random.default_rng(42)
    N = 40
    ref = rng.uniform(-0.7, 0.7, (N, 3))
    xs = _f32(np.array([ref @ _rotation(rng.normal(size=3), 0.4 + r).T + rng.normal(0.0, 0.04 + 0.02 * r, (N, 3)) for r in range(3)]))
    harmonic = _harmonic(ref, list(range(5, 25)))
    product = CustomCVForce('c*a*b*w + 3*w; c = 2*scale')
    product.addGlobalParameter('scale', 150.0)
    product.addCollectiveVariable('a', RMSDForce(ref, list(range(0, 12))))
    product.addCollectiveVariable('b', RMSDForce(ref, list(range(8, 30))))            # (overlaps a and w)
    product.addCollectiveVariable('w', RMSDForce(ref))
    table = CustomCVForce('depth*well(v)')
    table.addGlobalParameter('depth', 30.0)
    table.addCollectiveVariable('v', RMSDForce(ref, [39, 3, 17, 22, 8, 31, 12]))
    table.addTabulatedFunction('well', Continuous1DFunction(np.cos(np.linspace(0.0, 0.5, 33) * 9.0), 0.0, 0.5))
    bare = RMSDForce(ref, list(range(20, 40)))
    return N, ref, xs, [harmonic, product, table, bare]


GLOBALS = ['k', 'v0', 'scale', 'depth']
TABLE = np.array([[800.0, 0.05, 150.0, 30.0], [300.0, 0.1, 40.0, 10.0], [0.0, 0.05, 0.0, 55.0]])


def test_expressions_energies_forces_and_values(hip_engine_factory):
    N, ref, xs, fs = _expression_system()
    labels = np.array([1, 0, 2])
    eng = hip_engine_factory()
    desc = _setup(eng, _bare_system(N, *fs), xs, global_table=TABLE, labels=labels)
    assert desc['custom_terms']['000']['global_names'] == GLOBALS
    V, F, E = eng.custom_cv_values(), eng.get_forces(), eng.custom_energies()
    assert V.shape == (3, 6) and E.shape == (3, 4)
    assert np.array_equal(F, eng.get_forces(groups=1)) and not eng.get_forces(groups=2).any()
    for r in range(3):
        g = dict(zip(GLOBALS, TABLE[labels[r]]))
        per = [oracle.evaluate(f, xs[r], {k: v for k, v in g.items() if k in _names(f)}) for f in fs]
        _check_rmsd(V[r], np.concatenate([p[2] for p in per]))
        for j, p in enumerate(per):
            scale = np.abs(p[3]).sum(axis=(1, 2)).max() if p[3].size else 0.0         # |dE/dV| sum_i |grad_i| >= |dE/dV|
            assert abs(E[r, j] - p[0]) <= 1e-11 * abs(p[0]) + scale * (RMSD_RTOL * p[2].max() + RMSD_ATOL), (r, j, E[r, j], p[0])
        _check_forces(F[r], np.concatenate([p[3] for p in per]))


def _names(f):
    return [f.getGlobalParameterName(i) for i in range(f.getNumGlobalParameters())] if hasattr(f, 'getNumGlobalParameters') else []


def test_ukl_rows_under_three_states_globals(hip_engine_factory):
    N, ref, xs, fs = _expression_system()
    labels = np.array([2, 0, 1])
    eng = hip_engine_factory()
    _setup(eng, _bare_system(N, *fs), xs, global_table=TABLE, labels=labels)
    u = eng.compute_energies()
    want = np.array([[BETA * sum(oracle.evaluate(f, x, {k: v for k, v in zip(GLOBALS, row) if k in _names(f)})[0] for f in fs)
                      for row in TABLE] for x in xs])
    print('u_kl rows: max |got - want| / max|want| =', np.abs(u - want).max() / np.abs(want).max())
    assert np.allclose(u, want, rtol=1e-5, atol=1e-5 * np.abs(want).max())


# ---- 3. reproducibility ----------------------------------------------------------------------------------------------------------------------
def test_bit_identical_twice(hip_engine_factory):
    N, ref, xs, fs = _expression_system()
    out = []
    for _ in range(2):
        eng = hip_engine_factory()
        _setup(eng, _bare_system(N, *fs), xs, global_table=TABLE, labels=np.array([0, 1, 2]))
        out.append((eng.get_forces(), eng.custom_energies(), eng.custom_cv_values(), eng.compute_energies(), eng.get_forces(), eng.custom_energies()))
    for q in range(6):
        assert np.array_equal(out[0][q], out[1][q]), q                              # two handles
    assert np.array_equal(out[0][0], out[0][4]) and np.array_equal(out[0][1], out[0][5])          # one handle, twice


# ---- 4. end to end -----------------------------------------------------------------------------------------------------------------------
HEAVY = [1, 4, 5, 6, 8, 10, 14, 15, 16, 18]


def _restrained_alanine(k=5000.0):
    al = testsystems.AlanineDipeptideVacuum()
    x0 = np.asarray(al.positions, dtype=np.float64)
    rng = np.random.default_rng(3)
    target = x0.copy()
    target[HEAVY] += rng.normal(0.0, 0.03, (len(HEAVY), 3))                        # a conformation 0.05 nm off the starting one
    f = CustomCVForce('0.5*k_rmsd*v^2'); f.addGlobalParameter('k_rmsd', k)
    f.addCollectiveVariable('v', RMSDForce(target, HEAVY))
    al.system.addForce(f)
    return al, f


def test_minimisation_lowers_the_rmsd_restraint(hip_engine_factory):
    al, f = _restrained_alanine(k=50000.0)
    x = _f32(al.positions)
    eng = hip_engine_factory()
    _setup(eng, al.system, np.tile(x, (2, 1, 1)))
    before, v_before = eng.custom_energies()[:, 0], eng.custom_cv_values()[:, 0]
    eng.minimize(tolerance=1.0, max_iterations=300)
    after, v_after = eng.custom_energies()[:, 0], eng.custom_cv_values()[:, 0]
    y = eng.get_replicas()[0]
    want = np.array([oracle.evaluate(f, _f32(yr))[0] for yr in y])
    print('RMSD restraint: %s -> %s kJ/mol, RMSD %s -> %s nm' % (before, after, v_before, v_after))
    # (the target is a random 0.03 nm displacement of the heavy atoms that the bonds resist: the restraint cannot reach zero)
    assert np.all(after < before) and np.all(v_after < v_before) and np.all(np.abs(after - want) <= 1e-5 * np.abs(want))


class RmsdState(states.GlobalParameterState):
    k_rmsd = states.GlobalParameterState.GlobalParameter('k_rmsd', standard_value=1.0)


def _sampler_run(factory):
    from openmmtools_amd.multistate import MultiStateSampler
    al, f = _restrained_alanine()
    ks = np.array([5000.0, 1000.0, 0.0])
    ts = states.ThermodynamicState(al.system, 300.0)
    sts = states.create_thermodynamic_state_protocol(ts, {'k_rmsd': list(ks)}, composable_states=[RmsdState(k_rmsd=5000.0)])
    move = mcmc.LangevinSplittingDynamicsMove(timestep=1.0 * unit.femtosecond, collision_rate=1.0 / unit.picosecond, n_steps=20,
                                              reassign_velocities=True, splitting='V R O R V')
    engine = factory()
    s = MultiStateSampler(mcmc_moves=move, number_of_iterations=10 ** 9, engine=engine, seed=0xC0FFEE, online_analysis_interval=None)
    s.create(sts, [states.SamplerState(al.positions), states.SamplerState(al.positions)], storage=None)
    s.run(2)
    return s, engine, f, ks, sts


def test_multistate_sampler_over_the_spring_constant(hip_engine_factory):
    s, engine, f, ks, sts = _sampler_run(hip_engine_factory)
    u, x = np.array(s.energy_thermodynamic_states), engine.get_replicas()[0]
    assert u.shape == (2, 3)
    E1 = np.array([oracle.evaluate(f, _f32(xr), dict(k_rmsd=1.0))[0] for xr in x])  # 0.5 v^2: the energy is linear in k
    want = sts[0].beta * (ks[None, :] - ks[0]) * E1[:, None]
    got = u - u[:, :1]
    print('sampler u_kl: max |got - want| / max|want| =', np.abs(got - want).max() / np.abs(want).max())
    assert np.all(E1 > 0.0) and np.allclose(got, want, rtol=1e-5, atol=1e-5 * np.abs(want).max())
    s2 = _sampler_run(hip_engine_factory)[0]
    assert np.array_equal(s.replica_thermodynamic_states, s2.replica_thermodynamic_states)       # the same seed: the same permutation
    assert np.array_equal(np.array(s.energy_thermodynamic_states), np.array(s2.energy_thermodynamic_states))
