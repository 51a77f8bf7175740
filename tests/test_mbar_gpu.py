"""MBAR on the device (include/remd_hip_mbar.h, openmmtools_amd/csrc/mbar.hip, analysis.MBAR(solver='device')) against the numpy
solver, pass by pass and end to end.  The ensembles, the Python mirror and the rounding bounds are in tests/mbar_cases.py.

Every pass downstream of the column pass is compared with its numpy expression on the SAME inputs: the numpy side takes the
log denominator (and, for the observable columns, log_cA) the device returned, each of which is checked against numpy first.
A difference is then the summation order plus the 4 ulp of exp / log, which is what the bounds cover.

Covariances.  The pseudo-inverse in _theta_of amplifies the rounding of the Gram matrix by an unknown factor, so the bound on
dDelta_f and on the enthalpy / entropy outputs is 10 x the largest difference measured over the cases below (per output matrix,
max |device - numpy| / max |numpy|), and no looser than 1e-6: measured 5.7e-13 (the 65-state case), hence 5.7e-12."""
import functools
import numpy as np
import pytest
from openmmtools_amd import testsystems, states, mcmc, unit
from openmmtools_amd.multistate import ReplicaExchangeSampler, MultiStateReporter
from openmmtools_amd.multistate import analysis as an
import mbar_cases as mc

pytestmark = pytest.mark.gpu

COV_RTOL = min(10 * 5.7e-13, 1e-6)
U = mc.U


@functools.lru_cache(maxsize=None)
def _case(name):
    K, N_k = mc.CASES[name]
    u_kn, N_k, f_exact = mc.harmonic_case(K, N_k)
    u_kn.setflags(write=False)
    return u_kn, N_k, f_exact


@functools.lru_cache(maxsize=None)
def _numpy(name):
    u_kn, N_k, _ = _case(name)
    return an.MBAR(u_kn, N_k)


@functools.lru_cache(maxsize=None)
def _device(name):
    u_kn, N_k, _ = _case(name)
    return an.MBAR(u_kn, N_k, solver='device')


def _f_bound(f):
    return 1e-10 * max(1.0, float(np.max(np.abs(f))))


def _rel(dev, ref):
    """max |dev - ref| / max |ref| over the entries where ref is finite; the NaN patterns must agree"""
    dev, ref = np.asarray(dev), np.asarray(ref)
    assert np.array_equal(np.isnan(dev), np.isnan(ref)), 'NaN pattern differs'
    ok = np.isfinite(ref)
    if not ok.any():
        return 0.0
    scale = float(np.max(np.abs(ref[ok])))
    return float(np.max(np.abs(dev[ok] - ref[ok]))) / (scale if scale > 0 else 1.0)


def _compare_covariances(dev, ref, label):
    worst = 0.0
    D, dD = dev.compute_free_energy_differences()
    D0, dD0 = ref.compute_free_energy_differences()
    worst = max(worst, _rel(dD, dD0))
    assert np.max(np.abs(D - D0)) <= 2 * _f_bound(ref.f_k)
    r, r0 = dev.compute_entropy_and_enthalpy(), ref.compute_entropy_and_enthalpy()
    for key in ('dDelta_f', 'Delta_u', 'dDelta_u', 'Delta_s', 'dDelta_s'):
        worst = max(worst, _rel(r[key], r0[key]))
    print('covariance difference %s: %.3e' % (label, worst))
    return worst


@pytest.mark.parametrize('name', list(mc.CASES))
def test_free_energies_match_the_numpy_solver(name):
    dev, ref = _device(name), _numpy(name)
    print('max |f_dev - f_np| %s: %.3e' % (name, np.max(np.abs(dev.f_k - ref.f_k))))
    assert np.max(np.abs(dev.f_k - ref.f_k)) <= _f_bound(ref.f_k)
    assert dev.f_k[0] == 0.0


@pytest.mark.parametrize('name', [n for n, (K, N_k) in mc.CASES.items() if sum(N_k) >= 1000])
def test_free_energies_of_the_sampled_states_are_within_three_standard_errors(name):
    _, N_k, f_exact = _case(name)
    dev = _device(name)
    D, dD = dev.compute_free_energy_differences()
    s = np.flatnonzero(N_k > 0)
    exact = f_exact[None, :] - f_exact[:, None]
    i = s[0]
    z = np.abs(D[i, s[1:]] - exact[i, s[1:]]) / dD[i, s[1:]]
    print('largest |error| / standard error %s: %.2f' % (name, z.max()))
    assert np.all(z <= 3.0)


@pytest.mark.parametrize('name', list(mc.CASES))
def test_each_pass_against_numpy_at_an_unconverged_f(name):
    u_kn, N_k, _ = _case(name)
    K, N = u_kn.shape
    d = _device(name)._dev
    f = np.random.default_rng(5).normal(scale=0.7, size=K)
    s = N_k > 0
    Ks, Nk = int(s.sum()), N_k[s].astype(np.float64)
    # column pass: log_den and the objective
    ld, phi = d.log_denominator(f)
    a = f[s, None] - u_kn[s]
    ld_np = an._logsumexp(a, axis=0, b=Nk[:, None])
    b_ld = mc.lse_bound(Ks, ld_np, term_rel=9 * U)
    assert np.all(np.abs(ld - ld_np) <= b_ld)
    phi_np = ld_np.sum() - np.dot(Nk, f[s])
    assert abs(phi - phi_np) <= mc.sum_bound(N, np.abs(ld_np).sum()) + b_ld.sum() + 2 * K * U * np.abs(Nk * f[s]).sum() + 4 * np.spacing(abs(phi_np))
    # eq. 11, on the device's log_den
    arg = -u_kn - ld[None, :]
    f_new = d.self_consistent(f)
    f_new_np = -an._logsumexp(arg, axis=1)
    assert np.all(np.abs(f_new - f_new_np) <= mc.lse_bound(N, f_new_np, arg_abs=float(np.max(np.spacing(np.abs(arg))))))
    # the weights, the Newton parts and the Gram matrices
    log_W = (f[:, None] - u_kn) - ld[None, :]                      # [K][N]
    lw = d.log_weights(f)
    assert lw.shape == (N, K) and np.all(np.abs(lw - log_W.T) <= 4 * np.spacing(np.abs(log_W.T)))
    W = np.exp(log_W)
    W_sum, WWt, phi2 = d.newton_parts(f)
    assert phi2 == phi
    assert np.all(W_sum[~s] == 0) and np.all(WWt[~s] == 0) and np.all(WWt[:, ~s] == 0)
    assert np.all(np.abs(W_sum[s] - W[s].sum(axis=1)) <= mc.sum_bound(N, W[s].sum(axis=1), term_rel=8 * U))
    G_np = W @ W.T                                                  # [K][K]: W^T W of the [N][K] weights
    b_G = mc.sum_bound(N, G_np, term_rel=17 * U)
    assert np.all(np.abs(WWt[np.ix_(s, s)] - G_np[np.ix_(s, s)]) <= b_G[np.ix_(s, s)])
    G = d.gram(f)
    assert np.array_equal(G, G.T) and np.all(np.abs(G - G_np) <= b_G)
    assert np.array_equal(G[np.ix_(s, s)], WWt[np.ix_(s, s)])
    # the observable columns
    G2, log_cA = d.gram(f, with_observable=True)
    assert np.array_equal(G2[:K, :K], G)
    shift = u_kn.min() - 1.0
    log_A = np.log(u_kn - shift)
    raw = log_W + log_A
    d_arg = float(np.max(4 * np.spacing(np.abs(log_A)) + np.spacing(np.abs(raw))))      # a log of another library, then one more sum
    log_cA_np = an._logsumexp(raw, axis=1)
    assert np.all(np.abs(log_cA - log_cA_np) <= mc.lse_bound(N, log_cA_np, arg_abs=d_arg))
    arg2 = raw - log_cA[:, None]
    WA = np.exp(arg2)
    d_arg2 = d_arg + float(np.max(np.spacing(np.abs(arg2))))
    W_aug = np.concatenate([W, WA], axis=0)                         # [2K][N]
    G2_np = W_aug @ W_aug.T
    assert np.array_equal(G2, G2.T)
    assert np.all(np.abs(G2 - G2_np) <= mc.sum_bound(N, G2_np, term_rel=17 * U + 2 * d_arg2))


@pytest.mark.parametrize('name', list(mc.CASES))
def test_covariances_match_numpy(name):
    assert _compare_covariances(_device(name), _numpy(name), name) <= COV_RTOL


@pytest.mark.parametrize('name', ['2x65', '5x1000_alternating', '65x2015'])
def test_results_are_bit_identical_from_run_to_run(name):
    u_kn, N_k, _ = _case(name)
    first = _device(name)
    other = an.MBAR(u_kn, N_k, solver='device')
    assert np.array_equal(first.f_k, other.f_k)
    f = np.random.default_rng(6).normal(size=len(N_k))
    for m in (first._dev, other._dev):
        for call in (lambda: m.log_denominator(f)[0], lambda: m.self_consistent(f), lambda: m.newton_parts(f)[1], lambda: m.gram(f),
                     lambda: m.gram(f, with_observable=True)[0], lambda: m.log_weights(f)):
            assert np.array_equal(call(), call())
    assert np.array_equal(first._dev.gram(f, True)[0], other._dev.gram(f, True)[0])
    assert first._dev.log_denominator(f)[1] == other._dev.log_denominator(f)[1]
    assert np.array_equal(first._solve_device(np.zeros(len(N_k)), 1e-12, 100), first.f_k)
    assert np.array_equal(first.compute_free_energy_differences()[1], other.compute_free_energy_differences()[1], equal_nan=True)


def test_the_long_case_spans_three_chunks_of_every_kernel():
    d = _device('3x9001_three_chunks')._dev
    for C in (3, 6):
        col, row, gram = d.chunks(C)
        assert 9001 > 2 * col and 9001 > 2 * row and 9001 > 2 * gram


def test_create_refuses_by_message():
    from openmmtools_amd._engine import DeviceMBAR, MBAR_MAX_STATES
    u = np.zeros((2, 4))
    for u_kn, N_k, text in [(np.zeros((2, 0)), [0, 0], 'K and N must be at least 1'),
                            (np.zeros((0, 4)), [], 'K and N must be at least 1'),
                            (u, [2, 3], 'sum N_k = 5 is not N = 4'),
                            (u, [5, -1], 'negative or above N'),
                            (np.array([[0.0, np.inf], [0.0, 0.0]]), [1, 1], 'non-finite u_kn in sampled state 0'),
                            (np.array([[0.0, 0.0], [0.0, np.nan]]), [1, 1], 'non-finite u_kn in sampled state 1'),
                            (np.zeros((MBAR_MAX_STATES + 1, 1)), [1] + [0] * MBAR_MAX_STATES, 'exceeds REMD_MBAR_MAX_STATES = 512')]:
        with pytest.raises(RuntimeError, match=text):
            DeviceMBAR(u_kn, N_k)
    for device in (-1, 1 << 20):
        with pytest.raises(RuntimeError, match='bad device index'):
            DeviceMBAR(u, [2, 2], device=device)
    ok = DeviceMBAR(np.array([[0.0, 0.0], [0.0, np.inf]]), [2, 0])                  # +inf in an unsampled row is data
    assert ok.K == 2
    with pytest.raises(RuntimeError, match='no pass has run'):
        ok.last_ms()


# ---- numerical edge cases --------------------------------------------------------------------------------------------------------
def _both(u_kn, N_k, **kw):
    return an.MBAR(u_kn, N_k, solver='device', **kw), an.MBAR(u_kn, N_k, **kw)


def _outcome(fn):
    """what fn returns, or the type of the estimator's own failure (ParameterError, LinAlgError) it raises"""
    try:
        with np.errstate(all='ignore'):
            return fn()
    except (an.ParameterError, np.linalg.LinAlgError) as e:
        return type(e)


@pytest.mark.parametrize('rows', ['one', 'all'])
def test_a_constant_of_1e6_on_one_row_or_on_all(rows):
    """The max subtraction.  The device mirrors numpy's arithmetic, so it shares its limits:

    * on ALL rows numpy raises ParameterError('MBAR did not converge') (every f_k - u_kn carries a rounding of 1e6 x 2^-53 = 1e-10,
      and Newton stalls above relative_tolerance = 1e-12); the device must end the same way;
    * on ONE row both solve.  f_k and dDelta_f are held to numpy on the same input: f_k by the 1e-10 bound, dDelta_f by the issue's
      ceiling of 1e-6, because the weights of that row carry 1e-10 of relative rounding, 1e6 times that of the plain cases, so ten
      times their measured difference scaled by it (1e-5) lies above the ceiling.  The enthalpy and entropy outputs numpy cannot hold
      itself there: its observable is u - (min u - 1) of magnitude 1e6, and its own dDelta_u moves by 1.4e-4 (relative) when the
      constant is added.  They do not depend on the constant (Delta_u after taking it out), so the reference's own error is
      measured here, as numpy(with the constant) against numpy(without), and the device is held to ten times it against the same
      constant-free numpy result."""
    u_kn, N_k, _ = _case('5x1000_alternating')
    u = u_kn.copy()
    offset = np.zeros(5)
    if rows == 'one':
        u[3] += 1.0e6
        offset[3] = 1.0e6
    else:
        u += 1.0e6
    base = _numpy('5x1000_alternating')
    ref = _outcome(lambda: an.MBAR(u, N_k))
    dev = _outcome(lambda: an.MBAR(u, N_k, solver='device'))
    if isinstance(ref, type) or isinstance(dev, type):
        assert dev is ref
        return
    assert np.max(np.abs(dev.f_k - ref.f_k)) <= _f_bound(ref.f_k)
    assert np.max(np.abs((dev.f_k - offset) - base.f_k)) <= 1e-6    # 1e6 costs 2^-53 x 1e6 = 1e-10 per operation
    dD, dD0 = dev.compute_free_energy_differences()[1], ref.compute_free_energy_differences()[1]
    r, r0, rb = dev.compute_entropy_and_enthalpy(), ref.compute_entropy_and_enthalpy(), base.compute_entropy_and_enthalpy()
    print('1e6 on %s: dDelta_f %.3e, dDelta_f (entropy route) %.3e' % (rows, _rel(dD, dD0), _rel(r['dDelta_f'], r0['dDelta_f'])))
    assert _rel(dD, dD0) <= 1e-6 and _rel(r['dDelta_f'], r0['dDelta_f']) <= 1e-6
    shift = offset[None, :] - offset[:, None]
    for key in ('Delta_u', 'dDelta_u', 'Delta_s', 'dDelta_s'):
        take = shift if key == 'Delta_u' else 0.0
        own = _rel(r0[key] - take, rb[key])
        got = _rel(r[key] - take, rb[key])
        print('1e6 on %s: %s numpy against itself %.3e, device %.3e' % (rows, key, own, got))
        assert got <= 10 * own


def test_infinite_energies_in_an_unsampled_row():
    u_kn, N_k, _ = _case('5x1000_alternating')
    u = u_kn.copy()
    u[0, ::7] = np.inf
    u[4, 3] = np.inf
    dev, ref = _both(u, N_k)
    assert np.all(np.isfinite(ref.f_k))
    assert np.max(np.abs(dev.f_k - ref.f_k)) <= _f_bound(ref.f_k)
    D, dD = dev.compute_free_energy_differences()
    D0, dD0 = ref.compute_free_energy_differences()
    assert _rel(dD, dD0) <= COV_RTOL
    # numpy's u-weighted columns of those rows hold NaN (-inf + inf): the same exception type, or NaN in the same entries
    r, r0 = _outcome(dev.compute_entropy_and_enthalpy), _outcome(ref.compute_entropy_and_enthalpy)
    if isinstance(r0, type):
        assert r is r0
    else:
        for key in r0:
            assert np.array_equal(np.isnan(r[key]), np.isnan(r0[key])), key


def test_two_states_without_overlap_end_as_numpy_ends():
    """Centres 12 widths apart.  numpy neither raises nor returns NaN here: it returns f_1 = -9.479 and a dDelta_f of 1.8e6, both set
    by rounding, because without overlap the objective does not depend on f_1 beyond 1e-13 (the Hessian N_1 W_sum - N_1^2 sum W^2
    cancels to nothing).  So the device must end the same way (the same exception type, or values with NaN in the same entries), and
    what can be asked of values that rounding chooses is that they are a solution: the gradient N_k (sum_n W_kn - 1), evaluated by
    numpy at the device's f_k, vanishes within the rounding of that sum, N_k sum W (2 N 2^-53 + 8 x 2^-53 + 3 ulp(max |ln W|))."""
    rng = np.random.default_rng(8)
    x = np.concatenate([rng.normal(0.0, 1.0, 200), rng.normal(12.0, 1.0, 200)])
    u = np.stack([0.5 * x ** 2, 0.5 * (x - 12.0) ** 2])
    N_k = np.array([200, 200])

    def solve(solver):
        m = an.MBAR(u, N_k, solver=solver)
        return m.f_k, m.compute_free_energy_differences()[1]
    ref, dev = _outcome(lambda: solve('numpy')), _outcome(lambda: solve('device'))
    if isinstance(ref, type) or isinstance(dev, type):
        assert dev is ref
        return
    for a, b in zip(dev, ref):
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b))
    print('no overlap: f_1 numpy %.6f device %.6f' % (ref[0][1], dev[0][1]))
    for f in (ref[0], dev[0]):
        log_den = an._logsumexp(f[:, None] - u, axis=0, b=N_k[:, None].astype(np.float64))
        log_W = f[:, None] - u - log_den[None, :]
        W_sum = np.exp(log_W).sum(axis=1)
        bound = N_k * W_sum * ((2 * 400 + 8) * U + 3 * np.spacing(np.max(np.abs(log_W))))
        print('no overlap: gradient', N_k * (W_sum - 1.0), 'bound', bound)
        assert np.all(np.abs(N_k * (W_sum - 1.0)) <= bound)


@pytest.mark.parametrize('sign', [1.0, -1.0])
def test_a_start_far_from_the_solution(sign):
    u_kn, N_k, _ = _case('24x4800')
    f0 = sign * 50.0 * np.arange(24) / 23.0
    dev = an.MBAR(u_kn, N_k, solver='device', initial_f_k=f0)
    assert np.max(np.abs(dev.f_k - _numpy('24x4800').f_k)) <= _f_bound(dev.f_k)


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def _run(path, hip_engine_factory, solver):
    ho = testsystems.HarmonicOscillator()
    thermo = [states.ThermodynamicState(ho.system, T * unit.kelvin) for T in (300.0, 380.0, 480.0, 600.0)]
    ss = states.SamplerState(ho.positions, box_vectors=ho.system.getDefaultPeriodicBoxVectors())
    move = mcmc.LangevinSplittingDynamicsMove(timestep=2.0 * unit.femtosecond, collision_rate=5.0 / unit.picosecond,
                                              n_steps=40, reassign_velocities=True, splitting='V R O R V')
    s = ReplicaExchangeSampler(mcmc_moves=move, number_of_iterations=200, engine=hip_engine_factory(), seed=21,
                               online_analysis_interval=50, online_analysis_minimum_iterations=0, online_analysis_solver=solver)
    rep = MultiStateReporter(str(path), checkpoint_interval=100)
    s.create(thermo, [ss] * 4, storage=rep)
    s.run()
    return s, rep


def test_analyzer_and_online_analysis_on_a_replica_exchange_run(tmp_path, hip_engine_factory):
    s_np, rep_np = _run(tmp_path / 'numpy', hip_engine_factory, 'numpy')
    s_dev, rep_dev = _run(tmp_path / 'device', hip_engine_factory, 'device')
    assert 'online_analysis_solver' not in s_np.options and s_dev.options['online_analysis_solver'] == 'device'
    f_np = rep_np.read_online_analysis_data(None, 'f_k_offline')['f_k_offline']
    f_dev = rep_dev.read_online_analysis_data(None, 'f_k_offline')['f_k_offline']
    assert np.any(f_np != 0)
    assert np.max(np.abs(f_dev - f_np)) <= _f_bound(f_np)
    a_np = an.MultiStateSamplerAnalyzer(rep_np)
    a_dev = an.MultiStateSamplerAnalyzer(rep_np, analysis_kwargs={'solver': 'device'})
    assert a_dev.mbar.solver == 'device' and a_np.mbar.solver == 'numpy'
    D0, dD0 = a_np.get_free_energy()
    D, dD = a_dev.get_free_energy()
    assert np.max(np.abs(D - D0)) <= 2 * _f_bound(a_np.mbar.f_k)
    assert _rel(dD, dD0) <= COV_RTOL
