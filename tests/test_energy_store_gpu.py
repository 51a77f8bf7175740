"""The device energy store (include/remd_hip_energy_store.h, openmmtools_amd/csrc/energy_store.hip, analysis_kwargs=
{'assembly_solver': 'device'}) against the restated definitions of tests/energy_store_oracle.py and the analyzer's numpy methods.

Bounds.  u_n without weights is bit-equal to the oracle (the same additions in the same order) and within R 2^-52 sum_r |term| of the
numpy method (a reordering of R doubles).  The log-sum-exp term L is held to mpmath at 50 digits: the host's ``_logsumexp`` is measured
against it on the same rows and the device gets twice the host's worst deviation plus one unit in the last place of the result (the
two differ only in the rounding of exp and log).  With weights u_n = e + (-w + L) has 2 R + 1 terms, so against the numpy method
(2 R + 1) 2^-52 sum |term| plus the bound on L plus the host's own deviation from mpmath.  u_ln is bit-equal as uint64, N_l and n_ij
are equal.  g of several series: 1e-10 max(1, g), the same last lag, bit-identical across runs and first batches."""
import functools
import itertools
import mpmath
import numpy as np
import pytest
from openmmtools_amd._engine import DeviceEnergyStore, series_inefficiency_multiple
from openmmtools_amd.multistate import analysis as an
import energy_store_oracle as eo
import analysis_device_bits as adb

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52


@functools.lru_cache(maxsize=None)
def _chunks():
    store = DeviceEnergyStore(np.zeros((1, 1, 1)), None, np.zeros((1, 1), dtype=np.int32))
    try:
        return store.chunks()
    finally:
        store.close()


def test_the_work_split_is_the_one_the_shapes_were_chosen_for():
    assert _chunks() == (eo.EFFECTIVE_CHUNK, eo.GATHER_TILE, eo.COUNT_CHUNK, eo.HIST_MAX_STATES)
    assert series_inefficiency_multiple(eo.series(1, 3), first_batch=8)[4] == eo.SERIES_CHUNK


def _selections(T):
    every = np.arange(T, dtype=np.int64)
    return [np.zeros(0, dtype=np.int64), every[-1:], every, every[::-1].copy(), np.array([0, T - 1, 0, 0], dtype=np.int64)]


def _check_store(e, eu, st, label):
    """every pass of one store against the oracle and the numpy methods"""
    T, R, S = e.shape
    store = DeviceEnergyStore(e, eu, st)
    try:
        u = store.effective_energy()
        assert eo.same_bits_or_both_nan(u, eo.effective_energy(e, st)), label
        u_np = eo.host_effective_energy(e, st)
        terms = np.abs(e[np.arange(T)[:, None], np.arange(R)[None, :], st]).sum(axis=1)
        ok = np.isfinite(terms)
        assert np.all(np.abs(u - u_np)[ok] <= R * EPS * terms[ok]), label
        assert np.array_equal(np.isnan(u), np.isnan(u_np)) and np.array_equal(u[np.isinf(u)], u_np[np.isinf(u)]), label
        for iterations in _selections(T):
            u_ln, N_l = store.gather_u_ln(iterations)
            u_host, N_host = eo.host_u_ln(e, eu, st, iterations)
            assert eo.same_bits(u_ln, u_host), (label, iterations)
            assert eo.same_bits(u_ln, eo.gather_u_ln(e, eu, st, iterations)[0]), (label, iterations)
            assert N_l.dtype == N_host.dtype and np.array_equal(N_l, N_host), (label, iterations)
        for t_begin, t_end in [(0, T), (T // 2, T), (0, 1), (T, T), (0, min(2, T))]:
            n_ij = store.transition_counts(t_begin, t_end)
            assert np.array_equal(n_ij, eo.host_transition_counts(st, S, t_begin, t_end)), (label, t_begin, t_end)
            if t_end - t_begin < 2:
                assert not n_ij.any()
        assert store.last_ms() >= 0.0
    finally:
        store.close()


S_VALUES = [1, 2, 24, eo.GATHER_TILE, eo.GATHER_TILE + 1, eo.HIST_MAX_STATES, eo.HIST_MAX_STATES + 1]


@pytest.mark.parametrize('R', [1, 3, 24, 65])
@pytest.mark.parametrize('S', S_VALUES)
def test_every_pass_on_every_shape(R, S):
    """T in 1, 2, 3, 65 (three tiles of selections) and one more than the effective-energy chunk; U in 0, 2; random states (several
    replicas share one) and, for R == S, permutations; non-finite energies in unoccupied and in occupied entries"""
    for T, U in itertools.product([1, 2, 3, 65, eo.EFFECTIVE_CHUNK + 1], [0, 2]):
        kinds = ['shared'] + (['permutation'] if R == S else [])
        for kind in kinds:
            nonfinite = {1: None, 2: 'unoccupied', 3: 'occupied', 65: 'occupied'}.get(T)
            e, eu, st = eo.synthetic_store(T, R, S, U, kind, nonfinite=nonfinite)
            _check_store(e, eu, st, (T, R, S, U, kind))


@pytest.mark.parametrize('S', [2, eo.HIST_MAX_STATES, eo.HIST_MAX_STATES + 1])
@pytest.mark.parametrize('R,extra', [(1, 2), (3, 1)])
def test_counts_one_pair_past_a_chunk_and_one_cell_that_takes_them_all(S, R, extra):
    """(T - 1) R pairs = one more than a workgroup's chunk (R = 1) or the first multiple of R past it; on both sides of the histogram
    threshold; then a store where one cell receives every count"""
    T = -(-eo.COUNT_CHUNK // R) + extra
    assert (T - 1) * R > eo.COUNT_CHUNK >= (T - 2) * R
    for kind in ('shared', 'one_cell'):
        e, eu, st = eo.synthetic_store(T, R, S, 0, kind)
        store = DeviceEnergyStore(e, eu, st)
        n_ij = store.transition_counts(0, T)
        assert np.array_equal(n_ij, eo.host_transition_counts(st, S, 0, T))
        assert n_ij.sum() == (T - 1) * R
        assert np.array_equal(store.transition_counts(5, T - 3), eo.host_transition_counts(st, S, 5, T - 3))
        N_l = store.gather_u_ln(np.arange(T))[1]
        assert np.array_equal(N_l, np.bincount(st.reshape(-1), minlength=S))
        if kind == 'one_cell':
            assert n_ij[-1, -1] == (T - 1) * R and N_l[-1] == T * R
        store.close()


# ---- the log-sum-exp and the SAMS weights -------------------------------------------------------------------------------------------
def _mp_logsumexp(row):
    with mpmath.workdps(50):
        return float(mpmath.log(mpmath.fsum(mpmath.exp(mpmath.mpf(float(a))) for a in row)))


@pytest.mark.parametrize('S', [1, 2, 24, 65])
def test_the_logsumexp_term_against_mpmath(S):
    """one replica that stays in state 0, energies 0 and log_weights[:, 0] = 0: u_n = 0 + (-0 + L) is L itself"""
    T = 65
    lw, f_l = eo.log_weights_case(T, S)
    lw[:, 0] = 0.0
    lw[3, 1:] += 700.0
    lw[4, 1:] -= 800.0
    a = -f_l[None, :] + lw
    ref = np.array([_mp_logsumexp(row) for row in a])
    host = np.array([an._logsumexp(row) for row in a])
    store = DeviceEnergyStore(np.zeros((T, 1, S)), None, np.zeros((T, 1), dtype=np.int32))
    L = store.effective_energy(lw, f_l)
    store.close()
    host_dev, dev_dev = np.abs(host - ref).max(), np.abs(L - ref).max()
    print('S = %d: worst |L - mpmath| host %.3e device %.3e' % (S, host_dev, dev_dev))
    assert np.all(np.abs(L - ref) <= 2.0 * host_dev + np.spacing(np.abs(ref)))


@pytest.mark.parametrize('T,R,S', [(1, 1, 1), (3, 3, 2), (65, 24, 24), (eo.EFFECTIVE_CHUNK + 1, 65, 24), (65, 3, 65)])
def test_effective_energy_with_sams_weights(T, R, S):
    e, _, st = eo.synthetic_store(T, R, S, 0, 'shared')
    lw, f_l = eo.log_weights_case(T, S)
    a = -f_l[None, :] + lw
    ref = np.array([_mp_logsumexp(row) for row in a])
    host_dev = np.abs(np.array([an._logsumexp(row) for row in a]) - ref).max()
    oracle_dev = np.abs(eo.logsumexp_rows(a) - ref).max()
    L_bound = 2.0 * host_dev + np.spacing(np.abs(ref))                   # of the device's L against mpmath
    store = DeviceEnergyStore(e, None, st)
    u = store.effective_energy(lw, f_l)
    plain = store.effective_energy()
    store.close()
    t, r = np.arange(T)[:, None], np.arange(R)[None, :]
    terms = np.abs(e[t, r, st]).sum(axis=1) + np.abs(lw[t, st]).sum(axis=1) + np.abs(ref)
    # against the oracle: the same additions, L aside
    assert eo.same_bits(plain, eo.effective_energy(e, st))
    assert np.all(np.abs(u - eo.effective_energy(e, st, lw, f_l)) <= L_bound + oracle_dev + 3 * EPS * terms)
    # against the analyzer's numpy method
    u_np = eo.host_effective_energy(e, st, lw, f_l)
    print('T R S = %d %d %d: worst |u_dev - u_np| %.3e of a bound of %.3e' % (T, R, S, np.abs(u - u_np).max(),
                                                                           ((2 * R + 1) * EPS * terms + L_bound + host_dev).min()))
    assert np.all(np.abs(u - u_np) <= (2 * R + 1) * EPS * terms + L_bound + host_dev)


def test_weights_that_are_not_finite_propagate():
    e, _, st = eo.synthetic_store(5, 2, 3, 0, 'shared')
    lw, f_l = eo.log_weights_case(5, 3)
    lw[0] = -np.inf                                     # -w = +inf, L = -inf: NaN
    lw[1, :] = [np.inf, 0.0, 0.0]
    st[1] = 1                                           # nobody in the state of infinite weight: L = +inf
    lw[2, 2] = np.nan
    store = DeviceEnergyStore(e, None, st)
    u = store.effective_energy(lw, f_l)
    store.close()
    ref = eo.effective_energy(e, st, lw, f_l)
    assert np.isnan(u[0]) and u[1] == np.inf and np.isnan(u[2]) and np.isfinite(u[3:]).all()
    assert np.array_equal(np.isnan(u), np.isnan(ref)) and np.array_equal(np.isinf(u), np.isinf(ref))


# ---- several series -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [1, 3, 24])
@pytest.mark.parametrize('N', [2, 3, 100, eo.SERIES_CHUNK + 1])
def test_g_of_several_series_matches_the_host(K, N):
    A = eo.series(K, N)
    worst = 0.0
    for fast in (False, True):
        for mintime in (0, 3):
            g_np, _, last_np, _ = eo.inefficiency_multiple(A, fast=fast, mintime=mintime)        # (asserts the condition on every C)
            assert g_np == an.statistical_inefficiency_multiple(A, fast=fast, mintime=mintime)
            runs = [series_inefficiency_multiple(A, fast=fast, mintime=mintime, first_batch=b) for b in (None, None, 1, 3, 64)]
            g, status, last = runs[0][:3]
            assert status == 0 and last == last_np, (fast, mintime, last, last_np)
            assert abs(g - g_np) <= eo.G_RTOL * max(1.0, g_np), (fast, mintime, g, g_np)
            worst = max(worst, abs(g - g_np) / max(1.0, g_np))
            for other in runs[1:]:
                assert np.float64(other[0]).view(np.uint64) == np.float64(g).view(np.uint64) and other[1:3] == (status, last)
            assert an.statistical_inefficiency_multiple(A, fast=fast, mintime=mintime, solver='device') == g
    print('worst |g_dev - g_np| / max(1, g_np) K = %d N = %d: %.3e' % (K, N, worst))


def test_a_slow_walk_stops_several_batches_in():
    rng = np.random.default_rng(11)
    A = np.stack([eo.ar1(4000, 0.99, rng) for _ in range(3)])
    g_np, _, last_np, _ = eo.inefficiency_multiple(A)
    assert last_np > 4 * 64
    for b in (None, 1, 64):
        g, status, last = series_inefficiency_multiple(A, first_batch=b)[:3]
        assert status == 0 and last == last_np and abs(g - g_np) <= eo.G_RTOL * g_np
    assert series_inefficiency_multiple(A, first_batch=8)[3] > 0.0


def test_constant_series_are_status_1_and_the_hosts_value_error():
    A = np.full((3, 50), 2.5)
    g, status, last = series_inefficiency_multiple(A)[:3]
    assert np.isnan(g) and status == 1 and last == 0
    for solver in ('numpy', 'device'):
        with pytest.raises(ValueError, match='sample covariance is zero'):
            an.statistical_inefficiency_multiple(A, solver=solver)


def test_every_result_has_the_bits_recorded_before_the_passes_were_shared():
    """tests/golden/analysis_device_bits.npz (tests/analysis_device_bits.py): g as uint64, status and last lag of every several-series
    case; one case per kernel family of the MBAR passes and the effective energy with SAMS weights, whose scaffolding is shared"""
    adb.assert_same_bits(adb.several_series(eo.SERIES_CHUNK), 'several')
    now = adb.mbar_and_energy_store()
    adb.assert_same_bits({k: v for k, v in now.items() if k.startswith('mbar/')}, 'mbar')
    adb.assert_same_bits({k: v for k, v in now.items() if k.startswith('energy_store/')}, 'energy_store')


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_by_message_leave_the_store_usable():
    e, eu, st = eo.synthetic_store(5, 3, 4, 2, 'shared')
    for shape, message in [((0, 3, 4), 'T must be at least 1'), ((5, 0, 4), 'R must be at least 1'), ((5, 3, 0), 'S must be at least 1')]:
        with pytest.raises(RuntimeError, match=message):
            DeviceEnergyStore(np.zeros(shape), None, np.zeros(shape[:2], dtype=np.int32))
    with pytest.raises(RuntimeError, match='U must be 0 or 2'):
        DeviceEnergyStore(e, np.zeros((5, 3, 1)), st)
    with pytest.raises(RuntimeError, match='U must be 0 or 2'):
        DeviceEnergyStore(e, np.zeros((5, 3, 3)), st)
    bad = st.copy()
    bad[2, 1] = 4
    with pytest.raises(RuntimeError, match=r'states\[2\]\[1\] = 4 is outside 0 ... S - 1 = 3'):
        DeviceEnergyStore(e, eu, bad)
    bad[2, 1] = -1
    with pytest.raises(RuntimeError, match=r'states\[2\]\[1\] = -1 is outside'):
        DeviceEnergyStore(e, eu, bad)
    with pytest.raises(RuntimeError, match='bad device index'):
        DeviceEnergyStore(e, eu, st, device=-1)
    store = DeviceEnergyStore(e, eu, st)
    lw, f_l = eo.log_weights_case(5, 4)
    lib, h = store.lib, store.h
    with pytest.raises(RuntimeError, match='no pass has run'):
        store.last_ms()
    with pytest.raises(RuntimeError, match='log_weights and f_l go together'):
        store.effective_energy(lw, None)
    with pytest.raises(RuntimeError, match='log_weights and f_l go together'):
        store.effective_energy(None, f_l)
    with pytest.raises(RuntimeError, match=r'iterations\[1\] = 5 is outside 0 ... T - 1 = 4'):
        store.gather_u_ln([0, 5])
    with pytest.raises(RuntimeError, match=r'iterations\[0\] = -1 is outside'):
        store.gather_u_ln([-1])
    import ctypes as C
    assert lib.remd_energy_store_gather_u_ln(h, -1, None, None, (C.c_int64 * 6)()) != 0
    assert b'n_sel must not be negative' in lib.remd_last_error(None)
    for t_begin, t_end in [(-1, 3), (0, 6), (4, 3)]:
        with pytest.raises(RuntimeError, match=r'is outside 0 ... T = 5'):
            store.transition_counts(t_begin, t_end)
    # and the store still answers
    assert eo.same_bits(store.effective_energy(), eo.effective_energy(e, st))
    assert eo.same_bits(store.gather_u_ln([4, 0])[0], eo.gather_u_ln(e, eu, st, [4, 0])[0])
    assert np.array_equal(store.transition_counts(0, 5), eo.transition_counts(st, 4, 0, 5))
    store.close()
    A = eo.series(3, 100)
    for args, message in [((np.zeros((0, 5)),), 'K must be at least 1'), ((np.zeros((2, 1)),), 'N must be at least 2'),
                          ((A, False, -1), 'mintime must not be negative')]:
        with pytest.raises(RuntimeError, match=message):
            series_inefficiency_multiple(*args)
    for value in (np.nan, np.inf):
        B = A.copy()
        B[1, 7] = value
        with pytest.raises(RuntimeError, match='non-finite sample 7 of series 1'):
            series_inefficiency_multiple(B)
    with pytest.raises(RuntimeError, match='first_batch must be'):
        series_inefficiency_multiple(A, first_batch=65)
    assert series_inefficiency_multiple(A)[1] == 0


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sams', [False, True])
def test_analyzer_with_every_device_solver_against_the_defaults(tmp_path, sams):
    rep = eo.write_e2e_store(tmp_path / 'store', sams=sams)
    a_np = an.MultiStateSamplerAnalyzer(rep)
    a_dev = an.MultiStateSamplerAnalyzer(rep, analysis_kwargs={'assembly_solver': 'device', 'timeseries_solver': 'device', 'solver': 'device'})
    assert a_np.has_log_weights == sams
    assert a_dev.n_equilibration_iterations == a_np.n_equilibration_iterations
    g_np, g_dev = a_np.statistical_inefficiency, a_dev.statistical_inefficiency
    print('analyzer: n_equilibration %d, g numpy %.9f device %.9f' % (a_np.n_equilibration_iterations, g_np, g_dev))
    assert abs(g_dev - g_np) <= 1e-10 * g_np
    sel_np, sel_dev = a_np._decorrelated_selection(), a_dev._decorrelated_selection()
    assert np.array_equal(sel_dev[3], sel_np[3]) and len(sel_np[3]) > 10
    u_np, N_np = a_np._compute_mbar_decorrelated_energies(sel_np)
    u_dev, N_dev = a_dev._compute_mbar_decorrelated_energies(sel_dev)
    assert eo.same_bits(u_dev, u_np) and np.array_equal(N_dev, N_np) and N_dev.dtype == N_np.dtype
    store = a_dev._energy_store
    assert store is not None and (store.T, store.R, store.S, store.U) == (eo.E2E_T, eo.E2E_R, eo.E2E_S, 2)
    D0, _ = a_np.get_free_energy()
    D, _ = a_dev.get_free_energy()
    assert a_dev.mbar.solver == 'device' and a_dev._energy_store is store
    print('worst |Delta_f_dev - Delta_f_np| %.3e' % np.max(np.abs(D - D0)))
    assert np.max(np.abs(D - D0)) <= 1e-10 * max(1.0, float(np.max(np.abs(a_np.mbar.f_k))))
    m_np, m_dev = a_np.generate_mixing_statistics(), a_dev.generate_mixing_statistics()
    assert np.array_equal(m_dev.transition_matrix, m_np.transition_matrix) and np.array_equal(m_dev.eigenvalues, m_np.eigenvalues)
    assert abs(m_dev.statistical_inefficiency - m_np.statistical_inefficiency) <= eo.G_RTOL * m_np.statistical_inefficiency
    a_dev.clear()
    assert a_dev._energy_store is None and store.h is None
