"""The statistical inefficiency on the device (include/remd_hip_timeseries.h, openmmtools_amd/csrc/timeseries.hip,
analysis.*(solver='device')) against the host loop, origin by origin and end to end.  The series, the conditions every case asserts on
its input (no C within 1e-9 of zero, one distinct maximum of n_effective) and the bound are in tests/timeseries_cases.py.

Bound.  |g_dev - g_np| <= 1e-10 max(1, g_np) and the same last lag: both sides are f64 sums of at most 1e4 terms (1e4 x 2^-53 = 1e-12
a priori); 1e-10 is the margin the MBAR tests use.  Every test prints its worst difference."""
import functools
import numpy as np
import pytest
from openmmtools_amd import testsystems, states, mcmc, unit
from openmmtools_amd._engine import DeviceTimeseries, TIMESERIES_MAX_BATCH, series_inefficiency_multiple
from openmmtools_amd.multistate import ReplicaExchangeSampler, MultiStateReporter
from openmmtools_amd.multistate import analysis as an
import timeseries_cases as tc
import analysis_device_bits as adb

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _chunk():
    ts = DeviceTimeseries([0.0, 1.0])
    try:
        return ts.chunk()
    finally:
        ts.close()


def _sizes():
    return tc.sizes(_chunk())


def _compare(A, origins, label):
    """every origin, both schedules, mintime 0 and 3: the device in one call per setting, numpy origin by origin"""
    ts = DeviceTimeseries(A)
    worst = 0.0
    for fast in (False, True):
        for mintime in (0, 3):
            g, status, last = ts.inefficiency(origins, fast=fast, mintime=mintime)
            assert not status.any()
            for i, t in enumerate(origins):
                g_np, last_np, _ = tc.numpy_loop(A[t:], fast=fast, mintime=mintime)       # (asserts the condition on every C)
                worst = max(worst, abs(g[i] - g_np) / max(1.0, g_np))
                assert last[i] == last_np, (fast, mintime, t, last[i], last_np)
                assert abs(g[i] - g_np) <= tc.G_RTOL * max(1.0, g_np), (fast, mintime, t, g[i], g_np)
    ts.close()
    print('worst |g_dev - g_np| / max(1, g_np) %s: %.3e' % (label, worst))
    return worst


@pytest.mark.parametrize('kind', ['ar05', 'alternating', 'ar05_plus_1e6'])
@pytest.mark.parametrize('which', range(7))
def test_g_and_the_last_lag_match_the_host_loop(kind, which):
    N = _sizes()[which]
    _compare(tc.series(kind, N), tc.origins(N, _chunk()), '%s N = %d' % (kind, N))


def test_the_shapes_cover_every_origin_and_no_lag_at_all():
    chunk = _chunk()
    assert chunk == tc.CHUNK, 'tests/timeseries_cases.py chose its seeds for this chunk: choose them again'
    big = tc.origins(3 * chunk + 7, chunk)
    assert 0 in big and chunk in big and 2 * chunk in big and 3 * chunk in big and 3 * chunk + 5 in big
    assert any(t % chunk for t in big[1:-1])
    ts = DeviceTimeseries(tc.series('ar05', 2))
    g, status, last = ts.inefficiency([0])
    assert (g[0], status[0], last[0]) == (1.0, 0, 0)
    ts = DeviceTimeseries(tc.series('ar05', 5))
    g, status, last = ts.inefficiency([0], mintime=3)
    assert last[0] == 3                                                  # N = 5: lags 1, 2, 3, none of them above mintime


def test_a_slow_series_stops_several_batches_in():
    A = tc.series('ar099', 4000)
    _compare(A, [0, 7, 1000], 'ar099 N = 4000')
    ts = DeviceTimeseries(A)
    g, _, last = ts.inefficiency([0], fast=False)
    print('ar099: g = %.2f, last lag %d' % (g[0], last[0]))
    assert last[0] > 4 * TIMESERIES_MAX_BATCH                            # batches of 8, 16, 32, 64, 64, ...: the sixth or later


def test_the_alternating_series_sums_negative_terms_and_clamps():
    N = 3 * _chunk() + 7
    ts = DeviceTimeseries(tc.series('alternating', N))
    g, _, last = ts.inefficiency([0, 1], mintime=3)
    assert np.all(g == 1.0) and np.all(last >= 3)
    g, _, last = ts.inefficiency([0, 1], mintime=0)
    assert np.all(g == 1.0) and np.all(last == 0)                        # C(1) < 0 and 1 > mintime: nothing is summed


def test_a_constant_suffix_is_a_value_error_as_on_the_host():
    A = np.concatenate([tc.series('ar05', 100), np.full(100, 2.5)])
    ts = DeviceTimeseries(A)
    g, status, _ = ts.inefficiency([0, 50, 100, 150, 198])
    assert status.tolist() == [0, 0, 1, 1, 1]
    assert np.isnan(g[2:]).all() and np.isfinite(g[:2]).all()
    for solver in ('numpy', 'device'):
        with pytest.raises(ValueError, match='sample covariance is zero'):
            an.statistical_inefficiency(A[100:], solver=solver)
        with pytest.raises(ValueError, match='sample covariance is zero'):
            an.get_equilibration_data_per_sample(A, solver=solver)
        with pytest.raises(ValueError, match='sample covariance is zero'):
            an.subsample_correlated_data(A[100:], solver=solver)
        assert an.get_decorrelation_time(A, solver=solver) >= 1.0       # the whole series is not constant


def _ulps32(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(b)).astype(np.float64)))


def test_the_per_sample_scan_matches_the_host():
    A = tc.equilibrating_series(3 * _chunk() + 7)
    ref = an.get_equilibration_data_per_sample(A, fast=True, max_subset=100)
    dev = an.get_equilibration_data_per_sample(A, fast=True, max_subset=100, solver='device')
    tc.assert_distinct_maximum(ref[2])
    assert np.array_equal(dev[0], ref[0])
    for d, r in zip(dev, ref):
        assert d.dtype == r.dtype and d.shape == r.shape
    print('per-sample scan: g_i %.2f ulp, n_effective_i %.2f ulp (float32)' % (_ulps32(dev[1], ref[1]), _ulps32(dev[2], ref[2])))
    assert _ulps32(dev[1], ref[1]) <= 2 and _ulps32(dev[2], ref[2]) <= 2
    e_ref = an.get_equilibration_data(A)
    e_dev = an.get_equilibration_data(A, solver='device')
    assert e_dev[0] == e_ref[0] and 0 < e_ref[0]
    assert _ulps32(e_dev[1], e_ref[1]) <= 2 and _ulps32(e_dev[2], e_ref[2]) <= 2
    # the single-series entries
    tc.numpy_loop(A[e_ref[0]:])
    for fn in (an.statistical_inefficiency, an.get_decorrelation_time):
        g_np, g_dev = fn(A[e_ref[0]:]), fn(A[e_ref[0]:], solver='device')
        assert abs(g_dev - g_np) <= tc.G_RTOL * max(1.0, g_np)
    assert an.subsample_correlated_data(A[e_ref[0]:], solver='device') == an.subsample_correlated_data(A[e_ref[0]:])


def test_the_early_returns_are_the_hosts():
    for A, kw in [(np.full(50, 3.0), {}), (tc.series('ar05', 65), {'max_subset': 1}), (tc.series('ar05', 2), {})]:
        ref = an.get_equilibration_data_per_sample(A, **kw)
        dev = an.get_equilibration_data_per_sample(A, solver='device', **kw)
        for d, r in zip(dev, ref):
            assert np.array_equal(d, r) and d.dtype == r.dtype


def test_results_are_bit_identical_from_run_to_run_and_whatever_shares_the_call():
    N = 3 * _chunk() + 7
    A = tc.equilibrating_series(N)
    hundred = np.floor(np.arange(100) * N / 100).astype(int)
    first, other = DeviceTimeseries(A), DeviceTimeseries(A)
    for fast in (False, True):
        g, _, last = first.inefficiency(hundred, fast=fast)
        g2, _, last2 = first.inefficiency(hundred, fast=fast)
        g3, _, last3 = other.inefficiency(hundred[::-1].copy(), fast=fast)
        assert np.array_equal(g, g2) and np.array_equal(last, last2)
        assert np.array_equal(g, g3[::-1]) and np.array_equal(last, last3[::-1])
        for i in (0, 1, 37, 99):
            alone, _, last_alone = other.inefficiency([hundred[i]], fast=fast)
            assert alone[0] == g[i] and last_alone[0] == last[i]
    assert first.last_ms() > 0.0


def test_every_result_has_the_bits_recorded_before_the_passes_were_shared():
    """tests/golden/analysis_device_bits.npz (tests/analysis_device_bits.py): g as uint64, status and last lag of every single-series case"""
    adb.assert_same_bits(adb.single_series(_chunk()), 'single')


@pytest.mark.parametrize('N', [2, 100, tc.CHUNK + 1, 3 * tc.CHUNK + 7])
def test_one_series_through_the_several_series_entry_is_the_single_series_at_origin_0_to_the_bit(N):
    """K = 1: the normalisations differ by an exact factor 1.0 and the merge order (series, chunk) is the chunk order"""
    A = tc.series('ar05', N)
    ts = DeviceTimeseries(A)
    for fast, mintime in adb.SETTINGS:
        g, status, last = ts.inefficiency([0], fast=fast, mintime=mintime)
        g_k, status_k, last_k = series_inefficiency_multiple(A[None, :], fast=fast, mintime=mintime)[:3]
        assert np.float64(g_k).view(np.uint64) == g.view(np.uint64)[0], (fast, mintime, g_k, g[0])
        assert (status_k, last_k) == (status[0], last[0]), (fast, mintime)
    ts.close()


def test_refusals_by_message():
    with pytest.raises(RuntimeError, match='N must be at least 2'):
        DeviceTimeseries([1.0])
    with pytest.raises(RuntimeError, match='non-finite sample 1'):
        DeviceTimeseries([0.0, np.nan, 1.0])
    with pytest.raises(RuntimeError, match='non-finite sample 2'):
        DeviceTimeseries([0.0, 1.0, np.inf])
    with pytest.raises(RuntimeError, match='bad device index'):
        DeviceTimeseries([0.0, 1.0], device=-1)
    ts = DeviceTimeseries(tc.series('ar05', 65))
    with pytest.raises(RuntimeError, match='no pass has run'):
        ts.last_ms()
    with pytest.raises(RuntimeError, match=r'origin\[1\] = 64 is outside 0 ... N - 2 = 63'):
        ts.inefficiency([0, 64])
    with pytest.raises(RuntimeError, match=r'origin\[0\] = -1 is outside'):
        ts.inefficiency([-1])
    with pytest.raises(RuntimeError, match='S must be at least 1'):
        ts.inefficiency([])
    with pytest.raises(RuntimeError, match='mintime must not be negative'):
        ts.inefficiency([0], mintime=-1)
    g, _, _ = ts.inefficiency([63])                                      # N - 2 is the last origin there is
    assert g[0] == 1.0


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def _f_bound(f):
    return 1e-10 * max(1.0, float(np.max(np.abs(f))))


def test_analyzer_on_a_replica_exchange_run(tmp_path, hip_engine_factory):
    ho = testsystems.HarmonicOscillator()
    thermo = [states.ThermodynamicState(ho.system, T * unit.kelvin) for T in (300.0, 380.0, 480.0, 600.0)]
    ss = states.SamplerState(ho.positions, box_vectors=ho.system.getDefaultPeriodicBoxVectors())
    move = mcmc.LangevinSplittingDynamicsMove(timestep=2.0 * unit.femtosecond, collision_rate=5.0 / unit.picosecond,
                                              n_steps=40, reassign_velocities=True, splitting='V R O R V')
    s = ReplicaExchangeSampler(mcmc_moves=move, number_of_iterations=200, engine=hip_engine_factory(), seed=21, online_analysis_interval=None)
    rep = MultiStateReporter(str(tmp_path / 'store'), checkpoint_interval=100)
    s.create(thermo, [ss] * 4, storage=rep)
    s.run()
    a_np = an.MultiStateSamplerAnalyzer(rep)
    a_dev = an.MultiStateSamplerAnalyzer(rep, analysis_kwargs={'timeseries_solver': 'device'})
    # the conditions on the input, on the series both scan
    e, _, _, st = a_np._read_energies()
    u_n = a_np.get_effective_energy_timeseries(e, st)[1:]
    i_t, _, n_eff = an.get_equilibration_data_per_sample(u_n, max_subset=100)
    tc.assert_distinct_maximum(n_eff)
    for t in i_t:
        tc.numpy_loop(u_n[t:], fast=True)
    assert a_dev.n_equilibration_iterations == a_np.n_equilibration_iterations
    g_np, g_dev = a_np.statistical_inefficiency, a_dev.statistical_inefficiency
    print('analyzer: n_equilibration %d, g numpy %.6f device %.6f' % (a_np.n_equilibration_iterations, g_np, g_dev))
    assert abs(g_dev - g_np) <= 1e-6 * g_np
    assert np.array_equal(a_dev._decorrelated_selection()[3], a_np._decorrelated_selection()[3])
    D0, _ = a_np.get_free_energy()
    D, _ = a_dev.get_free_energy()
    assert a_dev.mbar.solver == 'numpy'
    assert np.max(np.abs(D - D0)) <= _f_bound(a_np.mbar.f_k)
