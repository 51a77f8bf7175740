"""The device timeseries passes' host side (include/remd_hip_timeseries.h, multistate/analysis.py solver='device'), without a GPU:
argument checks, the refusal of a library without the extension, the defaults, the input conditions of every case of the GPU tests,
and the chunked sums of openmmtools_amd/csrc/timeseries.hip restated in Python (tests/timeseries_cases.py) against the host loop."""
import inspect
import os
import numpy as np
import pytest
from openmmtools_amd import _engine
from openmmtools_amd.multistate import analysis as an
import oracle
import timeseries_cases as tc

CPU_LIB = os.path.join(os.path.dirname(os.path.abspath(oracle.__file__)), '_build', 'libremd_cpu.so')
FUNCTIONS = [an.statistical_inefficiency, an.get_decorrelation_time, an.get_equilibration_data_per_sample, an.get_equilibration_data,
             an.subsample_correlated_data]


@pytest.mark.parametrize('fn', FUNCTIONS, ids=lambda f: f.__name__)
def test_unknown_solver_is_a_value_error(fn):
    with pytest.raises(ValueError, match='solver'):
        fn(tc.series('ar05', 65), solver='bogus')


def test_unknown_timeseries_solver_of_the_analyzer_is_a_value_error():
    with pytest.raises(ValueError, match='timeseries_solver'):
        an.MultiStateSamplerAnalyzer(None, analysis_kwargs={'timeseries_solver': 'bogus'})
    an.MultiStateSamplerAnalyzer(None, analysis_kwargs={'timeseries_solver': 'device'})
    an.MultiStateSamplerAnalyzer(None, analysis_kwargs={'timeseries_solver': 'numpy'})


@pytest.mark.parametrize('fn', FUNCTIONS, ids=lambda f: f.__name__)
def test_device_solver_on_the_cpu_port_names_the_header(fn):
    assert os.path.exists(CPU_LIB), 'build() makes oracle/_build/libremd_cpu.so; without it this check would not run'
    with pytest.raises(NotImplementedError, match='include/remd_hip_timeseries.h'):
        fn(tc.series('ar05', 65), solver='device', lib_path=CPU_LIB)


def test_exports_are_an_extension():
    assert set(_engine.TIMESERIES_EXPORTS).isdisjoint(_engine.EXPORTS)
    assert set(_engine.TIMESERIES_EXPORTS).isdisjoint(_engine.MBAR_EXPORTS)
    assert _engine.TIMESERIES_MAX_BATCH == tc.MAX_BATCH


@pytest.mark.parametrize('fn', FUNCTIONS, ids=lambda f: f.__name__)
def test_the_default_solver_is_numpy(fn):
    p = inspect.signature(fn).parameters
    assert p['solver'].default == 'numpy' and p['lib_path'].default is None


def test_the_analyzer_scans_with_numpy_unless_told(monkeypatch):
    seen = []

    def record(series, **kw):
        seen.append(kw)
        return np.array([1]), np.array([1.0], np.float32), np.array([2.0], np.float32)
    monkeypatch.setattr(an, 'get_equilibration_data_per_sample', record)
    energies = np.zeros([1, 1, 8])
    states = np.zeros([1, 8], dtype=int)
    for kwargs, solver in [(None, 'numpy'), ({'timeseries_solver': 'device', 'lib_path': 'x.so'}, 'device')]:
        a = an.MultiStateSamplerAnalyzer(None, analysis_kwargs=kwargs)
        monkeypatch.setattr(a, 'get_effective_energy_timeseries', lambda e, s: np.arange(8.0))
        monkeypatch.setattr(a, '_sams_t0', lambda: None)
        a._get_equilibration_data(energies, states)
        assert seen[-1]['solver'] == solver and seen[-1]['lib_path'] == (kwargs or {}).get('lib_path')


# ---- the conditions on the inputs of the GPU tests, and the restated sums on the same inputs ---------------------------------------
CASES = [(kind, N) for kind in ('ar05', 'alternating', 'ar05_plus_1e6') for N in tc.sizes(tc.CHUNK)] + [('ar099', 4000)]


@pytest.mark.parametrize('kind,N', CASES)
def test_chunked_sums_and_both_lag_schedules_reproduce_the_host_loop(kind, N):
    A = tc.series(kind, N)
    worst = 0.0
    for fast in (False, True):
        for mintime in (0, 3):
            for t in tc.origins(N, tc.CHUNK):
                g_np, last_np, _ = tc.numpy_loop(A[t:], fast=fast, mintime=mintime)       # (asserts the condition on every C)
                g, last = tc.chunked_inefficiency(A, t, fast=fast, mintime=mintime)
                worst = max(worst, abs(g - g_np) / max(1.0, g_np))
                assert last == last_np, (fast, mintime, t)
                assert abs(g - g_np) <= tc.G_RTOL * max(1.0, g_np), (fast, mintime, t, g, g_np)
    print('worst |g_chunked - g_np| / max(1, g_np) %s N = %d: %.3e' % (kind, N, worst))


def test_what_the_cases_are_for():
    """no lag at N = 2; the alternating series sums negative C and clamps; the slow series stops several batches in"""
    g, last, visited = tc.numpy_loop(tc.series('ar05', 2))
    assert (g, last, visited) == (1.0, 0, [])
    g, last, visited = tc.numpy_loop(tc.series('ar05', 5), mintime=3)
    assert len(visited) == 3 and last == 3                                # the mintime rule alone decides: every lag is summed
    g, last, visited = tc.numpy_loop(tc.series('alternating', 3 * tc.CHUNK + 7), mintime=3)
    assert g == 1.0 and visited[0] < 0.0 and last >= 3
    g, last, visited = tc.numpy_loop(tc.series('ar099', 4000), fast=False)
    assert last > 4 * tc.MAX_BATCH and g > 50.0


def test_the_per_sample_series_has_one_maximum():
    N = 3 * tc.CHUNK + 7
    A = tc.equilibrating_series(N)
    for max_subset in (100, 1000):
        i_t, g_i, n_eff = an.get_equilibration_data_per_sample(A, fast=True, max_subset=max_subset)
        tc.assert_distinct_maximum(n_eff)
        assert 0 < n_eff.argmax() < len(n_eff) - 1
    for t in i_t[::100]:
        tc.numpy_loop(A[t:], fast=True)


def test_a_constant_suffix_is_nan_in_the_restated_sums_and_a_value_error_on_the_host():
    A = np.concatenate([tc.series('ar05', 100), np.full(100, 2.5)])
    assert np.isnan(tc.chunked_inefficiency(A, 100)[0]) and np.isfinite(tc.chunked_inefficiency(A, 50)[0])
    with pytest.raises(ValueError, match='sample covariance is zero'):
        an.statistical_inefficiency(A[100:])
    with pytest.raises(ValueError, match='sample covariance is zero'):
        an.get_equilibration_data_per_sample(A)
