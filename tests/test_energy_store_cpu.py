"""The device energy store's host side (include/remd_hip_energy_store.h, analysis_kwargs={'assembly_solver': 'device'},
statistical_inefficiency_multiple(solver='device')) without a GPU: the restated definitions of tests/energy_store_oracle.py against the
analyzer's present numpy methods, the log-sum-exp against mpmath, the options, and the refusal of a library without the extension.

Bounds.  u_n: the oracle adds in ascending r, numpy pairwise, so the two differ by a reordering of R doubles:
|u_oracle - u_numpy| <= R 2^-52 sum_r |term|.  With weights the sum has the R energies, the R log weights and L: (2 R + 1) terms, and the
two log-sum-exp differ by the order of S positive terms (S 2^-52 relative on the sum, that much absolute on its log) and the last
place of the result."""
import inspect
import os
import mpmath
import numpy as np
import pytest
from openmmtools_amd import _engine
from openmmtools_amd.multistate import analysis as an
import oracle
import energy_store_oracle as eo
import timeseries_cases as tc

CPU_LIB = os.path.join(os.path.dirname(os.path.abspath(oracle.__file__)), '_build', 'libremd_cpu.so')
EPS = 2.0 ** -52
SHAPES = [(1, 1, 1, 0), (2, 3, 2, 2), (3, 4, 4, 2), (17, 5, 7, 0), (40, 24, 24, 2)]


def _kind(R, S):
    return 'permutation' if R == S else 'shared'


@pytest.mark.parametrize('T,R,S,U', SHAPES)
def test_effective_energy_of_the_oracle_is_the_hosts_up_to_the_order_of_the_sum(T, R, S, U):
    e, _, st = eo.synthetic_store(T, R, S, U, _kind(R, S))
    u, u_np = eo.effective_energy(e, st), eo.host_effective_energy(e, st)
    terms = np.abs(e[np.arange(T)[:, None], np.arange(R)[None, :], st]).sum(axis=1)
    assert np.all(np.abs(u - u_np) <= R * EPS * terms)
    lw, f_l = eo.log_weights_case(T, S)
    u, u_np = eo.effective_energy(e, st, lw, f_l), eo.host_effective_energy(e, st, lw, f_l)
    L = eo.logsumexp_rows(-f_l[None, :] + lw)
    terms = terms + np.abs(lw[np.arange(T)[:, None], st]).sum(axis=1) + np.abs(L)
    assert np.all(np.abs(u - u_np) <= (2 * R + 1) * EPS * terms + S * EPS + np.spacing(np.abs(L)))


def test_effective_energy_propagates_what_is_not_finite_as_the_host_does():
    e, _, st = eo.synthetic_store(40, 5, 7, 0, nonfinite='occupied')
    u, u_np = eo.effective_energy(e, st), eo.host_effective_energy(e, st)
    assert np.isnan(u).any() and np.isinf(u).any() and np.isfinite(u).any()
    assert np.array_equal(np.isnan(u), np.isnan(u_np)) and np.array_equal(np.isinf(u), np.isinf(u_np))
    assert np.array_equal(np.sign(u[np.isinf(u)]), np.sign(u_np[np.isinf(u)]))
    e, _, st = eo.synthetic_store(40, 5, 7, 0, nonfinite='unoccupied')
    assert not np.isfinite(e).all() and np.isfinite(eo.effective_energy(e, st)).all()


@pytest.mark.parametrize('T,R,S,U', SHAPES)
@pytest.mark.parametrize('nonfinite', [None, 'occupied'])
def test_u_ln_and_N_l_of_the_oracle_are_the_hosts(T, R, S, U, nonfinite):
    e, eu, st = eo.synthetic_store(T, R, S, U, _kind(R, S), nonfinite=nonfinite)
    for iterations in ([], [T - 1], list(range(T)), list(range(T))[::-1], [0, T - 1, 0, 0]):
        iterations = np.array(iterations, dtype=np.int64)
        u_ln, N_l = eo.gather_u_ln(e, eu, st, iterations)
        u_np, N_np = eo.host_u_ln(e, eu, st, iterations)
        assert np.array_equal(u_ln, u_np, equal_nan=True) and np.array_equal(N_l, N_np)
        assert N_l.sum() == R * len(iterations) and (U == 0 or N_l[0] == N_l[-1] == 0)


@pytest.mark.parametrize('T,R,S,U', SHAPES)
def test_transition_counts_of_the_oracle_are_the_host_loops(T, R, S, U):
    for kind in (_kind(R, S), 'one_cell'):
        st = eo.synthetic_store(T, R, S, U, kind)[2]
        for t_begin, t_end in [(0, T), (T // 2, T), (0, 1), (T, T), (0, min(2, T))]:
            n_ij = eo.transition_counts(st, S, t_begin, t_end)
            assert np.array_equal(n_ij, eo.host_transition_counts(st, S, t_begin, t_end))
            assert n_ij.sum() == max(0, t_end - 1 - t_begin) * R
    assert n_ij[-1, -1] == n_ij.sum()                                     # 'one_cell': one cell receives every count


@pytest.mark.parametrize('K', [1, 3, 24])
@pytest.mark.parametrize('N', [2, 3, 100, eo.SERIES_CHUNK + 1])
def test_several_series_of_the_oracle_are_the_hosts(K, N):
    A = eo.series(K, N)
    for fast in (False, True):
        for mintime in (0, 3):
            g, status, last, visited = eo.inefficiency_multiple(A, fast=fast, mintime=mintime)     # (asserts the condition on every C)
            assert status == 0 and g == an.statistical_inefficiency_multiple(A, fast=fast, mintime=mintime)
            assert (last == 0 and not visited) if N == 2 else len(visited) >= 1
    if K == 1 and N > 3:
        assert abs(g - an.statistical_inefficiency(A[0], fast=True, mintime=3)) <= 1e-12 * g      # one series: the single-series g


def test_a_constant_set_of_series_has_status_1_and_is_the_hosts_value_error():
    A = np.full((3, 50), 2.5)
    g, status, last, _ = eo.inefficiency_multiple(A)
    assert np.isnan(g) and status == 1 and last == 0
    with pytest.raises(ValueError, match='sample covariance is zero'):
        an.statistical_inefficiency_multiple(A)


def _mp_logsumexp(row):
    with mpmath.workdps(50):
        return float(mpmath.log(mpmath.fsum(mpmath.exp(mpmath.mpf(float(a))) for a in row)))


@pytest.mark.parametrize('S', [1, 2, 24, 65])
def test_logsumexp_of_the_oracle_against_mpmath(S):
    lw, f_l = eo.log_weights_case(40, S)
    a = -f_l[None, :] + lw
    a[3] += 700.0                                                         # exp overflows without the shift
    a[4] -= 800.0                                                         # and underflows
    ref = np.array([_mp_logsumexp(row) for row in a])
    got = eo.logsumexp_rows(a)
    host = np.array([an._logsumexp(row) for row in a])
    # S terms of relative error 2^-52 each in exp and in the running sum, the log of a sum >= 1 (the largest term is exp(0)), the last
    # place of the result
    bound = 2 * S * EPS + np.spacing(np.abs(ref))
    print('S = %d: oracle %.3e, host %.3e (worst |L - mpmath|)' % (S, np.abs(got - ref).max(), np.abs(host - ref).max()))
    assert np.all(np.abs(got - ref) <= bound) and np.all(np.abs(host - ref) <= bound)
    assert eo.logsumexp_rows(np.array([[-np.inf, -np.inf]]))[0] == -np.inf
    assert eo.logsumexp_rows(np.array([[np.inf, 0.0]]))[0] == np.inf
    assert np.isnan(eo.logsumexp_rows(np.array([[np.nan, 0.0]]))[0])


# ---- options, signatures, refusals ------------------------------------------------------------------------------------------------
def test_unknown_assembly_solver_of_the_analyzer_is_a_value_error():
    with pytest.raises(ValueError, match='assembly_solver'):
        an.MultiStateSamplerAnalyzer(None, analysis_kwargs={'assembly_solver': 'bogus'})
    assert an.MultiStateSamplerAnalyzer(None, analysis_kwargs={'assembly_solver': 'device'})._assembles_on_device
    assert not an.MultiStateSamplerAnalyzer(None, analysis_kwargs={'assembly_solver': 'numpy'})._assembles_on_device
    assert not an.MultiStateSamplerAnalyzer(None)._assembles_on_device


def test_the_default_solver_of_several_series_is_numpy():
    p = inspect.signature(an.statistical_inefficiency_multiple).parameters
    assert list(p) == ['A_kn', 'fast', 'mintime', 'solver', 'device', 'lib_path']
    assert p['solver'].default == 'numpy' and p['device'].default == 0 and p['lib_path'].default is None
    with pytest.raises(ValueError, match='solver'):
        an.statistical_inefficiency_multiple(eo.series(3, 100), solver='bogus')


def test_ragged_series_on_the_device_are_a_value_error():
    A = eo.series(3, 100)
    with pytest.raises(ValueError, match='one common length'):
        an.statistical_inefficiency_multiple([A[0], A[1][:90], A[2]], solver='device')
    assert an.statistical_inefficiency_multiple([A[0], A[1][:90], A[2]]) >= 1.0


def test_exports_are_an_extension():
    for other in (_engine.EXPORTS, _engine.MBAR_EXPORTS, _engine.TIMESERIES_EXPORTS):
        assert set(_engine.ENERGY_STORE_EXPORTS).isdisjoint(other)
    assert _engine.SERIES_MAX_BATCH == 64


def test_both_device_paths_on_the_cpu_port_name_the_header():
    assert os.path.exists(CPU_LIB), 'build() makes oracle/_build/libremd_cpu.so; without it this check would not run'
    with pytest.raises(NotImplementedError, match='include/remd_hip_energy_store.h'):
        an.statistical_inefficiency_multiple(eo.series(3, 100), solver='device', lib_path=CPU_LIB)
    e, eu, st = eo.synthetic_store(3, 4, 4, 2, 'permutation')
    with pytest.raises(NotImplementedError, match='include/remd_hip_energy_store.h'):
        _engine.DeviceEnergyStore(e, eu, st, lib_path=CPU_LIB)
    a = eo.numpy_analyzer(e, eu, st)
    a._kwargs.update(assembly_solver='device', lib_path=CPU_LIB)
    a._read_records = lambda: (e, eu, None, st)
    with pytest.raises(NotImplementedError, match='include/remd_hip_energy_store.h'):
        a.get_effective_energy_timeseries(np.moveaxis(e, 0, -1), np.moveaxis(st, 0, -1))
    with pytest.raises(NotImplementedError, match='include/remd_hip_energy_store.h'):
        a.generate_mixing_statistics(number_equilibrated=0)


def test_the_numpy_analyzer_never_makes_a_store(tmp_path):
    rep = eo.write_e2e_store(tmp_path / 'store', sams=False)
    a = an.MultiStateSamplerAnalyzer(rep)
    a.get_free_energy()
    a.generate_mixing_statistics()
    assert a._energy_store is None
    a.clear()


# ---- the conditions on the inputs of the end-to-end GPU test ------------------------------------------------------------------------
@pytest.mark.parametrize('sams', [False, True])
def test_the_end_to_end_store_meets_the_conditions_of_the_scan(tmp_path, sams):
    """the host scan finds a variance at every origin, no C within 1e-9 of zero, one distinct maximum of n_effective; the state walk
    meets the condition on C too; with SAMS several replicas share a state and the weights are found"""
    rep = eo.write_e2e_store(tmp_path / 'store', sams=sams)
    a = an.MultiStateSamplerAnalyzer(rep)
    assert a.has_log_weights == sams
    e, eu, _, st = a._read_energies()
    assert e.shape == (eo.E2E_R, eo.E2E_S, eo.E2E_T) and eu.shape == (eo.E2E_R, 2, eo.E2E_T)
    rows_are_permutations = all(sorted(row) == list(range(eo.E2E_S)) for row in st.T)
    assert rows_are_permutations != sams
    u_n = a.get_effective_energy_timeseries(e, st)[1:]
    i_t, _, n_eff = an.get_equilibration_data_per_sample(u_n, max_subset=100)           # (raises where a suffix has no variance)
    tc.assert_distinct_maximum(n_eff)
    for t in i_t:
        tc.numpy_loop(u_n[t:], fast=True)
    n_eq = a.n_equilibration_iterations
    assert 0 < n_eq < eo.E2E_T // 2
    eo.inefficiency_multiple(np.transpose(st.T[n_eq:]).astype(np.float64))
    D, dD = a.get_free_energy()
    assert np.all(np.isfinite(D)) and D.shape == (eo.E2E_S + 2, eo.E2E_S + 2)
