"""The device MBAR solver's host side (include/remd_hip_mbar.h, multistate/analysis.py::MBAR(solver='device')), without a GPU:
argument checks, the refusal of a library without the extension, the Gram entry of the covariance algebra, the sampler option,
and the chunked reductions of openmmtools_amd/csrc/mbar.hip restated in Python (tests/mbar_cases.py) against numpy within the
a-priori rounding bounds."""
import os
import numpy as np
import pytest
from openmmtools_amd import testsystems, states, mcmc, unit, _engine
from openmmtools_amd.multistate import ParallelTemperingSampler, MultiStateReporter
from openmmtools_amd.multistate import analysis as an
from oracle_engine import OracleEngine
import oracle
import mbar_cases as mc

CPU_LIB = os.path.join(os.path.dirname(os.path.abspath(oracle.__file__)), '_build', 'libremd_cpu.so')


def test_unknown_solver_is_a_value_error():
    u_kn, N_k, _ = mc.harmonic_case(2, [5, 5])
    with pytest.raises(ValueError, match='solver'):
        an.MBAR(u_kn, N_k, solver='bogus')
    with pytest.raises(ValueError, match='online_analysis_solver'):
        ParallelTemperingSampler(online_analysis_solver='bogus')
    assert an.MBAR(u_kn, N_k).solver == 'numpy'


def test_device_solver_on_the_cpu_port_names_the_header():
    assert os.path.exists(CPU_LIB), 'build() makes oracle/_build/libremd_cpu.so; without it this check would not run'
    u_kn, N_k, _ = mc.harmonic_case(2, [5, 5])
    with pytest.raises(NotImplementedError, match='include/remd_hip_mbar.h'):
        an.MBAR(u_kn, N_k, solver='device', lib_path=CPU_LIB)
    assert set(_engine.MBAR_EXPORTS).isdisjoint(_engine.EXPORTS)


def _theta_of_before(W, N_k):
    """MBAR._theta_of as it was before the Gram entry point"""
    G = W.T @ W
    evals, V = np.linalg.eigh(G)
    evals = np.clip(evals, 0.0, None)
    S = np.sqrt(evals)
    M = np.eye(W.shape[1]) - (S[:, None] * (V.T @ (np.asarray(N_k, dtype=np.float64)[:, None] * V))) * S[None, :]
    return (V * S[None, :]) @ np.linalg.pinv(M, rcond=1e-10) @ (V * S[None, :]).T


@pytest.mark.parametrize('name', ['2x65', '5x1000_alternating', '17x1037'])
def test_theta_through_the_gram_entry_is_the_old_theta_bit_for_bit(name):
    K, N_k = mc.CASES[name]
    u_kn, N_k, _ = mc.harmonic_case(K, N_k)
    mbar = an.MBAR(u_kn, N_k)
    W = np.exp(mbar.log_W_nk)
    old = _theta_of_before(W, N_k)
    assert np.array_equal(an.MBAR._theta_of(W, N_k), old, equal_nan=True)
    assert np.array_equal(an.MBAR._theta_of_gram(W.T @ W, N_k), old, equal_nan=True)
    assert np.array_equal(mbar._theta(), old, equal_nan=True)


def _sampler(tmp_path, **kw):
    ho = testsystems.HarmonicOscillator()
    ts = states.ThermodynamicState(ho.system, 300.0 * unit.kelvin)
    ss = states.SamplerState(ho.positions, box_vectors=ho.system.getDefaultPeriodicBoxVectors())
    move = mcmc.LangevinSplittingDynamicsMove(timestep=2.0 * unit.femtosecond, collision_rate=5.0 / unit.picosecond,
                                              n_steps=10, reassign_velocities=True, splitting='V R O R V')
    s = ParallelTemperingSampler(mcmc_moves=move, number_of_iterations=2, engine=OracleEngine(), seed=11, online_analysis_interval=None, **kw)
    rep = MultiStateReporter(str(tmp_path / 'store'), checkpoint_interval=1)
    s.create(ts, [ss], storage=rep, min_temperature=300.0, max_temperature=600.0, n_temperatures=3)
    return s, rep


def test_sampler_option_round_trips_and_is_not_stored_at_its_default(tmp_path):
    (tmp_path / 'a').mkdir(); (tmp_path / 'b').mkdir()
    s, rep = _sampler(tmp_path / 'a')
    assert s.online_analysis_solver == 'numpy'
    assert 'online_analysis_solver' not in s.options and 'online_analysis_solver' not in rep.read_dict('options')['kwargs']
    s.run()
    back = ParallelTemperingSampler.from_storage(rep, engine=OracleEngine())
    assert back.online_analysis_solver == 'numpy' and back.options == s.options
    s2, rep2 = _sampler(tmp_path / 'b', online_analysis_solver='device')
    assert s2.options['online_analysis_solver'] == 'device' and rep2.read_dict('options')['kwargs']['online_analysis_solver'] == 'device'
    s2.run()
    back2 = ParallelTemperingSampler.from_storage(rep2, engine=OracleEngine())
    assert back2.online_analysis_solver == 'device' and back2.options == s2.options


def test_analyzer_hands_the_solver_to_mbar(tmp_path):
    s, rep = _sampler(tmp_path)
    s.run()
    a = an.MultiStateSamplerAnalyzer(rep, n_equilibration_iterations=0, statistical_inefficiency=1.0, analysis_kwargs={'solver': 'bogus'})
    with pytest.raises(ValueError, match='solver'):
        a.mbar


@pytest.mark.parametrize('name', ['2x65', '5x1000_alternating', '3x9001_three_chunks'])
def test_chunked_max_sum_merge_is_logsumexp_within_the_rounding_bound(name):
    """the row pass (chunks of 4096) and, on the same data, chunks of 64 and of 1000 (a last chunk of one sample at N = 9001)"""
    K, N_k = mc.CASES[name]
    u_kn, N_k, _ = mc.harmonic_case(K, N_k)
    u_kn[0] += 1.0e3                                     # a row far from the others: the maximum matters
    N = u_kn.shape[1]
    rng = np.random.default_rng(1)
    f = rng.normal(size=K)
    sampled = N_k > 0
    log_den = an._logsumexp(f[sampled, None] - u_kn[sampled], axis=0, b=N_k[sampled, None].astype(np.float64))
    a = -u_kn - log_den[None, :]
    ref = an._logsumexp(a, axis=1)
    for chunk in (4096, 64, 1000):
        got = np.array([mc.chunked_logsumexp(a[k], chunk) for k in range(K)])
        assert np.all(np.abs(got - ref) <= mc.lse_bound(N, ref, arg_abs=float(np.max(np.spacing(np.abs(a)))))), (chunk, got - ref)
    # rows with +inf entries, and a row of nothing else: -inf terms add nothing, an empty row gives -inf as _logsumexp does
    b = a.copy()
    b[0, ::3] = -np.inf
    b[-1, :] = -np.inf
    with np.errstate(divide='ignore'):
        ref = an._logsumexp(b, axis=1)
        got = np.array([mc.chunked_logsumexp(b[k], 64) for k in range(K)])
    assert got[-1] == ref[-1] == -np.inf
    assert np.all(np.abs(got[:-1] - ref[:-1]) <= mc.lse_bound(N, ref[:-1], arg_abs=float(np.max(np.spacing(np.abs(a))))))


@pytest.mark.parametrize('name', ['2x65', '17x1037'])
def test_chunked_gram_sum_is_the_gram_matrix_within_the_rounding_bound(name):
    K, N_k = mc.CASES[name]
    u_kn, N_k, _ = mc.harmonic_case(K, N_k)
    mbar = an.MBAR(u_kn, N_k)
    W = np.exp(mbar.log_W_nk)
    N = W.shape[0]
    ref = W.T @ W
    abs_terms = np.abs(W).T @ np.abs(W)
    for chunk in (256, 16):
        got = mc.chunked_gram(W, chunk)
        assert np.all(np.abs(got - ref) <= mc.sum_bound(N, abs_terms, term_rel=mc.U)), chunk
