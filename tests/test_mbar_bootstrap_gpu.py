"""Bootstrap replicates of MBAR on the device (include/remd_hip_mbar.h remd_mbar_bootstrap_*, openmmtools_amd/csrc/mbar_bootstrap.hip,
analysis.MBAR(solver='device', n_bootstraps=B)) against the numpy solver: the multiplicities exactly, each batched pass against its
numpy expression on the same inputs (as tests/test_mbar_gpu.py does for the unweighted passes, with every term scaled by c_n, which
costs one more product: one more unit roundoff per term), and end to end.  Ensembles and bounds: tests/mbar_cases.py.

Measured on an MI355X (the share of each bound that is used is printed by the tests): see the docstrings of the end-to-end tests."""
import functools
import numpy as np
import pytest
from openmmtools_amd.multistate import analysis as an
from openmmtools_amd.multistate import _philox as ph
import mbar_cases as mc

pytestmark = pytest.mark.gpu

U = mc.U
SEED = 0x5EEDB007C0FFEE
B = 4
COUNT_CASES = ['1x1', '2x63', '2x64', '2x65', '3x257_ends_unsampled', '5x1000_alternating', '3x9001_three_chunks', '17x1037']
PASS_CASES = ['2x65', '3x257_ends_unsampled', '5x1000_alternating', '17x1037', '65x2015', '3x9001_three_chunks']
END_CASES = ['2x63', '3x257_ends_unsampled', '5x1000_alternating', '17x1037', '65x2015']


@functools.lru_cache(maxsize=None)
def _case(name):
    K, N_k = mc.CASES[name]
    u_kn, N_k, _ = mc.harmonic_case(K, N_k)
    u_kn.setflags(write=False)
    return u_kn, N_k


def _shuffled(name):
    """(u_kn with its columns shuffled, the state of each column)"""
    u_kn, N_k = _case(name)
    perm = np.random.default_rng(12).permutation(u_kn.shape[1])
    return u_kn[:, perm], np.repeat(np.arange(len(N_k)), N_k)[perm]


@functools.lru_cache(maxsize=None)
def _numpy(name):
    u_kn, N_k = _case(name)
    return an.MBAR(u_kn, N_k, n_bootstraps=B, bootstrap_seed=SEED)


@functools.lru_cache(maxsize=None)
def _device(name):
    u_kn, N_k = _case(name)
    return an.MBAR(u_kn, N_k, solver='device', n_bootstraps=B, bootstrap_seed=SEED)


def _f_bound(f):
    return 1e-10 * max(1.0, float(np.max(np.abs(f))))


@pytest.mark.parametrize('name', COUNT_CASES)
def test_counts_are_the_numpy_counts(name):
    u_kn, N_k = _case(name)
    d = _device(name)._dev
    assert d.bootstrap_max_batch() == min(1024, (1 << 24) // u_kn.shape[1])
    d.bootstrap_draw(SEED, 3, 5)
    got = d.bootstrap_counts(3, 5)
    assert got.dtype == np.uint32 and got.shape == (5, u_kn.shape[1])
    for i in range(5):
        assert np.array_equal(got[i], ph.bootstrap_counts(SEED, 3 + i, N_k))
    assert np.array_equal(d.bootstrap_counts(5, 2), got[2:4])
    u_s, labels = _shuffled(name)
    d.bootstrap_draw(SEED + 1, 0, 3, labels)
    got = d.bootstrap_counts(0, 3)
    for i in range(3):
        assert np.array_equal(got[i], ph.bootstrap_counts(SEED + 1, i, N_k, labels))


@pytest.mark.parametrize('name', PASS_CASES)
def test_each_batched_pass_against_numpy_at_unconverged_f(name):
    u_kn, N_k = _case(name)
    K, N = u_kn.shape
    d = _device(name)._dev
    reps = np.array([6, 4, 5, 8, 7])                                 # out of order, five: a full group of replicates and one more
    d.bootstrap_draw(SEED, 4, 5)
    counts = d.bootstrap_counts(4, 5)[reps - 4].astype(np.float64)    # [nb][N], in the order of reps
    F = np.random.default_rng(5).normal(scale=0.7, size=(reps.size, K))
    s = N_k > 0
    Ks, Nk = int(s.sum()), N_k[s].astype(np.float64)
    ld, phi = d.bootstrap_log_denominator(reps, F)
    f_new = d.bootstrap_self_consistent(reps, F)
    W_sum, WWt, phi2 = d.bootstrap_newton_parts(reps, F)
    assert np.array_equal(phi2, phi)
    rng = np.random.default_rng(6)
    u_ln = np.array(u_kn[[0, K - 1]]) * 1.2 + 0.1
    u_ln[1, 3] = np.inf
    A = np.stack([rng.uniform(0.5, 2.0, N) for _ in range(3)])
    obs = np.array([0, K, K + 1])
    f_l, log_cA = d.bootstrap_rows(reps, F, u_ln, A, obs)
    assert np.array_equal(d.bootstrap_rows(reps, F, u_ln=u_ln)[0], f_l)
    assert np.array_equal(d.bootstrap_rows(reps, F, A_in=A[:1], obs_state=obs[:1])[1], log_cA[:, :1])
    for i in range(reps.size):
        f, c = F[i], counts[i]
        # column pass: log_den does not know the multiplicities; phi does
        ld_np = an._logsumexp(f[s, None] - u_kn[s], axis=0, b=Nk[:, None])
        b_ld = mc.lse_bound(Ks, ld_np, term_rel=9 * U)
        assert np.all(np.abs(ld[i] - ld_np) <= b_ld)
        phi_np = np.dot(c, ld_np) - np.dot(Nk, f[s])
        assert abs(phi[i] - phi_np) <= (mc.sum_bound(N, np.abs(c * ld_np).sum(), term_rel=U) + np.dot(c, b_ld) + 2 * K * U * np.abs(Nk * f[s]).sum()
                                        + 4 * np.spacing(abs(phi_np)))
        # eq. 11 weighted, on the device's log_den; the samples with c_n = 0 do not enter (not even the maximum)
        nz = c > 0
        arg = -u_kn[:, nz] - ld[i][None, nz]
        f_new_np = -an._logsumexp(arg, axis=1, b=c[None, nz])
        assert np.all(np.abs(f_new[i] - f_new_np) <= mc.lse_bound(N, f_new_np, term_rel=9 * U, arg_abs=float(np.max(np.spacing(np.abs(arg))))))
        # the Newton parts
        W = np.exp((f[:, None] - u_kn) - ld[i][None, :])              # [K][N]
        cW = W * c[None, :]
        assert np.all(W_sum[i][~s] == 0) and np.all(WWt[i][~s] == 0) and np.all(WWt[i][:, ~s] == 0)
        assert np.all(np.abs(W_sum[i][s] - cW[s].sum(axis=1)) <= mc.sum_bound(N, cW[s].sum(axis=1), term_rel=9 * U))
        G_np = cW @ W.T
        assert np.array_equal(WWt[i], WWt[i].T)
        assert np.all(np.abs(WWt[i] - G_np)[np.ix_(s, s)] <= mc.sum_bound(N, G_np, term_rel=18 * U)[np.ix_(s, s)])
        # the rows of perturbed states and observables
        arg_l = -u_ln[:, nz] - ld[i][None, nz]
        f_l_np = -an._logsumexp(arg_l, axis=1, b=c[None, nz])
        finite = np.where(np.isfinite(arg_l), arg_l, 0.0)
        assert np.all(np.abs(f_l[i] - f_l_np) <= mc.lse_bound(N, f_l_np, term_rel=9 * U, arg_abs=float(np.max(np.spacing(np.abs(finite))))))
        f_cat, u_cat = np.concatenate([f, f_l[i]]), np.concatenate([u_kn, u_ln], axis=0)
        log_A = np.log(A[:, nz])
        raw = ((f_cat[obs, None] - u_cat[obs][:, nz]) - ld[i][None, nz]) + log_A
        finite = np.where(np.isfinite(raw), raw, 0.0)
        d_arg = float(np.max(4 * np.spacing(np.abs(log_A)) + np.spacing(np.abs(finite))))
        log_cA_np = an._logsumexp(raw, axis=1, b=c[None, nz])
        assert np.all(np.abs(log_cA[i] - log_cA_np) <= mc.lse_bound(N, log_cA_np, term_rel=9 * U, arg_abs=d_arg))


def test_the_wide_and_the_long_case_span_tiles_and_chunks():
    """65 sampled states: two Gram tiles per edge (64 columns each).  9001 samples: three row chunks of 4096, two Gram chunks (the
    weighted Gram pass takes at most 32 chunks of a multiple of 256 samples: ceil(9001 / 32) -> 512) and 36 column workgroups."""
    assert sum(1 for n in mc.CASES['65x2015'][1] if n > 0) == 65 > 64
    d = _device('3x9001_three_chunks')._dev
    col, row, _ = d.chunks(3)
    assert 9001 > 2 * col and 9001 > 2 * row and 9001 > 512


@pytest.mark.parametrize('name', END_CASES)
def test_end_to_end_against_the_numpy_solver(name):
    """f_k_boots within the project's bound between two solves of one problem; the bootstrap errors of the three methods within 1e-8
    relative.  Used on an MI355X: at most 1.9e-5 of the first bound (1.9e-15) and 4.2e-5 of the second (4.2e-13), both at 65x2015."""
    u_kn, N_k = _case(name)
    K, N = u_kn.shape
    dev, ref = _device(name), _numpy(name)
    assert dev.f_k_boots.shape == (B, K) and np.all(dev.f_k_boots[:, 0] == 0.0)
    diff = float(np.max(np.abs(dev.f_k_boots - ref.f_k_boots)))
    print('%s: max |f_boots dev - numpy| %.3e = %.3e of the bound' % (name, diff, diff / _f_bound(ref.f_k_boots)))
    assert diff <= _f_bound(ref.f_k_boots)
    rng = np.random.default_rng(7)
    u_ln = np.array(u_kn[[0, K - 1, K // 2]]) * 0.9 + 0.2
    A = rng.normal(size=N) + 2.0
    worst = 0.0

    def rel(got, want):
        scale = float(np.max(np.abs(want)))
        return float(np.max(np.abs(got - want))) / (scale if scale > 0 else 1.0)
    pairs = [(dev.compute_free_energy_differences(uncertainty_method='bootstrap')[1], ref.compute_free_energy_differences(uncertainty_method='bootstrap')[1]),
             (dev.compute_perturbed_free_energies(u_ln, uncertainty_method='bootstrap')['dDelta_f'],
              ref.compute_perturbed_free_energies(u_ln, uncertainty_method='bootstrap')['dDelta_f'])]
    for u in (None, u_ln):
        for output in ('averages', 'differences'):
            pairs.append((dev.compute_expectations(A, u_kn=u, output=output, uncertainty_method='bootstrap')['sigma'],
                          ref.compute_expectations(A, u_kn=u, output=output, uncertainty_method='bootstrap')['sigma']))
    for got, want in pairs:
        assert got.shape == want.shape and np.all(np.isfinite(got))
        worst = max(worst, rel(got, want))
    print('%s: bootstrap errors differ by %.3e relative = %.3e of the bound' % (name, worst, worst / 1e-8))
    assert worst <= 1e-8
    if N > 1:
        assert np.max(pairs[0][0]) > 0
    const = dev.compute_expectations(np.full(N, 3.5), uncertainty_method='bootstrap')
    assert np.all(const['sigma'] == 0.0) and np.all(const['mu'] == 3.5)


def test_shuffled_sample_states_end_to_end():
    u_s, labels = _shuffled('5x1000_alternating')
    _, N_k = _case('5x1000_alternating')
    dev = an.MBAR(u_s, N_k, solver='device', n_bootstraps=B, bootstrap_seed=SEED, sample_states=labels)
    ref = an.MBAR(u_s, N_k, n_bootstraps=B, bootstrap_seed=SEED, sample_states=labels)
    assert np.max(np.abs(dev.f_k_boots - ref.f_k_boots)) <= _f_bound(ref.f_k_boots)


@pytest.mark.parametrize('name', ['5x1000_alternating', '65x2015'])
def test_a_replicate_does_not_depend_on_its_batch(name):
    m = _device(name)
    d = m._dev
    d.bootstrap_draw(SEED, 0, 5)
    five = m._solve_bootstrap_device(np.arange(5))
    assert np.array_equal(five[:B], m.f_k_boots)
    d.bootstrap_draw(SEED, 2, 1)
    alone = m._solve_bootstrap_device(np.array([2]))
    d.bootstrap_draw(SEED, 0, 2)
    first = m._solve_bootstrap_device(np.array([0, 1]))
    d.bootstrap_draw(SEED, 2, 3)
    rest = m._solve_bootstrap_device(np.array([2, 3, 4]))
    assert np.array_equal(alone[0], five[2]) and np.array_equal(rest[0], five[2])
    assert np.array_equal(np.concatenate([first, rest]), five)
    # and one pass at an unconverged f: replicate 2 first of three, or last of five in another order
    F = np.random.default_rng(8).normal(scale=0.5, size=(5, m.K))
    a = d.bootstrap_newton_parts(np.array([2, 3, 4]), F[[2, 3, 4]])
    d.bootstrap_draw(SEED, 0, 5)
    b = d.bootstrap_newton_parts(np.array([4, 0, 1, 3, 2]), F[[4, 0, 1, 3, 2]])
    for x, y in zip(a, b):
        assert np.array_equal(x[0], y[4])


@pytest.mark.parametrize('name', ['2x65', '17x1037'])
def test_two_runs_are_bit_identical(name):
    u_kn, N_k = _case(name)
    first = _device(name)
    other = an.MBAR(u_kn, N_k, solver='device', n_bootstraps=B, bootstrap_seed=SEED)
    assert np.array_equal(first.f_k_boots, other.f_k_boots)
    A = np.random.default_rng(9).normal(size=u_kn.shape[1])
    for m in (first, other):
        assert np.array_equal(m.compute_expectations(A, uncertainty_method='bootstrap')['sigma'],
                              first.compute_expectations(A, uncertainty_method='bootstrap')['sigma'])
    assert not np.array_equal(an.MBAR(u_kn, N_k, solver='device', n_bootstraps=B, bootstrap_seed=SEED + 1).f_k_boots, first.f_k_boots)


@pytest.mark.parametrize('name', ['5x1000_alternating', '17x1037'])
def test_defaults_leave_the_device_solver_as_it_is(name):
    u_kn, N_k = _case(name)
    plain = an.MBAR(u_kn, N_k, solver='device')
    assert plain.f_k_boots is None
    boot = _device(name)
    assert np.array_equal(plain.f_k, boot.f_k)
    for method in (None, 'svd'):
        assert np.array_equal(plain.compute_free_energy_differences()[1], boot.compute_free_energy_differences(uncertainty_method=method)[1], equal_nan=True)
    with pytest.raises(an.ParameterError, match='without any bootstraps'):
        plain.compute_free_energy_differences(uncertainty_method='bootstrap')


def test_refusals_by_message():
    u_kn, N_k = _case('3x257_ends_unsampled')
    d = _device('3x257_ends_unsampled')._dev
    f = np.zeros((1, 3))
    for nb in (0, -2):
        with pytest.raises(RuntimeError, match='at least 1 is needed'):
            d.bootstrap_draw(SEED, 0, nb)
    with pytest.raises(RuntimeError, match='exceeds the 1024 replicates that may be resident'):
        d.bootstrap_draw(SEED, 0, 1025)
    with pytest.raises(RuntimeError, match='no replicate has been drawn'):             # (a refused draw leaves nothing resident)
        d.bootstrap_self_consistent([0], f)
    labels = np.full(257, 1)
    for bad, text in [(np.where(np.arange(257) == 9, 0, labels), r'sample_states\[9\] = 0 is not a sampled state'),
                      (np.where(np.arange(257) == 9, 3, labels), r'sample_states\[9\] = 3 is not a sampled state'),
                      (np.where(np.arange(257) == 9, -1, labels), r'sample_states\[9\] = -1 is not a sampled state')]:
        with pytest.raises(RuntimeError, match=text):
            d.bootstrap_draw(SEED, 0, 2, bad)
    u2, N2 = _case('2x63')
    d2 = _device('2x63')._dev
    with pytest.raises(RuntimeError, match='names state 1 more often than N_k = 31'):
        d2.bootstrap_draw(SEED, 0, 2, np.repeat([0, 1], [31, 32]))
    d.bootstrap_draw(SEED, 10, 3, labels)
    with pytest.raises(RuntimeError, match='at least 1 is needed'):
        d.bootstrap_self_consistent(np.zeros(0, dtype=np.int32), np.zeros((0, 3)))
    for reps in ([9], [13], [10, 11, 13]):
        with pytest.raises(RuntimeError, match='is outside the drawn range 10 ... 12'):
            d.bootstrap_newton_parts(reps, np.zeros((len(reps), 3)))
    with pytest.raises(RuntimeError, match='outside the drawn range'):
        d.bootstrap_counts(9, 2)
    for bad in (np.nan, np.inf):
        with pytest.raises(RuntimeError, match='f_b of replicate 11 holds a non-finite value'):
            d.bootstrap_log_denominator([10, 11], np.array([[0.0, 0.0, 0.0], [0.0, bad, 0.0]]))
    with pytest.raises(RuntimeError, match='L and I are both 0'):
        d.bootstrap_rows([10], f)
    assert d.bootstrap_self_consistent([12], f).shape == (1, 3)
    assert d.last_ms() >= 0.0
