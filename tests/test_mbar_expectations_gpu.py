"""The augmented Gram pass on the device (remd_mbar_augmented_gram of include/remd_hip_mbar.h, openmmtools_amd/csrc/mbar.hip) and the
MBAR methods built on it (compute_perturbed_free_energies, compute_expectations, compute_multiple_expectations, compute_overlap,
compute_effective_sample_number with solver='device') against the numpy path of the same class on the same input.

Bounds, none of them new: f_l, log_cA and mu are held to the 1e-10 the README states for the device solver's free energies, in the
form tests/test_mbar_gpu.py gives it (_f_bound: 1e-10 x max(1, max |value|)); dDelta_f, sigma, the overlap matrix and the effective
sample numbers to COV_RTOL of tests/test_mbar_gpu.py line 21 (min(10 x 5.7e-13, 1e-6) = 5.7e-12, as max |device - numpy| /
max |numpy| per output, _rel there)."""
import functools
import numpy as np
import pytest
from openmmtools_amd.multistate import analysis as an

pytestmark = pytest.mark.gpu

COV_RTOL = min(10 * 5.7e-13, 1e-6)          # tests/test_mbar_gpu.py:21
L_OF = lambda K: (0, 1, K + 3)
I_OF = (0, 1, 4)


def _f_bound(v):
    return 1e-10 * max(1.0, float(np.max(np.abs(v))))


def _rel(dev, ref):
    """max |dev - ref| / max |ref| over the entries where ref is finite; the NaN patterns must agree (tests/test_mbar_gpu.py)"""
    dev, ref = np.asarray(dev), np.asarray(ref)
    assert dev.shape == ref.shape
    assert np.array_equal(np.isnan(dev), np.isnan(ref)), 'NaN pattern differs'
    ok = np.isfinite(ref)
    if not ok.any():
        return 0.0
    scale = float(np.max(np.abs(ref[ok])))
    return float(np.max(np.abs(dev[ok] - ref[ok]))) / (scale if scale > 0 else 1.0)


@functools.lru_cache(maxsize=None)
def _chunk_sizes():
    """(column, row, Gram) samples per workgroup as the library reports them.  The Gram chunk is the same for every C and N of this
    file (its floor); each problem below checks that against its own object."""
    from openmmtools_amd._engine import DeviceMBAR
    d = DeviceMBAR(np.zeros((1, 1)), [1])
    try:
        return d.chunks(8)
    finally:
        d.close()


def _n_samples(label):
    col, row, gram = _chunk_sizes()
    return {'gram-1': gram - 1, 'gram+1': gram + 1, 'row-1': row - 1, 'row+1': row + 1, 'three rows': 2 * row + 1}[label]


def _split(N, K, unsampled=()):
    """N_k: N samples over the sampled states of K, unevenly"""
    s = [k for k in range(K) if k not in unsampled]
    w = np.arange(1, len(s) + 1, dtype=np.float64)
    n = np.floor(N * w / w.sum()).astype(np.int64)
    n[0] += N - n.sum()
    N_k = np.zeros(K, dtype=np.int64)
    N_k[s] = n
    return N_k


@functools.lru_cache(maxsize=None)
def _problem(K, N, unsampled=(), L_max=8):
    """(x, u_kn, N_k, u_ln [L_max][N], numpy MBAR, device MBAR) of 1-D oscillators; computed once and left unchanged"""
    N_k = _split(N, K, unsampled)
    k = np.arange(K)
    c, s = 2.0 * k / K, 1.0 + 0.5 * k / K
    rng = np.random.default_rng(4100 + 7 * K + N)
    x = np.concatenate([rng.normal(c[i], s[i], size=int(N_k[i])) for i in range(K)])
    u_kn = (x[None, :] - c[:, None]) ** 2 / (2.0 * s[:, None] ** 2)
    l = np.arange(L_max)
    cl, sl = 0.1 + 1.9 * l / L_max, 1.05 + 0.4 * l / L_max
    u_ln = (x[None, :] - cl[:, None]) ** 2 / (2.0 * sl[:, None] ** 2)
    for a in (x, u_kn, u_ln):
        a.setflags(write=False)
    return x, u_kn, N_k, u_ln, an.MBAR(u_kn, N_k), an.MBAR(u_kn, N_k, solver='device')


def _observables(x, I):
    return np.stack([x, x * x, np.cos(x), -np.abs(x) - 3.0][:I])


def _compare_pass(ref, dev, u_ln, A, obs):
    """one call of the device against the numpy expression at the numpy solver's f_k; returns the measured differences"""
    A_in = None if A is None else A - (A.min() - 1.0)
    f_l0, log_cA0, G0 = ref._augmented_gram(u_ln, A_in, obs)
    f_l, log_cA, G = dev._dev.augmented_gram(ref.f_k, u_ln, A_in, obs)
    K, L, I = ref.K, len(f_l0), len(log_cA0)
    assert f_l.shape == (L,) and log_cA.shape == (I,) and G.shape == (K + L + I,) * 2
    assert np.array_equal(G, G.T)
    out = [0.0, 0.0, 0.0]
    if L:
        out[0] = float(np.max(np.abs(f_l - f_l0)))
        assert out[0] <= _f_bound(f_l0)
    if I:
        out[1] = float(np.max(np.abs(log_cA - log_cA0)))
        assert out[1] <= _f_bound(log_cA0)
    N_ext = np.concatenate([ref.N_k, np.zeros(L + I, dtype=np.int64)])
    err0 = an.MBAR._error_of_differences(an.MBAR._theta_of_gram(G0, N_ext))
    err = an.MBAR._error_of_differences(an.MBAR._theta_of_gram(G, N_ext))
    out[2] = _rel(err, err0)
    assert out[2] <= COV_RTOL
    return out


@pytest.mark.parametrize('label', ['gram-1', 'gram+1', 'row-1', 'row+1', 'three rows'])
@pytest.mark.parametrize('K', [1, 2, 5])
def test_the_pass_at_chunk_edges_for_every_count_of_states_and_observables(K, label):
    N = _n_samples(label)
    x, u_kn, N_k, u_ln, ref, dev = _problem(K, N)
    col, row, gram = _chunk_sizes()
    worst = [0.0, 0.0, 0.0]
    for L in L_OF(K):
        for I in I_OF:
            if L == 0 and I == 0:
                continue                                            # refused: see test_refusals_by_message
            assert dev._dev.chunks(K + L + I) == (col, row, gram)
            obs = (3 * np.arange(I) + 1) % (K + L) if I else None   # stored and perturbed columns both
            got = _compare_pass(ref, dev, u_ln[:L] if L else None, _observables(x, I) if I else None, obs)
            worst = [max(a, b) for a, b in zip(worst, got)]
    if label == 'three rows':
        assert N > 2 * row and N > 2 * gram and N > 2 * col
    print('K = %d, N = %d: f_l %.2e, log_cA %.2e, errors of differences %.2e' % ((K, N) + tuple(worst)))


def test_more_columns_than_one_gram_tile():
    """145 columns: three rows of the 64-column tiles of mbar.hip (MBAR_TILE), the last one 17 wide, diagonal and off-diagonal tiles"""
    K, N = 5, 600
    x, u_kn, N_k, u_ln, ref, dev = _problem(K, N, L_max=70)
    A = np.stack([np.cos(0.05 * (i + 1) * x) + 0.01 * i * x for i in range(70)])
    obs = (3 * np.arange(70) + 1) % (K + 70)
    A_in = A - (A.min() - 1.0)
    f_l0, log_cA0, G0 = ref._augmented_gram(u_ln, A_in, obs)
    f_l, log_cA, G = dev._dev.augmented_gram(ref.f_k, u_ln, A_in, obs)
    assert G.shape == (145, 145) and np.array_equal(G, G.T)
    assert np.max(np.abs(f_l - f_l0)) <= _f_bound(f_l0) and np.max(np.abs(log_cA - log_cA0)) <= _f_bound(log_cA0)
    # Entry by entry, a priori (u = 2^-53; every term is positive, so sum |terms| = G0).  A sum of N terms taken in another order:
    # 2 N u.  Each of the two factors of a term is an exp whose argument carries f_l (another order of an N-term sum: 2 N u, as
    # tests/mbar_cases.py lse_bound) and, for an observable on a perturbed column, log_cA (2 N u of its own sum plus twice the f_l
    # in its arguments: 6 N u): 8 N u per factor, 16 N u per term.  The exp, log and subtraction ulps are covered by 512 u.
    bound = (18 * N + 512) * 2.0 ** -53 * G0
    print('145 columns: largest |G - G0| / bound %.3f' % np.max(np.abs(G - G0) / bound))
    assert np.all(np.abs(G - G0) <= bound)


@pytest.mark.parametrize('K,unsampled', [(2, ()), (5, (0, 3))])
def test_public_methods_match_the_numpy_path(K, unsampled):
    """every new method with solver='device' against solver='numpy': sampled and perturbed states, both outputs, state-dependent
    observables, an unsampled state among the K, a +inf entry and a constant observable"""
    N = _n_samples('gram+1')
    x, u_kn, N_k, u_ln, ref, dev = _problem(K, N, unsampled)
    assert np.max(np.abs(dev.f_k - ref.f_k)) <= _f_bound(ref.f_k)
    u_inf = u_ln[:K + 3].copy()
    u_inf[1, ::9] = np.inf
    for u in (u_ln[:1], u_ln[:K + 3], u_inf):
        r, r0 = dev.compute_perturbed_free_energies(u), ref.compute_perturbed_free_energies(u)
        assert np.max(np.abs(r['Delta_f'] - r0['Delta_f'])) <= 2 * _f_bound(r0['Delta_f'])
        assert _rel(r['dDelta_f'], r0['dDelta_f']) <= COV_RTOL
    worst, worst_mu = 0.0, 0.0
    for A in (x, -np.abs(x) - 3.0):
        for u in (None, u_ln[:K + 3], u_inf):
            for output in ('averages', 'differences'):
                r, r0 = dev.compute_expectations(A, u, output=output), ref.compute_expectations(A, u, output=output)
                if output == 'averages':
                    worst_mu = max(worst_mu, _rel(r['mu'], r0['mu']))
                    assert np.max(np.abs(r['mu'] - r0['mu'])) <= _f_bound(r0['mu'])
                else:                                               # a difference of two averages: twice, as Delta_f above
                    assert np.max(np.abs(r['mu'] - r0['mu'])) <= 2 * _f_bound(r0['mu'])
                worst = max(worst, _rel(r['sigma'], r0['sigma']))
    A_kn = np.stack([np.cos((k + 1) * x) for k in range(K)])
    r, r0 = dev.compute_expectations(A_kn, state_dependent=True), ref.compute_expectations(A_kn, state_dependent=True)
    assert np.max(np.abs(r['mu'] - r0['mu'])) <= _f_bound(r0['mu'])
    worst_mu = max(worst_mu, _rel(r['mu'], r0['mu']))
    worst = max(worst, _rel(r['sigma'], r0['sigma']))
    A_in = _observables(x, 4)
    r, r0 = (m.compute_multiple_expectations(A_in, u_inf[1], compute_covariance=True) for m in (dev, ref))
    assert np.max(np.abs(r['mu'] - r0['mu'])) <= _f_bound(r0['mu'])
    worst_mu = max(worst_mu, _rel(r['mu'], r0['mu']))
    worst = max(worst, _rel(r['sigma'], r0['sigma']), _rel(r['covariances'], r0['covariances']))
    print('K = %d: mu %.2e (relative to the largest), sigma and covariances %.2e' % (K, worst_mu, worst))
    assert worst <= COV_RTOL
    assert worst_mu <= 1e-10                            # the 1e-10 as a relative bound too, where every |mu| is below 1
    # a constant observable: exactly 0, not NaN, on the device too
    for u in (None, u_inf):
        r = dev.compute_expectations(np.full(N, -2.5), u)
        assert np.all(r['mu'] == -2.5) and np.all(r['sigma'] == 0.0)
    r = dev.compute_multiple_expectations(np.stack([x, np.full(N, 4.0)]), u_ln[2], compute_covariance=True)
    assert r['sigma'][1] == 0.0 and r['sigma'][0] > 0.0 and np.all(r['covariances'][1] == 0.0)
    # overlap and effective sample numbers from the device's Gram matrix
    o, o0 = dev.compute_overlap(), ref.compute_overlap()
    assert _rel(o['matrix'], o0['matrix']) <= COV_RTOL and _rel(o['eigenvalues'], o0['eigenvalues']) <= COV_RTOL
    assert abs(o['scalar'] - o0['scalar']) <= COV_RTOL
    assert np.max(np.abs(o['matrix'].sum(axis=1) - 1.0)) <= 1e-12
    assert _rel(dev.compute_effective_sample_number()['n_eff'], ref.compute_effective_sample_number()['n_eff']) <= COV_RTOL


def test_two_calls_and_two_objects_give_identical_bits():
    K, N = 5, _n_samples('three rows')
    x, u_kn, N_k, u_ln, ref, dev = _problem(K, N)
    other = an.MBAR(u_kn, N_k, solver='device')
    A_in = _observables(x, 4)
    A_in = A_in - (A_in.min() - 1.0)
    obs = np.array([0, 6, 4, 12])
    f = np.random.default_rng(9).normal(scale=0.5, size=K)
    first = dev._dev.augmented_gram(f, u_ln, A_in, obs)
    for m in (dev._dev, other._dev, dev._dev):
        again = m.augmented_gram(f, u_ln, A_in, obs)
        assert all(np.array_equal(a, b) for a, b in zip(first, again))
    a, b = dev.compute_expectations(x, u_ln, output='differences'), other.compute_expectations(x, u_ln, output='differences')
    assert np.array_equal(a['mu'], b['mu']) and np.array_equal(a['sigma'], b['sigma'], equal_nan=True)
    # the plain columns are those of remd_mbar_gram, to the bit: same arithmetic, same chunks wherever the chunk size is the same
    G = dev._dev.gram(f)
    assert dev._dev.chunks(K) == dev._dev.chunks(K + 8 + 4)
    assert np.array_equal(first[2][:K, :K], G)
    other._dev.close()


def test_refusals_by_message():
    from openmmtools_amd._engine import MBAR_MAX_STATES, _dp
    K, N = 2, 8
    x, u_kn, N_k, u_ln, ref, dev = _problem(K, N)
    d = dev._dev
    f = ref.f_k
    ones = np.ones((1, N))
    with pytest.raises(RuntimeError, match='L and I are both 0'):
        d.augmented_gram(f)
    with pytest.raises(RuntimeError, match=r'C = K \+ L \+ I = %d exceeds 2 x REMD_MBAR_MAX_STATES = %d' % (2 * MBAR_MAX_STATES + 1, 2 * MBAR_MAX_STATES)):
        d.augmented_gram(f, u_ln=np.zeros((2 * MBAR_MAX_STATES - K, N)), A_in=ones, obs_state=[0])
    for obs in (-1, K + 1):
        with pytest.raises(RuntimeError, match=r'obs_state\[0\] = %d is outside 0 ... %d' % (obs, K)):
            d.augmented_gram(f, u_ln=u_ln[:1], A_in=ones, obs_state=[obs])
    for bad in (0.0, -1.0, np.inf, np.nan):
        A = ones.copy()
        A[0, 3] = bad
        with pytest.raises(RuntimeError, match='A_in of observable 0 holds a non-positive or non-finite value'):
            d.augmented_gram(f, A_in=A, obs_state=[1])
    for bad in (np.nan, -np.inf):
        u = u_ln[:2].copy()
        u[1, 2] = bad
        with pytest.raises(RuntimeError, match='u_ln of perturbed state 1 holds a NaN or -inf'):
            d.augmented_gram(f, u_ln=u)
    with pytest.raises(RuntimeError, match='perturbed state 0 has no sample with a non-zero weight'):
        d.augmented_gram(f, u_ln=np.full((1, N), np.inf))
    assert d.last_ms() > 0.0                             # that refusal comes after the column and row passes: their time is kept
    # a negative count cannot come through DeviceMBAR (it takes the counts from the shapes): the entry point itself
    g = np.empty((K + 1, K + 1))
    fk = np.ascontiguousarray(f)
    for L, I in ((-1, 1), (1, -1)):
        rc = d.lib.remd_mbar_augmented_gram(d.h, _dp(fk), L, None, I, None, None, None, None, _dp(g))
        assert rc != 0 and 'is negative' in d.lib.remd_last_error(None).decode()
    # the Python methods refuse the same inputs before the device sees them, as the numpy path does
    with pytest.raises(an.ParameterError, match='NaN or -inf'):
        dev.compute_perturbed_free_energies(np.full((1, N), np.nan))
    with pytest.raises(an.ParameterError, match='no sample with a non-zero weight'):
        dev.compute_expectations(x, np.full((1, N), np.inf))
    # and the object still works afterwards
    assert np.all(np.isfinite(d.augmented_gram(f, u_ln=u_ln[:1])[2]))
