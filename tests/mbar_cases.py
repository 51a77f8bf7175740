"""Shared by tests/test_mbar_device_cpu.py and tests/test_mbar_gpu.py: the harmonic-oscillator ensembles, a Python mirror of the
device's chunked reductions (openmmtools_amd/csrc/mbar.hip), and the a-priori rounding bounds of a sum taken in another order.

Rounding bounds.  With u = 2^-53, a sum of m terms taken in any order differs from the exact sum by at most (m - 1) u sum|terms|
to first order, so two orders differ by at most 2 m u sum|terms| (the issue's bound).  Each term carries the relative error of how
it was made: exp and log of two libraries differ by at most 4 ulp = 8 u (relative for exp, of the value for log), a product adds u.
A log-sum-exp returns ln S + M, so the relative error of S becomes an absolute one, plus 4 ulp of the value for the log."""
import numpy as np

U = 2.0 ** -53


def harmonic_case(K, N_k, seed=20240, spread=2.0, widen=0.5):
    """1-D harmonic oscillators u_k(x) = (x - c_k)^2 / (2 s_k^2) with centres c_k = spread k / K and widths s_k = 1 + widen k / K:
    exact samples of the sampled states, (u_kn [K][N], N_k, f_k - f_0 = -ln(s_k / s_0))."""
    rng = np.random.default_rng(seed)
    N_k = np.asarray(N_k, dtype=np.int64)
    k = np.arange(K)
    c, s = spread * k / K, 1.0 + widen * k / K
    x = np.concatenate([rng.normal(c[i], s[i], size=int(N_k[i])) for i in range(K)])
    u_kn = (x[None, :] - c[:, None]) ** 2 / (2.0 * s[:, None] ** 2)
    return u_kn, N_k, -np.log(s / s[0])


def even(K, n):
    return [n] * K


# (K, N_k): the shapes of the issue.  The last spans 3 chunks of the row pass (4096 samples), 36 of the Gram pass (256 samples at
# this width) and 36 workgroups of the column pass (256 samples).
CASES = {
    '1x1': (1, [1]),
    '2x63': (2, [32, 31]),
    '2x64': (2, [32, 32]),
    '2x65': (2, [33, 32]),
    '3x257_ends_unsampled': (3, [0, 257, 0]),
    '5x1000_alternating': (5, [0, 300, 0, 700, 0]),
    '17x1037': (17, even(17, 61)),
    '65x2015': (65, even(65, 31)),
    '24x4800': (24, even(24, 200)),
    '3x9001_three_chunks': (3, [3000, 3001, 3000]),
}


# ---- the device's reductions, restated -----------------------------------------------------------------------------------------
# What is restated is the chunking and the merge: the (max, scaled sum) pair per chunk with its guards and the merge in chunk order,
# and the per-chunk Gram partials summed in chunk order.  The order INSIDE a chunk is not the device's (np.sum is pairwise where the
# device strides lanes and folds waves; the Gram partial adds sample by sample where the device stages 16): any order inside a
# chunk obeys the same a-priori bound, which is all these functions are checked against.
def _guard(m):
    return m if np.isfinite(m) else 0.0


def chunked_logsumexp(a, chunk):
    """ln sum exp(a) as the row pass takes it: a (max, scaled sum) pair per chunk, merged in chunk order."""
    a = np.asarray(a, dtype=np.float64)
    pairs = []
    for n0 in range(0, a.size, chunk):
        c = a[n0:n0 + chunk]
        m = np.max(c)
        pairs.append((m, float(np.sum(np.exp(c - _guard(m))))))
    M = _guard(np.max([p[0] for p in pairs]))
    S = 0.0
    for m, s in pairs:
        if s != 0.0:
            S += s * np.exp(_guard(m) - M)
    with np.errstate(divide='ignore'):
        return float(np.log(S) + M)


def chunked_gram(W, chunk):
    """W^T W ([N][C] -> [C][C]) as the Gram pass takes it: one partial per chunk of samples, each accumulated sample by sample,
    summed in chunk order."""
    W = np.asarray(W, dtype=np.float64)
    G = np.zeros((W.shape[1], W.shape[1]))
    for n0 in range(0, W.shape[0], chunk):
        P = np.zeros_like(G)
        for row in W[n0:n0 + chunk]:
            P += row[:, None] * row[None, :]
        G += P
    return G


# ---- bounds ----------------------------------------------------------------------------------------------------------------------
def sum_bound(m, abs_terms, term_rel=0.0):
    """|sum in one order - sum in another| for m terms whose makers differ by a relative term_rel per term"""
    return (2.0 * m * U + term_rel) * abs_terms


def lse_bound(m, value, term_rel=8 * U, arg_abs=0.0):
    """the same for ln sum exp: the relative error of S (terms: exp, 8 u; the merge of the chunks: one more exp and a product,
    9 u; arguments that differ by arg_abs shift the result by as much, twice with the maximum) plus 4 ulp of the value"""
    with np.errstate(invalid='ignore'):
        ulp = np.where(np.isfinite(value), np.spacing(np.abs(value)), 0.0)
    return 2.0 * m * U + term_rel + 9 * U + 2.0 * arg_abs + 4.0 * ulp
