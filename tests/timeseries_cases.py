"""What the tests of the device timeseries passes share (include/remd_hip_timeseries.h, openmmtools_amd/csrc/timeseries.hip): the
series, the numpy loop with a record of what it visits, and the kernels' chunked sums restated in Python.

Condition on the inputs.  The loop stops at the first C(t) <= 0, so a C that is zero to rounding would let the order of a sum decide
where it stops, and no bound on g could hold.  ``numpy_loop`` therefore ASSERTS that every |C| the numpy loop visits, the one it
stops at included, is at least 1e-9 (seven orders above the rounding of a sum of 1e4 terms), and ``assert_distinct_maximum`` that the
two largest n_effective of a per-sample scan differ by more than 1e-5 relative (g_i is stored as float32: 6e-8).  The seeds below were
chosen so that every case meets both; tests/test_timeseries_device_cpu.py checks all of them without a GPU."""
import functools
import numpy as np
from openmmtools_amd.multistate import analysis as an

CHUNK = 2048            # TS_CHUNK of csrc/timeseries.hip, for the tests without a device (the GPU tests read remd_timeseries_chunks)
BLOCK = 256
MAX_BATCH = 64          # REMD_TIMESERIES_MAX_BATCH
C_FLOOR = 1e-9
G_RTOL = 1e-10          # |g_dev - g_np| <= G_RTOL * max(1, g_np): both are f64 sums of at most 1e4 terms (1e4 x 2^-53 = 1e-12)


def ar1(N, rho, seed):
    """x_n = rho x_{n-1} + sqrt(1 - rho^2) e_n, stationary from the first sample on"""
    rng = np.random.default_rng(seed)
    e = rng.normal(size=N)
    x = np.empty(N)
    x[0] = e[0]
    s = np.sqrt(1.0 - rho * rho)
    for n in range(1, N):
        x[n] = rho * x[n - 1] + s * e[n]
    return x


SEEDS = {'ar05': 101, 'alternating': 202, 'ar05_plus_1e6': 101, 'ar099': 303}


@functools.lru_cache(maxsize=None)
def series(kind, N):
    """The series of the tests, read-only.  'alternating' is AR(1) with rho = -0.9: neighbours have opposite signs, C(t) = (-0.9)^t,
    and the four lags summed while t <= mintime = 3 add up to less than nothing, so g clamps to 1."""
    seed = SEEDS[kind] + N
    if kind == 'ar05':
        x = ar1(N, 0.5, seed)
    elif kind == 'alternating':
        x = ar1(N, -0.9, seed)
    elif kind == 'ar05_plus_1e6':
        x = ar1(N, 0.5, seed) + 1.0e6
    elif kind == 'ar099':
        x = ar1(N, 0.99, seed)
    else:
        raise KeyError(kind)
    x.setflags(write=False)
    return x


def sizes(chunk):
    return [2, 3, 5, chunk - 1, chunk, chunk + 1, 3 * chunk + 7]


def origins(N, chunk):
    """0, inside a chunk, exactly on every chunk boundary, N - 2 (every origin there is for N <= 5)"""
    if N <= 5:
        return list(range(N - 1))
    cand = [0, chunk // 2 + 3, chunk + chunk // 3, N - 2] + list(range(chunk, N - 1, chunk))
    return sorted({t for t in cand if 0 <= t <= N - 2})


def numpy_loop(A, fast=False, mintime=3):
    """(g, last lag added, [C visited]) by the loop of analysis.statistical_inefficiency, restated so that it can record; the result
    is asserted to be that function's, and every |C| to be at least C_FLOOR"""
    A = np.asarray(A, dtype=np.float64)
    N = A.size
    dA = A - A.mean()
    sigma2 = np.mean(dA * dA)
    assert sigma2 > 0.0
    g, t, increment, last, visited = 1.0, 1, 1, 0, []
    while t < N - 1:
        C = np.dot(dA[:N - t], dA[t:]) / (float(N - t) * sigma2)
        visited.append(C)
        if C <= 0.0 and t > mintime:
            break
        g += 2.0 * C * (1.0 - float(t) / float(N)) * float(increment)
        last = t
        t += increment
        if fast:
            increment += 1
    g = max(g, 1.0)
    assert g == an.statistical_inefficiency(A, fast=fast, mintime=mintime)
    assert all(abs(c) >= C_FLOOR for c in visited), 'a C of %.3e: choose another seed' % min(abs(c) for c in visited)
    return g, last, visited


def assert_distinct_maximum(n_effective_i):
    top = np.sort(np.asarray(n_effective_i, dtype=np.float64))[-2:]
    assert top[1] - top[0] > 1e-5 * top[1], 'the two largest n_effective are %r: choose another seed' % (top,)


def equilibrating_series(N, seed=404):
    """AR(1), rho = 0.9, on top of a transient that decays over N / 10 samples: the maximum of n_effective lies inside the series"""
    x = ar1(N, 0.9, seed) + 6.0 * np.exp(-np.arange(N) / (N / 10.0))
    x.setflags(write=False)
    return x


# ---- the kernels' sums, restated -------------------------------------------------------------------------------------------------
def _block_sum(values, n0, chunk=CHUNK, block=BLOCK):
    """One workgroup's sum over the samples [n0, n0 + chunk): ``values`` holds their terms, 0 where the kernel skips a sample (an
    added 0.0 changes nothing).  Thread i adds the samples i, i + block, ... in order; the lanes of a wave are folded by halves
    (__shfl_down by 32, 16, ... 1), the waves added in wave order."""
    v = np.zeros(chunk)
    v[:values.size] = values
    acc = np.zeros(block)
    for row in v.reshape(chunk // block, block):
        acc = acc + row
    waves = acc.reshape(block // 64, 64).copy()
    o = 32
    while o > 0:
        waves[:, :o] = waves[:, :o] + waves[:, o:2 * o]
        o //= 2
    total = waves[0, 0]
    for w in waves[1:, 0]:
        total = total + w
    return total


def _chunked(terms, lo, hi, chunk):
    """sum of terms(n) for n in [lo, hi): per chunk [c * chunk, (c + 1) * chunk) clipped to the range, merged in chunk order"""
    total = 0.0
    for c in range(lo // chunk, (hi - 1) // chunk + 1):
        n0 = c * chunk
        a, b = max(n0, lo), min(n0 + chunk, hi)
        vals = np.zeros(b - n0)
        vals[a - n0:] = terms(a, b)
        total = total + _block_sum(vals, n0, chunk)
    return total


def chunked_inefficiency(A, origin, fast=False, mintime=3, chunk=CHUNK):
    """(g, last lag) of the suffix A[origin:] as csrc/timeseries.hip computes it: two-pass moments and lag sums per chunk of absolute
    sample indices, the mean subtracted on the fly, the walk over the lags as the host loop has it"""
    A = np.asarray(A, dtype=np.float64)
    N = A.size
    Ns = N - origin
    mean = _chunked(lambda a, b: A[a:b], origin, N, chunk) / float(Ns)
    sigma2 = _chunked(lambda a, b: (A[a:b] - mean) ** 2, origin, N, chunk) / float(Ns)
    if sigma2 == 0.0:
        return float('nan'), 0
    g, t, increment, last = 1.0, 1, 1, 0
    while t < Ns - 1:
        s = _chunked(lambda a, b: (A[a:b] - mean) * (A[a + t:b + t] - mean), origin, N - t, chunk)
        C = s / (float(Ns - t) * sigma2)
        if C <= 0.0 and t > mintime:
            break
        g += 2.0 * C * (1.0 - float(t) / float(Ns)) * float(increment)
        last = t
        t += increment
        if fast:
            increment += 1
    return max(g, 1.0), last
