"""Philox4x32-10 in vectorised numpy, and the bootstrap draws it feeds: the host side of REMD_STREAM_BOOTSTRAP (csrc/rng.h), so that
``MBAR(solver='numpy')`` resamples exactly as the device does (include/remd_hip_mbar.h)."""
import numpy as np

STREAM_BOOTSTRAP = 9

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """The four output words [4][...] (uint32) of the counters ``c0 .. c3`` (broadcast against each other) under the key (k0, k1)."""
    c = [np.asarray(x, dtype=np.uint64) & _MASK for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]                               # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> _S32) ^ c[1] ^ np.uint64(k0), p1 & _MASK, (p0 >> _S32) ^ c[3] ^ np.uint64(k1), p0 & _MASK]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack(c).astype(np.uint32)


def remd_philox(seed, stream, a, b, t):
    """remd_philox of csrc/rng.h: key = the 64-bit seed, counter = (a, b, (u32) t, stream ^ ((u32)(t >> 32) << 8))."""
    seed, t = int(seed) & 0xFFFFFFFFFFFFFFFF, int(t)
    return philox4x32_10(a, b, t & 0xFFFFFFFF, (int(stream) ^ (((t >> 32) & 0xFFFFFFFF) << 8)) & 0xFFFFFFFF, seed & 0xFFFFFFFF, seed >> 32)


def bootstrap_indices(seed, state, replicate, n_k):
    """The ``n_k`` draws of state ``state`` in bootstrap replicate ``replicate``: indices into the state's samples in ascending order.
    Draw j takes the counter (j >> 1, state, replicate) and the word (w0 << 32) | w1 (even j) or (w2 << 32) | w3 (odd j); the index
    is floor(x n_k / 2^64) by an exact integer high multiply."""
    n_k = int(n_k)
    if not 0 <= n_k < 2 ** 32:
        raise ValueError('a state must have fewer than 2^32 samples')
    w = remd_philox(seed, STREAM_BOOTSTRAP, np.arange((n_k + 1) // 2, dtype=np.uint64), int(state), replicate).astype(np.uint64)
    hi = np.stack([w[0], w[2]], axis=1).reshape(-1)[:n_k]             # the high and low halves of x, draw by draw
    lo = np.stack([w[1], w[3]], axis=1).reshape(-1)[:n_k]
    nk = np.uint64(n_k)
    return ((hi * nk + ((lo * nk) >> _S32)) >> _S32).astype(np.int64)  # (no term reaches 2^64 with n_k < 2^32)


def bootstrap_counts(seed, replicate, N_k, sample_states=None):
    """The multiplicities c_n [N] (uint32) of one replicate: every state with N_k > 0 draws N_k times from its own samples, which
    are those n with ``sample_states[n] == k`` (None: blocks, the first N_0 samples from state 0 and so on)."""
    N_k = np.asarray(N_k, dtype=np.int64)
    N = int(N_k.sum())
    labels = np.repeat(np.arange(N_k.size), N_k) if sample_states is None else np.asarray(sample_states, dtype=np.int64)
    order = np.argsort(labels, kind='stable')                         # the samples of state 0 ascending, then of state 1, ...
    starts = np.concatenate([[0], np.cumsum(N_k)])
    counts = np.zeros(N, dtype=np.int64)
    for k in np.flatnonzero(N_k > 0):
        own = order[starts[k]:starts[k + 1]]
        counts += np.bincount(own[bootstrap_indices(seed, k, replicate, N_k[k])], minlength=N)
    return counts.astype(np.uint32)
