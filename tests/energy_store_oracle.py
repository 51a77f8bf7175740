"""What the tests of the device energy store share (include/remd_hip_energy_store.h, openmmtools_amd/csrc/energy_store.hip): the four
definitions of the header restated in plain numpy and Python, with every sum in the order the header states, the synthetic stores, and
the record-container store of the end-to-end tests.

Order.  ``np.cumsum`` adds sequentially, so ``_ascending_sum`` is 0.0 + x_0 + x_1 + ... in ascending index, the order of the kernels.
The statistical inefficiency of several series is restated with the host function's own operations (its result is asserted equal) so
that it can record the last lag and every C it visits; as in tests/timeseries_cases.py every |C| visited must be at least C_FLOOR, or
the order of a sum could decide where the walk stops and no bound on g could hold."""
import numpy as np
from openmmtools_amd.multistate import analysis as an

SERIES_CHUNK = 2048     # TS_CHUNK of csrc/timeseries.hip, for the tests without a device
EFFECTIVE_CHUNK, GATHER_TILE, COUNT_CHUNK, HIST_MAX_STATES = 256, 32, 8192, 64      # what remd_energy_store_chunks reports
C_FLOOR = 1e-9
G_RTOL = 1e-10          # |g_dev - g_np| <= G_RTOL * max(1, g_np): the figure of the timeseries extension


def _ascending_sum(x):
    """0.0 + x[..., 0] + x[..., 1] + ... along the last axis, sequentially"""
    x = np.asarray(x, dtype=np.float64)
    zero = np.zeros(x.shape[:-1] + (1,))
    with np.errstate(invalid='ignore', over='ignore'):
        return np.cumsum(np.concatenate([zero, x], axis=-1), axis=-1)[..., -1]


def logsumexp_rows(a):
    """L of the header for every row of a [T][S]: shifted by the row's maximum where that is finite (else by 0), summed in ascending s"""
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        m = np.fmax.reduce(a, axis=-1, initial=-np.inf)
        m = np.where(np.isfinite(m), m, 0.0)
        return np.log(_ascending_sum(np.exp(a - m[..., None]))) + m


def effective_energy(energies, states, log_weights=None, f_l=None):
    """u_n [T] of energies [T][R][S], states [T][R]; with log_weights [T][S] and f_l [S]: e + (-w + L)"""
    energies = np.asarray(energies, dtype=np.float64)
    T, R, S = energies.shape
    t, r = np.arange(T)[:, None], np.arange(R)[None, :]
    u = _ascending_sum(energies[t, r, states])
    if log_weights is None:
        return u
    log_weights = np.asarray(log_weights, dtype=np.float64)
    w = _ascending_sum(log_weights[t, states])
    L = logsumexp_rows(-np.asarray(f_l, dtype=np.float64)[None, :] + log_weights)
    with np.errstate(invalid='ignore'):
        return u + (-w + L)


def gather_u_ln(energies, unsampled, states, iterations):
    """(u_ln [U + S][R * n_sel], N_l [U + S]): column r * n_sel + j is (iterations[j], r)"""
    T, R, S = energies.shape
    U = 0 if unsampled is None else unsampled.shape[2]
    iterations = np.asarray(iterations, dtype=np.int64)
    first, n_sel = U // 2, len(iterations)
    u_ln = np.zeros([U + S, R * n_sel])
    N_l = np.zeros([U + S], dtype=np.int64)
    u_ln[first:first + S] = energies[iterations].transpose(2, 1, 0).reshape(S, R * n_sel)      # [j][r][s] -> [s][r][j]
    if U:
        u_ln[[0, -1]] = unsampled[iterations].transpose(2, 1, 0).reshape(2, R * n_sel)
    np.add.at(N_l, first + states[iterations].reshape(-1), 1)
    return u_ln, N_l


def transition_counts(states, S, t_begin, t_end):
    n_ij = np.zeros([S, S], dtype=np.int64)
    for t in range(t_begin, t_end - 1):
        for a, b in zip(states[t], states[t + 1]):
            n_ij[a, b] += 1
    return n_ij


def inefficiency_multiple(A_kn, fast=False, mintime=3, check=True):
    """(g, status, last lag added, [C visited]) of K series of one length: the pooled mean and variance, C(t) the pooled sum over the
    series over K (N - t) sigma2, the term 2 C (1 - t / N) increment, until the first C <= 0 at t > mintime or t >= N - 1; max(g, 1)"""
    A = np.asarray(A_kn, dtype=np.float64)
    K, N = A.shape
    mu = sum(a.sum() for a in A) / float(K * N)
    dA = [a - mu for a in A]
    sigma2 = sum((d * d).sum() for d in dA) / float(K * N)
    if sigma2 == 0.0:
        return float('nan'), 1, 0, []
    g, t, increment, last, visited = 1.0, 1, 1, 0, []
    while t < N - 1:
        num = 0.0
        for d in dA:
            num += (d[:N - t] * d[t:]).sum()
        C = (num / float(K * (N - t))) / sigma2
        visited.append(C)
        if C <= 0.0 and t > mintime:
            break
        g += 2.0 * C * (1.0 - float(t) / float(N)) * float(increment)
        last = t
        t += increment
        if fast:
            increment += 1
    if check:
        assert all(abs(c) >= C_FLOOR for c in visited), 'a C of %.3e: choose another seed' % min(abs(c) for c in visited)
    return max(g, 1.0), 0, last, visited


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def ar1(N, rho, rng):
    e = rng.normal(size=N)
    x = np.empty(N)
    x[0] = e[0]
    s = np.sqrt(1.0 - rho * rho)
    for n in range(1, N):
        x[n] = rho * x[n - 1] + s * e[n]
    return x


def series(K, N, seed=0):
    """K AR(1) series (rho = 0.6) of length N around different means"""
    rng = np.random.default_rng(1000 * K + N + 7919 * seed)
    return np.stack([ar1(N, 0.6, rng) + 0.3 * k for k in range(K)])


def synthetic_store(T, R, S, U, kind='shared', nonfinite=None, seed=0):
    """(energies [T][R][S], unsampled [T][R][U] or None, states [T][R] int32).  kind 'permutation' (R == S: every row a permutation),
    'shared' (random states: several replicas share one, as in SAMS) or 'one_cell' (every replica stays in state S - 1).
    nonfinite None, 'unoccupied' (+inf, -inf, NaN only where no replica is) or 'occupied' (also in occupied entries)."""
    rng = np.random.default_rng(seed + 1000003 * T + 1009 * R + 13 * S + U)
    energies = rng.normal(size=(T, R, S)) * 10.0 ** rng.integers(-3, 4, size=(T, R, 1))
    unsampled = rng.normal(size=(T, R, U)) if U else None
    if kind == 'permutation':
        assert R == S
        states = np.stack([rng.permutation(S) for _ in range(T)])
    elif kind == 'one_cell':
        states = np.full((T, R), S - 1)
    else:
        states = rng.integers(0, S, size=(T, R))
    states = states.astype(np.int32)
    if nonfinite:
        special = np.array([np.inf, -np.inf, np.nan])
        occupied = np.zeros((T, R, S), dtype=bool)
        occupied[np.arange(T)[:, None], np.arange(R)[None, :], states] = True
        hit = rng.random((T, R, S)) < 0.2
        if nonfinite == 'unoccupied':
            hit &= ~occupied
        energies = np.where(hit, special[rng.integers(0, 3, size=(T, R, S))], energies)
        if U:
            unsampled = np.where(rng.random((T, R, U)) < 0.2, special[rng.integers(0, 3, size=(T, R, U))], unsampled)
    return energies, unsampled, states


def log_weights_case(T, S, seed=0):
    """(log_weights [T][S], f_l [S]) like a SAMS run's: the weights drift towards -f"""
    rng = np.random.default_rng(77 + seed + 31 * T + S)
    f_l = np.concatenate([[0.0], np.cumsum(rng.normal(size=S - 1) * 3.0)])
    ramp = 1.0 - np.exp(-np.arange(T) / max(1.0, T / 5.0))
    return -f_l[None, :] * ramp[:, None] + 0.5 * rng.normal(size=(T, S)), f_l


def numpy_analyzer(energies, unsampled, states, log_weights=None, f_l=None):
    """The analyzer's present numpy methods on arrays: an analyzer without a reporter whose records are the arrays given"""
    class _File:
        def __init__(self, a):
            self.a = a

        def read(self, index=slice(None)):
            return self.a[index]

    class _Reporter:
        _files = {'log_weights': _File(log_weights)}
        _meta = {'n_states': energies.shape[2]}

        def read_online_analysis_data(self, iteration, *keys):
            if log_weights is None:
                raise ValueError('no logZ in storage')
            return {'logZ': -np.asarray(f_l), 'log_weights': log_weights[-1]}

        def read_replica_thermodynamic_states(self):
            return states.astype(np.int64)
    return an.MultiStateSamplerAnalyzer(_Reporter())


def host_effective_energy(energies, states, log_weights=None, f_l=None):
    a = numpy_analyzer(energies, None, states, log_weights, f_l)
    return a.get_effective_energy_timeseries(np.moveaxis(energies, 0, -1), np.moveaxis(states, 0, -1))


def host_u_ln(energies, unsampled, states, iterations):
    T, R, S = energies.shape
    eu = np.zeros((T, R, 0)) if unsampled is None else unsampled
    e, u, st = (np.moveaxis(a, 0, -1) for a in (energies, eu, states))
    a = numpy_analyzer(energies, unsampled, states)
    return a._compute_mbar_decorrelated_energies((e[..., iterations], u[..., iterations], st[..., iterations], iterations))


def host_transition_counts(states, S, t_begin, t_end):
    """the loop of generate_mixing_statistics"""
    n_ij = np.zeros([S, S], np.int64)
    for it in range(t_begin, t_end - 1):
        np.add.at(n_ij, (states[it], states[it + 1]), 1)
    return n_ij


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def same_bits_or_both_nan(a, b):
    """bit for bit, except that any NaN matches any NaN (an addition does not promise a NaN's sign and payload)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and same_bits(a[~nan], b[~nan])


# ---- the record-container store of the end-to-end tests -----------------------------------------------------------------------------
E2E_R = E2E_S = 4
E2E_T = 300


def e2e_records(sams, seed=5):
    """(energies [T][4][4], unsampled [T][4][2], states [T][4], log_weights [T][4] or None, logZ [4] or None): harmonic wells of
    widths sigma_s, every replica an AR(1) walk scaled by the width of the state it occupies, a transient over the first iterations.
    Without SAMS the state rows are permutations changed by a neighbour swap per iteration; with SAMS every replica walks alone."""
    rng = np.random.default_rng(seed + int(sams))
    T, R, S = E2E_T, E2E_R, E2E_S
    sigma = np.array([1.0, 1.3, 1.7, 2.2])
    sigma_u = np.array([0.9, 2.5])
    states = np.zeros((T, R), dtype=np.int32)
    row = np.arange(R) % S
    for t in range(T):
        if sams:
            row = np.clip(row + rng.integers(-1, 2, size=R), 0, S - 1)
        elif t:
            i = rng.integers(0, R - 1)
            pos = np.argsort(row)                       # the replicas in states i and i + 1 trade places
            if rng.random() < 0.6:
                row = row.copy()
                row[pos[i]], row[pos[i + 1]] = row[pos[i + 1]], row[pos[i]]
        states[t] = row
    z = np.stack([ar1(T, 0.5, rng) for _ in range(R)], axis=1)
    x = z * sigma[states] * (1.0 + 2.0 * np.exp(-np.arange(T) / 25.0))[:, None]
    energies = 0.5 * x[:, :, None] ** 2 / sigma[None, None, :] ** 2
    unsampled = 0.5 * x[:, :, None] ** 2 / sigma_u[None, None, :] ** 2
    if not sams:
        return energies, unsampled, states, None, None
    logZ = -np.log(sigma / sigma[0])
    lw = -logZ[None, :] * (1.0 - np.exp(-np.arange(T) / 40.0))[:, None] + 0.05 * rng.normal(size=(T, S))
    return energies, unsampled, states, lw, logZ


def write_e2e_store(path, sams):
    from openmmtools_amd import testsystems, states as st, unit
    from openmmtools_amd.multistate import MultiStateReporter
    energies, unsampled, state_indices, lw, logZ = e2e_records(sams)
    T, R, S = energies.shape
    ho = testsystems.HarmonicOscillator()
    thermo = [st.ThermodynamicState(ho.system, 300.0 * unit.kelvin) for _ in range(S)]
    rep = MultiStateReporter(str(path), open_mode='w', checkpoint_interval=1000)
    rep.initialize(R, S, 2, 1)
    rep.write_thermodynamic_states(thermo, thermo[:2])
    for it in range(T):
        rep.write_replica_thermodynamic_states(state_indices[it], it)
        rep.write_energies(energies[it], np.ones((R, S), dtype=np.int8), unsampled[it], it)
        if sams:
            rep.write_online_analysis_data(it, logZ=logZ, log_weights=lw[it])
        rep.write_last_iteration(it)
    return rep
