"""Cost of the device energy store (include/remd_hip_energy_store.h) next to the analyzer's numpy loops, at R = S = 24, U = 2 and
T = 10 000 and 105 000 stored iterations: the upload, each of the four calls, and get_free_energy() / generate_mixing_statistics() as a
whole with analysis_kwargs['assembly_solver'] = 'numpy' (the loops the analyzer had before the store) and 'device'.  Every figure is the
median of --repeats timed runs after one untimed run, with the range; wall-clock milliseconds unless it says kernel.

    python tools/energy_store_microbench.py [--sizes 10000,105000] [--repeats 5] > profiles/energy_store_cost.txt
"""
import argparse
import os
import sys
import time
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from openmmtools_amd._engine import DeviceEnergyStore, series_inefficiency_multiple      # noqa: E402
from openmmtools_amd.multistate import analysis as an                                    # noqa: E402

R = S = 24
U = 2


def records(T, seed=3):
    """a replica-exchange-like store: harmonic wells of growing width, every replica an AR(1) walk scaled by the width of its state,
    a transient over the first T / 20 iterations, neighbour swaps between the states"""
    rng = np.random.default_rng(seed)
    sigma = 1.0 + 0.08 * np.arange(S)
    sigma_u = np.array([0.95, sigma[-1] + 0.1])
    states = np.empty((T, R), dtype=np.int32)
    where = np.arange(S)                                  # the replica in each state
    row = np.empty(R, dtype=np.int32)
    z = np.empty((T, R))
    x = rng.normal(size=R)
    for t in range(T):
        a = np.arange(t % 2, S - 1, 2)                    # the even or the odd neighbour pairs, each swapped with probability 0.7
        a = a[rng.random(a.size) < 0.7]
        where[a], where[a + 1] = where[a + 1], where[a].copy()
        row[where] = np.arange(S)
        states[t] = row
        x = 0.8 * x + 0.6 * rng.normal(size=R)
        z[t] = x
    pos = z * sigma[states] * (1.0 + 2.0 * np.exp(-np.arange(T) / (T / 20.0)))[:, None]
    energies = 0.5 * pos[:, :, None] ** 2 / sigma[None, None, :] ** 2
    unsampled = 0.5 * pos[:, :, None] ** 2 / sigma_u[None, None, :] ** 2
    return energies, unsampled, states


class ArrayReporter:
    """the reporter surface the analyzer reads, answered from arrays (no files: the reads cost the same on both sides)"""

    def __init__(self, energies, unsampled, states):
        self.e, self.eu, self.st = energies, unsampled, states.astype(np.int64)
        self._files = {}
        self._meta = {'n_states': energies.shape[2]}

    def read_energies(self):
        return self.e, np.ones(self.e.shape, dtype=np.int8), self.eu

    def read_replica_thermodynamic_states(self):
        return self.st

    def read_last_iteration(self, last_checkpoint=True):
        return None if last_checkpoint else self.e.shape[0] - 1

    def read_online_analysis_data(self, iteration, *keys):
        raise ValueError('no logZ in storage')


def timed(fn, repeats):
    fn()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return np.median(ms), min(ms), max(ms), out


def line(label, stats, extra=''):
    print('  %-58s %10.2f ms  (%.2f ... %.2f)%s' % (label, stats[0], stats[1], stats[2], extra))


def analyzer(rep, assembly):
    return an.MultiStateSamplerAnalyzer(rep, unbias_restraint=False, analysis_kwargs={
        'assembly_solver': assembly, 'timeseries_solver': 'device', 'solver': 'device'})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='10000,105000')
    ap.add_argument('--repeats', type=int, default=5)
    args = ap.parse_args()
    print('energy store: R = S = %d, U = %d; median of %d runs after one untimed run, (min ... max)' % (R, U, args.repeats))
    for T in (int(t) for t in args.sizes.split(',')):
        energies, unsampled, states = records(T)
        e_rs, eu_rs, st_rs = (np.moveaxis(a, 0, -1) for a in (energies, unsampled, states.astype(np.int64)))
        host = an.MultiStateSamplerAnalyzer(ArrayReporter(energies, unsampled, states))
        mb = (energies.nbytes + unsampled.nbytes + states.nbytes) / 1e6
        print('\nT = %d (%.0f MB of records)' % (T, mb))

        up = timed(lambda: DeviceEnergyStore(energies, unsampled, states).close(), args.repeats)
        line('upload (create + destroy)', up, '  %.1f GB/s' % (mb / up[0]))
        store = DeviceEnergyStore(energies, unsampled, states)

        ref = timed(lambda: host.get_effective_energy_timeseries(e_rs, st_rs), args.repeats)
        dev = timed(store.effective_energy, args.repeats)
        line('effective energy, numpy loop', ref)
        line('effective energy, device (call, read-back included)', dev, '  kernel %.3f ms' % store.last_ms())

        n_eq, g = T // 10, 4.0
        iterations = np.arange(T)[n_eq:][an.subsample_correlated_data(np.zeros(T - n_eq), g=g)].astype(np.int64)
        for name, sel in (('decorrelated (%d iterations)' % len(iterations), iterations), ('every iteration', np.arange(T, dtype=np.int64))):
            ref = timed(lambda: host._compute_mbar_decorrelated_energies((e_rs[..., sel], eu_rs[..., sel], st_rs[..., sel], sel)), args.repeats)
            dev = timed(lambda: store.gather_u_ln(sel), args.repeats)
            moved = 2.0 * (S + U) * R * len(sel) * 8                      # read once, written once
            kernel = store.last_ms()
            assert np.array_equal(ref[3][0].view(np.uint64), dev[3][0].view(np.uint64)) and np.array_equal(ref[3][1], dev[3][1])
            line('u_ln / N_l, %s, numpy' % name, ref)
            line('u_ln / N_l, %s, device (call, read-back included)' % name, dev,
                 '  kernels %.3f ms = %.0f GB/s of %.0f MB moved' % (kernel, moved / kernel / 1e6, moved / 1e6))

        def host_counts():
            n_ij = np.zeros([S, S], np.int64)
            for it in range(n_eq, T - 1):
                np.add.at(n_ij, (states[it], states[it + 1]), 1)
            return n_ij
        ref = timed(host_counts, args.repeats)
        dev = timed(lambda: store.transition_counts(n_eq, T), args.repeats)
        assert np.array_equal(ref[3], dev[3])
        line('transition counts, numpy loop', ref)
        line('transition counts, device (call, read-back included)', dev, '  kernel %.3f ms' % store.last_ms())

        A = np.ascontiguousarray(states[n_eq:].T, dtype=np.float64)
        ref = timed(lambda: an.statistical_inefficiency_multiple(A), args.repeats)
        dev = timed(lambda: series_inefficiency_multiple(A, first_batch=8), args.repeats)
        line('several series g (K = %d, N = %d), numpy' % A.shape, ref, '  g = %.6f' % ref[3])
        line('several series g, device (upload included)', dev, '  g = %.6f, last lag %d, kernels %.3f ms' % (dev[3][0], dev[3][2], dev[3][3]))
        store.close()

        rep = ArrayReporter(energies, unsampled, states)
        for what in ('get_free_energy', 'generate_mixing_statistics'):
            results = {}
            for assembly in ('numpy', 'device'):
                def whole():
                    a = analyzer(rep, assembly)
                    try:
                        return getattr(a, what)()
                    finally:
                        a.clear()
                results[assembly] = timed(whole, args.repeats)
                line('%s(), assembly_solver = %r (store upload included)' % (what, assembly), results[assembly])
            a, b = results['numpy'][3], results['device'][3]
            worst = max(float(np.max(np.abs(np.asarray(x) - np.asarray(y)))) for x, y in zip(a, b))
            print('  %-58s %10.3e' % ('worst difference between the two results', worst))


if __name__ == '__main__':
    main()
