"""MBAR(solver='numpy') against MBAR(solver='device') on synthetic harmonic-oscillator ensembles: the end-to-end solve and the
device time of every pass (events around the kernels of one call, include/remd_hip_mbar.h: remd_mbar_last_ms).

    python tools/mbar_microbench.py [--out profiles/mbar_cost.txt] [--shapes 24x2000,128x2000] [--repeats 5]

Each timing is the median of `repeats` runs after one warm-up run, with the spread (min .. max) next to it.  The host side runs
with the threads the environment gives it (OMP_NUM_THREADS); the figure is printed."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                                   # noqa: E402
from openmmtools_amd.multistate import analysis as an                # noqa: E402


def ensemble(K, n_per_state, seed=7):
    rng = np.random.default_rng(seed)
    k = np.arange(K)
    c, s = 2.0 * k / K, 1.0 + 0.5 * k / K
    x = np.concatenate([rng.normal(c[i], s[i], size=n_per_state) for i in range(K)])
    return (x[None, :] - c[:, None]) ** 2 / (2.0 * s[:, None] ** 2), np.full(K, n_per_state, dtype=np.int64)


def timed(fn, repeats):
    fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), min(t), max(t)


def device_ms(dev, fn, repeats):
    fn()
    t = []
    for _ in range(repeats):
        fn()
        t.append(dev.last_ms())
    return statistics.median(t), min(t), max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--shapes', default='24x2000,128x2000')
    ap.add_argument('--repeats', type=int, default=5)
    args = ap.parse_args()
    lines = ['MBAR solver cost: numpy against device.  ms, median of %d after one warm-up (min .. max).  host threads: %s'
             % (args.repeats, os.environ.get('OMP_NUM_THREADS', 'unset'))]
    for shape in args.shapes.split(','):
        K, n = (int(v) for v in shape.split('x'))
        u_kn, N_k = ensemble(K, n)
        N = u_kn.shape[1]
        lines.append('')
        lines.append('K = %d, N = %d (u_kn %.1f MB)' % (K, N, u_kn.nbytes / 1e6))
        ref = [None]
        dev = [None]

        def solve_numpy():
            ref[0] = an.MBAR(u_kn, N_k)

        def solve_device():
            dev[0] = an.MBAR(u_kn, N_k, solver='device')
        lines.append('  solve, numpy                      %10.2f (%.2f .. %.2f)' % timed(solve_numpy, args.repeats))
        lines.append('  solve, device (upload included)   %10.2f (%.2f .. %.2f)' % timed(solve_device, args.repeats))
        m = dev[0]
        d = m._dev
        f = m.f_k
        lines.append('  max |f_device - f_numpy|          %10.3e' % np.max(np.abs(m.f_k - ref[0].f_k)))
        lines.append('  covariance, numpy                 %10.2f (%.2f .. %.2f)' % timed(ref[0].compute_free_energy_differences, args.repeats))
        lines.append('  covariance, device                %10.2f (%.2f .. %.2f)' % timed(m.compute_free_energy_differences, args.repeats))
        lines.append('  entropy and enthalpy, numpy       %10.2f (%.2f .. %.2f)' % timed(ref[0].compute_entropy_and_enthalpy, args.repeats))
        lines.append('  entropy and enthalpy, device      %10.2f (%.2f .. %.2f)' % timed(m.compute_entropy_and_enthalpy, args.repeats))
        lines.append('  device kernels of one call:')
        for label, fn in [('log_denominator (column pass)', lambda: d.log_denominator(f, want_log_den=False)),
                          ('self_consistent (column + row)', lambda: d.self_consistent(f)),
                          ('newton_parts (column + row + Gram K)', lambda: d.newton_parts(f)),
                          ('gram K (column + Gram)', lambda: d.gram(f)),
                          ('gram 2K (column + row + Gram)', lambda: d.gram(f, with_observable=True)),
                          ('log_weights (column + transpose)', lambda: d.log_weights(f))]:
            lines.append('    %-38s %9.3f (%.3f .. %.3f)' % ((label,) + device_ms(d, fn, args.repeats)))
        flops = 2.0 * N * K * (K + 1) / 2
        g = device_ms(d, lambda: d.gram(f), args.repeats)[0] - device_ms(d, lambda: d.log_denominator(f, want_log_den=False), args.repeats)[0]
        if g > 0:
            lines.append('    Gram K alone: %.3f ms = %.1f GFLOP/s of f64 FMA on the lower triangle' % (g, flops / g / 1e6))
        lines.append('  the same passes in numpy, one call each:')
        s = N_k > 0
        Nk = N_k[s].astype(np.float64)

        def np_logden():
            return an._logsumexp(f[s, None] - u_kn[s], axis=0, b=Nk[:, None])
        ld = np_logden()

        def np_gram():
            W = np.exp(f[:, None] - u_kn - ld[None, :])
            return W @ W.T
        lines.append('    %-38s %9.2f (%.2f .. %.2f)' % (('log denominator',) + timed(np_logden, args.repeats)))
        lines.append('    %-38s %9.2f (%.2f .. %.2f)' % (('eq. 11 row pass',) + timed(lambda: an._logsumexp(-u_kn - ld[None, :], axis=1), args.repeats)))
        lines.append('    %-38s %9.2f (%.2f .. %.2f)' % (('exp + Gram K',) + timed(np_gram, args.repeats)))
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
