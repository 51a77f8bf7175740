"""MBAR(solver='numpy') against MBAR(solver='device') on synthetic harmonic-oscillator ensembles: the end-to-end solve and the
device time of every pass (events around the kernels of one call, include/remd_hip_mbar.h: remd_mbar_last_ms).

    python tools/mbar_microbench.py [--out profiles/mbar_cost.txt] [--append] [--shapes 24x2000,128x2000] [--repeats 5]
                                    [--section solve|expectations|all]

`--section expectations` times compute_perturbed_free_energies, compute_expectations and compute_multiple_expectations (one
remd_mbar_augmented_gram each on the device) and the overlap outputs at the same shapes.

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


def solve_section(lines, args, u_kn, N_k):
    K, N = u_kn.shape
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


def expectations_section(lines, args, u_kn, N_k):
    """compute_perturbed_free_energies (L = K), compute_expectations (one observable at the K states) and
    compute_multiple_expectations (4 observables at one state), numpy against device: the whole call, the kernels of the device's one
    remd_mbar_augmented_gram (measured by events), and an ESTIMATE of what is left of the device call: the wall time less the kernels and
    less _theta_of_gram timed on a stand-in matrix of the same size (upload of u_ln / A_in, their checks, the [C][C] read-back)"""
    K, N = u_kn.shape
    ref, m = an.MBAR(u_kn, N_k), an.MBAR(u_kn, N_k, solver='device')
    d = m._dev
    u_ln = 0.9 * u_kn + 0.05                              # the same oscillators at another temperature: L = K perturbed states
    A_n, A_in = u_kn[0], u_kn[:4]
    theta = [0.0]

    def theta_ms(C):                                      # an ESTIMATE of the call's eigh + pinv: _theta_of_gram of identity / N at C columns, not of the call's own matrix
        G = np.eye(C) / N
        theta[0] = timed(lambda: an.MBAR._theta_of_gram(G, np.concatenate([N_k, np.zeros(C - K, dtype=np.int64)])), args.repeats)[0]
        return theta[0]
    for label, C, per_call_mb, call in [
            ('perturbed free energies, L = K', 2 * K, u_ln.nbytes / 1e6, lambda mb: mb.compute_perturbed_free_energies(u_ln)),
            ('expectations of one observable, K states', 2 * K, K * A_n.nbytes / 1e6, lambda mb: mb.compute_expectations(A_n)),
            ('4 observables at one perturbed state', K + 5, (u_ln[:1].nbytes + A_in.nbytes) / 1e6,
             lambda mb: mb.compute_multiple_expectations(A_in, u_ln[0]))]:
        t_np = timed(lambda: call(ref), args.repeats)
        t_dev = timed(lambda: call(m), args.repeats)
        kernels = d.last_ms()
        algebra = theta_ms(C)
        lines.append('  %s (C = %d, %.1f MB uploaded per call)' % (label, C, per_call_mb))
        lines.append('    numpy                              %10.2f (%.2f .. %.2f)' % t_np)
        lines.append('    device                             %10.2f (%.2f .. %.2f)%s' % (t_dev + ('   SLOWER than numpy' if t_dev[0] > t_np[0] else '',)))
        lines.append('      its kernels %.3f ms (measured); Theta estimated %.2f ms (eigh + pinv of a C x C stand-in, host, both paths); the rest by subtraction (upload, checks, read-back) %.2f ms = %.0f %%'
                     % (kernels, algebra, t_dev[0] - kernels - algebra, 100.0 * (t_dev[0] - kernels - algebra) / t_dev[0]))
    for label, call in [('overlap', lambda mb: mb.compute_overlap()), ('effective sample number', lambda mb: mb.compute_effective_sample_number())]:
        lines.append('  %-36s numpy %10.2f (%.2f .. %.2f)' % ((label,) + timed(lambda: call(ref), args.repeats)))
        lines.append('  %-36s device%10.2f (%.2f .. %.2f)' % (('',) + timed(lambda: call(m), args.repeats)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--shapes', default='24x2000,128x2000')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--section', default='all', choices=['solve', 'expectations', 'all'])
    ap.add_argument('--append', action='store_true', help='add to --out instead of replacing it')
    args = ap.parse_args()
    what = {'solve': 'solver', 'expectations': 'expectations and perturbed free energies', 'all': 'solver and expectations'}[args.section]
    lines = ['MBAR %s cost: numpy against device.  ms, median of %d after one warm-up (min .. max).  host threads: %s'
             % (what, args.repeats, os.environ.get('OMP_NUM_THREADS', 'unset'))]
    for shape in args.shapes.split(','):
        K, n = (int(v) for v in shape.split('x'))
        u_kn, N_k = ensemble(K, n)
        N = u_kn.shape[1]
        lines.append('')
        lines.append('K = %d, N = %d (u_kn %.1f MB)' % (K, N, u_kn.nbytes / 1e6))
        if args.section in ('solve', 'all'):
            solve_section(lines, args, u_kn, N_k)
        if args.section in ('expectations', 'all'):
            expectations_section(lines, args, u_kn, N_k)
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'a' if args.append else 'w') as fh:
            fh.write(('\n' if args.append else '') + text)


if __name__ == '__main__':
    main()
