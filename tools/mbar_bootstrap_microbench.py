"""Bootstrap uncertainties of MBAR, numpy against device: MBAR(n_bootstraps=B) end to end (upload and host algebra included) on
synthetic harmonic-oscillator ensembles, the device kernels' share of the call and the Newton iterations per replicate.

    python tools/mbar_bootstrap_microbench.py [--out profiles/mbar_bootstrap_cost.txt] [--shapes 24x2000,128x2000] [--bootstraps 200]
                                              [--numpy-bootstraps 200,2] [--repeats 3]

What is timed is the B resampled solves alone: the time of MBAR(n_bootstraps=B) less the time of MBAR() on the same matrix, each the
median of `repeats` runs after one warm-up.  ``--numpy-bootstraps`` gives the B of the numpy solver per shape (a smaller B where the
full B would take minutes); its time is also given per replicate and scaled to the device's B.  The kernels' time is the sum of
remd_mbar_last_ms over every device call the replicates made (events around the launches)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                                   # noqa: E402
from openmmtools_amd import _engine                                  # noqa: E402
from openmmtools_amd.multistate import analysis as an                # noqa: E402
from mbar_microbench import ensemble                                 # noqa: E402

PASSES = ['bootstrap_draw', 'bootstrap_self_consistent', 'bootstrap_newton_parts', 'bootstrap_log_denominator', 'bootstrap_rows']


class Meter:
    """device milliseconds, calls and replicates of every bootstrap pass, summed while installed over _engine.DeviceMBAR"""

    def __init__(self):
        self.reset()
        self._saved = {}

    def reset(self):
        self.ms = dict.fromkeys(PASSES, 0.0)
        self.calls = dict.fromkeys(PASSES, 0)
        self.replicates = dict.fromkeys(PASSES, 0)

    def __enter__(self):
        for name in PASSES:
            real = self._saved[name] = getattr(_engine.DeviceMBAR, name)

            def wrapped(dev, *args, _real=real, _name=name, **kwargs):
                out = _real(dev, *args, **kwargs)
                self.ms[_name] += dev.last_ms()
                self.calls[_name] += 1
                self.replicates[_name] += args[2] if _name == 'bootstrap_draw' else len(args[0])
                return out
            setattr(_engine.DeviceMBAR, name, wrapped)
        return self

    def __exit__(self, *exc):
        for name, real in self._saved.items():
            setattr(_engine.DeviceMBAR, name, real)


def median_ms(fn, repeats):
    fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def shape_section(lines, K, n, B, B_numpy, repeats):
    u_kn, N_k = ensemble(K, n)
    N = u_kn.shape[1]
    lines.append('')
    lines.append('K = %d, N = %d (u_kn %.1f MB), B = %d' % (K, N, u_kn.nbytes / 1e6, B))
    base_np = median_ms(lambda: an.MBAR(u_kn, N_k), repeats)
    ref = [None]

    def numpy_boot():
        ref[0] = an.MBAR(u_kn, N_k, n_bootstraps=B_numpy)
    t_np = median_ms(numpy_boot, repeats) - base_np
    lines.append('  numpy,  B = %-4d                    %12.1f ms = %.1f ms per replicate -> %.1f s at B = %d (full solve alone %.1f ms)'
                 % (B_numpy, t_np, t_np / B_numpy, t_np / B_numpy * B / 1e3, B, base_np))
    base_dev = median_ms(lambda: an.MBAR(u_kn, N_k, solver='device'), repeats)
    dev = [None]
    meter = Meter()

    def device_boot():
        meter.reset()
        dev[0] = an.MBAR(u_kn, N_k, solver='device', n_bootstraps=B)
    with meter:
        t_dev = median_ms(device_boot, repeats) - base_dev
    kernels = sum(meter.ms.values())
    lines.append('  device, B = %-4d                    %12.1f ms = %.2f ms per replicate (full solve with upload alone %.1f ms)'
                 % (B, t_dev, t_dev / B, base_dev))
    lines.append('    numpy / device per replicate      %12.1f x' % ((t_np / B_numpy) / (t_dev / B)))
    lines.append('    kernels                           %12.1f ms = %.0f %% of the call; the rest is host: batched K x K solves, checks, copies'
                 % (kernels, 100.0 * kernels / t_dev))
    for name in PASSES[:4]:
        lines.append('      %-28s %8.2f ms in %3d calls, %5d replicate-passes' % (name, meter.ms[name], meter.calls[name], meter.replicates[name]))
    lines.append('    Newton iterations per replicate   %12.2f (batches of at most %d replicates)'
                 % (meter.replicates['bootstrap_newton_parts'] / float(B), dev[0]._dev.bootstrap_max_batch()))
    lines.append('    max |f_boots device - numpy| over the first %d replicates: %.3e'
                 % (B_numpy, np.max(np.abs(dev[0].f_k_boots[:B_numpy] - ref[0].f_k_boots))))
    ratio = dev[0].compute_free_energy_differences(uncertainty_method='bootstrap')[1][0, K - 1] / dev[0].compute_free_energy_differences()[1][0, K - 1]
    lines.append('    bootstrap / asymptotic dDelta_f[0, K-1]: %.4f' % ratio)
    A = u_kn[0]
    with meter:
        meter.reset()
        t = median_ms(lambda: dev[0].compute_expectations(A, uncertainty_method='bootstrap'), repeats)
        lines.append('  compute_expectations(bootstrap), device, K observables x B: %.1f ms (kernels of one call %.1f ms, %.1f MB uploaded per batch)'
                     % (t, sum(meter.ms.values()) / (repeats + 1), K * A.nbytes / 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--shapes', default='24x2000,128x2000')
    ap.add_argument('--bootstraps', type=int, default=200)
    ap.add_argument('--numpy-bootstraps', default='200,2')
    ap.add_argument('--repeats', type=int, default=3)
    args = ap.parse_args()
    shapes = args.shapes.split(',')
    b_numpy = [int(v) for v in args.numpy_bootstraps.split(',')]
    lines = ['MBAR bootstrap cost: numpy against device, the B resampled solves alone.  Median of %d after one warm-up.  host threads: %s'
             % (args.repeats, os.environ.get('OMP_NUM_THREADS', 'unset'))]
    for shape, bn in zip(shapes, b_numpy):
        K, n = (int(v) for v in shape.split('x'))
        shape_section(lines, K, n, args.bootstraps, bn, args.repeats)
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
