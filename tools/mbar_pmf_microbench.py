"""Free energy surfaces over binned samples, numpy against device: MBAR.compute_pmf on synthetic harmonic-oscillator ensembles with
50 bins along the coordinate and with 64 x 64 bins over the coordinate and a second, independent one; asymptotic and bootstrap
uncertainties; the dense route (compute_perturbed_free_energies with one +inf-padded row per bin) at 50 bins; the device kernels'
share of each call; and the compiler's resource usage of the kernels of csrc/mbar_pmf.hip.

    python tools/mbar_pmf_microbench.py [--out profiles/mbar_pmf_cost.txt] [--shapes 24x2000,128x2000] [--bootstraps 200]
                                        [--numpy-bootstraps 200,8] [--repeats 3] [--no-resources]

Every time is one call of compute_pmf on a solved estimator (the solve and the replicates' solves are profiles/mbar_cost.txt and
profiles/mbar_bootstrap_cost.txt), the median of `repeats` after one warm-up.  Both solvers work on one solution: the numpy estimator
is the device one with its device taken away.  ``--numpy-bootstraps`` gives the replicates the numpy bootstrap is timed at per shape;
its time is scaled to the device's B.  The kernels' time is the sum of remd_mbar_last_ms over the device calls of one compute_pmf."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                                   # noqa: E402
from openmmtools_amd import _engine                                  # noqa: E402
from openmmtools_amd.multistate import analysis as an                # noqa: E402

PASSES = ['pmf', 'gram', 'augmented_gram', 'bootstrap_draw', 'bootstrap_pmf', 'bootstrap_rows']
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'openmmtools_amd', 'csrc')


def ensemble(K, n_per_state, seed=7):
    """tools/mbar_microbench.py's ensemble with its coordinate x and a second coordinate y that no state depends on"""
    rng = np.random.default_rng(seed)
    k = np.arange(K)
    c, s = 2.0 * k / K, 1.0 + 0.5 * k / K
    x = np.concatenate([rng.normal(c[i], s[i], size=n_per_state) for i in range(K)])
    y = np.random.default_rng(seed + 1).normal(0.0, 1.0, size=x.size)
    return (x[None, :] - c[:, None]) ** 2 / (2.0 * s[:, None] ** 2), np.full(K, n_per_state, dtype=np.int64), x, y


class Meter:
    """device milliseconds and calls of every pass, summed while installed over _engine.DeviceMBAR"""

    def __init__(self):
        self.reset()
        self._saved = {}

    def reset(self):
        self.ms = dict.fromkeys(PASSES, 0.0)
        self.calls = dict.fromkeys(PASSES, 0)

    def __enter__(self):
        for name in PASSES:
            real = self._saved[name] = getattr(_engine.DeviceMBAR, name)

            def wrapped(dev, *args, _real=real, _name=name, **kwargs):
                out = _real(dev, *args, **kwargs)
                self.ms[_name] += dev.last_ms()
                self.calls[_name] += 1
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


def without_device(m, n_bootstraps):
    """the numpy estimator on the device estimator's solution, with its first n_bootstraps replicates"""
    h = an.MBAR.__new__(an.MBAR)
    h.__dict__.update(m.__dict__)
    h._dev, h._log_W, h.solver = None, None, 'numpy'
    h.n_bootstraps, h.f_k_boots = n_bootstraps, m.f_k_boots[:n_bootstraps]
    return h


def metered(meter, fn, repeats):
    """(median ms of fn, kernel ms of one call, {pass: (ms, calls)} of one call)"""
    with meter:
        t = median_ms(fn, repeats)
        meter.reset()
        fn()
        return t, sum(meter.ms.values()), {k: (meter.ms[k], meter.calls[k]) for k in PASSES if meter.calls[k]}


def shape_section(lines, K, n, B, B_numpy, repeats):
    u_kn, N_k, x, y = ensemble(K, n)
    N = u_kn.shape[1]
    dev = an.MBAR(u_kn, N_k, solver='device', n_bootstraps=B)
    host = without_device(dev, B_numpy)
    host.log_W_nk                                                     # (kept by the estimator: not part of a call)
    u_n = u_kn[K // 2]
    ex = np.linspace(np.percentile(x, 1), np.percentile(x, 99), 51)
    layouts = [('50 bins', an.bin_samples(x, ex)),
               ('64 x 64 bins', an.bin_samples(np.stack([x, y], axis=1), [np.linspace(ex[0], ex[-1], 65), np.linspace(-2.5, 2.5, 65)]))]
    lines.append('')
    lines.append('K = %d, N = %d (u_kn %.1f MB), B = %d' % (K, N, u_kn.nbytes / 1e6, B))
    meter = Meter()
    for label, (bin_n, nbins) in layouts:
        used = np.count_nonzero(np.bincount(bin_n[bin_n >= 0], minlength=nbins))
        lines.append('  %s: %d of %d hold a sample, %d samples binned' % (label, used, nbins, np.count_nonzero(bin_n >= 0)))
        method = None
        try:
            host.compute_pmf(u_n, bin_n, nbins)
        except ValueError as e:                                           # K + non-empty bins + 1 above MBAR.PMF_MAX_COLUMNS
            method = 'bootstrap'
            lines.append('    asymptotic   refused by both solvers: %s' % e)
        if method is None:
            t_np = median_ms(lambda: host.compute_pmf(u_n, bin_n, nbins), repeats)
            t_dev, kernels, parts = metered(meter, lambda: dev.compute_pmf(u_n, bin_n, nbins), repeats)
            lines.append('    asymptotic   numpy %10.1f ms   device %10.1f ms   numpy / device %6.2f x' % (t_np, t_dev, t_np / t_dev))
            lines.append('                 kernels %.2f ms = %.0f %% of the device call (%s); the rest is host: grouping, upload, Theta over %d columns'
                         % (kernels, 100.0 * kernels / t_dev, ', '.join('%s %.2f' % (k, v[0]) for k, v in parts.items()), K + used))
            t0 = time.perf_counter()
            dev._theta_of_gram(np.eye(K + used), np.zeros(K + used))
            lines.append('                 the host eigendecomposition and pseudo-inverse at %d columns alone: %.1f ms'
                         % (K + used, (time.perf_counter() - t0) * 1e3))
        t_npb = median_ms(lambda: host.compute_pmf(u_n, bin_n, nbins, uncertainty_method='bootstrap'), 1)
        t_devb, kernels, parts = metered(meter, lambda: dev.compute_pmf(u_n, bin_n, nbins, uncertainty_method='bootstrap'), repeats)
        scaled = t_npb / B_numpy * B
        lines.append('    bootstrap    numpy %10.1f ms at B = %d -> %.1f ms at B = %d   device %10.1f ms   numpy / device %6.1f x'
                     % (t_npb, B_numpy, scaled, B, t_devb, scaled / t_devb))
        lines.append('                 kernels %.2f ms = %.0f %% of the device call (%s)'
                     % (kernels, 100.0 * kernels / t_devb, ', '.join('%s %.2f in %d' % (k, v[0], v[1]) for k, v in parts.items())))
        a, b = host.compute_pmf(u_n, bin_n, nbins, uncertainty_method=method), dev.compute_pmf(u_n, bin_n, nbins, uncertainty_method=method)
        ok = np.isfinite(a['f_i'])
        lines.append('                 max |f_i device - numpy| %.2e, max relative difference of df_i %.2e (%s)'
                     % (np.max(np.abs(a['f_i'][ok] - b['f_i'][ok])), np.nanmax(np.abs(a['df_i'][a['df_i'] > 0] - b['df_i'][a['df_i'] > 0]) / a['df_i'][a['df_i'] > 0]),
                        'asymptotic' if method is None else 'bootstrap, the first %d replicates against all %d: not comparable' % (B_numpy, B) if B_numpy != B else 'bootstrap'))
    bin_n, nbins = layouts[0][1]
    rows = np.where(bin_n[None, :] == np.arange(nbins)[:, None], u_n[None, :], np.inf)
    t_np = median_ms(lambda: host.compute_perturbed_free_energies(rows), repeats)
    t_dev, kernels, _ = metered(meter, lambda: dev.compute_perturbed_free_energies(rows), repeats)
    lines.append('  the dense route at 50 bins (compute_perturbed_free_energies, u_ln [50][N] = %.1f MB, all but N entries +inf):' % (rows.nbytes / 1e6))
    lines.append('    asymptotic   numpy %10.1f ms   device %10.1f ms (kernels %.2f ms)' % (t_np, t_dev, kernels))
    t_devb, kernels, _ = metered(meter, lambda: dev.compute_perturbed_free_energies(rows, uncertainty_method='bootstrap'), repeats)
    lines.append('    bootstrap                            device %10.1f ms (kernels %.2f ms)' % (t_devb, kernels))


def kernel_resources():
    """the -Rpass-analysis=kernel-resource-usage remarks of csrc/mbar_pmf.hip for gfx950, one line per kernel"""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    with tempfile.TemporaryDirectory() as tmp:
        p = subprocess.run([hipcc, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-Rpass-analysis=kernel-resource-usage', '-c',
                            os.path.join(CSRC, 'mbar_pmf.hip'), '-o', os.path.join(tmp, 'mbar_pmf.o')], capture_output=True, text=True)
    rows, cur = [], None
    for line in p.stderr.splitlines():
        m = re.search(r'remark: +(Function Name|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)', line)
        if not m:
            continue
        if m.group(1) == 'Function Name':
            cur = {'name': subprocess.run(['c++filt', m.group(2)], capture_output=True, text=True).stdout.strip().split('(')[0]}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(1).split(' ')[0]] = m.group(2)
    out = ['Kernel resources (gfx950, -Rpass-analysis=kernel-resource-usage):',
           '  %-42s %6s %16s %8s %24s' % ('kernel', 'VGPRs', 'LDS bytes/block', 'scratch', 'occupancy (waves/SIMD)')]
    for r in rows:
        if 'mbar_pmf' in r['name']:
            out.append('  %-42s %6s %16s %8s %24s' % (r['name'].replace('void ', ''), r.get('VGPRs'), r.get('LDS'), r.get('ScratchSize'), r.get('Occupancy')))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--shapes', default='24x2000,128x2000')
    ap.add_argument('--bootstraps', type=int, default=200)
    ap.add_argument('--numpy-bootstraps', default='200,8')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--no-resources', action='store_true')
    args = ap.parse_args()
    lines = ['MBAR free energy surfaces over binned samples: one compute_pmf call, numpy against device.  Median of %d after one warm-up '
             '(numpy bootstrap: one run after one warm-up).  host threads: %s' % (args.repeats, os.environ.get('OMP_NUM_THREADS', 'unset'))]
    for shape, bn in zip(args.shapes.split(','), args.numpy_bootstraps.split(',')):
        K, n = (int(v) for v in shape.split('x'))
        shape_section(lines, K, n, args.bootstraps, min(int(bn), args.bootstraps), args.repeats)
    if not args.no_resources:
        lines.append('')
        lines.extend(kernel_resources())
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
