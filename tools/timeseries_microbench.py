"""The equilibration scan and the statistical inefficiency, solver='numpy' against solver='device' (include/remd_hip_timeseries.h), on
AR(1) series with g of about 200, and analyzer.get_free_energy() end to end on a stored replica-exchange run.

    python tools/timeseries_microbench.py [--out profiles/timeseries_cost.txt] [--sizes 10000,100000,1000000] [--repeats 5]
                                          [--run-seconds 60]

Each timing is the median of `repeats` runs after one warm-up run, with the spread (min .. max) next to it; the device figures
include making the DeviceTimeseries (the upload).  `device kernels` is remd_timeseries_last_ms: events around the launches.  The
stored run is a 4-replica harmonic-oscillator exchange run, extended until `--run-seconds` of wall time are spent."""
import argparse
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                                   # noqa: E402
from openmmtools_amd import _engine                                  # noqa: E402
from openmmtools_amd.multistate import analysis as an                # noqa: E402


def ar1(N, g, seed=9):
    rho = (g - 1.0) / (g + 1.0)
    e = np.random.default_rng(seed).normal(size=N)
    x = np.empty(N)
    x[0] = e[0]
    s = np.sqrt(1.0 - rho * rho)
    for n in range(1, N):
        x[n] = rho * x[n - 1] + s * e[n]
    return x


def timed(fn, repeats):
    fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), min(t), max(t)


def kernel_ms(A, origins, fast, repeats):
    ts = _engine.DeviceTimeseries(A)
    ts.inefficiency(origins, fast=fast)
    t = []
    for _ in range(repeats):
        ts.inefficiency(origins, fast=fast)
        t.append(ts.last_ms())
    ts.close()
    return statistics.median(t), min(t), max(t)


def stored_run(path, seconds):
    from openmmtools_amd import testsystems, states, mcmc, unit
    from openmmtools_amd.multistate import ReplicaExchangeSampler, MultiStateReporter
    ho = testsystems.HarmonicOscillator()
    thermo = [states.ThermodynamicState(ho.system, T * unit.kelvin) for T in (300.0, 380.0, 480.0, 600.0)]
    ss = states.SamplerState(ho.positions, box_vectors=ho.system.getDefaultPeriodicBoxVectors())
    move = mcmc.LangevinSplittingDynamicsMove(timestep=2.0 * unit.femtosecond, collision_rate=5.0 / unit.picosecond,
                                              n_steps=5, reassign_velocities=True, splitting='V R O R V')
    s = ReplicaExchangeSampler(mcmc_moves=move, number_of_iterations=1000, engine=_engine.HipEngine(), seed=21, online_analysis_interval=None)
    rep = MultiStateReporter(path, checkpoint_interval=100000)
    s.create(thermo, [ss] * 4, storage=rep)
    t0 = time.perf_counter()
    s.run()
    while time.perf_counter() - t0 < seconds:
        s.extend(2000)
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--sizes', default='10000,100000,1000000')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--run-seconds', type=float, default=60.0)
    args = ap.parse_args()
    R = args.repeats
    lines = ['Equilibration scan and statistical inefficiency: numpy against device.  ms, median of %d after one warm-up (min .. max).  '
             'host threads: %s' % (R, os.environ.get('OMP_NUM_THREADS', 'unset'))]
    for N in (int(v) for v in args.sizes.split(',')):
        A = ar1(N, 200.0)
        out = {}

        def scan(solver):
            out[solver] = an.get_equilibration_data_per_sample(A, fast=True, max_subset=100, solver=solver)

        def single(solver):
            out['g_' + solver] = an.statistical_inefficiency(A, fast=False, solver=solver)
        lines.append('')
        lines.append('N = %d (AR(1), series %.2f MB)' % (N, A.nbytes / 1e6))
        lines.append('  get_equilibration_data_per_sample(max_subset=100, fast=True)')
        lines.append('    numpy                           %10.2f (%.2f .. %.2f)' % timed(lambda: scan('numpy'), R))
        lines.append('    device (upload included)        %10.2f (%.2f .. %.2f)' % timed(lambda: scan('device'), R))
        i_t = np.floor(np.arange(100) * N / 100).astype(int)
        lines.append('    device kernels                  %10.3f (%.3f .. %.3f)' % kernel_ms(A, i_t, True, R))
        same = np.array_equal(out['numpy'][0], out['device'][0]) and out['numpy'][2].argmax() == out['device'][2].argmax()
        lines.append('    max |g_i device - numpy| / g_i  %10.3e (float32), same origins and same maximum: %s'
                     % (np.max(np.abs(out['device'][1].astype(float) - out['numpy'][1]) / out['numpy'][1]), same))
        lines.append('  statistical_inefficiency(fast=False)')
        lines.append('    numpy                           %10.2f (%.2f .. %.2f)' % timed(lambda: single('numpy'), R))
        lines.append('    device (upload included)        %10.2f (%.2f .. %.2f)' % timed(lambda: single('device'), R))
        lines.append('    device kernels                  %10.3f (%.3f .. %.3f)' % kernel_ms(A, [0], False, R))
        ts = _engine.DeviceTimeseries(A)
        last = ts.inefficiency([0], fast=False)[2][0]
        ts.close()
        lines.append('    g numpy %.6f, device %.6f, |difference| / g %.3e, last lag %d'
                     % (out['g_numpy'], out['g_device'], abs(out['g_device'] - out['g_numpy']) / out['g_numpy'], last))
    if args.run_seconds > 0:
        with tempfile.TemporaryDirectory() as tmp:
            rep = stored_run(os.path.join(tmp, 'store'), args.run_seconds)
            lines.append('')
            result = {}

            def free_energy(label, kwargs):
                a = an.MultiStateSamplerAnalyzer(rep, analysis_kwargs=kwargs)
                result[label] = (a.get_free_energy()[0], a.n_equilibration_iterations, a.statistical_inefficiency, a.mbar.N)
            rows = []
            for label, kwargs in [('both numpy', {}), ('MBAR on the device', {'solver': 'device'}),
                                  ('timeseries on the device', {'timeseries_solver': 'device'}),
                                  ('both on the device', {'solver': 'device', 'timeseries_solver': 'device'})]:
                rows.append('    %-31s %10.2f (%.2f .. %.2f)' % ((label,) + timed(lambda: free_energy(label, kwargs), R)))
            D0, n_eq, g_t, n_mbar = result['both numpy']
            a = an.MultiStateSamplerAnalyzer(rep)
            e, _, _, st = a._read_energies()
            t_read = timed(lambda: a._read_energies(), R)
            t_series = timed(lambda: a.get_effective_energy_timeseries(e, st), R)
            u_n = a.get_effective_energy_timeseries(e, st)[1:]
            lines.append('analyzer.get_free_energy() on a stored 4-replica run of %d iterations (a new analyzer each time; n_equilibration %d, '
                         'g %.3f, %d samples in MBAR)' % (e.shape[-1] - 1, n_eq, g_t, n_mbar))
            lines += rows
            lines.append('  of which, host in every configuration:')
            lines.append('    reading the energies            %10.2f (%.2f .. %.2f)' % t_read)
            lines.append('    effective-energy timeseries     %10.2f (%.2f .. %.2f)' % t_series)
            lines.append('  the scan alone on that timeseries (max_subset=100, fast=True):')
            lines.append('    numpy                           %10.2f (%.2f .. %.2f)'
                         % timed(lambda: an.get_equilibration_data_per_sample(u_n, max_subset=100), R))
            lines.append('    device (upload included)        %10.2f (%.2f .. %.2f)'
                         % timed(lambda: an.get_equilibration_data_per_sample(u_n, max_subset=100, solver='device'), R))
            for label in ('MBAR on the device', 'timeseries on the device', 'both on the device'):
                D, n, g, _ = result[label]
                lines.append('  %-33s max |Delta_f - numpy| %.3e, n_equilibration %d, g %.6f' % (label + ':', np.max(np.abs(D - D0)), n, g))
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
