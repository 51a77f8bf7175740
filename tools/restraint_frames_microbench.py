"""Cost of re-evaluating a restraint at the stored frames: the numpy solver of multistate/analysis.py against remd_restraint_frames
(csrc/restraint_frames.hip) at host-guest size -- 24 replicas x 10 000 iterations, groups of 126 and 30 atoms (the whole pair is the
analysis subset).  Wall time of a device call includes the upload of the frames; the kernels' own time comes from the events the
library records around its launches.  The kernel reads 12 bytes per atom and frame (and 12 per frame of box) once: bytes / kernel time
is the rate it reaches.

    python tools/restraint_frames_microbench.py [--replicas 24] [--iterations 10000] [--out profiles/restraint_frames_cost.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openmmtools_amd import _engine                                   # noqa: E402
from openmmtools_amd.multistate import analysis as an                 # noqa: E402


def _stats(samples):
    s = np.sort(np.asarray(samples))
    return '%10.2f (%.2f .. %.2f)' % (np.median(s), s[0], s[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--replicas', type=int, default=24)
    ap.add_argument('--iterations', type=int, default=10000)
    ap.add_argument('--n1', type=int, default=126)
    ap.add_argument('--n2', type=int, default=30)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--numpy-repeats', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    F, n_atoms = args.replicas * args.iterations, args.n1 + args.n2
    rng = np.random.default_rng(2024)
    lines = []

    def say(text=''):
        print(text, flush=True)
        lines.append(text)

    for periodic in (0, 1):
        box = (np.array([4.0, 4.2, 3.9]) + rng.uniform(-0.05, 0.05, size=(F, 3))).astype(np.float32) if periodic else None
        pos = np.empty((F, n_atoms, 3), dtype=np.float32)
        step = 1 << 14
        for f0 in range(0, F, step):                                   # (generated in slices: no f64 copy of the whole trajectory)
            n = min(step, F - f0)
            centre = rng.uniform(1.0, 3.0, size=(n, 1, 3))
            x = centre + rng.uniform(-0.5, 0.5, size=(n, n_atoms, 3))
            x[:, args.n1:, :] += rng.normal(size=(n, 1, 3)) * 0.3
            if periodic:
                L = box[f0:f0 + n, None, :].astype(np.float64)
                x -= L * np.floor(x / L)                               # atoms wrapped one by one, as a barostat leaves them
            pos[f0:f0 + n] = x
        masses = rng.uniform(1.0, 16.0, n_atoms)
        desc = dict(kind=0, K=800.0, r0=0.0, periodic=periodic, atoms1=np.arange(args.n1, dtype=np.int32),
                    atoms2=np.arange(args.n1, n_atoms, dtype=np.int32), weights1=None, weights2=None)
        nbytes = F * (n_atoms * 12 + (12 if periodic else 0))
        say('%s restraint: %d replicas x %d iterations = %d frames, groups of %d + %d atoms (frames %.1f MB)'
            % ('periodic' if periodic else 'non-periodic', args.replicas, args.iterations, F, args.n1, args.n2, nbytes / 1e6))
        t_np = []
        for _ in range(args.numpy_repeats):
            t0 = time.perf_counter()
            E_np, r_np = an.restraint_frames_numpy(desc, pos, box, masses)
            t_np.append((time.perf_counter() - t0) * 1e3)
        say('  numpy solver, ms                       %s' % _stats(t_np))
        _engine.restraint_frames(desc, pos, box, masses)               # warm-up: the code object, the first allocations
        t_dev, t_ker = [], []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            E, r = _engine.restraint_frames(desc, pos, box, masses)    # (synchronous: the results are on the host when it returns)
            t_dev.append((time.perf_counter() - t0) * 1e3)
            t_ker.append(_engine.restraint_frames_last_ms())
        say('  device call, upload included, ms       %s' % _stats(t_dev))
        say('  its kernels alone (events), ms         %s' % _stats(t_ker))
        say('  kernel rate                            %10.1f GB/s of frames read once' % (nbytes / (np.median(t_ker) * 1e-3) / 1e9))
        say('  numpy / device call                    %10.1f x' % (np.median(t_np) / np.median(t_dev)))
        say('  max |E_device - E_numpy| / max |E|     %10.3e' % (np.abs(E - E_np).max() / np.abs(E_np).max()))
        say('  max |r_device - r_numpy|, nm           %10.3e' % np.abs(r - r_np).max())
        say()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write('Restraint at stored frames: numpy solver against remd_restraint_frames.  ms, median (min .. max); numpy %d runs, device '
                     '%d after one warm-up.\n\n' % (args.numpy_repeats, args.repeats))
            fh.write('\n'.join(lines))


if __name__ == '__main__':
    main()
