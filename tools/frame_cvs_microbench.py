"""Cost of the collective variables of stored frames: analysis.frame_cvs_numpy against _engine.frame_cvs (csrc/frame_cvs.hip), the
device call timed whole (host wall clock around the call: table set-up, the upload of the frames in chunks, the kernels, the download)
and its kernels alone (device events, remd_frame_cvs' kernel_ms).  Seeded synthetic frames of the shapes of the package's test systems.
Needs an MI355X.

    python tools/frame_cvs_microbench.py [OUTPUT]      (default: profiles/frame_cvs_cost.txt)
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from openmmtools_amd import _engine                         # noqa: E402
from openmmtools_amd.multistate import analysis as an       # noqa: E402

REPEATS = 5


def shapes():
    rng = np.random.default_rng(2025)
    ref = rng.uniform(-0.6, 0.6, (156, 3))
    phi_psi = [an.DihedralCV(4, 6, 8, 14), an.DihedralCV(6, 8, 14, 16)]
    host_guest = [an.DistanceCV(list(range(126)), list(range(126, 156))), an.RMSDCV(ref, list(range(126)))]
    return [('phi/psi, 22 atoms, 24 x 10000 frames', phi_psi, 22, 24 * 10000),
            ('host-guest distance (126 + 30 atoms) + RMSD of the 126, 24 x 10000 frames', host_guest, 156, 24 * 10000),
            ('phi/psi, 22 atoms, 24 x 200 frames', phi_psi, 22, 24 * 200),
            ('host-guest distance + RMSD, 156 atoms, 24 x 200 frames', host_guest, 156, 24 * 200)]


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'frame_cvs_cost.txt')
    lines = ['# collective variables of stored frames: tools/frame_cvs_microbench.py on an MI355X; milliseconds, min ... max of %d calls after' % REPEATS,
             '# one warm-up call (numpy: 2 calls); device call = host wall clock of _engine.frame_cvs (tables, upload in chunks, kernels,',
             '# download); kernels = device events around the launches alone; frames f32, boxes f32, periodic variables']
    for name, cvs, n_atoms, F in shapes():
        rng = np.random.default_rng(F + n_atoms)
        pos = rng.uniform(0.0, 3.0, (F, n_atoms, 3)).astype(np.float32)
        box = (3.0 + rng.uniform(-0.1, 0.1, (F, 3))).astype(np.float32)
        masses = rng.uniform(1.0, 16.0, n_atoms)
        t_host = []
        for _ in range(2):
            t0 = time.perf_counter(); host = an.frame_cvs_numpy(cvs, pos, box, masses); t_host.append(1e3 * (time.perf_counter() - t0))
        dev = _engine.frame_cvs(cvs, pos, box, masses)                        # warm-up: the code object, the first allocations
        t_call, t_kernel = [], []
        for _ in range(REPEATS):
            timing = {}
            t0 = time.perf_counter(); dev = _engine.frame_cvs(cvs, pos, box, masses, timing=timing); t_call.append(1e3 * (time.perf_counter() - t0))
            t_kernel.append(timing['kernel_ms'])
        diff = float(np.abs(dev - host).max())
        lines += ['', name, '  frames %.1f MB' % (pos.nbytes / 1e6),
                  '  numpy        %9.2f ... %9.2f ms' % (min(t_host), max(t_host)),
                  '  device call  %9.2f ... %9.2f ms   (numpy / device call: %.1fx)' % (min(t_call), max(t_call), min(t_host) / min(t_call)),
                  '  kernels      %9.3f ... %9.3f ms   (%.0f%% of the call)' % (min(t_kernel), max(t_kernel), 100.0 * min(t_kernel) / min(t_call)),
                  '  max |device - numpy| %.2e' % diff]
        print('\n'.join(lines[-6:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
