"""What an RMSD collective variable costs: one force evaluation with energies (HipEngine.custom_energies, host wall time with the
synchronisation it ends in) of a System of 3000 particles that holds one custom bond, next to the same System with a harmonic
CustomCVForce over one RMSDForce of 30, 300 and 3000 particles, at 8 and 24 replicas.

    python tools/custom_cv_microbench.py [--out FILE] [--replicas 8,24] [--repeats 20]

The difference of the two columns is the three launches of csrc/custom_cv.hip (superposition, expression, spread).  Each timing is
the median of `repeats` calls after two warm-up calls, with the spread (min .. max) next to it.  Appends to --out."""
import argparse
import copy
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                                   # noqa: E402
from custom_tabulated_microbench import engine_of, timed             # noqa: E402
from openmmtools_amd.system import System, CustomBondForce, CustomCVForce, RMSDForce   # noqa: E402

N = 3000


def systems(n_cv):
    rng = np.random.default_rng(n_cv)
    x = rng.uniform(-2.0, 2.0, (N, 3))
    base = System()
    for _ in range(N):
        base.addParticle(12.0)
    bond = CustomBondForce('0.5*kb*(r-0.1)^2'); bond.addGlobalParameter('kb', 100.0); bond.addBond(0, 1, [])
    base.addForce(bond)
    restrained = copy.deepcopy(base)
    f = CustomCVForce('0.5*k*v^2'); f.addGlobalParameter('k', 1000.0)
    f.addCollectiveVariable('v', RMSDForce(x + rng.normal(0.0, 0.05, x.shape), [int(p) for p in rng.permutation(N)[:n_cv]]))
    restrained.addForce(f)
    return base, restrained, x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--replicas', default='8,24')
    ap.add_argument('--repeats', type=int, default=20)
    a = ap.parse_args()
    lines = ['custom_cv_microbench: custom_energies() of %d particles, ms per call: median (min .. max) of %d' % (N, a.repeats)]
    for R in (int(r) for r in a.replicas.split(',')):
        for n_cv in (30, 300, 3000):
            base, restrained, x = systems(n_cv)
            t0 = timed(engine_of(base, x, None, R).custom_energies, a.repeats)
            eng = engine_of(restrained, x, None, R)
            t1 = timed(eng.custom_energies, a.repeats)
            lines.append('R = %2d, RMSD over %4d particles (RMSD %.4f nm): without %.4f (%.4f .. %.4f), with %.4f (%.4f .. %.4f), difference %.4f'
                         % (R, n_cv, eng.custom_cv_values()[0, 0], *t0, *t1, t1[0] - t0[0]))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'a') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
