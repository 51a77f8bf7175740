"""What a tabulated function costs in a custom force: one force evaluation with energies (HipEngine.custom_energies, host wall time
with the synchronisation it ends in), the analytic expression against the same energy as a table, both in one build.

    python tools/custom_tabulated_microbench.py [--out FILE] [--replicas 8,24] [--repeats 20]

1. CustomLennardJonesFluidMixture (1000 particles, no long-range correction: a table refuses it): its Lennard-Jones string against
   a 2048-point Continuous1DFunction of r over [0.2 nm, cutoff] sampled from the same string.
2. 70 custom torsions on 200 atoms: k (1 + cos(2 theta + 1)) against a periodic 2048-point table of theta sampled from it.

Each timing is the median of `repeats` calls after two warm-up calls, with the spread (min .. max) next to it.  Appends to --out."""
import argparse
import copy
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                                   # noqa: E402
from openmmtools_amd import testsystems                              # noqa: E402
from openmmtools_amd._engine import HipEngine                        # noqa: E402
from openmmtools_amd.system import (System, system_to_desc, CustomNonbondedForce, CustomTorsionForce, Continuous1DFunction)   # noqa: E402

BETA = 1.0 / (0.008314462618153242 * 300.0)


def timed(fn, repeats):
    fn(); fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), min(t), max(t)


def engine_of(system, x, box, R):
    desc = system_to_desc(system, box=box)
    eng = HipEngine()
    eng.set_system(desc)
    eng.set_states(np.full(1, BETA))
    eng.set_custom_globals(np.tile(desc['custom_terms']['000']['global_defaults'], (1, 1)))
    rng = np.random.default_rng(R)
    xs = np.array([x + rng.normal(0.0, 0.002, x.shape) for _ in range(R)], dtype=np.float32).astype(np.float64)
    eng.set_replicas(R, 0, xs, None, np.zeros((R, 3)) if box is None else np.tile(box, (R, 1)), np.zeros(R, dtype=np.int64))
    return eng


def fluid_pair():
    """(analytic System, tabulated System, positions, box)"""
    fluid = testsystems.CustomLennardJonesFluidMixture(nparticles=1000, dispersion_correction=False)
    analytic = fluid.system
    tabulated = copy.deepcopy(analytic)
    a = [f for f in analytic.getForces() if isinstance(f, CustomNonbondedForce)][0]
    t = [f for f in tabulated.getForces() if isinstance(f, CustomNonbondedForce)][0]
    text = a.getEnergyFunction()
    sigma, epsilon = (float(text.split('%s = ' % n)[1].split(';')[0]) for n in ('sigma', 'epsilon'))
    r = np.linspace(0.2, a.getCutoffDistance(), 2048)
    t.setEnergyFunction('tab(r)')
    t.addTabulatedFunction('tab', Continuous1DFunction(4.0 * epsilon * ((sigma / r) ** 12 - (sigma / r) ** 6), 0.2, a.getCutoffDistance()))
    box = np.diag(np.asarray(analytic.getDefaultPeriodicBoxVectors(), dtype=np.float64)).astype(np.float32).astype(np.float64)
    return analytic, tabulated, np.asarray(fluid.positions, dtype=np.float64), box


def torsion_pair():
    rng = np.random.default_rng(70)
    x = rng.uniform(-1.4, 1.4, (200, 3))
    out = []
    for tabulated in (False, True):
        s = System()
        for _ in range(200):
            s.addParticle(12.0)
        f = CustomTorsionForce('k*per(theta)' if tabulated else 'k*(1 + cos(2*theta + 1))')
        f.addPerTorsionParameter('k')
        if tabulated:
            th = np.linspace(-math.pi, math.pi, 2048)
            y = 1.0 + np.cos(2.0 * th + 1.0)
            y[-1] = y[0]
            f.addTabulatedFunction('per', Continuous1DFunction(y, -math.pi, math.pi, periodic=True))
        for t in range(70):
            f.addTorsion(t, (t + 50) % 200, (t + 100) % 200, (t + 150) % 200, [5.0 + 0.1 * t])
        s.addForce(f)
        out.append(s)
    return out[0], out[1], x, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--replicas', default='8,24')
    ap.add_argument('--repeats', type=int, default=20)
    args = ap.parse_args()
    lines = ['Tabulated against analytic custom-force expressions: one force evaluation with energies, host wall ms, median of %d after'
             ' two warm-up calls (min .. max)' % args.repeats]
    for title, pair in (('CustomLennardJonesFluidMixture, 1000 particles: Lennard-Jones string against a 2048-point table of r', fluid_pair),
                        ('70 custom torsions on 200 atoms: k (1 + cos(2 theta + 1)) against a periodic 2048-point table', torsion_pair)):
        analytic, tabulated, x, box = pair()
        lines += ['', title]
        for R in (int(v) for v in args.replicas.split(',')):
            e = []
            for label, system in (('analytic', analytic), ('tabulated', tabulated)):
                eng = engine_of(system, x, box, R)
                lines.append('  R = %2d %-9s %9.3f (%.3f .. %.3f)' % ((R, label) + timed(eng.custom_energies, args.repeats)))
                e.append(eng.custom_energies()[:, -1])
            lines.append('  R = %2d largest relative difference of the two energies: %.2e' % (R, np.max(np.abs(e[0] - e[1]) / np.abs(e[0]))))
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'a') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
