"""What a tabulated function of two arguments costs in a custom force: one force evaluation with energies (HipEngine.custom_energies,
host wall time with the synchronisation it ends in), a closed form against the same energy through a table, both in one build.

    python tools/custom_tabulated2d_microbench.py [--out FILE] [--replicas 8,24] [--repeats 20]

1. 70 custom torsions on 200 atoms: k (1 + cos(2 theta + 1)) (1.5 + sin(phase)), phase a per-torsion parameter, against a periodic
   24 x 24 Continuous2DFunction of (theta, phase) over [-pi, pi]^2 sampled from it (a CMAP-sized map; the two energies differ by the
   interpolation error of 24 points per period, which is printed).
2. CustomLennardJonesFluidMixture (1000 particles, no long-range correction: a table refuses it): its Lennard-Jones string against the
   same energy with epsilon and sigma looked up in 2 x 2 Discrete2DFunctions of the particles' types (the parameter `charge`, which
   the string does not read, carries the type).

Each timing is the median of `repeats` calls after two warm-up calls, with the spread (min .. max) next to it.  Appends to --out."""
import argparse
import copy
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                                   # noqa: E402
from custom_tabulated_microbench import engine_of, timed             # noqa: E402
from openmmtools_amd import testsystems                              # noqa: E402
from openmmtools_amd.system import (System, CustomNonbondedForce, CustomTorsionForce, Continuous2DFunction, Discrete2DFunction)   # noqa: E402


def torsion_pair():
    rng = np.random.default_rng(70)
    x = rng.uniform(-1.4, 1.4, (200, 3))
    out = []
    for tabulated in (False, True):
        s = System()
        for _ in range(200):
            s.addParticle(12.0)
        f = CustomTorsionForce('k*map(theta, phase)' if tabulated else 'k*(1 + cos(2*theta + 1))*(1.5 + sin(phase))')
        f.addPerTorsionParameter('k')
        f.addPerTorsionParameter('phase')
        if tabulated:
            g = np.linspace(-math.pi, math.pi, 24)
            v = (1.0 + np.cos(2.0 * g[None, :] + 1.0)) * (1.5 + np.sin(g[:, None]))          # [j][i] = f(theta_i, phase_j)
            v[:, -1], v[-1, :] = v[:, 0], v[0, :]
            f.addTabulatedFunction('map', Continuous2DFunction(24, 24, v.reshape(-1), -math.pi, math.pi, -math.pi, math.pi, periodic=True))
        for t in range(70):
            f.addTorsion(t, (t + 50) % 200, (t + 100) % 200, (t + 150) % 200, [5.0 + 0.1 * t, -3.0 + 6.0 * ((0.618 * t) % 1.0)])
        s.addForce(f)
        out.append(s)
    return out[0], out[1], x, None


def fluid_pair():
    """(the string's System, the type tables' System, positions, box)"""
    fluid = testsystems.CustomLennardJonesFluidMixture(nparticles=1000, dispersion_correction=False)
    analytic = fluid.system
    tabulated = copy.deepcopy(analytic)
    a = [f for f in analytic.getForces() if isinstance(f, CustomNonbondedForce)][0]
    t = [f for f in tabulated.getForces() if isinstance(f, CustomNonbondedForce)][0]
    text = a.getEnergyFunction()
    sigma, epsilon = (float(text.split('%s = ' % n)[1].split(';')[0]) for n in ('sigma', 'epsilon'))
    t.setEnergyFunction('4*eps(charge1,charge2)*((sig(charge1,charge2)/r)^12 - (sig(charge1,charge2)/r)^6)')
    t.addTabulatedFunction('eps', Discrete2DFunction(2, 2, [epsilon] * 4))
    t.addTabulatedFunction('sig', Discrete2DFunction(2, 2, [sigma] * 4))
    for i in range(t.getNumParticles()):
        p = t.getParticleParameters(i)
        t.setParticleParameters(i, [float(i % 2)] + list(p[1:]))
    box = np.diag(np.asarray(analytic.getDefaultPeriodicBoxVectors(), dtype=np.float64)).astype(np.float32).astype(np.float64)
    return analytic, tabulated, np.asarray(fluid.positions, dtype=np.float64), box


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--replicas', default='8,24')
    ap.add_argument('--repeats', type=int, default=20)
    args = ap.parse_args()
    lines = ['Tables of two arguments against closed forms in custom-force expressions: one force evaluation with energies, host wall ms,'
             ' median of %d after two warm-up calls (min .. max)' % args.repeats]
    for title, pair in (('70 custom torsions on 200 atoms: k (1 + cos(2 theta + 1)) (1.5 + sin(phase)) against a periodic 24 x 24 map of (theta, phase)', torsion_pair),
                        ('CustomLennardJonesFluidMixture, 1000 particles: Lennard-Jones string against 2 x 2 type lookups of epsilon and sigma', fluid_pair)):
        analytic, tabulated, x, box = pair()
        lines += ['', title]
        for R in (int(v) for v in args.replicas.split(',')):
            e = []
            for label, system in (('closed', analytic), ('tabulated', tabulated)):
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
