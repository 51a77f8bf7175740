"""What a CMAPTorsionForce costs: one force evaluation with energies (HipEngine.custom_energies, host wall time with the synchronisation
it ends in) of a chain with 70 and with 2000 torsion pairs on three 24 x 24 maps, at 8 and 24 replicas, through csrc/cmap.hip and, beside
it, through the workaround the force replaces: one CustomCompoundBondForce(8, 'm(dihedral(p1,p2,p3,p4), dihedral(p5,p6,p7,p8))') per
map with the periodic Continuous2DFunction on the edge-repeated grid (csrc/custom_compound.hip: the stack machine, eight seeded passes).

    python tools/cmap_microbench.py [--out FILE] [--replicas 8,24] [--repeats 20]

Both columns hold the launch and the synchronisation of an otherwise empty System (its one custom bond is timed alone as `base`); a
difference from base inside base's own spread is no measurement, so the ratio printed is that of the whole calls.
Each timing is the median of `repeats` calls after two warm-up calls, with the spread (min .. max) next to it.  Appends to --out."""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                                   # noqa: E402
from custom_tabulated_microbench import engine_of, timed             # noqa: E402
from openmmtools_amd.system import System, CustomBondForce, CustomCompoundBondForce, CMAPTorsionForce, Continuous2DFunction   # noqa: E402

SIZE = 24


def chain(n_atoms, seed):
    """a random walk of 0.15 nm bonds whose consecutive bonds are never nearly parallel"""
    rng = np.random.default_rng(seed)
    x = np.zeros((n_atoms, 3))
    prev = np.array([1.0, 0.0, 0.0])
    for i in range(1, n_atoms):
        while True:
            d = rng.normal(size=3); d /= np.linalg.norm(d)
            if abs(np.dot(d, prev)) < 0.8:
                break
        x[i] = x[i - 1] + 0.15 * d
        prev = d
    return x


def maps():
    a = 2.0 * math.pi * np.arange(SIZE) / SIZE
    phi, psi = a[None, :], a[:, None]
    return [(8.0 + (3.0 + k) * np.cos(phi) + 2.0 * np.sin(2.0 * psi) + 1.5 * np.cos(phi - psi)).reshape(-1) for k in range(3)]


def systems(n_terms):
    n_atoms = n_terms + 4
    x = chain(n_atoms, n_terms)

    def bare():
        s = System()
        for _ in range(n_atoms):
            s.addParticle(12.0)
        return s
    base = bare()
    bond = CustomBondForce('0.5*kb*(r-0.1)^2'); bond.addGlobalParameter('kb', 100.0); bond.addBond(0, 1, [])
    base.addForce(bond)
    terms = [((5 * t + 1) % 3, t, t + 1, t + 2, t + 3, t + 1, t + 2, t + 3, t + 4) for t in range(n_terms)]
    dedicated = bare()
    f = CMAPTorsionForce()
    for energy in maps():
        f.addMap(SIZE, energy)
    for row in terms:
        f.addTorsion(*row)
    dedicated.addForce(f)
    workaround = bare()
    for m, energy in enumerate(maps()):
        grid = energy.reshape(SIZE, SIZE)
        grid = np.concatenate([grid, grid[:1]], axis=0)
        grid = np.concatenate([grid, grid[:, :1]], axis=1)
        c = CustomCompoundBondForce(8, 'm(dihedral(p1,p2,p3,p4), dihedral(p5,p6,p7,p8))')
        c.addTabulatedFunction('m', Continuous2DFunction(SIZE + 1, SIZE + 1, grid.reshape(-1), 0.0, 2.0 * math.pi, 0.0, 2.0 * math.pi, periodic=True))
        for row in terms:
            if row[0] == m:
                c.addBond(list(row[1:]), [])
        workaround.addForce(c)
    return base, dedicated, workaround, x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--replicas', default='8,24')
    ap.add_argument('--repeats', type=int, default=20)
    a = ap.parse_args()
    lines = ['cmap_microbench: custom_energies(), three %d x %d maps, ms per call: median (min .. max) of %d' % (SIZE, SIZE, a.repeats)]
    for R in (int(r) for r in a.replicas.split(',')):
        for n_terms in (70, 2000):
            base, dedicated, workaround, x = systems(n_terms)
            t0 = timed(engine_of(base, x, None, R).custom_energies, a.repeats)
            d = engine_of(dedicated, x, None, R)
            t1 = timed(d.custom_energies, a.repeats)
            w = engine_of(workaround, x, None, R)
            t2 = timed(w.custom_energies, a.repeats)
            same = abs(d.custom_energies().sum() - w.custom_energies().sum()) / abs(w.custom_energies().sum())
            lines.append('R = %2d, %4d torsion pairs: base %.4f (%.4f .. %.4f), CMAPTorsionForce %.4f (%.4f .. %.4f), compound-bond workaround '
                         '%.4f (%.4f .. %.4f); above base %+.4f against %+.4f; whole calls, workaround / CMAPTorsionForce: %.2f; energies agree to %.1e'
                         % (R, n_terms, *t0, *t1, *t2, t1[0] - t0[0], t2[0] - t0[0], t2[0] / t1[0], same))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'a') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
