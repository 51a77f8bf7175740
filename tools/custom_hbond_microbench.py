"""What a CustomHbondForce costs: one force evaluation with energies (HipEngine.custom_energies, host wall time with the synchronisation
it ends in) of 64 x 64, 512 x 512 and 2048 x 2048 donors x acceptors of three particles each at a liquid-like density (33 donors and 33
acceptors per nm^3, CutoffNonPeriodic, 1 nm), at 8 and 24 replicas, once with a distance-only expression and once with a distance, two
angles and a dihedral, through csrc/custom_hbond.hip; and, beside it, the same interaction as explicit bonds of a
CustomCompoundBondForce(6, ...) over the pairs that are in range at the start positions (csrc/custom_compound.hip), at the sizes where
that list stays below MAX_LIST bonds.

    python tools/custom_hbond_microbench.py [--out FILE] [--replicas 8,24] [--repeats 20] [--sizes 64,512,2048]

Each timing is the median of `repeats` calls after two warm-up calls, with the spread (min .. max) next to it.  Appends to --out."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                                   # noqa: E402
from custom_tabulated_microbench import engine_of, timed             # noqa: E402
from openmmtools_amd.system import System, CustomHbondForce, CustomCompoundBondForce   # noqa: E402

DENSITY, CUTOFF, MAX_LIST = 33.0, 1.0, 120000
EXPRESSIONS = {
    'distance': ('k*(distance(d1,a1)-0.3)^2*step(0.5-distance(d1,a1))', 'k*(distance(p1,p4)-0.3)^2*step(0.5-distance(p1,p4))'),
    'distance + 2 angles + dihedral': (
        'k*(distance(d1,a1)-0.3)^2*cos(angle(d2,d1,a1))^2*cos(angle(d1,a1,a2))^2*(1+cos(dihedral(d2,d1,a1,a2)))*step(0.5-distance(d1,a1))',
        'k*(distance(p1,p4)-0.3)^2*cos(angle(p2,p1,p4))^2*cos(angle(p1,p4,p5))^2*(1+cos(dihedral(p2,p1,p4,p5)))*step(0.5-distance(p1,p4))'),
}


def layout(n, seed):
    """n donors (atoms 3 i ...) and n acceptors (atoms 3 n + 3 j ...) of three particles, the first ones uniform in a cube of the density"""
    rng = np.random.default_rng(seed)
    L = (n / DENSITY) ** (1.0 / 3.0)
    x = np.zeros((6 * n, 3))
    x[0::3] = rng.uniform(0.0, L, (2 * n, 3))
    for k in (1, 2):
        u = rng.normal(size=(2 * n, 3))
        x[k::3] = x[k - 1::3] + 0.1 * u / np.linalg.norm(u, axis=1, keepdims=True)
    return x


def systems(n, x, texts):
    def bare():
        s = System()
        for _ in range(6 * n):
            s.addParticle(12.0)
        return s
    hb = CustomHbondForce(texts[0])
    hb.addGlobalParameter('k', 10.0)
    for i in range(n):
        hb.addDonor(3 * i, 3 * i + 1, 3 * i + 2)
        hb.addAcceptor(3 * (n + i), 3 * (n + i) + 1, 3 * (n + i) + 2)
    hb.setNonbondedMethod(CustomHbondForce.CutoffNonPeriodic)
    hb.setCutoffDistance(CUTOFF)
    dedicated = bare()
    dedicated.addForce(hb)
    d1, a1 = x[0:3 * n:3], x[3 * n::3]
    r = np.linalg.norm(a1[None, :, :] - d1[:, None, :], axis=2)
    I, J = np.nonzero(r < CUTOFF)
    listed = None
    if len(I) <= MAX_LIST:
        c = CustomCompoundBondForce(6, texts[1])
        c.addGlobalParameter('k', 10.0)
        for i, j in zip(I.tolist(), J.tolist()):
            c.addBond([3 * i, 3 * i + 1, 3 * i + 2, 3 * (n + j), 3 * (n + j) + 1, 3 * (n + j) + 2], [])
        listed = bare()
        listed.addForce(c)
    return dedicated, listed, len(I)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--replicas', default='8,24')
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--sizes', default='64,512,2048')
    a = ap.parse_args()
    lines = ['custom_hbond_microbench: custom_energies(), host wall time, ms per call: median (min .. max) of %d calls after 2 warm-up calls' % a.repeats]
    for name, texts in EXPRESSIONS.items():
        for n in (int(v) for v in a.sizes.split(',')):
            x = layout(n, n)
            dedicated, listed, n_pairs = systems(n, x, texts)
            for R in (int(r) for r in a.replicas.split(',')):
                d = engine_of(dedicated, x, None, R)
                t1 = timed(d.custom_energies, a.repeats)
                line = '%-30s %4d x %4d (%5d tiles, %6d pairs in range), R = %2d: CustomHbondForce %.4f (%.4f .. %.4f)' % (
                    name, n, n, ((n + 63) // 64) ** 2, n_pairs, R, *t1)
                if listed is not None:
                    w = engine_of(listed, x, None, R)
                    t2 = timed(w.custom_energies, a.repeats)
                    ed, ew = d.custom_energies().sum(), w.custom_energies().sum()
                    line += ', explicit compound bonds %.4f (%.4f .. %.4f); listed / CustomHbondForce %.2f; energies agree to %.1e' % (
                        *t2, t2[0] / t1[0], abs(ed - ew) / max(abs(ew), 1e-300))
                else:
                    line += ', explicit compound bonds: not run (the list exceeds %d bonds)' % MAX_LIST
                lines.append(line)
                print(line, flush=True)
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
