"""What a CustomNonbondedForce costs (csrc/custom_nonbonded.hip; profiles/custom_nonbonded_cost.txt).

  python tools/custom_nonbonded_cost.py lanes            host only: the share of lanes active in the evaluation stage (pairs evaluated
                                                         / 64 batches, a tile of p pairs running ceil(p / 64) batches) of the systems below
  python tools/custom_nonbonded_cost.py launches         on a GPU, to be run under a kernel trace: 12 force evaluations with energies of
                                                         WCAFluid (216), CustomLennardJonesFluidMixture (1000) and a 4096-particle fluid as a
                                                         CustomNonbondedForce, and of the LennardJonesFluid twins on the built-in pair path,
                                                         each with 8 and with 24 replicas
  python tools/custom_nonbonded_cost.py trace FILE.csv   the mean duration of every kernel of such a trace, by kernel and grid
"""
import csv
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from openmmtools_amd import testsystems
from openmmtools_amd.system import System, CustomNonbondedForce, NonbondedForce, system_to_desc

BETA = 1.0 / (0.008314462618153242 * 120.0)


def custom_lj_fluid(n):
    """LennardJonesFluid(n) with its NonbondedForce replaced by a CustomNonbondedForce of the same cutoff, switch and correction"""
    lj = testsystems.LennardJonesFluid(nparticles=n)
    nb = [f for f in lj.system.getForces() if isinstance(f, NonbondedForce)][0]
    sigma, epsilon = nb.getParticleParameters(0)[1:]
    c = CustomNonbondedForce('4*epsilon*((sigma/r)^12 - (sigma/r)^6); sigma = %r; epsilon = %r' % (sigma, epsilon))
    s = System()
    for i in range(n):
        s.addParticle(lj.system.getParticleMass(i))
        c.addParticle([])
    s.setDefaultPeriodicBoxVectors(*lj.system.getDefaultPeriodicBoxVectors())
    c.setNonbondedMethod(CustomNonbondedForce.CutoffPeriodic)
    c.setCutoffDistance(nb.getCutoffDistance())
    c.setUseSwitchingFunction(True)
    c.setSwitchingDistance(nb.getSwitchingDistance())
    c.setUseLongRangeCorrection(True)
    s.addForce(c)
    return s, lj.positions


def cases():
    wca, mix = testsystems.WCAFluid(), testsystems.CustomLennardJonesFluidMixture()
    big, big_x = custom_lj_fluid(4096)
    return [('WCAFluid(216)', wca.system, wca.positions, testsystems.LennardJonesFluid(nparticles=216)),
            ('CustomLennardJonesFluidMixture(1000)', mix.system, mix.positions, testsystems.LennardJonesFluid(nparticles=1000)),
            ('custom LJ fluid (4096)', big, big_x, testsystems.LennardJonesFluid(nparticles=4096))]


def lanes():
    for name, system, x, _ in cases():
        f = [g for g in system.getForces() if isinstance(g, CustomNonbondedForce)][0]
        L = np.diag(system.getDefaultPeriodicBoxVectors())
        x = np.asarray(x, dtype=np.float32).astype(np.float64)
        n, rc = len(x), f.getCutoffDistance()
        pairs = batches = 0
        nb = (n + 63) // 64
        for ib in range(nb):
            xi = x[64 * ib:64 * ib + 64]
            d = x[None, 64 * ib:, :] - xi[:, None, :]
            d -= L * np.rint(d / L)
            inside = (d * d).sum(axis=2) < rc * rc
            jj = np.arange(64 * ib, n)[None, :]
            inside &= jj > (64 * ib + np.arange(len(xi)))[:, None]
            per_tile = np.add.reduceat(inside.sum(axis=0), np.arange(0, n - 64 * ib, 64))
            pairs += int(per_tile.sum())
            batches += int(np.ceil(per_tile / 64.0).sum())
        print('%-38s N %5d  tiles %5d  pairs %8d  batches %6d  active lanes %.3f  batches per tile %.2f'
              % (name, n, nb * (nb + 1) // 2, pairs, batches, pairs / (64.0 * max(batches, 1)), batches / (nb * (nb + 1) / 2.0)))


def launches():
    from openmmtools_amd._engine import HipEngine
    for name, system, x, twin in cases():
        for R in (8, 24):
            for tag, s, pos in (('custom', system, x), ('built-in', twin.system, twin.positions)):
                eng = HipEngine()
                desc = system_to_desc(s)
                eng.set_system(desc)
                eng.set_states(np.full(1, BETA))
                if desc.get('custom_terms'):
                    eng.set_custom_globals(np.zeros((1, len(desc['custom_globals']['names']))) + desc['custom_globals']['defaults'])
                box = np.tile(np.diag(s.getDefaultPeriodicBoxVectors()), (R, 1))
                xs = np.tile(np.asarray(pos, dtype=np.float64), (R, 1, 1))
                for it in range(12):
                    eng.set_replicas(R, 0, xs, None, box, np.zeros(R, dtype=np.int64))      # (forgets the forces: the next call evaluates)
                    eng.compute_energies()
                eng.sync()
                print('%s, %s, %d replicas: done' % (name, tag, R), flush=True)
                eng.close()


def trace(path):
    rows = {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            key = (r['Kernel_Name'].replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0][-60:], r.get('Grid_Size_X', r.get('Grid_Size', '')), r.get('Grid_Size_Y', ''))
            rows.setdefault(key, []).append(int(r['End_Timestamp']) - int(r['Start_Timestamp']))
    for key, v in sorted(rows.items()):
        v = np.array(v[len(v) // 6:], dtype=np.float64)              # (the first launches of a configuration are left out)
        print('%-62s grid %8s x %3s  launches %4d  mean %9.1f us  min %9.1f us' % (key[0], key[1], key[2], len(v), v.mean() / 1e3, v.min() / 1e3))


if __name__ == '__main__':
    what = sys.argv[1] if len(sys.argv) > 1 else 'lanes'
    if what == 'lanes':
        lanes()
    elif what == 'launches':
        launches()
    else:
        trace(sys.argv[2])
