"""What a CustomManyParticleForce costs: one force evaluation with energies (HipEngine.custom_energies, host wall time with the
synchronisation it ends in) of the three-body term of testsystems.StillingerWeberFluid (mW water at liquid density, UniqueCentralParticle,
CutoffPeriodic at 1.8 sigma) alone, at 512 and 4096 particles and 8 and 24 replicas, through csrc/custom_manyparticle.hip (the
neighbour-row launch and the set launch together); and of an Axilrod-Teller term on the 1000 particles of
testsystems.CustomLennardJonesFluidMixture at a 1 nm cutoff (SinglePermutation).  The lattice gives every particle 6 neighbours (15 pairs
per central particle, a quarter of one batch), so two more cases stand beside it: the 512-particle fluid after 1000 BAOAB steps of 5 fs
at 300 K under both of its forces (a liquid's rows; the mean and largest row are printed), and rows near their capacity: a smooth
three-body term on the 512-particle lattice at a cutoff of 0.955 nm, 122 neighbours and 7381 candidate pairs per central particle.

    python tools/custom_manyparticle_microbench.py [--out FILE] [--replicas 8,24] [--repeats 20] [--sizes 512,4096]

Each timing is the median of `repeats` calls after two warm-up calls, with the spread (min .. max) next to it.  Appends to --out."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                                   # noqa: E402
from custom_tabulated_microbench import engine_of, timed, BETA       # noqa: E402
from openmmtools_amd._engine import HipEngine                        # noqa: E402
from openmmtools_amd.system import system_to_desc                    # noqa: E402
from openmmtools_amd import testsystems                              # noqa: E402
from openmmtools_amd.system import System, CustomManyParticleForce   # noqa: E402

AXILROD_TELLER = ('nu*(1+3*cos(angle(p2,p1,p3))*cos(angle(p1,p2,p3))*cos(angle(p1,p3,p2)))/(distance(p1,p2)*distance(p2,p3)*distance(p1,p3))^3; '
                  'nu=1e-4')


def only(system, force):
    """a System with the particles and box of ``system`` and ``force`` alone"""
    s = System()
    for m in system.masses:
        s.addParticle(m)
    s.setDefaultPeriodicBoxVectors(*system.getDefaultPeriodicBoxVectors())
    s.addForce(force)
    return s


def thermalised(ts, n_steps=1000):
    """the positions of test system ``ts`` after n_steps BAOAB steps of 5 fs at 300 K under all of its forces"""
    box = np.diag(ts.system.getDefaultPeriodicBoxVectors())
    desc = system_to_desc(ts.system, box=box)
    eng = HipEngine()
    eng.set_system(desc)
    eng.set_states(np.full(1, BETA))
    eng.set_custom_globals(np.tile(desc['custom_terms']['000']['global_defaults'], (1, 1)))
    eng.set_integrator('V R O R V', 0.005, 1.0, n_steps, True, 1e-8)
    eng.seed(5)
    eng.set_replicas(1, 0, np.asarray([ts.positions], dtype=np.float32).astype(np.float64), None, box[None, :], np.zeros(1, dtype=np.int64))
    eng.propagate(0)
    x = eng.get_replicas()[0][0]
    eng.close()
    return x


def rows(x, box, cutoff):
    """(mean, largest) neighbour count within ``cutoff`` under the box"""
    d = x[None, :, :] - x[:, None, :]
    d -= box * np.rint(d / box)
    n = ((d * d).sum(axis=2) < cutoff * cutoff).sum(axis=1) - 1
    return float(n.mean()), int(n.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--replicas', default='8,24')
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--sizes', default='512,4096')
    a = ap.parse_args()
    lines = ['custom_manyparticle_microbench: custom_energies(), host wall time, ms per call: median (min .. max) of %d calls after 2 warm-up calls' % a.repeats]
    cases = []
    for n in (int(v) for v in a.sizes.split(',')):
        ts = testsystems.StillingerWeberFluid(nparticles=n)
        cases.append(('mW three-body term, %d particles' % n, only(ts.system, ts.system.getForces()[1]), ts.positions))
    ts = testsystems.StillingerWeberFluid(nparticles=512)
    three = ts.system.getForces()[1]
    box512 = np.diag(ts.system.getDefaultPeriodicBoxVectors())
    x = thermalised(ts)
    cases.append(('mW three-body term, 512 particles after 1000 steps at 300 K (rows: mean %.1f, largest %d)' % rows(x, box512, three.getCutoffDistance()),
                  only(ts.system, three), x))
    dense = CustomManyParticleForce(3, 'exp(-3*(distance(p1,p2)+distance(p1,p3)))*(cos(angle(p2,p1,p3))+1/3)^2')
    for _ in range(512):
        dense.addParticle([], 0)
    dense.setPermutationMode(CustomManyParticleForce.UniqueCentralParticle)
    dense.setNonbondedMethod(CustomManyParticleForce.CutoffPeriodic)
    dense.setCutoffDistance(0.955)
    cases.append(('rows near capacity: 512-particle lattice, cutoff 0.955 nm (rows: mean %.1f, largest %d)' % rows(ts.positions, box512, 0.955),
                  only(ts.system, dense), ts.positions))
    lj = testsystems.CustomLennardJonesFluidMixture(nparticles=1000)
    at = CustomManyParticleForce(3, AXILROD_TELLER)
    for _ in range(1000):
        at.addParticle([], 0)
    at.setNonbondedMethod(CustomManyParticleForce.CutoffPeriodic)
    at.setCutoffDistance(1.0)
    cases.append(('Axilrod-Teller on the 1000-particle Lennard-Jones mixture, cutoff 1 nm', only(lj.system, at), lj.positions))
    for name, system, x in cases:
        box = np.diag(system.getDefaultPeriodicBoxVectors())
        for R in (int(r) for r in a.replicas.split(',')):
            e = engine_of(system, x, box, R)
            t = timed(e.custom_energies, a.repeats)
            line = '%-96s R = %2d: %.4f (%.4f .. %.4f), energy of replica 0 %.6g kJ/mol' % (name, R, *t, e.custom_energies()[0, 0])
            lines.append(line)
            print(line, flush=True)
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
