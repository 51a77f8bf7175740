"""What a CustomGBForce on the general path costs (openmmtools_amd/custom_gb.py compile_custom_gb, csrc/custom_gb.hip): one force evaluation
with energies (the potential read back: host wall time with the synchronisation it ends in) of the OBC2 model written so that the
recognizer refuses it (one pair of parentheses more), beside the same model on csrc/gbsa.hip, on testsystems.AlanineDipeptideImplicit
(22 atoms, NoCutoff), testsystems.CustomGBForceSystem (140 ions, CutoffPeriodic 2 nm) and a synthetic droplet of 2000 particles
(NoCutoff, the GB force alone), at 8 and 24 replicas; and the HCT strings of AlanineDipeptideImplicit(implicitSolvent='HCT').

    python tools/custom_gb_expr_microbench.py [--out FILE] [--replicas 8,24] [--repeats 20] [--sizes 22,140,2000]

Each timing is the median of `repeats` calls after two warm-up calls, with the spread (min .. max) next to it.  Appends to --out.  The
five launches of one evaluation are told apart by a kernel trace of this program (rocprofv3 --kernel-trace --stats -- python
tools/custom_gb_expr_microbench.py --sizes 2000 --replicas 8 --repeats 5)."""
import argparse
import copy
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                                   # noqa: E402
from custom_tabulated_microbench import timed, BETA                  # noqa: E402
from openmmtools_amd._engine import HipEngine                        # noqa: E402
from openmmtools_amd.system import System, NonbondedForce, CustomGBForce, system_to_desc   # noqa: E402
from openmmtools_amd import testsystems                              # noqa: E402

TEMPLATE_TANH, GENERAL_TANH = 'tanh(1*psi-0.8*psi^2+4.85*psi^3)', 'tanh((1*psi-0.8*psi^2+4.85*psi^3))'


def obc2_custom(n, charge, radius, scale, method=0, cutoff=1.0):
    """the OBC2 strings of testsystems.CustomGBForceSystem with numbers for the dielectrics"""
    ref = [f for f in testsystems.CustomGBForceSystem().system.getForces() if isinstance(f, CustomGBForce)][0]
    f = copy.deepcopy(ref)
    f.particles = [(float(q), float(r), float(s)) for q, r, s in zip(charge, radius, scale)]
    f.setNonbondedMethod(method); f.setCutoffDistance(cutoff)
    return f


def general(system):
    """the System with its CustomGBForce in strings the recognizer refuses: the same model on the general path"""
    s = copy.deepcopy(system)
    for f in s.forces:
        if isinstance(f, CustomGBForce):
            name, text, kind = f.computed[1]
            assert TEMPLATE_TANH in text
            f.computed[1] = (name, text.replace(TEMPLATE_TANH, GENERAL_TANH), kind)
    return s


def droplet(n):
    rng = np.random.default_rng(n)
    side = int(np.ceil(n ** (1.0 / 3.0)))
    x = np.array([[a, b, c] for a in range(side) for b in range(side) for c in range(side)], dtype=np.float64)[:n] * 0.35 + rng.uniform(-0.03, 0.03, (n, 3))
    s = System()
    nb = NonbondedForce()
    nb.setNonbondedMethod(NonbondedForce.NoCutoff)
    for _ in range(n):
        s.addParticle(12.0)
        nb.addParticle(0.0, 0.3, 0.0)
    s.addForce(nb)
    s.addForce(obc2_custom(n, rng.uniform(-0.5, 0.5, n), rng.uniform(0.12, 0.2, n), rng.uniform(0.7, 0.9, n)))
    return s, x


def engine_of(system, x, box, R):
    desc = system_to_desc(system, box=box)
    eng = HipEngine()
    eng.set_system(desc)
    eng.set_states(np.full(1, BETA))
    if 'custom_terms' in desc:
        eng.set_custom_globals(np.zeros((1, 0)))
    rng = np.random.default_rng(R)
    xs = np.array([x + rng.normal(0.0, 0.002, x.shape) for _ in range(R)], dtype=np.float32).astype(np.float64)
    eng.set_replicas(R, 0, xs, None, np.zeros((R, 3)) if box is None else np.tile(box, (R, 1)), np.zeros(R, dtype=np.int64))
    return eng, 'custom_terms' in desc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--replicas', default='8,24')
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--sizes', default='22,140,2000')
    a = ap.parse_args()
    sizes = [int(v) for v in a.sizes.split(',')]
    lines = ['custom_gb_expr_microbench: one force evaluation with energies, host wall time, ms per call: median (min .. max) of %d calls after 2 warm-up calls' % a.repeats]
    cases = []
    if 22 in sizes:
        al = testsystems.AlanineDipeptideImplicit()
        gb = al.system.forces[-1]
        p = np.array(gb.particles, dtype=np.float64)
        template = copy.deepcopy(al.system)
        template.forces[-1] = obc2_custom(22, p[:, 0], p[:, 1], p[:, 2])
        x = np.asarray(al.positions, dtype=np.float64)
        cases += [('AlanineDipeptideImplicit (22), OBC2 on gbsa.hip', template, x, None), ('AlanineDipeptideImplicit (22), OBC2 on custom_gb.hip', general(template), x, None),
                  ('AlanineDipeptideImplicit (22), HCT on custom_gb.hip', testsystems.AlanineDipeptideImplicit(implicitSolvent='HCT').system, x, None)]
    if 140 in sizes:
        ions = testsystems.CustomGBForceSystem()
        box = np.diag(ions.system.getDefaultPeriodicBoxVectors())
        x = np.asarray(ions.positions, dtype=np.float64)
        cases += [('CustomGBForceSystem (140, cutoff 2 nm), OBC2 on gbsa.hip', ions.system, x, box), ('CustomGBForceSystem (140, cutoff 2 nm), OBC2 on custom_gb.hip', general(ions.system), x, box)]
    for n in sizes:
        if n not in (22, 140):
            s, x = droplet(n)
            cases += [('droplet (%d, NoCutoff), OBC2 on gbsa.hip' % n, s, x, None), ('droplet (%d, NoCutoff), OBC2 on custom_gb.hip' % n, general(s), x, None)]
    for name, system, x, box in cases:
        for R in (int(r) for r in a.replicas.split(',')):
            e, is_general = engine_of(system, x, box, R)
            assert is_general == ('custom_gb.hip' in name)
            read = lambda: e.get_replicas(positions=False, velocities=False, potential=True)[2]
            force = lambda: (e.set_replicas(R, 0, e.get_replicas()[0], None, np.zeros((R, 3)) if box is None else np.tile(box, (R, 1)), np.zeros(R, dtype=np.int64)), read())
            t = timed(lambda: force(), a.repeats)
            line = '%-72s R = %2d: %.4f (%.4f .. %.4f), potential of replica 0 %.8g kJ/mol' % (name, R, *t, read()[0])
            lines.append(line)
            print(line, flush=True)
            e.close()
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
