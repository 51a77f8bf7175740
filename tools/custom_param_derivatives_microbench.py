"""Cost of one HipEngine.custom_energy_parameter_derivatives() call against one energy evaluation (custom_energies()), for 70 custom
torsions and for the six-particle Boresch compound bond, at 8 and 24 replicas.  Both calls end in a device-to-host copy and a stream
synchronisation, so each figure is the wall-clock time of a whole host call: launch latency, kernels, copy.  Median, minimum and maximum
of 200 timed calls after 20 warm-up calls.  Prints the table; the text goes to profiles/custom_param_derivatives_cost.txt by hand, with the
compiler's resource usage and the headline benchmark beside it.

    python tools/custom_param_derivatives_microbench.py
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from openmmtools_amd._engine import HipEngine                                     # noqa: E402
from openmmtools_amd.system import System, system_to_desc, CustomTorsionForce, CustomCompoundBondForce   # noqa: E402

BETA = 1.0 / (0.008314462618153242 * 300.0)
BORESCH = ('lambda_restraints*0.5*(K_r*(distance(p3,p4)-r_aA0)^2 + K_thetaA*(angle(p2,p3,p4)-theta_A0)^2 + K_thetaB*(angle(p3,p4,p5)-theta_B0)^2'
           ' + K_phi*(2-cos(dihedral(p1,p2,p3,p4)-phi_A0)-cos(dihedral(p3,p4,p5,p6)-phi_C0)))')


def torsions():
    rng = np.random.default_rng(1)
    f = CustomTorsionForce('lam*k*(1+cos(n*theta-ph))')
    f.addGlobalParameter('lam', 0.5)
    for name in ('k', 'n', 'ph'):
        f.addPerTorsionParameter(name)
    for i in range(70):
        f.addTorsion(i, i + 1, i + 2, i + 3, [rng.uniform(1.0, 9.0), float(1 + i % 3), rng.uniform(-3.0, 3.0)])
    f.addEnergyParameterDerivative('lam')
    return f, np.cumsum(rng.normal(0.0, 0.08, (73, 3)) + [0.1, 0.0, 0.0], axis=0)


def boresch():
    f = CustomCompoundBondForce(6, BORESCH)
    for n, v in dict(lambda_restraints=0.7, K_r=4184.0, r_aA0=0.45, K_thetaA=41.84, theta_A0=1.9, K_thetaB=41.84, theta_B0=1.4, K_phi=30.0,
                     phi_A0=0.3, phi_C0=-1.1).items():
        f.addGlobalParameter(n, v)
    f.addBond([0, 1, 2, 3, 4, 5])
    f.addEnergyParameterDerivative('lambda_restraints')
    x = np.array([[0.0, 0.0, 0.0], [0.15, 0.02, 0.0], [0.22, 0.14, 0.03], [0.6, 0.3, 0.1], [0.72, 0.25, 0.2], [0.8, 0.36, 0.27]])
    return f, x


def timed(call, n=200, warm=20):
    for _ in range(warm):
        call()
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e6)
    return np.median(t), min(t), max(t)


def main():
    print('%-22s %3s  %-28s %-28s' % ('system', 'R', 'derivative call (us)', 'energy evaluation (us)'))
    for name, make in (('70 custom torsions', torsions), ('Boresch compound bond', boresch)):
        for R in (8, 24):
            f, x = make()
            s = System()
            for _ in range(len(x)):
                s.addParticle(12.0)
            s.addForce(f)
            desc = system_to_desc(s)
            eng = HipEngine()
            eng.set_system(desc)
            eng.set_states(np.full(R, BETA))
            d = np.array(desc['custom_globals']['defaults'], dtype=np.float64)
            table = np.tile(d, (R, 1))
            table[:, 0] = np.linspace(0.1, 1.0, R)
            eng.set_custom_globals(table)
            eng.set_replicas(R, 0, np.stack([x + 0.001 * r for r in range(R)]), None, np.zeros((R, 3)), np.arange(R))
            a, b = timed(eng.custom_energy_parameter_derivatives), timed(eng.custom_energies)
            print('%-22s %3d  median %6.1f (%6.1f ... %6.1f)   median %6.1f (%6.1f ... %6.1f)' % ((name, R) + a + b))


if __name__ == '__main__':
    main()
