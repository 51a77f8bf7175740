"""Cost of one HipEngine.custom_energy_parameter_derivatives_at_states() call against the only route there was before it: K calls of
custom_energy_parameter_derivatives(), the replicas relabelled to state l before call l (set_labels).  The systems of
tools/custom_param_derivatives_microbench.py (70 custom torsions, the Boresch compound bond) and one of each kind with a staging
launch the fused call runs once instead of K times (a centroid bond, a donor-acceptor force, a many-particle force), at 8 and 24
replicas with K = 24 states.

Host wall time: the whole call or loop of calls, each ending in a device-to-host copy and a stream synchronisation; 20 warm-up
repeats, then 100 timed ones: median (minimum ... maximum) in microseconds.  Kernel time: the engine's event profile over the launches
of the call ('custom_dpar_states' / 'custom_dpar': the staging launches, the part's kernel and the reduce), per call, in a run of its
own (the events serialise the stream).  Also the size of the partial buffer of the fused call, R K n (wavefronts) doubles.
Prints the table; the text goes to profiles/custom_param_derivatives_states_cost.txt by hand.

    python tools/custom_param_derivatives_states_microbench.py
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from custom_param_derivatives_microbench import torsions, boresch, BETA                               # noqa: E402
from openmmtools_amd._engine import HipEngine                                                           # noqa: E402
from openmmtools_amd.system import (System, system_to_desc, CustomCentroidBondForce, CustomHbondForce,   # noqa: E402
                                    CustomManyParticleForce)

K = 24


def centroid():
    rng = np.random.default_rng(2)
    f = CustomCentroidBondForce(2, 'lam*0.5*kc*(distance(g1,g2)-0.35)^2')
    f.addGlobalParameter('lam', 0.5); f.addGlobalParameter('kc', 800.0)
    f.addGroup(list(range(126))); f.addGroup(list(range(126, 156)))
    f.addBond([0, 1])
    f.addEnergyParameterDerivative('lam')
    return f, np.concatenate([rng.uniform(0.0, 1.0, (126, 3)), rng.uniform(1.2, 1.6, (30, 3))])


def hbond():
    rng = np.random.default_rng(3)
    f = CustomHbondForce('lam*kd*ka*(distance(d1,a1)-0.3)^2*(1+cos(angle(d2,d1,a1)))^1.5')
    f.addGlobalParameter('lam', 0.5)
    f.addPerDonorParameter('kd'); f.addPerAcceptorParameter('ka')
    for k in range(128):
        f.addDonor(2 * k, 2 * k + 1, -1, [rng.uniform(50.0, 90.0)])
    for k in range(128):
        f.addAcceptor(256 + k, -1, -1, [rng.uniform(0.5, 1.5)])
    f.setNonbondedMethod(CustomHbondForce.CutoffNonPeriodic)
    f.setCutoffDistance(0.6)
    f.addEnergyParameterDerivative('lam')
    return f, rng.uniform(0.0, 2.0, (384, 3))


def manyparticle():
    rng = np.random.default_rng(4)
    f = CustomManyParticleForce(3, 'lam*eps1*exp(-3*(distance(p1,p2)+distance(p1,p3)))*(cos(angle(p2,p1,p3))+1/3)^2')
    f.addGlobalParameter('lam', 0.5); f.addPerParticleParameter('eps')
    for k in range(216):
        f.addParticle([rng.uniform(20.0, 30.0)], 0)
    f.setPermutationMode(CustomManyParticleForce.SinglePermutation)
    f.setNonbondedMethod(CustomManyParticleForce.CutoffNonPeriodic)
    f.setCutoffDistance(0.45)
    f.addEnergyParameterDerivative('lam')
    grid = np.array([[i, j, k] for i in range(6) for j in range(6) for k in range(6)], dtype=np.float64) * 0.3
    return f, grid + rng.uniform(-0.04, 0.04, grid.shape)


def timed(call, n=100, warm=20):
    for _ in range(warm):
        call()
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e6)
    return np.median(t), min(t), max(t)


def kernel_us(eng, call, scope, n=50):
    """device microseconds of the launches under the profile scope, per scope that was timed (the profile samples the launches of
    a class), times the scopes one ``call`` opens"""
    eng.profile_enable(1, scope)
    eng.profile_reset()
    for _ in range(n):
        call()
    timed_scopes, ms = eng.profile_get(scope)
    eng.profile_enable(0)
    return 1e3 * ms / max(timed_scopes, 1) * (K if scope == 'custom_dpar' else 1)


def main():
    print('K = %d states; microseconds per whole result [R][K][n]' % K)
    print('%-24s %3s  %-34s %-34s %10s %10s  %s' % ('system', 'R', 'one at-states call: host', 'K own-state calls: host', 'kernels', 'kernels', 'partials'))
    # (the wavefronts of the padded term space: 64 terms, one tile of 64 donors x 64 acceptors, or one central particle each)
    for name, make, waves in (('70 custom torsions', torsions, 2), ('Boresch compound bond', boresch, 1), ('centroid bond 126 + 30', centroid, 1),
                              ('128 x 128 donor-acceptor', hbond, 4), ('216-particle three-body', manyparticle, 216)):
        for R in (8, 24):
            f, x = make()
            s = System()
            for _ in range(len(x)):
                s.addParticle(12.0)
            s.addForce(f)
            desc = system_to_desc(s)
            eng = HipEngine()
            eng.set_system(desc)
            eng.set_states(np.full(K, BETA))
            d = np.array(desc['custom_globals']['defaults'], dtype=np.float64)
            table = np.tile(d, (K, 1))
            table[:, 0] = np.linspace(0.1, 1.0, K)
            eng.set_custom_globals(table)
            own = np.arange(R) % K
            eng.set_replicas(R, 0, np.stack([x + 0.001 * r for r in range(R)]), None, np.zeros((R, 3)), own)
            out = np.empty((R, K, len(eng.custom_derivative_names)))

            def loop():
                for l in range(K):
                    eng.set_labels(np.full(R, l, dtype=np.int64))
                    out[:, l, :] = eng.custom_energy_parameter_derivatives()
                eng.set_labels(own)
            fused = eng.custom_energy_parameter_derivatives_at_states()
            loop()
            assert np.array_equal(fused, out, equal_nan=True), 'the two routes differ'
            a, b = timed(eng.custom_energy_parameter_derivatives_at_states), timed(loop)
            ka, kb = kernel_us(eng, eng.custom_energy_parameter_derivatives_at_states, 'custom_dpar_states'), kernel_us(eng, loop, 'custom_dpar')
            print('%-24s %3d  median %7.1f (%7.1f ... %8.1f)  median %7.1f (%7.1f ... %8.1f) %10.1f %10.1f  %s'
                  % ((name, R) + a + b + (ka, kb, '%d wavefronts: %d bytes' % (waves, 8 * R * K * out.shape[2] * waves))))


if __name__ == '__main__':
    main()
