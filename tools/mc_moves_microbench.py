"""Host wall time per iteration of the Metropolized two-move prefix alone -- displacement + rotation of the guest of
testsystems.HostGuestExplicit (atoms 126 .. 155) -- with the proposals on the host and on the device (mcmc.MetropolizedMove
``proposal=``; csrc/mc_moves.hip), at 8 and 24 replicas on the same build.  What is timed is MultiStateSampler._propagate_replicas
of SequenceMove([MCDisplacementMove, MCRotationMove]): everything an iteration spends on the two moves, transfers, host work and
synchronisation included.  Also timed: one full energy evaluation (potential of every replica, one synchronisation), of which the
device path makes three per iteration and the host path four.  One JSON line per (replicas, proposal); medians over --repeats
iterations after --warmup, with the spread."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from openmmtools_amd import testsystems, states, mcmc, unit
from openmmtools_amd.multistate import MultiStateSampler
from openmmtools_amd._engine import HipEngine

GUEST = list(range(126, 156))


def measure(n_replicas, proposal, repeats, warmup):
    hg = testsystems.HostGuestExplicit()
    seq = mcmc.SequenceMove([mcmc.MCDisplacementMove(displacement_sigma=0.1 * unit.nanometer, atom_subset=GUEST, proposal=proposal),
                             mcmc.MCRotationMove(atom_subset=GUEST, proposal=proposal)])
    eng = HipEngine()
    s = MultiStateSampler(mcmc_moves=seq, number_of_iterations=10 ** 9, engine=eng, seed=1, online_analysis_interval=None)
    thermo = [states.ThermodynamicState(hg.system, t * unit.kelvin) for t in np.linspace(300.0, 330.0, n_replicas)]
    ss = states.SamplerState(hg.positions, box_vectors=hg.system.getDefaultPeriodicBoxVectors())
    s.create(thermo, [ss] * n_replicas, storage=None)
    times, evals = [], []
    for it in range(1, warmup + repeats + 1):
        eng.sync()
        t0 = time.perf_counter()
        s._propagate_replicas(rng_iteration=it)
        eng.sync()
        t1 = time.perf_counter()
        eng.get_replicas(positions=False, velocities=False, potential=True)
        t2 = time.perf_counter()
        if it > warmup:
            times.append(1e3 * (t1 - t0)); evals.append(1e3 * (t2 - t1))
    moves = s._mcmc_moves[0].move_list
    out = dict(replicas=n_replicas, proposal=proposal, repeats=repeats, ms_per_iteration_median=float(np.median(times)),
               ms_per_iteration_min=float(np.min(times)), ms_per_iteration_max=float(np.max(times)),
               ms_one_evaluation_median=float(np.median(evals)),
               accepted=[sum(m.move_list[k].n_accepted for m in s._mcmc_moves) for k in range(len(moves))],
               proposed=[sum(m.move_list[k].n_proposed for m in s._mcmc_moves) for k in range(len(moves))])
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('--replicas', type=int, nargs='+', default=[8, 24])
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    for n in a.replicas:
        rows = {}
        for proposal in ('host', 'device'):
            rows[proposal] = measure(n, proposal, a.repeats, a.warmup)
            print(json.dumps(rows[proposal]), flush=True)
        h, d = rows['host'], rows['device']
        print(json.dumps(dict(replicas=n, host_over_device=h['ms_per_iteration_median'] / d['ms_per_iteration_median'],
                              evaluation_share_of_device_path=3.0 * d['ms_one_evaluation_median'] / d['ms_per_iteration_median'])), flush=True)


if __name__ == '__main__':
    main()
