"""CustomGBForce implicit solvent on the device (csrc/gbsa.hip with remd_set_gb_model, include/remd_hip_gb.h): testsystems.CustomGBForceSystem
-- 140 ions, a CutoffPeriodic NonbondedForce and an OBC2 CustomGBForce with a 2 nm periodic cutoff -- against the f64 oracle
(tests/custom_gb_oracle.py, pinned to the reference's strings by tests/test_custom_gb_cpu.py), plain and alchemical."""
import os

import numpy as np
import pytest

from custom_gb_oracle import custom_gb_energy_forces
from oracle.forcefield import ForceFieldOracle
from oracle.alchemical_regions import total_state_energies, total_energy_forces
from openmmtools_amd import alchemy, states, mcmc, unit, testsystems as ts
from openmmtools_amd.system import system_to_desc, System, NonbondedForce, GBSAOBCForce, CustomGBForce

pytestmark = pytest.mark.gpu
KB = 0.008314462618153242
BOX = np.full(3, 10.0)


def _replica_positions(x0, R, box_edge, spread=0.05):
    """R replicas at different positions: jittered, the later ones shifted through the periodic boundary"""
    out = []
    for r in range(R):
        x = x0 + spread * np.random.default_rng(100 + r).normal(size=x0.shape) + 0.37 * r
        out.append(np.mod(x, box_edge))
    return np.stack(out)


def _plain_check(eng, system, x0, box, R=4):
    desc = system_to_desc(system)
    assert desc['gbsa']['method'] == 2
    eng.set_system(desc)
    eng.set_states(np.array([1.0 / (KB * 300.0)]))
    eng.set_integrator('V R O R V', 0.002, 1.0, 10, True, 1e-8)
    eng.seed(3)
    x = _replica_positions(x0, R, box[0])
    eng.set_replicas(R, 0, x, None, np.tile(box, (R, 1)), np.zeros(R, dtype=int))
    _, U = eng.compute_energies(want_potential=True)
    xd = eng.get_replicas()[0]
    f = eng.get_forces()
    d0 = dict(desc); gb = d0.pop('gbsa')
    es = []
    for r in range(R):
        e1, f1 = custom_gb_energy_forces(xd[r], gb, 1.0, box)
        e0, f0 = ForceFieldOracle(d0).energy_forces(xd[r], box)
        es.append(e1)
        assert np.isclose(U[r], e0 + e1, rtol=1e-5, atol=1e-5 * abs(e1)), (r, U[r], e0 + e1)
        assert np.abs(f[r] - (f0 + f1)).max() < 2e-4 * np.abs(f0 + f1).max(), r
    assert np.ptp(es) > 1.0                      # the replicas see different GB energies
    assert not np.any(eng.propagate(0))
    assert np.all(np.isfinite(eng.compute_energies()))


def test_custom_gb_system_per_replica_energies_and_forces(hip_engine_factory):
    s = ts.CustomGBForceSystem()
    _plain_check(hip_engine_factory(), s.system, s.positions, BOX)


def _small_periodic(n=48, edge=4.0, cutoff=1.5):
    """a CustomGBForceSystem in miniature (N <= 64): the small one-launch kernel is NoCutoff only, so this takes the three launches"""
    big = ts.CustomGBForceSystem()
    gb0 = big.system.getForce(1)
    s = System()
    s.setDefaultPeriodicBoxVectors([edge, 0, 0], [0, edge, 0], [0, 0, edge])
    nb = NonbondedForce(); nb.setNonbondedMethod(NonbondedForce.CutoffPeriodic); nb.setCutoffDistance(cutoff)
    gb = CustomGBForce(); gb.setNonbondedMethod(CustomGBForce.CutoffPeriodic); gb.setCutoffDistance(cutoff)
    for p in gb0.per_particle:
        gb.addPerParticleParameter(p)
    for name, v in gb0.globals:
        gb.addGlobalParameter(name, v)
    for c in gb0.computed:
        gb.addComputedValue(*c)
    for t in gb0.energy_terms:
        gb.addEnergyTerm(*t)
    for i in range(n):
        s.addParticle(39.9)
        q, rad, sc = gb0.particles[i if i < n // 2 else 140 - n + i]
        nb.addParticle(q, 0.335, 0.001603)
        gb.addParticle([q, rad, sc])
    s.addForce(nb); s.addForce(gb)
    g = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing='ij'), axis=-1).reshape(-1, 3)[:n] * (edge / 4) + 0.3
    return s, g.astype(np.float64), np.full(3, edge)


def test_small_periodic_system_takes_the_three_launches_and_is_correct(hip_engine_factory):
    s, x0, box = _small_periodic()
    _plain_check(hip_engine_factory(), s, x0, box)


LS = np.array([[1.0], [1.0], [1.0], [0.5], [0.0]])
LE = np.array([[1.0], [0.5], [0.0], [0.0], [0.0]])


def test_alchemical_custom_gb_ukl_over_a_lambda_ladder(hip_engine_factory):
    s = ts.CustomGBForceSystem()
    asys = alchemy.AbsoluteAlchemicalFactory().create_alchemical_system(s.system, alchemy.AlchemicalRegion(alchemical_atoms=range(6)))
    desc = system_to_desc(asys)
    assert desc['gbsa']['alchemical'].tolist() == [1] * 6 + [0] * 134 and desc['gbsa']['method'] == 2
    eng = hip_engine_factory()
    eng.set_system(desc)
    beta = 1.0 / (KB * 300.0)
    K = len(LS)
    eng.set_states(np.full(K, beta))
    eng.set_region_lambdas(LS, LE)
    eng.set_integrator('V R O R V', 0.002, 1.0, 10, True, 1e-8)
    eng.seed(8)
    labels = np.array([0, 1, 2, 4])
    R = len(labels)
    eng.set_replicas(R, 0, _replica_positions(s.positions, R, 10.0), None, np.tile(BOX, (R, 1)), labels)
    rows, U = eng.compute_energies(want_potential=True)
    xd = eng.get_replicas()[0]
    f = eng.get_forces()
    d0 = dict(desc); gb = d0.pop('gbsa')
    for r, k in enumerate(labels):
        egb = np.array([custom_gb_energy_forces(xd[r], gb, LE[q, 0], BOX, forces=False)[0] for q in range(K)])
        ref = total_state_energies(d0, xd[r], BOX, LS, LE) + egb
        assert np.ptp(egb) > 10.0
        assert np.allclose(rows[r], beta * ref, rtol=1e-5, atol=1e-5 * np.abs(beta * ref).max()), np.abs(rows[r] - beta * ref).max()
        assert np.isclose(U[r], ref[k], rtol=1e-5, atol=1e-5 * np.abs(ref).max())
        f_ref = total_energy_forces(d0, xd[r], BOX, LS[k], LE[k])[1] + custom_gb_energy_forces(xd[r], gb, LE[k, 0], BOX)[1]
        assert np.abs(f[r] - f_ref).max() < 2e-4 * np.abs(f_ref).max()
    assert not np.any(eng.propagate(0))


def _droplet(n, custom, obc1=False):
    """NoCutoff ions with OBC2 GB: as a GBSAOBCForce, or as the shape-A CustomGBForce strings with the same constants (or OBC1's)"""
    g = np.stack(np.meshgrid(*[np.arange(6)] * 3, indexing='ij'), axis=-1).reshape(-1, 3) * 0.38
    x = g[np.argsort(np.linalg.norm(g - g.mean(0), axis=1), kind='stable')[:n]].astype(np.float64)
    s = System()
    nb = NonbondedForce(); nb.setNonbondedMethod(NonbondedForce.NoCutoff)
    rng = np.random.default_rng(5)
    params = [(0.3 if i % 2 == 0 else -0.3, 0.15 + 0.05 * rng.random(), 0.7 + 0.2 * rng.random()) for i in range(n)]
    if custom:
        ref = ts.CustomGBForceSystem().system.getForce(1)
        gb = CustomGBForce()
        for p in ref.per_particle:
            gb.addPerParticleParameter(p)
        for name, expr, kind in ref.computed:
            if obc1:
                expr = expr.replace('tanh(1*psi-0.8*psi^2+4.85*psi^3)', 'tanh(0.8*psi-0*psi^2+2.909125*psi^3)')
            gb.addComputedValue(name, expr, kind)
        for expr, kind in ref.energy_terms:                   # the dielectrics as numbers: GBSAOBCForce's defaults 1 and 78.5
            expr = expr.replace('testsystems_CustomGBForceSystem_solventDielectric', '78.5').replace('testsystems_CustomGBForceSystem_soluteDielectric', '1.0')
            gb.addEnergyTerm(expr, kind)
    else:
        gb = GBSAOBCForce()
    for i, (q, rad, sc) in enumerate(params):
        s.addParticle(39.9)
        nb.addParticle(q, 0.34, 0.5)
        gb.addParticle([q, rad, sc]) if custom else gb.addParticle(q, rad, sc)
    s.addForce(nb); s.addForce(gb)
    return s, x


@pytest.mark.parametrize('n', [22, 150])
def test_nocutoff_shape_a_is_bit_identical_to_gbsaobcforce(hip_engine_factory, n):
    out = []
    for custom in (False, True):
        system, x0 = _droplet(n, custom)
        eng = hip_engine_factory()
        eng.set_system(system_to_desc(system))
        eng.set_states(np.array([1.0 / (KB * 300.0)]))
        eng.set_integrator('V R O R V', 0.001, 1.0, 5, True, 1e-8)
        eng.seed(6)
        x = np.stack([x0 + 0.004 * (r + 1) * np.random.default_rng(r).normal(size=x0.shape) for r in range(2)])
        eng.set_replicas(2, 0, x, None, np.zeros((2, 3)), np.zeros(2, dtype=int))
        _, U = eng.compute_energies(want_potential=True)
        out.append((U.copy(), eng.get_forces().copy()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def _sampler(engine, n_replicas, storage=None, n_iterations=3, phases=None, system=None, positions=None):
    from openmmtools_amd.multistate import ReplicaExchangeSampler
    if system is None:
        s = ts.CustomGBForceSystem()
        system, positions = s.system, s.positions
    if phases is not None:
        engine.set_phases(phases)
    temperatures = np.geomspace(300.0, 600.0, n_replicas)
    ths = [states.ThermodynamicState(system, float(T) * unit.kelvin) for T in temperatures]
    ss = states.SamplerState(positions, box_vectors=system.getDefaultPeriodicBoxVectors())
    move = mcmc.LangevinSplittingDynamicsMove(timestep=2.0 * unit.femtosecond, collision_rate=1.0 / unit.picosecond, n_steps=20,
                                              reassign_velocities=True, splitting='V R O R V')
    r = ReplicaExchangeSampler(mcmc_moves=move, number_of_iterations=n_iterations, engine=engine, seed=0xC6B, online_analysis_interval=None)
    r.create(ths, [ss], storage=storage)
    return r


def test_two_blocks_equal_one_block(hip_engine_factory):
    """the phased path runs NoCutoff and PME systems (api.hip phases_for), not CutoffPeriodic ones: a NoCutoff CustomGBForce with OBC1's
    constants, so that the blocks must be given the model (remd_gbsa_clone)"""
    system, x0 = _droplet(150, True, obc1=True)
    assert system_to_desc(system)['gbsa']['alpha'] == 0.8
    runs = []
    for phases in (1, 2):
        eng = hip_engine_factory()
        s = _sampler(eng, 8, phases=phases, n_iterations=10 ** 6, system=system, positions=x0)
        out = []
        for _ in range(3):
            s.run(1)
            out.append((np.array(s._replica_thermodynamic_states), np.array(s.energy_thermodynamic_states), eng.get_replicas()[0]))
        runs.append((out, eng.phases_active()))
    assert (runs[0][1], runs[1][1]) == (1, 2)
    for it, (a, b) in enumerate(zip(runs[0][0], runs[1][0])):
        for q, name in enumerate(('labels', 'u_kl', 'positions')):
            assert np.array_equal(a[q], b[q]), (it, name)


def test_24_replica_exchange_on_custom_gb_system_resumes_from_its_store(hip_engine_factory, tmp_path):
    from openmmtools_amd.multistate import ReplicaExchangeSampler, MultiStateReporter
    rep = MultiStateReporter(str(tmp_path / 'gb.nc'), checkpoint_interval=1, layout='records')
    s = _sampler(hip_engine_factory(), 24, storage=rep, n_iterations=4)
    s.run()
    assert s.iteration == 4 and np.all(np.isfinite(s.energy_thermodynamic_states))
    n = np.asarray(s._n_proposed_matrix)
    assert n.sum() > 0 and np.array_equal(n, n.T)
    acc = np.asarray(s._n_accepted_matrix)
    assert np.array_equal(acc, acc.T)
    rep.close()
    res = ReplicaExchangeSampler.from_storage(str(tmp_path / 'gb.nc'), engine=hip_engine_factory())
    assert res.iteration == 4
    assert res._thermodynamic_states[0].system.fingerprint() == ts.CustomGBForceSystem().system.fingerprint()
    res.extend(2)
    assert res.iteration == 6 and np.all(np.isfinite(res.energy_thermodynamic_states))
    res._reporter.close()
