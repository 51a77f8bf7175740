"""GPU: the Metropolized displacement and rotation moves on the device (include/remd_hip_mcmoves.h, csrc/mc_moves.hip,
``proposal='device'``) against tests/mc_device_oracle.py.

Bounds.  A proposed coordinate is computed in f64 from f32 inputs and rounded once; the oracle does the same with numpy's
library functions, which differ from the device's by a few f64 units in the last place -- enough to flip the f32 rounding only
at a tie.  So every moved coordinate lies within ONE f32 unit in the last place of the oracle's value rounded to f32, and
everything that is not moved is compared bit for bit."""
import copy
import numpy as np
import pytest
import mc_device_oracle as mco
from openmmtools_amd import testsystems, states, mcmc, unit
from openmmtools_amd.constants import kB
from openmmtools_amd.multistate import MultiStateSampler, ReplicaExchangeSampler
from openmmtools_amd.system import system_to_desc

pytestmark = pytest.mark.gpu
DISPLACEMENT, ROTATION = 0, 1
PROPOSE_BLOCK = 256              # MC_BLOCK of csrc/mc_moves.hip: the lanes of one propose workgroup


def _engine(factory, desc, x, box, T, seed, r_begin=0, R_global=None, phases=None):
    eng = factory()
    if phases is not None:
        eng.set_phases(phases)
    eng.set_system(desc)
    eng.set_states(1.0 / (kB * np.asarray(T, dtype=np.float64)))
    eng.seed(seed)
    R_global = len(T) if R_global is None else R_global
    eng.set_replicas(R_global, r_begin, x, None, box, np.arange(R_global, dtype=np.int64))
    return eng


def _ulp32(a):
    return np.spacing(np.abs(np.asarray(a, dtype=np.float32))).astype(np.float64)


# ---- 1. proposals, exact -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def gas(hip_engine_factory):
    """300 non-interacting particles (charge 0, epsilon 0) in a periodic box: the potential is flat, every move is accepted."""
    g = testsystems.IdealGas(nparticles=300, volume=27.0 * unit.nanometer ** 3)
    R, seed = 3, 20240611
    x = np.stack([g.positions + 0.01 * r for r in range(R)])
    eng = _engine(hip_engine_factory, system_to_desc(g.system), x, np.full((R, 3), 3.0), [250.0, 300.0, 350.0], seed)
    return eng, R, seed


@pytest.mark.parametrize('n_atoms', [1, 2, 64, 65, PROPOSE_BLOCK + 1])
def test_proposals_match_the_oracle_to_one_f32_unit_and_touch_nothing_else(gas, n_atoms):
    eng, R, seed = gas
    atoms = np.random.RandomState(n_atoms).permutation(300)[:n_atoms]            # out of order, not contiguous
    if n_atoms > 1:
        atoms[:2] = sorted(atoms[:2], reverse=True)
    assert n_atoms == 1 or (np.any(np.diff(atoms) < 0) and np.any(np.abs(np.diff(atoms)) > 1))
    rest = np.setdiff1d(np.arange(300), atoms)
    sigma, iteration = 0.3, 1000 + n_atoms
    x0 = eng.get_replicas()[0]
    acc = eng.mc_rigid_moves([(DISPLACEMENT, atoms, sigma, 0)], iteration)
    x1 = eng.get_replicas()[0]
    acc2 = eng.mc_rigid_moves([(ROTATION, atoms, 0.0, 1)], iteration)
    x2 = eng.get_replicas()[0]
    assert acc.shape == (1, R) and np.all(acc == 1) and np.all(acc2 == 1)
    worst = 0.0
    for r in range(R):
        want1 = mco.displace(x0[r, atoms], seed, iteration, 0, r, sigma).astype(np.float32).astype(np.float64)
        want2 = mco.rotate(x1[r, atoms], seed, iteration, 1, r).astype(np.float32).astype(np.float64)
        for got, want in ((x1[r, atoms], want1), (x2[r, atoms], want2)):
            err = np.abs(got - want) / _ulp32(want)
            worst = max(worst, err.max())
            assert np.all(err <= 1.0), (n_atoms, r, err.max())
        assert np.abs(x1[r, atoms] - x0[r, atoms]).max() > 1e-3
        assert n_atoms == 1 or np.abs(x2[r, atoms] - x1[r, atoms]).max() > 1e-3
        assert np.array_equal(x1[r, rest], x0[r, rest]) and np.array_equal(x2[r, rest], x0[r, rest])
    print('subset of', n_atoms, ': worst error in f32 units in the last place', worst)


# ---- 2. decisions, 3. sampling: a particle in a harmonic well ---------------------------------------------------------------------------
WELL_K, WELL_T, WELL_SIGMA = 100.0, (200.0, 300.0, 450.0), 0.08


def _well_engine(factory, seed):
    ho = testsystems.HarmonicOscillator(K=WELL_K * unit.kilojoules_per_mole / unit.nanometer ** 2, mass=12.0 * unit.amu)
    return _engine(factory, system_to_desc(ho.system), np.zeros((3, 1, 3)), np.zeros((3, 3)), WELL_T, seed)


def _oracle_well_run(seed, n_iterations):
    """The oracle's own trajectory: f32 positions as the device stores them, U = K |x|^2 / 2 in f64, its own decisions.
    Returns the flags [n][3] and the smallest |u - exp(-delta)| met."""
    beta = 1.0 / (kB * np.asarray(WELL_T))
    x = np.zeros((3, 3))
    flags, margin = np.zeros((n_iterations, 3), dtype=np.int32), np.inf
    for it in range(n_iterations):
        for r in range(3):
            new = mco.displace(x[r][None], seed, it + 1, 0, r, WELL_SIGMA)[0].astype(np.float32).astype(np.float64)
            delta = beta[r] * 0.5 * WELL_K * ((new ** 2).sum() - (x[r] ** 2).sum())
            u = mco.acceptance_uniform(seed, it + 1, 0, r)
            margin = min(margin, abs(u - np.exp(-delta)))
            if mco.accepts(delta, u):
                flags[it, r] = 1
                x[r] = new
    return flags, margin


def test_decisions_are_the_oracles_on_every_trial(hip_engine_factory):
    n = 60
    for seed in range(100, 140):                      # chosen on the CPU: the first seed whose 180 trials all lie outside the margin
        want, margin = _oracle_well_run(seed, n)
        if margin > 1e-4:
            break
    assert margin > 1e-4, 'no seed found whose trials all lie outside the margin'
    eng = _well_engine(hip_engine_factory, seed)
    got = np.stack([eng.mc_rigid_moves([(DISPLACEMENT, [0], WELL_SIGMA, 0)], it + 1)[0] for it in range(n)])
    print('seed', seed, 'smallest |u - exp(-delta)|', margin, 'accepted per replica', got.sum(0).tolist(), want.sum(0).tolist())
    assert np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()
    assert 0 < got.sum() < got.size


def test_device_displacements_sample_the_boltzmann_distribution_of_each_state(hip_engine_factory):
    n = 1500
    move = mcmc.MCDisplacementMove(displacement_sigma=WELL_SIGMA * unit.nanometer, proposal='device')
    ho = testsystems.HarmonicOscillator(K=WELL_K * unit.kilojoules_per_mole / unit.nanometer ** 2, mass=12.0 * unit.amu)
    s = MultiStateSampler(mcmc_moves=move, number_of_iterations=n, engine=hip_engine_factory(), seed=13, online_analysis_interval=None)
    ss = states.SamplerState(np.zeros((1, 3)), box_vectors=ho.system.getDefaultPeriodicBoxVectors())
    s.create([states.ThermodynamicState(ho.system, t * unit.kelvin) for t in WELL_T], [copy.deepcopy(ss) for _ in WELL_T], storage=None)
    s.run(1)                                           # the sampler's own path once: flags credited to the moves
    assert all(m.n_proposed == 1 for m in s._mcmc_moves)
    eng, x2, accepted = s._engine, np.zeros(3), np.zeros(3)
    description = [move.device_description(1) + (0,)]
    for it in range(2, n + 1):                         # the engine call the sampler makes, without the sampler's bookkeeping around it
        accepted += eng.mc_rigid_moves(description, it)[0]
        if it > 100:
            x2 += (eng.get_replicas(velocities=False)[0][:, 0, :] ** 2).sum(axis=1) / 3.0
    want = kB * np.array(WELL_T) / WELL_K
    got = x2 / (n - 100)
    frac = accepted / (n - 1)
    print('<x^2> / (kT / K)', (got / want).tolist(), 'acceptance', frac.tolist())
    assert np.all(np.abs(got / want - 1.0) < 0.15), got / want
    assert 0.2 < frac[0] < frac[1] < frac[2] < 0.95, frac


# ---- 4. rejection restores to the bit, 5. sharding, 7. phases: alanine dipeptide in water -------------------------------------------------
SOLUTE = list(range(22))
ALA_T = (300.0, 320.0, 340.0)


@pytest.fixture(scope='module')
def alanine():
    al = testsystems.AlanineDipeptideExplicit()
    edges = np.array([al.system.getDefaultPeriodicBoxVectors()[k][k] for k in range(3)], dtype=np.float64)
    return al, edges


def test_device_rejections_restore_solute_forces_and_potential_exactly(hip_engine_factory, alanine):
    al, edges = alanine
    seq = mcmc.SequenceMove([mcmc.MCRotationMove(atom_subset=SOLUTE, proposal='device'),
                             mcmc.MCDisplacementMove(displacement_sigma=0.005 * unit.nanometer, atom_subset=SOLUTE, proposal='device')])
    s = ReplicaExchangeSampler(mcmc_moves=seq, number_of_iterations=2, engine=hip_engine_factory(), seed=2, online_analysis_interval=None)
    thermo = [states.ThermodynamicState(al.system, t * unit.kelvin) for t in ALA_T]
    s.create(thermo, [states.SamplerState(al.positions, box_vectors=al.system.getDefaultPeriodicBoxVectors())], storage=None)
    x0 = np.stack([st.positions for st in s.sampler_states]).astype(np.float32)
    s.run()
    x1 = np.stack([st.positions for st in s.sampler_states]).astype(np.float32)
    rot = [m.move_list[0] for m in s._mcmc_moves]
    disp = [m.move_list[1] for m in s._mcmc_moves]
    assert sum(m.n_proposed for m in rot) == 6 and sum(m.n_accepted for m in rot) == 0
    assert sum(m.n_proposed for m in disp) == 6 and sum(m.n_accepted for m in disp) >= 1
    assert np.array_equal(x1[:, 22:], x0[:, 22:])              # water never moves: no dynamics in this sequence
    # the same two moves straight on the engine, with everything a rejection has to restore read before and after
    eng = s._engine
    described = [m.device_description(al.system.getNumParticles()) + (k,) for k, m in enumerate(seq.move_list)]
    # the rotation alone: every replica rejects, and gets back everything it had
    eng.compute_energies()                                     # (the spatial order of the evaluations below is made here, for these positions)
    xb, fb, ub = eng.get_replicas()[0], eng.get_forces(), eng.get_replicas(positions=False, velocities=False, potential=True)[2]
    assert not eng.mc_rigid_moves(described[:1], 9).any()
    xa, fa, ua = eng.get_replicas()[0], eng.get_forces(), eng.get_replicas(positions=False, velocities=False, potential=True)[2]
    assert np.array_equal(xa, xb) and np.array_equal(fa, fb) and np.array_equal(ua, ub)
    # the sequence, until a replica has rejected both moves and another has accepted the displacement (a nudge of 0.005 nm is
    # accepted far more often than not, so the first takes some trials)
    seen_both_rejected = seen_accepted = False
    for iteration in range(10, 110):
        eng.compute_energies()                                 # (the spatial order of the evaluations below is made here, for these positions)
        xb, fb, ub = eng.get_replicas()[0], eng.get_forces(), eng.get_replicas(positions=False, velocities=False, potential=True)[2]
        acc = eng.mc_rigid_moves(described, iteration)
        xa, fa, ua = eng.get_replicas()[0], eng.get_forces(), eng.get_replicas(positions=False, velocities=False, potential=True)[2]
        assert np.all(acc[0] == 0)
        assert np.array_equal(xa[:, 22:], xb[:, 22:])
        for r in range(3):
            if acc[1, r] == 0:
                seen_both_rejected = True
                assert np.array_equal(xa[r], xb[r]) and np.array_equal(fa[r], fb[r]) and ua[r] == ub[r], (iteration, r)
            else:
                seen_accepted = True
                shift = xa[r, :22] - xb[r, :22]
                assert np.abs(shift[0]).max() > 1e-5 and ua[r] != ub[r]
                # one vector for the whole body: each coordinate is rounded once, to half a unit of the largest coordinate's f32 spacing
                assert np.abs(shift - np.median(shift, axis=0)).max() <= 2.0 ** -23 * np.abs(xa[r, :22]).max(), (iteration, r)
        if seen_both_rejected and seen_accepted:
            break
    print('iterations until both cases were seen', iteration - 9)
    assert seen_both_rejected and seen_accepted


def test_flags_and_positions_do_not_depend_on_the_sharding(hip_engine_factory, alanine):
    al, edges = alanine
    desc = system_to_desc(al.system)
    T = (300.0, 315.0, 330.0, 345.0)
    rng = np.random.RandomState(4)
    x = np.tile(al.positions, (4, 1, 1))
    x[:, :22] += 0.001 * rng.normal(size=(4, 1, 3))            # (each replica's solute nudged as a body: four different trials)
    box = np.tile(edges, (4, 1))
    moves = [(DISPLACEMENT, SOLUTE[::-1], 0.004, 0), (ROTATION, SOLUTE, 0.0, 1), (DISPLACEMENT, SOLUTE, 0.004, 2)]
    whole = _engine(hip_engine_factory, desc, x, box, T, seed=77)
    halves = [_engine(hip_engine_factory, desc, x[b:b + 2], box[b:b + 2], T, seed=77, r_begin=b, R_global=4) for b in (0, 2)]
    for iteration in (1, 2):
        acc = whole.mc_rigid_moves(moves, iteration)
        acc_h = np.concatenate([h.mc_rigid_moves(moves, iteration) for h in halves], axis=1)
        assert np.array_equal(acc, acc_h), (acc, acc_h)
        assert np.array_equal(whole.get_replicas()[0], np.concatenate([h.get_replicas()[0] for h in halves]))
    print('accepted', acc.tolist())
    assert np.abs(whole.get_replicas()[0][:, :22] - x[:, :22].astype(np.float32)).max() > 1e-4      # (something was accepted)


def test_phased_propagation_sees_the_moved_positions(hip_engine_factory, alanine):
    al, edges = alanine
    out = []
    for phases in (1, 2):
        eng = hip_engine_factory()
        eng.set_phases(phases)
        seq = mcmc.SequenceMove([mcmc.MCDisplacementMove(displacement_sigma=0.005 * unit.nanometer, atom_subset=SOLUTE, proposal='device'),
                                 mcmc.MCRotationMove(atom_subset=SOLUTE, proposal='device'),
                                 mcmc.LangevinDynamicsMove(timestep=1.0 * unit.femtosecond, collision_rate=1.0 / unit.picosecond, n_steps=4)])
        s = MultiStateSampler(mcmc_moves=seq, number_of_iterations=1, engine=eng, seed=5, online_analysis_interval=None)
        thermo = [states.ThermodynamicState(al.system, t * unit.kelvin) for t in np.linspace(300.0, 350.0, 6)]
        ss = states.SamplerState(al.positions, box_vectors=al.system.getDefaultPeriodicBoxVectors())
        s.create(thermo, [copy.deepcopy(ss) for _ in thermo], storage=None)
        s.run()
        x, v = eng.get_replicas()[:2]
        out.append((x, v, eng.phases_active(), [m.move_list[0].n_accepted for m in s._mcmc_moves]))
    print('phases', out[0][2], out[1][2], 'accepted displacements', out[0][3])
    assert out[0][2] == 1 and out[1][2] == 2
    assert out[0][3] == out[1][3] and sum(out[0][3]) >= 1
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert np.abs(out[0][0][:, 22:] - al.positions[None, 22:]).max() > 1e-4          # (the dynamics did run)


# ---- 6. virtual sites -----------------------------------------------------------------------------------------------------------------
def test_sites_follow_their_parents_after_accepted_and_rejected_moves(hip_engine_factory):
    import virtual_sites_oracle
    box = testsystems.WaterBox(box_edge=1.25 * unit.nanometers, cutoff=0.6 * unit.nanometers, model='tip4pew')
    desc = system_to_desc(box.system, ewald_split='reference')
    table = desc['virtual_sites']
    R = 3
    eng = _engine(hip_engine_factory, desc, np.tile(box.positions, (R, 1, 1)), np.full((R, 3), 1.25), [300.0, 320.0, 340.0], seed=9)
    water = [3, 0, 2, 1]                                      # one whole molecule: the site and its three parents
    assert 3 in table['site'] and set(table['parent'][list(table['site']).index(3)][:3]) == {0, 1, 2}
    # a nudge of 0.001 nm is mostly accepted, a jump of 0.3 nm lands on a neighbour and is mostly rejected
    moves = [(DISPLACEMENT, water, 0.001, 0), (DISPLACEMENT, water, 0.3, 1), (ROTATION, water, 0.0, 2)]
    seen = set()
    for iteration in range(1, 9):
        xb = eng.get_replicas()[0]
        acc = eng.mc_rigid_moves(moves, iteration)
        x = eng.get_replicas()[0]
        seen.update(int(a) for a in acc.flat)
        ref = virtual_sites_oracle.place_table(table, x)
        for r in range(R):
            bound = 2.0 ** -24 * np.abs(x[r, :4]).max()
            assert np.abs(x[r, 3] - ref[r, 3]).max() <= bound, (iteration, r)
            assert np.array_equal(x[r, 4:], xb[r, 4:])
            if not acc[:, r].any():
                assert np.array_equal(x[r], xb[r])
        if seen == {0, 1}:
            break
    assert seen == {0, 1}, 'needs an accepted and a rejected move'


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_name_what_is_wrong(hip_engine_factory):
    ho = testsystems.HarmonicOscillator(K=WELL_K * unit.kilojoules_per_mole / unit.nanometer ** 2, mass=12.0 * unit.amu)
    bare = hip_engine_factory()
    bare.set_system(system_to_desc(ho.system))
    bare.set_states(1.0 / (kB * np.asarray(WELL_T)))
    with pytest.raises(RuntimeError, match='replicas not set'):
        bare.mc_rigid_moves([(DISPLACEMENT, [0], 0.1, 0)], 1)
    eng = _well_engine(hip_engine_factory, 3)
    ok = (DISPLACEMENT, [0], 0.1, 0)
    x0 = eng.get_replicas()[0]
    for moves, message in (([], 'n_moves must be 1 .. 16'), ([ok] * 17, 'n_moves must be 1 .. 16'),
                           ([(2, [0], 0.1, 0)], 'unknown kind'), ([ok, (-1, [0], 0.1, 1)], 'unknown kind'),
                           ([(ROTATION, [], 0.0, 0)], 'at least one atom'),
                           ([(ROTATION, [1], 0.0, 0)], 'atom index out of range'), ([(DISPLACEMENT, [-1], 0.1, 0)], 'atom index out of range'),
                           ([(ROTATION, [0, 0], 0.0, 0)], 'named twice'),
                           ([(DISPLACEMENT, [0], -0.1, 0)], 'sigma'), ([(DISPLACEMENT, [0], float('nan'), 0)], 'sigma'),
                           ([(DISPLACEMENT, [0], float('inf'), 0)], 'sigma'), ([(DISPLACEMENT, [0], 0.1, -1)], 'position')):
        with pytest.raises(RuntimeError, match=message):
            eng.mc_rigid_moves(moves, 1)
    assert np.array_equal(eng.get_replicas()[0], x0)           # a refused call left the replicas alone
    assert eng.mc_rigid_moves([ok] * 16, 1).shape == (16, 3)   # and the handle goes on working, at the largest n_moves
