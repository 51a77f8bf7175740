"""CPU-only: the random stream of the device Monte Carlo moves as tests/mc_device_oracle.py restates it, and the host side of
``proposal='device'`` (mcmc.MetropolizedMove, MultiStateSampler) without a GPU."""
import copy
import pickle
import numpy as np
import pytest
import mc_device_oracle as mco
from openmmtools_amd import testsystems, states, mcmc, unit, utils
from openmmtools_amd.multistate import MultiStateSampler
from oracle_engine import OracleEngine


def test_rotation_matrices_are_the_references_and_proper_rotations():
    for replica in range(6):
        for position in (0, 3):
            q = mco.quaternion(11, 5, position, replica)
            m = mco.rotation_matrix(11, 5, position, replica)
            assert np.allclose(m, mcmc.MCRotationMove._rotation_matrix_from_quaternion(q), rtol=0, atol=4e-16)
            assert np.allclose(m @ m.T, np.eye(3), atol=1e-14) and abs(np.linalg.det(m) - 1.0) < 1e-14
            assert abs(np.dot(q, q) - 1.0) < 1e-15


def test_displacement_normals_have_mean_zero_and_variance_one():
    n = 3000
    g = np.array([mco.normals(2024, it, 1, 7) for it in range(n)])
    assert np.all(np.isfinite(g))
    # standard error of the mean of n unit normals 1 / sqrt(n), of their variance sqrt(2 / n)
    assert np.all(np.abs(g.mean(0)) < 4.0 / np.sqrt(n)), g.mean(0)
    assert np.all(np.abs(g.var(0) - 1.0) < 4.0 * np.sqrt(2.0 / n)), g.var(0)
    u = np.array([mco.acceptance_uniform(2024, it, 1, 7) for it in range(n)])
    assert 0.0 <= u.min() and u.max() < 1.0 and abs(u.mean() - 0.5) < 4.0 / np.sqrt(12.0 * n)


def test_draws_differ_across_replica_position_and_iteration():
    base = (9, 4, 2, 5)                                  # seed, iteration, position, replica
    seen = {mco.uniforms(*base) + (mco.acceptance_uniform(*base),)}
    for other in ((9, 5, 2, 5), (9, 4, 3, 5), (9, 4, 2, 6), (10, 4, 2, 5)):
        draws = mco.uniforms(*other) + (mco.acceptance_uniform(*other),)
        assert all(set(draws).isdisjoint(s) for s in seen)
        seen.add(draws)
    assert len(set(mco.uniforms(*base) + (mco.acceptance_uniform(*base),))) == 5            # the five uniforms of one trial too
    assert mco.uniforms(*base) == mco.uniforms(*base)
    assert mco.displacement(9, 4, 2, 5, 0.25) == pytest.approx(0.25 * mco.normals(9, 4, 2, 5), abs=0)


def test_unknown_proposal_is_a_value_error():
    for klass in (mcmc.MCDisplacementMove, mcmc.MCRotationMove, mcmc.MetropolizedMove):
        with pytest.raises(ValueError, match='bogus'):
            klass(proposal='bogus')
    assert mcmc.MCDisplacementMove(proposal='host').proposal == 'host' == mcmc.MCRotationMove().proposal
    assert mcmc.MCDisplacementMove(proposal='device').proposal == 'device' == mcmc.MCRotationMove(proposal='device').proposal


def test_device_proposal_on_an_engine_without_the_entry_point_names_the_header():
    ho = testsystems.HarmonicOscillator(K=100.0 * unit.kilojoules_per_mole / unit.nanometer ** 2, mass=12.0 * unit.amu)
    thermo = [states.ThermodynamicState(ho.system, t * unit.kelvin) for t in (250.0, 300.0)]
    ss = states.SamplerState(np.zeros((1, 3)), box_vectors=ho.system.getDefaultPeriodicBoxVectors())
    move = mcmc.MCDisplacementMove(displacement_sigma=0.1 * unit.nanometer, proposal='device')
    s = MultiStateSampler(mcmc_moves=move, number_of_iterations=1, engine=OracleEngine(), seed=1, online_analysis_interval=None)
    s.create(thermo, [ss, copy.deepcopy(ss)], storage=None)
    with pytest.raises(NotImplementedError, match='remd_hip_mcmoves.h'):
        s.run()
    assert all(m.n_proposed == 0 for m in s._mcmc_moves)


def test_default_moves_pickle_and_serialize_as_before():
    d = mcmc.MCDisplacementMove(displacement_sigma=0.2 * unit.nanometer, atom_subset=[1, 2])
    r = mcmc.MCRotationMove(atom_subset=[0, 3, 4])
    assert set(d.__dict__) == {'n_accepted', 'n_proposed', 'atom_subset', 'displacement_sigma'}
    assert set(r.__dict__) == {'n_accepted', 'n_proposed', 'atom_subset'}
    for move in (d, r, mcmc.MCDisplacementMove(proposal='host')):
        assert b'proposal' not in pickle.dumps(move)
        ser = utils.serialize(move)
        assert 'proposal' not in ser
        back = utils.deserialize(ser)
        assert back.proposal == 'host' and pickle.dumps(back) == pickle.dumps(move)
    # a move written before the attribute existed (no such key in its state) comes back as a host move
    old = mcmc.MCRotationMove.__new__(mcmc.MCRotationMove)
    old.__setstate__(dict(n_accepted=3, n_proposed=5, atom_subset=[0, 1]))
    assert old.proposal == 'host' and old.statistics == dict(n_accepted=3, n_proposed=5)


def test_device_moves_round_trip_with_their_flag(tmp_path):
    from openmmtools_amd.multistate import MultiStateReporter
    seq = mcmc.SequenceMove([mcmc.MCDisplacementMove(displacement_sigma=0.3 * unit.nanometer, atom_subset=[2, 0], proposal='device'),
                             mcmc.MCRotationMove(atom_subset=[0, 1, 2], proposal='device'), mcmc.MCRotationMove(atom_subset=[0, 1, 2])])
    for back in (pickle.loads(pickle.dumps(seq)), copy.deepcopy(seq), utils.deserialize(utils.serialize(seq))):
        assert [m.proposal for m in back.move_list] == ['device', 'device', 'host']
        assert pickle.dumps(back) == pickle.dumps(seq)
    ser = utils.serialize(seq.move_list[0])
    assert ser['proposal'] == 'device'
    rep = MultiStateReporter(str(tmp_path / 'store'), open_mode='w', checkpoint_interval=1)
    rep.write_mcmc_moves([seq, seq])
    stored = rep.read_mcmc_moves()
    rep.close()
    assert [[m.proposal for m in s.move_list] for s in stored] == [['device', 'device', 'host']] * 2
    seq.move_list[0].statistics = dict(n_accepted=2, n_proposed=4)
    assert seq.move_list[0].n_accepted == 2 and seq.move_list[0].proposal == 'device'


def test_a_subclass_with_its_own_proposal_is_refused_by_name():
    class Jitter(mcmc.MCDisplacementMove):
        def _propose_positions(self, positions, rng=None):
            return positions + 0.01

    class Plain(mcmc.MCRotationMove):
        pass

    with pytest.raises(NotImplementedError, match='Jitter'):
        Jitter(proposal='device').device_description(5)
    kind, atoms, sigma = Plain(atom_subset=[4, 1], proposal='device').device_description(5)
    assert kind == 1 and atoms.tolist() == [4, 1] and atoms.dtype == np.int32
    kind, atoms, sigma = mcmc.MCDisplacementMove(displacement_sigma=2.0 * unit.angstrom, atom_subset=[3], proposal='device').device_description(5)
    assert kind == 0 and atoms.tolist() == [3] and abs(sigma - 0.2) < 1e-15
    assert mcmc.MCRotationMove(proposal='device').device_description(4)[1].tolist() == [0, 1, 2, 3]
    # through the sampler: the refusal comes before anything is sent to an engine
    ho = testsystems.HarmonicOscillator()
    s = MultiStateSampler(mcmc_moves=Jitter(proposal='device'), number_of_iterations=1, engine=_RecordingEngine(), seed=1,
                          online_analysis_interval=None)
    s.create([states.ThermodynamicState(ho.system, 300.0 * unit.kelvin)],
             [states.SamplerState(np.zeros((1, 3)), box_vectors=ho.system.getDefaultPeriodicBoxVectors())], storage=None)
    with pytest.raises(NotImplementedError, match='Jitter'):
        s.run()
    assert s._engine.calls == []


class _RecordingEngine(OracleEngine):
    """The f64 oracle engine with an ``mc_rigid_moves`` that records what the sampler sends and accepts every other trial."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def mc_rigid_moves(self, moves, iteration):
        self.calls.append(([(k, a.tolist(), s, p) for k, a, s, p in moves], int(iteration)))
        acc = np.zeros((len(moves), self.R), dtype=np.int32)
        acc[:, ::2] = 1
        return acc


def test_consecutive_device_moves_go_to_the_engine_in_one_call_and_are_credited_per_state():
    """SequenceMove([device, device, host, device]): one call for the first two, the host path for the third, one call for the
    fourth -- in order; the flags are credited to the moves of the state each replica is in."""
    ho = testsystems.HarmonicOscillator(K=100.0 * unit.kilojoules_per_mole / unit.nanometer ** 2, mass=12.0 * unit.amu)
    thermo = [states.ThermodynamicState(ho.system, t * unit.kelvin) for t in (200.0, 300.0, 450.0)]
    ss = states.SamplerState(np.zeros((1, 3)), box_vectors=ho.system.getDefaultPeriodicBoxVectors())
    seq = mcmc.SequenceMove([mcmc.MCDisplacementMove(displacement_sigma=0.05 * unit.nanometer, proposal='device'),
                             mcmc.MCRotationMove(proposal='device'),
                             mcmc.MCDisplacementMove(displacement_sigma=0.05 * unit.nanometer),
                             mcmc.MCDisplacementMove(displacement_sigma=0.07 * unit.nanometer, proposal='device')])
    eng = _RecordingEngine()
    s = MultiStateSampler(mcmc_moves=seq, number_of_iterations=2, engine=eng, seed=3, online_analysis_interval=None)
    s.create(thermo, [copy.deepcopy(ss) for _ in thermo], storage=None)
    s.run()
    want = [[(0, [0], 0.05, 0), (1, [0], 0.0, 1)], [(0, [0], 0.07, 3)]]
    assert [c[0] for c in eng.calls] == want * 2 and [c[1] for c in eng.calls] == [1, 1, 2, 2]
    for k, state_moves in enumerate(s._mcmc_moves):          # no mixing: replica r stays in state r; replicas 0 and 2 were accepted
        for place in (0, 1, 3):
            m = state_moves.move_list[place]
            assert (m.n_accepted, m.n_proposed) == (2 if k in (0, 2) else 0, 2)
        assert state_moves.move_list[2].n_proposed == 2     # the host move in between ran its own path
    # moves that differ between states in nothing but the proposal are refused like any other difference
    mixed = [mcmc.MCDisplacementMove(proposal=p) for p in ('host', 'device', 'host')]
    s2 = MultiStateSampler(mcmc_moves=mixed, number_of_iterations=1, engine=_RecordingEngine(), seed=3, online_analysis_interval=None)
    with pytest.raises(NotImplementedError, match='identical'):
        s2.create(thermo, [copy.deepcopy(ss) for _ in thermo], storage=None)
        s2.run()
