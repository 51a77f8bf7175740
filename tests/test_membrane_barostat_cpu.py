"""CPU: the NPgammaT ensemble of ThermodynamicState (MonteCarloAnisotropicBarostat / MonteCarloMembraneBarostat Systems, states.py:507,
1314-1353, 1656-1843, 1909-1916) and the f64 oracle of the per-axis Monte Carlo moves (membrane_barostat_oracle.py), pinned by the
exact ideal-gas distributions independently of the device."""
import os
import pickle
import numpy as np
import pytest
import oracle
from openmmtools_amd import testsystems as ts, states, mcmc, unit, _engine
from openmmtools_amd.states import ThermodynamicState, ThermodynamicsError, SamplerState
from openmmtools_amd.system import (MonteCarloAnisotropicBarostat, MonteCarloMembraneBarostat, System, system_to_desc)
from openmmtools_amd.multistate import ParallelTemperingSampler, MultiStateSampler, MultiStateReporter
from oracle.forcefield import ForceFieldOracle
import membrane_barostat_oracle as mbo
from membrane_barostat_oracle import check_ideal_gas_statistics, N_MOVES, N_BURN_IN

KB = 0.008314462618153242
BAR_NM = unit.bar * unit.nanometer
CPU_LIB = os.path.join(os.path.dirname(os.path.abspath(oracle.__file__)), '_build', 'libremd_cpu.so')
Membrane = MonteCarloMembraneBarostat


def _with(system, *forces):
    """a copy of ``system`` (same particles, forces and box) with ``forces`` added"""
    s = System()
    s.masses, s.constraints, s._box = list(system.masses), list(system.constraints), system._box
    s.forces = list(system.forces) + list(forces)
    return s


def _raises(code, fn):
    with pytest.raises(ThermodynamicsError) as e:
        fn()
    assert e.value.code == code
    assert str(e.value) == ThermodynamicsError.error_messages[code].format('MonteCarloFlexibleBarostat')
    return e.value


def test_force_classes_have_openmms_accessors():
    a = MonteCarloAnisotropicBarostat((1.0 * unit.bar, 2.0 * unit.bar, 3.0 * unit.bar), 300.0, True, False, True)
    assert a.getDefaultPressure() == (1.0 * unit.bar, 2.0 * unit.bar, 3.0 * unit.bar) and a.getDefaultTemperature() == 300.0
    assert (a.getScaleX(), a.getScaleY(), a.getScaleZ()) == (True, False, True) and a.getFrequency() == 25
    a.setFrequency(10); a.setDefaultTemperature(310.0); a.setDefaultPressure((5.0,) * 3)
    assert a.getFrequency() == 10 and a.getDefaultTemperature() == 310.0 and a.getDefaultPressure() == (5.0, 5.0, 5.0)
    assert (Membrane.XYIsotropic, Membrane.XYAnisotropic, Membrane.ZFree, Membrane.ZFixed, Membrane.ConstantVolume) == (0, 1, 0, 1, 2)
    m = Membrane(1.0 * unit.bar, 20.0 * BAR_NM, 300.0, Membrane.XYAnisotropic, Membrane.ConstantVolume, 15)
    assert m.getDefaultPressure() == 1.0 * unit.bar and m.getDefaultSurfaceTension() == 20.0 * BAR_NM
    assert abs(BAR_NM - 0.06022140857) < 1e-9                                   # the factor of include/remd_hip.h
    assert (m.getXYMode(), m.getZMode(), m.getFrequency(), m.getDefaultTemperature()) == (1, 2, 15, 300.0)
    m.setXYMode(Membrane.XYIsotropic); m.setZMode(Membrane.ZFree); m.setDefaultSurfaceTension(3.0); m.setDefaultPressure(2.0)
    assert (m.getXYMode(), m.getZMode(), m.getDefaultSurfaceTension(), m.getDefaultPressure()) == (0, 0, 3.0, 2.0)
    assert not m.usesPeriodicBoundaryConditions() and not a.usesPeriodicBoundaryConditions()
    # no energy: the descriptor of the System (and its fingerprint) is the one without the barostat
    lj = ts.LennardJonesFluid(nparticles=64)
    assert _with(lj.system, m).fingerprint() == lj.system.fingerprint()
    assert _with(lj.system, m).usesPeriodicBoundaryConditions()


def test_membrane_state_has_a_surface_tension_and_its_reduced_potential():
    """A state on a System with a membrane barostat is an NPgammaT state: u = beta (U + p V - gamma A_xy)."""
    lj = ts.LennardJonesFluid(nparticles=64)
    p, g, T = 30.0 * unit.bar, 20.0 * BAR_NM, 120.0
    system = _with(lj.system, Membrane(p, g, 300.0, Membrane.XYIsotropic, Membrane.ZFree, 10))
    state = ThermodynamicState(system, T)
    assert state.pressure == p and state.surface_tension == g and state.barostat_frequency == 10
    npt = ThermodynamicState(lj.system, T, pressure=p)
    assert npt.surface_tension is None
    ss = SamplerState(lj.positions, box_vectors=np.diag([3.0, 4.0, 5.0]))
    ss.potential_energy = -12.5
    assert ss.area_xy == 12.0
    beta = 1.0 / (KB * T)
    assert np.isclose(state.reduced_potential(ss), beta * (-12.5 + p * 60.0 - g * 12.0), rtol=1e-14, atol=0)
    assert np.isclose(state.reduced_potential(ss) - npt.reduced_potential(ss), -beta * g * 12.0, rtol=1e-12, atol=0)
    assert np.isclose(ThermodynamicState._compute_reduced_potential(1.0, T, 2.0, 3.0, 4.0, 0.5), beta * (1.0 + 6.0 - 2.0), rtol=1e-14, atol=0)
    # given values override the barostat's
    state = ThermodynamicState(system, T, pressure=2.0 * p, surface_tension=3.0 * g)
    assert state.pressure == 2.0 * p and state.surface_tension == 3.0 * g
    # the barostat is a copy of the System's carrying the state's numbers
    b = state.barostat
    assert isinstance(b, Membrane) and b is not system.getForce(system.getNumForces() - 1)
    assert (b.getDefaultPressure(), b.getDefaultSurfaceTension(), b.getDefaultTemperature()) == (2.0 * p, 3.0 * g, T)
    assert (b.getXYMode(), b.getZMode(), b.getFrequency()) == (Membrane.XYIsotropic, Membrane.ZFree, 10)
    assert system.getForce(system.getNumForces() - 1).getDefaultPressure() == p
    state.surface_tension = 5.0
    assert state.surface_tension == 5.0 and state.barostat.getDefaultSurfaceTension() == 5.0
    back = pickle.loads(pickle.dumps(state))
    assert back.surface_tension == 5.0 and back.pressure == 2.0 * p and isinstance(back.barostat, Membrane)
    # compound states keep the ensemble
    cs = states.CompoundThermodynamicState(state, [states.AlchemicalState()])
    assert cs.surface_tension == 5.0 and isinstance(cs.barostat, Membrane)


def test_state_rules_of_the_barostats():
    lj = ts.LennardJonesFluid(nparticles=64)
    p, g, T = 30.0 * unit.bar, 20.0 * BAR_NM, 120.0
    memb = Membrane(p, g, T, Membrane.XYIsotropic, Membrane.ZFree)
    aniso = MonteCarloAnisotropicBarostat((p, p, p), T)
    E = ThermodynamicsError
    _raises(E.MULTIPLE_BAROSTATS, lambda: ThermodynamicState(_with(lj.system, memb, aniso), T))
    _raises(E.UNSUPPORTED_ANISOTROPIC_BAROSTAT,
            lambda: ThermodynamicState(_with(lj.system, MonteCarloAnisotropicBarostat((p, p, p), T, False, False, False)), T))
    _raises(E.UNSUPPORTED_ANISOTROPIC_BAROSTAT,
            lambda: ThermodynamicState(_with(lj.system, MonteCarloAnisotropicBarostat((p, 2 * p, p), T)), T))
    # the pressure of an unscaled axis does not matter; the state's pressure is the first scaled axis'
    st = ThermodynamicState(_with(lj.system, MonteCarloAnisotropicBarostat((7.0, p, p), T, False, True, True)), T)
    assert st.pressure == p and st.surface_tension is None
    b = st.barostat
    assert isinstance(b, MonteCarloAnisotropicBarostat) and b.getDefaultPressure() == (p, p, p) and b.getDefaultTemperature() == T
    assert (b.getScaleX(), b.getScaleY(), b.getScaleZ()) == (False, True, True)

    class MonteCarloFlexibleBarostat(MonteCarloAnisotropicBarostat):
        pass
    err = _raises(E.UNSUPPORTED_BAROSTAT, lambda: ThermodynamicState(_with(lj.system, MonteCarloFlexibleBarostat((p, p, p), T)), T))
    assert 'MonteCarloFlexibleBarostat' in str(err)
    # a surface tension needs a membrane barostat
    _raises(E.INCOMPATIBLE_ENSEMBLE, lambda: ThermodynamicState(lj.system, T, pressure=p, surface_tension=g))
    _raises(E.INCOMPATIBLE_ENSEMBLE, lambda: ThermodynamicState(_with(lj.system, aniso), T, surface_tension=g))
    _raises(E.INCOMPATIBLE_ENSEMBLE, lambda: ThermodynamicState(ts.HarmonicOscillator().system, 300.0, surface_tension=g))
    for plain in (ThermodynamicState(lj.system, T, pressure=p), ThermodynamicState(_with(lj.system, aniso), T), ThermodynamicState(lj.system, T)):
        _raises(E.SURFACE_TENSION_NOT_SUPPORTED, lambda: setattr(plain, 'surface_tension', g))
        plain.surface_tension = None
        assert plain.surface_tension is None
    ms = ThermodynamicState(_with(lj.system, memb), T)
    _raises(E.SURFACE_TENSION_NOT_SUPPORTED, lambda: setattr(ms, 'surface_tension', None))
    assert ms.surface_tension == g
    # plain NPT keeps its settings object, NVT has no barostat
    assert isinstance(ThermodynamicState(lj.system, T, pressure=p).barostat, states.MonteCarloBarostatSettings)
    assert ThermodynamicState(lj.system, T).barostat is None
    _raises(E.BAROSTATED_NONPERIODIC, lambda: ThermodynamicState(_with(ts.HarmonicOscillator().system, memb), 300.0))
    # compatibility: type, modes and scale flags
    def S(force):
        return ThermodynamicState(_with(lj.system, force), T)
    assert ms.is_state_compatible(S(Membrane(2 * p, 3 * g, 2 * T, Membrane.XYIsotropic, Membrane.ZFree)))
    assert not ms.is_state_compatible(S(Membrane(p, g, T, Membrane.XYAnisotropic, Membrane.ZFree)))
    assert not ms.is_state_compatible(S(Membrane(p, g, T, Membrane.XYIsotropic, Membrane.ZFixed)))
    assert not ms.is_state_compatible(S(aniso)) and not ms.is_state_compatible(ThermodynamicState(lj.system, T, pressure=p))
    assert not ms.is_state_compatible(ThermodynamicState(lj.system, T))
    assert S(aniso).is_state_compatible(S(MonteCarloAnisotropicBarostat((2 * p,) * 3, T)))
    assert not S(aniso).is_state_compatible(S(MonteCarloAnisotropicBarostat((p, p, p), T, True, True, False)))
    assert not S(aniso).is_state_compatible(ThermodynamicState(lj.system, T, pressure=p))
    assert ms._is_barostat_type_consistent(memb) and not ms._is_barostat_type_consistent(aniso)


# ---- the oracle's moves against the exact ideal-gas distributions ----------------------------------------------------------------

def _ideal_gas(kind, axes, zmode, gamma_of_box):
    """LennardJonesFluid(64, epsilon = 0) at 300 K, 30 bar under the schedule of tests/test_npt_cpu.py::test_oracle_barostat_ideal_gas_volume:
    6000 moves of one replica, the first 1000 dropped (the energy is zero, so no dynamics is needed in between).  The start is far from
    equilibrium (the membrane case starts at 13.6 nm^2 and ends around 48.6) and the volume step grows by 1.1 per ten moves only, which is
    why the burn-in is that long."""
    N, T, p, R = 64, 300.0, 30.0 * unit.bar, 1
    lj = ts.LennardJonesFluid(nparticles=N, epsilon=0.0)
    box0 = np.diag(lj.system.getDefaultPeriodicBoxVectors()).copy()
    gamma = gamma_of_box(p, box0)
    baro = mbo.AxisOracleBarostat(ForceFieldOracle(system_to_desc(lj.system)), 11, [[i] for i in range(N)], kind, axes, zmode, gamma)
    x = [lj.positions.copy() for _ in range(R)]
    box = [box0.copy() for _ in range(R)]
    boxes = []
    for a in range(N_MOVES):
        for r in range(R):
            x[r], box[r], _ = baro.attempt(x[r], box[r], KB * T, p, r, a)
        if a >= N_BURN_IN:
            boxes.append(np.array(box))
    return N, KB * T, p, gamma, box0, np.array(boxes), baro


def _oracle_counts(baro, R):
    return (np.array([baro.state[r]['attempted'] for r in range(R)]), np.array([baro.state[r]['accepted'] for r in range(R)]))


def test_oracle_anisotropic_x_only_ideal_gas():
    """Only x is scaled: P(V) ~ V^N exp(-beta p V) on V = Lx Ly0 Lz0, so <V> = (N + 1) kT / p; Ly and Lz never change."""
    N, kT, p, _, box0, boxes, baro = _ideal_gas(mbo.ANISOTROPIC, 1, 0, lambda p, box: 0.0)
    assert np.all(boxes[..., 1] == box0[1]) and np.all(boxes[..., 2] == box0[2])
    na, nc = _oracle_counts(baro, 1)
    assert np.all(na[:, 0] == N_MOVES) and np.all(na[:, 1:] == 0)
    check_ideal_gas_statistics(np.prod(boxes, axis=-1), (N + 1) * kT / p, N, na, nc, [0])


def test_oracle_membrane_xy_isotropic_z_fixed_ideal_gas():
    """XYIsotropic + ZFixed with gamma = p Lz0 / 2: V = A Lz0, the weight is A^N exp(-beta (p Lz0 - gamma) A), so
    <A> = (N + 1) kT / (p Lz0 - gamma); Lx / Ly is constant and Lz unchanged."""
    N, kT, p, gamma, box0, boxes, baro = _ideal_gas(mbo.MEMBRANE, mbo.XY_ISOTROPIC, mbo.Z_FIXED, lambda p, box: 0.5 * p * box[2])
    assert p * box0[2] - gamma > 0
    assert np.all(boxes[..., 2] == box0[2])
    assert np.allclose(boxes[..., 0] / boxes[..., 1], box0[0] / box0[1], rtol=1e-12, atol=0)
    na, nc = _oracle_counts(baro, 1)
    assert np.all(na[:, 0] == N_MOVES) and np.all(na[:, 1:] == 0)
    check_ideal_gas_statistics(boxes[..., 0] * boxes[..., 1], (N + 1) * kT / (p * box0[2] - gamma), N, na, nc, [0])


def test_oracle_axis_choice_and_constant_volume():
    """every allowed axis is drawn, only allowed axes move, and ConstantVolume keeps V to f64 rounding"""
    lj = ts.LennardJonesFluid(nparticles=64)
    sysm = ForceFieldOracle(system_to_desc(lj.system))
    mols = [[i] for i in range(64)]
    box0 = np.diag(lj.system.getDefaultPeriodicBoxVectors()).copy()
    for kind, axes, zmode, moving in ((mbo.ANISOTROPIC, 7, 0, [0, 1, 2]), (mbo.ANISOTROPIC, 6, 0, [1, 2]), (mbo.MEMBRANE, mbo.XY_ANISOTROPIC, mbo.Z_FIXED, [0, 1]),
                                      (mbo.MEMBRANE, mbo.XY_ISOTROPIC, mbo.Z_FREE, [0, 2]), (mbo.MEMBRANE, mbo.XY_ANISOTROPIC, mbo.CONSTANT_VOLUME, [0, 1])):
        baro = mbo.AxisOracleBarostat(sysm, 3, mols, kind, axes, zmode, 20.0 * BAR_NM)
        assert baro.allowed_axes() == moving
        x, box = lj.positions.copy(), box0.copy()
        for a in range(24):
            x, box, _ = baro.attempt(x, box, KB * 120.0, 40.0 * unit.bar, 0, a)
        st = baro.state[0]
        assert [k for k in range(3) if st['attempted'][k] > 0] == moving and st['attempted'].sum() == 24 and st['accepted'].sum() > 0
        follows = [1] if (kind == mbo.MEMBRANE and axes == mbo.XY_ISOTROPIC) else []            # y goes with x
        follows += [2] if (kind == mbo.MEMBRANE and zmode == mbo.CONSTANT_VOLUME) else []          # z answers the plane
        still = [k for k in range(3) if k not in moving + follows]
        assert np.all(box[still] == box0[still]) and np.any(box != box0)
        if zmode == mbo.CONSTANT_VOLUME and kind == mbo.MEMBRANE:
            assert abs(np.prod(box) / np.prod(box0) - 1.0) < 24 * 4 * 2.0 ** -52 and box[2] != box0[2]


# ---- sampler and engine plumbing ------------------------------------------------------------------------------------------------

def _npgt_states(lj, xymode=Membrane.XYIsotropic, zmode=Membrane.ZFree, T=120.0):
    system = _with(lj.system, Membrane(30.0 * unit.bar, 20.0 * BAR_NM, T, xymode, zmode))
    return ThermodynamicState(system, T), SamplerState(lj.positions, box_vectors=lj.system.getDefaultPeriodicBoxVectors())


def _move():
    return mcmc.LangevinSplittingDynamicsMove(timestep=2.0 * unit.femtosecond, collision_rate=1.0 / unit.picosecond, n_steps=50,
                                              reassign_velocities=True, splitting='V R O R V')


def test_sampler_on_npgammat_states_uses_the_membrane_move_and_its_ukl(tmp_path):
    lj = ts.LennardJonesFluid(nparticles=64)
    tstate, ss = _npgt_states(lj)
    eng = mbo.AxisOracleEngine(ForceFieldOracle)
    path = str(tmp_path / 'npgt')
    s = ParallelTemperingSampler(mcmc_moves=_move(), number_of_iterations=2, engine=eng, seed=3)
    s.create(tstate, [ss], storage=MultiStateReporter(path, checkpoint_interval=1), min_temperature=120.0, max_temperature=150.0, n_temperatures=3)
    assert eng._axis == (mbo.MEMBRANE, Membrane.XYIsotropic, Membrane.ZFree) and np.all(eng.tension == 20.0 * BAR_NM)
    s.run()
    assert isinstance(eng._baro, mbo.AxisOracleBarostat)
    _, na, _ = eng.barostat_axis_stats()
    assert np.all(na.sum(axis=1) == 4) and np.all(na[:, 1] == 0)
    s._sampler_states_stale = True
    s._sync_sampler_states()
    box0 = np.diag(lj.system.getDefaultPeriodicBoxVectors())
    for st in s.sampler_states:
        assert np.any(st.box_edges != box0)
    # u_kl = the states' own reduced potentials of the replicas' sampler states
    U = eng.potentials()
    for r, st in enumerate(s.sampler_states):
        st.potential_energy = U[r]
        ref = [t.reduced_potential(st) for t in s._thermodynamic_states]
        assert np.allclose(s.energy_thermodynamic_states[r], ref, rtol=1e-10)
        plain = [ThermodynamicState(lj.system, t.temperature, pressure=t.pressure).reduced_potential(st) for t in s._thermodynamic_states]
        assert np.allclose(np.array(plain) - ref, [t.beta * t.surface_tension * st.area_xy for t in s._thermodynamic_states], rtol=1e-9)
    # the record container round-trips the NPgammaT sampler, resume included
    energies, labels = s.energy_thermodynamic_states.copy(), s.replica_thermodynamic_states.copy()
    del s
    back = ParallelTemperingSampler.from_storage(path, engine=mbo.AxisOracleEngine(ForceFieldOracle))
    assert [t.surface_tension for t in back._thermodynamic_states] == [20.0 * BAR_NM] * 3
    assert all(isinstance(t.barostat, Membrane) for t in back._thermodynamic_states)
    assert np.array_equal(back.replica_thermodynamic_states, labels) and np.allclose(back.energy_thermodynamic_states, energies)
    back.extend(1)
    assert back.iteration == 3 and back._engine._axis == (mbo.MEMBRANE, Membrane.XYIsotropic, Membrane.ZFree)


def test_sampler_refuses_mixed_barostats_and_pools():
    lj = ts.LennardJonesFluid(nparticles=64)
    a, ss = _npgt_states(lj)
    b, _ = _npgt_states(lj, zmode=Membrane.ZFixed)
    s = MultiStateSampler(mcmc_moves=_move(), number_of_iterations=1, engine=mbo.AxisOracleEngine(ForceFieldOracle), seed=3)
    with pytest.raises(ValueError, match='different barostats'):
        s.create([a, b], [ss, ss], storage=None)
    s = MultiStateSampler(mcmc_moves=_move(), number_of_iterations=1, engine=mbo.AxisOracleEngine(ForceFieldOracle), seed=3)
    with pytest.raises(ValueError, match='NPT and NVT'):
        s.create([a, ThermodynamicState(lj.system, 120.0)], [ss, ss], storage=None)
    from openmmtools_amd.multistate._engine_pool import EnginePool
    with pytest.raises(NotImplementedError, match='remd_hip_barostat.h'):
        EnginePool(mbo.AxisOracleEngine(ForceFieldOracle), [[0], [1]]).set_barostat_axes(np.ones(2), None, 1, 7, 0, 25)


def test_barostat_move_on_npgammat_states():
    lj = ts.LennardJonesFluid(nparticles=64)
    tstate, ss = _npgt_states(lj, xymode=Membrane.XYAnisotropic, zmode=Membrane.ZFixed)
    eng = mbo.AxisOracleEngine(ForceFieldOracle)
    sampler = mcmc.MCMCSampler(tstate, ss, move=mcmc.MonteCarloBarostatMove(n_attempts=6), engine=eng, seed=5)
    sampler.run(2)
    _, na, nc = eng.barostat_axis_stats()
    assert na.sum() == 12 and na[0, 2] == 0 and nc.sum() > 0
    box = sampler.sampler_state.box_edges
    box0 = np.diag(lj.system.getDefaultPeriodicBoxVectors())
    assert box[2] == box0[2] and np.any(box[:2] != box0[:2])


def test_a_library_without_the_extension_says_so():
    """include/remd_hip_barostat.h is GPU-only: the CPU port of the ABI does not export it, and the engine names the header"""
    eng = _engine.HipEngine(lib_path=CPU_LIB)
    assert not hasattr(eng.lib, 'remd_set_barostat_axes')
    with pytest.raises(NotImplementedError, match='remd_set_barostat_axes.*include/remd_hip_barostat.h'):
        eng.set_barostat_axes(np.ones(2), None, _engine.BAROSTAT_ANISOTROPIC, 7, 0, 25)
    with pytest.raises(NotImplementedError, match='remd_get_barostat_axis_stats.*include/remd_hip_barostat.h'):
        eng.barostat_axis_stats()


def test_the_netcdf4_layout_is_refused_by_name(tmp_path, caplog):
    """the .nc layout stores Systems as XML, which is not written for the two barostats: 'auto' falls back to the record container
    with the usual warning, 'netcdf4' raises naming the force"""
    import logging
    from openmmtools_amd.multistate._reference_store import ReferenceStoreWriter
    lj = ts.LennardJonesFluid(nparticles=64)
    tstate, ss = _npgt_states(lj)
    assert ReferenceStoreWriter.can_store([tstate], [], [_move()]) == 'a System with a MonteCarloMembraneBarostat'
    assert ReferenceStoreWriter.can_store([ThermodynamicState(lj.system, 120.0, pressure=1.0)], [], [_move()]) is None
    s = MultiStateSampler(mcmc_moves=_move(), number_of_iterations=1, engine=mbo.AxisOracleEngine(ForceFieldOracle), seed=3)
    rep = MultiStateReporter(str(tmp_path / 'auto.nc'), checkpoint_interval=1)
    with caplog.at_level(logging.WARNING):
        s.create([tstate], [ss], storage=rep)
    assert rep.layout == 'records' and 'MonteCarloMembraneBarostat' in caplog.text
    s = MultiStateSampler(mcmc_moves=_move(), number_of_iterations=1, engine=mbo.AxisOracleEngine(ForceFieldOracle), seed=3)
    with pytest.raises(NotImplementedError, match='MonteCarloMembraneBarostat'):
        s.create([tstate], [ss], storage=MultiStateReporter(str(tmp_path / 'forced.nc'), checkpoint_interval=1, layout='netcdf4'))
