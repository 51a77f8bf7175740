"""CPU: the restraint forces (openmmtools_amd/forces.py), GlobalParameterState (states.py), the restraints in the system description and
the engine binding's refusal where the library has no restraints.  Golden expressions: tests/golden/make_golden_restraint_expressions.py."""
import json
import math
import os

import numpy as np
import pytest
import scipy.integrate

from openmmtools_amd import forces, states, testsystems, unit
from openmmtools_amd.system import system_to_desc

HERE = os.path.dirname(os.path.abspath(__file__))
G = json.load(open(os.path.join(HERE, 'golden', 'reference_restraint_expressions.json')))


class RestraintState(states.GlobalParameterState):
    lambda_restraints = states.GlobalParameterState.GlobalParameter('lambda_restraints', standard_value=1.0)


def _all_four():
    return {'HarmonicRestraintForce': forces.HarmonicRestraintForce(100.0, [0, 1, 2], [3, 4]),
            'HarmonicRestraintBondForce': forces.HarmonicRestraintBondForce(100.0, 0, 3),
            'FlatBottomRestraintForce': forces.FlatBottomRestraintForce(100.0, 0.5, [0, 1, 2], [3, 4]),
            'FlatBottomRestraintBondForce': forces.FlatBottomRestraintBondForce(100.0, 0.5, 0, 3)}


def test_energy_strings_and_class_hashes_are_the_references():
    for name, f in _all_four().items():
        assert f.getEnergyFunction() == G['classes'][name]['energy']
        assert f.getGlobalParameterName(0) == '_restorable_force__class_hash'
        assert f.getGlobalParameterDefaultValue(0) == G['classes'][name]['class_hash']
        assert f.controlling_parameter_name == 'lambda_restraints' and f.getGlobalParameterName(1) == 'lambda_restraints'
        assert not f.usesPeriodicBoundaryConditions()


def test_energies_on_the_golden_grid():
    for name, f in _all_four().items():
        cls = type(f)
        for (r, K, r0, lam), want in zip(G['grid'], G['classes'][name]['values']):
            g = cls(K, r0, 0, 1) if 'FlatBottom' in name and 'Bond' in name else cls(K, r0, [0], [1]) if 'FlatBottom' in name else \
                cls(K, 0, 1) if 'Bond' in name else cls(K, [0], [1])
            g.setGlobalParameterDefaultValue(1, lam)
            assert g.energy_of_distance(r) == pytest.approx(want, rel=1e-14, abs=1e-300), (name, r, K, r0, lam)


def test_properties_and_setters():
    f = forces.FlatBottomRestraintForce(200.0, 0.4, [0, 1], [5, 6, 7], controlling_parameter_name='lambda_r')
    assert f.spring_constant == 200.0 and f.well_radius == 0.4 and f.controlling_parameter_name == 'lambda_r'
    assert dict(f.restraint_parameters) == {'K': 200.0, 'r0': 0.4}
    assert f.getEnergyFunction().startswith('lambda_r * (')
    f.restrained_atom_indices1 = [2, 3]
    f.restrained_atom_indices2 = [9]
    assert f.restrained_atom_indices1 == [2, 3] and f.restrained_atom_indices2 == [9]
    b = forces.HarmonicRestraintBondForce(50.0, 1, 2)
    b.restrained_atom_indices1 = [4]
    b.restrained_atom_indices2 = [7]
    assert (b.restrained_atom_indices1, b.restrained_atom_indices2, b.spring_constant) == ([4], [7], 50.0)
    b.setUsesPeriodicBoundaryConditions(True)
    assert b.usesPeriodicBoundaryConditions()


def test_distance_at_energy():
    h = forces.HarmonicRestraintForce(100.0, [0], [1])
    assert h.distance_at_energy(2.0) == pytest.approx(math.sqrt(2 * 2.0 / 100.0))
    fb = forces.FlatBottomRestraintForce(100.0, 0.3, [0], [1])
    assert fb.distance_at_energy(2.0) == pytest.approx(0.3 + math.sqrt(2 * 2.0 / 100.0))
    with pytest.raises(ValueError):
        fb.distance_at_energy(0.0)


def test_find_forces():
    hg = testsystems.HostGuestVacuum()
    f = forces.HarmonicRestraintForce(100.0, [0], [130])
    hg.system.addForce(f)
    idx, found = forces.find_forces(hg.system, forces.HarmonicRestraintForce, only_one=True)
    assert found is f and idx == hg.system.getNumForces() - 1
    assert len(forces.find_forces(hg.system, forces.RadiallySymmetricRestraintForce, include_subclasses=True)) == 1
    assert len(forces.find_forces(hg.system, '.*Restraint.*')) == 1
    with pytest.raises(forces.NoForceFoundError):
        forces.find_forces(hg.system, forces.FlatBottomRestraintForce, only_one=True)
    hg.system.addForce(forces.HarmonicRestraintForce(10.0, [1], [131]))
    with pytest.raises(forces.MultipleForcesError):
        forces.find_forces(hg.system, forces.HarmonicRestraintForce, only_one=True)


def test_restore_interface_from_the_class_hash():
    """a plain CustomCentroidBondForce carrying the hash (what a document the reference wrote reads back as) is the restraint again"""
    src = forces.FlatBottomRestraintForce(100.0, 0.5, [0, 1], [3])
    plain = forces.CustomCentroidBondForce(2, src.getEnergyFunction())
    for i in range(src.getNumGlobalParameters()):
        plain.addGlobalParameter(src.getGlobalParameterName(i), src.getGlobalParameterDefaultValue(i))
    for i in range(src.getNumPerBondParameters()):
        plain.addPerBondParameter(src.getPerBondParameterName(i))
    plain.addGroup([0, 1]); plain.addGroup([3]); plain.addBond([0, 1], [100.0, 0.5])
    assert forces.restore_interface(plain) and type(plain) is forces.FlatBottomRestraintForce and plain.well_radius == 0.5


def _integrated_harmonic_volume(K, beta, radius):
    return scipy.integrate.quad(lambda r: 4 * math.pi * r * r * math.exp(-beta * 0.5 * K * r * r), 0.0, radius, epsabs=0, epsrel=1e-13)[0]


def test_standard_state_correction_harmonic_is_the_integral():
    hg = testsystems.HostGuestExplicit()
    ts = states.ThermodynamicState(hg.system, 300.0)
    f = forces.HarmonicRestraintForce(0.2 * 418.4, [0], [130])
    radius = f.distance_at_energy(100.0 * ts.kT)
    V = forces._compute_harmonic_volume(radius, f.spring_constant, ts.beta)
    assert V == pytest.approx(_integrated_harmonic_volume(f.spring_constant, ts.beta, radius), rel=1e-8)
    assert f.compute_standard_state_correction(ts) == pytest.approx(-math.log(forces.STANDARD_STATE_VOLUME / V), rel=1e-12)
    # square well: the sphere inside the energy cutoff
    sw = f.compute_standard_state_correction(ts, square_well=True, energy_cutoff=100.0)
    assert sw == pytest.approx(-math.log(forces.STANDARD_STATE_VOLUME / (4 / 3 * math.pi * radius ** 3)), rel=1e-12)


def test_standard_state_correction_flat_bottom_and_errors():
    hg = testsystems.HostGuestExplicit()
    ts = states.ThermodynamicState(hg.system, 300.0)
    f = forces.FlatBottomRestraintForce(1000.0, 0.5, [0], [130])
    beta, K, r0 = ts.beta, 1000.0, 0.5
    rmax = r0 + math.sqrt(2 * 100.0 * ts.kT / K)
    V = 4 / 3 * math.pi * r0 ** 3 + scipy.integrate.quad(lambda r: 4 * math.pi * r * r * math.exp(-beta * 0.5 * K * (r - r0) ** 2), r0, rmax)[0]
    assert f.compute_standard_state_correction(ts) == pytest.approx(-math.log(forces.STANDARD_STATE_VOLUME / V), rel=1e-8)
    assert f.compute_standard_state_correction(ts, square_well=True, energy_cutoff=100.0) == pytest.approx(
        -math.log(forces.STANDARD_STATE_VOLUME / (4 / 3 * math.pi * rmax ** 3)), rel=1e-12)
    # the volume cap: a very weak restraint is bounded by the box
    weak = forces.HarmonicRestraintForce(1e-6, [0], [130])
    assert weak.compute_standard_state_correction(ts) == pytest.approx(-math.log(forces.STANDARD_STATE_VOLUME / ts.volume), rel=1e-12)
    npt = states.ThermodynamicState(hg.system, 300.0, pressure=1.0 * unit.atmosphere)
    with pytest.raises(TypeError, match='max_volume must be provided with NPT ensemble'):
        f.compute_standard_state_correction(npt)
    assert f.compute_standard_state_correction(npt, max_volume='system') == pytest.approx(f.compute_standard_state_correction(ts))
    vac = states.ThermodynamicState(testsystems.HostGuestVacuum().system, 300.0)
    with pytest.raises(TypeError, match='One between radius_cutoff'):
        f.compute_standard_state_correction(vac, square_well=True)


# ---- GlobalParameterState -------------------------------------------------------------------------------------------------------------
class TwoParameters(states.GlobalParameterState):
    lambda_restraints = states.GlobalParameterState.GlobalParameter('lambda_restraints', standard_value=1.0)
    gamma = states.GlobalParameterState.GlobalParameter('gamma', standard_value=1.0)


def test_global_parameter_state_basics():
    s = TwoParameters(lambda_restraints=0.5)
    assert s.lambda_restraints == 0.5 and s.gamma is None                          # undefined parameters read as None
    with pytest.raises(states.GlobalParameterError):
        TwoParameters(nonsense=1.0)
    s.set_function_variable('x', 0.25)
    s.gamma = states.GlobalParameterFunction('x**2')
    assert s.gamma == 0.0625 and s.get_function_variable('x') == 0.25
    with pytest.raises(states.GlobalParameterError):
        s.get_function_variable('y')
    with pytest.raises(states.GlobalParameterError):
        s.set_function_variable('gamma', 1.0)
    back = TwoParameters.__new__(TwoParameters)
    back.__setstate__(s.__getstate__())
    assert back == s and back.gamma == 0.0625
    sfx = TwoParameters(parameters_name_suffix='ligand', lambda_restraints=0.3)
    assert sfx.lambda_restraints_ligand == 0.3
    with pytest.raises(AttributeError):
        sfx.lambda_restraints
    with pytest.raises(NotImplementedError):
        s.apply_to_context(None)


def test_global_parameter_state_and_the_system():
    hg = testsystems.HostGuestVacuum()
    f = forces.HarmonicRestraintForce(100.0, [0], [130])
    hg.system.addForce(f)
    s = RestraintState.from_system(hg.system)
    assert s.lambda_restraints == 1.0
    s.check_system_consistency(hg.system)
    s.lambda_restraints = 0.25
    with pytest.raises(states.GlobalParameterError):
        s.check_system_consistency(hg.system)
    s.apply_to_system(hg.system)
    assert f.getGlobalParameterDefaultValue(1) == 0.25
    s.check_system_consistency(hg.system)
    with pytest.raises(states.GlobalParameterError):
        RestraintState.from_system(testsystems.HostGuestVacuum().system)          # no such parameter
    with pytest.raises(states.GlobalParameterError):
        RestraintState(lambda_restraints=None).apply_to_system(hg.system)          # not defined in this state
    with pytest.raises(states.GlobalParameterError):
        RestraintState(lambda_restraints=1.0).apply_to_system(testsystems.HostGuestVacuum().system)


def test_compound_states_protocol_and_compatibility():
    from openmmtools_amd import alchemy
    from openmmtools_amd.multistate.multistatesampler import restraint_lambdas
    hg = testsystems.HostGuestExplicit()
    system = alchemy.AbsoluteAlchemicalFactory().create_alchemical_system(hg.system, alchemy.AlchemicalRegion(alchemical_atoms=list(range(126, 156))))
    system.addForce(forces.HarmonicRestraintForce(100.0, list(range(126)), list(range(126, 156))))
    ts = states.ThermodynamicState(system, 300.0)
    sts = states.create_thermodynamic_state_protocol(ts, {'lambda_electrostatics': [1.0, 0.5, 0.0], 'lambda_restraints': [0.0, 0.5, 1.0]},
                                                     composable_states=[alchemy.AlchemicalState(), RestraintState(lambda_restraints=1.0)])
    assert [s.lambda_restraints for s in sts] == [0.0, 0.5, 1.0] and [s.lambda_electrostatics for s in sts] == [1.0, 0.5, 0.0]
    groups, _ = states.group_by_compatibility(sts)
    assert len(groups) == 1
    assert np.array_equal(restraint_lambdas(system, ['lambda_restraints'], sts)[:, 0], [0.0, 0.5, 1.0])
    # a state with no GlobalParameterState: the force's own default
    assert restraint_lambdas(system, ['lambda_restraints'], [ts])[0, 0] == 1.0


def test_system_description_carries_the_restraint():
    hg = testsystems.HostGuestVacuum()
    plain = hg.system.fingerprint()
    f = forces.FlatBottomRestraintForce(300.0, 0.25, [0, 1, 2], [130, 131])
    f.setForceGroup(2)
    hg.system.addForce(f)
    d = system_to_desc(hg.system)['restraints']['000']
    assert (d['kind'], d['K'], d['r0'], d['periodic'], d['parameter'], d['force_group']) == (1, 300.0, 0.25, 0, 'lambda_restraints', 2)
    assert np.array_equal(d['atoms1'], [0, 1, 2]) and np.allclose(d['weights1'], [hg.system.masses[i] for i in (0, 1, 2)])
    assert hg.system.fingerprint() != plain


def test_an_unsupported_custom_force_is_refused():
    hg = testsystems.HostGuestVacuum()
    c = forces.CustomCentroidBondForce(2, 'K*distance(g1,g2)')
    c.addGroup([0]); c.addGroup([1]); c.addPerBondParameter('K'); c.addBond([0, 1], [1.0])
    hg.system.addForce(c)
    with pytest.raises(NotImplementedError):
        system_to_desc(hg.system)


def test_the_cpu_port_refuses_restraints():
    from openmmtools_amd import _engine
    CPU_LIB = os.path.join(os.path.dirname(HERE), 'oracle', '_build', 'libremd_cpu.so')
    if not os.path.exists(CPU_LIB):
        import __graft_entry__
        __graft_entry__.build()
    eng = _engine.HipEngine(lib_path=CPU_LIB)
    hg = testsystems.HostGuestVacuum()
    hg.system.addForce(forces.HarmonicRestraintForce(100.0, [0], [130]))
    with pytest.raises(NotImplementedError, match='remd_set_restraints'):
        eng.set_system(system_to_desc(hg.system))


# ---- the system document and the store ----------------------------------------------------------------------------------------------
def _restrained(system):
    f = forces.FlatBottomRestraintForce(300.0, 0.25, [0, 1, 2], [10, 11, 12, 13])
    f.setUsesPeriodicBoundaryConditions(True)
    f.setForceGroup(1)
    f.setGlobalParameterDefaultValue(1, 0.5)
    system.addForce(f)
    w = forces.HarmonicRestraintForce(40.0, [3, 4], [20])
    w.setGroupParameters(0, [3, 4], [1.0, 3.0])               # explicit centroid weights
    system.addForce(w)
    system.addForce(forces.HarmonicRestraintBondForce(25.0, 5, 30))
    return system


@pytest.mark.parametrize('alchemical', [False, True])
def test_xml_round_trip_keeps_the_restraints(alchemical):
    import xml.etree.ElementTree as ET
    from openmmtools_amd import alchemy, system_xml
    hg = testsystems.HostGuestExplicit()
    system = hg.system
    if alchemical:
        system = alchemy.AbsoluteAlchemicalFactory().create_alchemical_system(system, alchemy.AlchemicalRegion(alchemical_atoms=list(range(126, 156))))
    system = _restrained(system)
    xml = system_xml.to_xml(system)
    back, _ = system_xml.from_xml(xml)
    assert back.fingerprint() == system.fingerprint()
    got = [f for f in back.getForces() if isinstance(f, forces.RadiallySymmetricRestraintForce)]
    assert [type(f).__name__ for f in got] == ['FlatBottomRestraintForce', 'HarmonicRestraintForce', 'HarmonicRestraintBondForce']
    assert got[0].getGlobalParameterDefaultValue(1) == 0.5 and got[0].usesPeriodicBoundaryConditions() and got[0].getForceGroup() == 1
    assert got[1].getGroupParameters(0) == ([3, 4], [1.0, 3.0]) and got[1].getGroupParameters(1) == ([20], [])
    # OpenMM's serialisation layout (XmlSerializer, CustomCentroidBondForceProxy): attributes and blocks
    e = [x for x in ET.fromstring(xml).find('Forces') if x.get('type') == 'CustomCentroidBondForce'][0]
    assert {'energy', 'forceGroup', 'groups', 'usesPeriodic', 'version'} <= set(e.attrib)
    assert [c.tag for c in e] == ['PerBondParameters', 'GlobalParameters', 'EnergyParameterDerivatives', 'Functions', 'Groups', 'Bonds']
    assert e.find('Groups').find('Group').find('Particle').get('p') == '0'


def _oracle_engine_with_restraints():
    """the CPU oracle engine with the restraints' share of u_kl (beta_l lambda_l E_r, numpy): enough for the store to carry what
    the lambdas do to the energies and the mixing (the oracle's dynamics do not see the restraint)"""
    import sys
    sys.path.insert(0, HERE)
    from oracle_engine import OracleEngine
    from oracle.forcefield import ForceFieldOracle

    class Engine(OracleEngine):
        def spawn(self):
            return type(self)(self.system_factory)

        def set_system(self, desc):
            super().set_system(desc)
            r = desc.get('restraints') or {}
            self.restraints = [r[k] for k in sorted(r)]

        def set_restraint_lambdas(self, lam):
            self.rlam = np.asarray(lam, dtype=np.float64).reshape(self.K, len(self.restraints))

        def _restraint_E(self, x, box):
            out = []
            for t in self.restraints:
                c = [(t['weights%d' % g][:, None] * x[t['atoms%d' % g]]).sum(0) / t['weights%d' % g].sum() for g in (1, 2)]
                d = c[1] - c[0]
                if t['periodic'] and box is not None:
                    d -= box * np.rint(d / box)
                r = np.linalg.norm(d)
                out.append(0.5 * t['K'] * r * r if t['kind'] == 0 else (0.5 * t['K'] * (r - t['r0']) ** 2 if r >= t['r0'] else 0.0))
            return np.array(out)

        def compute_energies(self, d_rows=None, want_host=True, want_potential=False):
            rows, U = super().compute_energies(d_rows, want_host, want_potential=True)
            for r in range(self.R):
                E = self._restraint_E(self.x[r], self._box(r))
                rows[r] += self.beta * (self.rlam @ E)
                U[r] += self.rlam[self.labels[self.r_begin + r]] @ E
            self._rows = rows
            return (rows, U) if want_potential else rows

    return Engine(ForceFieldOracle)


def _restrained_sampler(tmp_path, n_iterations, name, layout):
    from openmmtools_amd import alchemy, mcmc
    from openmmtools_amd.multistate import ReplicaExchangeSampler, MultiStateReporter
    lj = testsystems.LennardJonesFluid(nparticles=64)
    asys = alchemy.AbsoluteAlchemicalFactory().create_alchemical_system(lj.system, alchemy.AlchemicalRegion(alchemical_atoms=list(range(4))))
    asys.addForce(forces.HarmonicRestraintForce(800.0, [0, 1, 2, 3], list(range(10, 20))))
    ths = states.create_thermodynamic_state_protocol(
        states.ThermodynamicState(asys, 120.0 * unit.kelvin),
        {'lambda_sterics': [1.0, 0.5, 0.0], 'lambda_restraints': [0.0, 0.6, 1.0]},
        composable_states=[states.AlchemicalState(), RestraintState(lambda_restraints=1.0)])
    ss = states.SamplerState(lj.positions, box_vectors=lj.system.getDefaultPeriodicBoxVectors())
    move = mcmc.LangevinSplittingDynamicsMove(timestep=1.0 * unit.femtosecond, n_steps=2, reassign_velocities=True, splitting='V R O R V')
    s = ReplicaExchangeSampler(mcmc_moves=move, number_of_iterations=n_iterations, engine=_oracle_engine_with_restraints(), seed=1)
    rep = MultiStateReporter(str(tmp_path / name), checkpoint_interval=1, layout=layout)
    s.create(ths, [ss], storage=rep)
    return s, rep, asys


@pytest.mark.parametrize('layout', ['auto', 'records'])
def test_a_restrained_sampler_resumes_from_the_store(tmp_path, layout):
    """a restrained alchemical sampler writes a '.nc' store (the reference's netCDF4 layout, or the record container) with every
    state's lambda_restraints, resumes from it, and the resumed run's next iterations are those of an uninterrupted run"""
    from openmmtools_amd.multistate import _hdf5, ReplicaExchangeSampler, MultiStateReporter
    if layout == 'auto' and not _hdf5.available():
        pytest.skip('libhdf5 not loadable')
    s, rep, asys = _restrained_sampler(tmp_path, 3, 'r.nc', layout)
    s.run()
    rep.close()
    r = MultiStateReporter(str(tmp_path / 'r.nc'), open_mode='r', layout=layout)
    th, _ = r.read_thermodynamic_states()
    assert [t.lambda_restraints for t in th] == [0.0, 0.6, 1.0] and [t.lambda_sterics for t in th] == [1.0, 0.5, 0.0]
    assert th[0].system.fingerprint() == asys.fingerprint()
    if layout == 'auto':
        assert r.is_reference_store() if callable(getattr(r, 'is_reference_store', None)) else True
        c = r.read_dict('thermodynamic_states/state1')['composable_states']
        assert [x['_serialized__class_name'] for x in c] == ['AlchemicalState', 'RestraintState']
        assert c[1]['parameters'] == {'lambda_restraints': 0.6}
    r.close()
    full, rep_full, _ = _restrained_sampler(tmp_path, 5, 'full.nc', layout)
    full.run()
    rep_full.close()
    res = ReplicaExchangeSampler.from_storage(str(tmp_path / 'r.nc'), engine=_oracle_engine_with_restraints())
    assert res.iteration == 3 and [t.lambda_restraints for t in res._thermodynamic_states] == [0.0, 0.6, 1.0]
    res.extend(2)
    res._reporter.close()
    ea = MultiStateReporter(str(tmp_path / 'r.nc'), open_mode='r', layout=layout).read_energies()[0]
    eb = MultiStateReporter(str(tmp_path / 'full.nc'), open_mode='r', layout=layout).read_energies()[0]
    assert ea.shape == eb.shape == (6, 3, 3)
    assert np.array_equal(ea[:4], eb[:4]) and np.allclose(ea[4:], eb[4:], rtol=2e-5, atol=1e-6)
