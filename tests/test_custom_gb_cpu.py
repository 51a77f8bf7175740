"""CustomGBForce of the OBC family without a GPU: the f64 oracle against the reference's own strings, the recognizer (openmmtools_amd/
custom_gb.py) and what it refuses, the alchemical factory's rewrite, System documents and stores, testsystems.CustomGBForceSystem, and
the CPU port's refusal of a cutoff model (include/remd_hip_gb.h is GPU-only)."""
import json
import os

import numpy as np
import pytest
import torch

import oracle
from custom_gb_oracle import custom_gb_energy_torch
from openmmtools_amd import alchemy, states, system_xml, testsystems as ts
from openmmtools_amd.system import system_to_desc, CustomGBForce, System, NonbondedForce
from openmmtools_amd.custom_gb import recognize_custom_gb, alchemically_modify_custom_gb, unmodify_custom_gb, OBC2_MODEL
from openmmtools_amd import _alchemical_xml as ax

HERE = os.path.dirname(os.path.abspath(__file__))
G = json.load(open(os.path.join(HERE, 'golden', 'reference_custom_gb.json')))
CPU_LIB = os.path.join(os.path.dirname(os.path.abspath(oracle.__file__)), '_build', 'libremd_cpu.so')
OBC1 = dict(alpha=0.8, beta=0.0, gamma=2.909125)


def test_oracle_reproduces_the_reference_strings_with_periodic_cutoffs():
    assert len(G['cases']) == 9 and {c['model'] for c in G['cases']} == {'OBC2', 'OBC1'}
    assert any(c['cutoff'] is None for c in G['cases'])
    for c in G['cases']:
        e, I, B = custom_gb_energy_torch(torch.tensor(c['x'], dtype=torch.float64), c['charge'], c['radius'], c['scale'], c['alchemical'],
                                         c['lambda_electrostatics'], OBC1 if c['model'] == 'OBC1' else None, c['box'], c['cutoff'],
                                         G['globals']['testsystems_CustomGBForceSystem_soluteDielectric'],
                                         G['globals']['testsystems_CustomGBForceSystem_solventDielectric'], True, return_parts=True)
        assert np.isclose(float(e), c['energy'], rtol=1e-12, atol=0.0), (float(e), c['energy'])
        assert np.allclose(I.numpy(), c['I'], rtol=1e-12, atol=1e-14) and np.allclose(B.numpy(), c['B'], rtol=1e-12, atol=0.0)


def test_the_cases_cross_the_boundary_and_straddle_the_cutoff():
    for c in G['cases']:
        if c['cutoff'] is None:
            continue
        x, L = np.array(c['x']), np.array(c['box'])
        d = x[:, None] - x[None]
        raw = np.linalg.norm(d, axis=-1)
        img = np.linalg.norm(d - L * np.round(d / L), axis=-1)
        assert np.any(img < 0.5 * raw)                                   # a pair closer through the boundary
        iu = np.triu_indices(len(x), 1)
        near = np.abs(img[iu] - c['cutoff'])
        assert (near < 0.05).sum() >= 2 and np.any(img[iu] < c['cutoff']) and np.any(img[iu] > c['cutoff'])


def test_custom_gb_force_system_mirrors_the_reference():
    s = ts.CustomGBForceSystem()
    nb, gb = s.system.getForce(0), s.system.getForce(1)
    c = G['constants']
    assert c['numMolecules'] == '70' and c['boxSize'] == '10.0 * unit.nanometers' and c['mass'] == '39.9 * unit.amu'
    assert c['sigma'] == '3.35 * unit.angstrom' and c['epsilon'] == '0.001603 * unit.kilojoule_per_mole' and c['cutoff'] == '2.0 * unit.nanometers'
    assert s.system.getNumParticles() == 140 and all(m == 39.9 for m in s.system.masses)
    assert np.allclose(s.system.getDefaultPeriodicBoxVectors(), 10.0 * np.eye(3))
    assert nb.getNonbondedMethod() == NonbondedForce.CutoffPeriodic and nb.getCutoffDistance() == 2.0
    assert gb.getNonbondedMethod() == CustomGBForce.CutoffPeriodic and gb.getCutoffDistance() == 2.0
    assert [[n, e, ['SingleParticle', 'ParticlePair', 'ParticlePairNoExclusions'][k]] for n, e, k in gb.computed] == G['computed_values']
    assert [[e, ['SingleParticle', 'ParticlePair', 'ParticlePairNoExclusions'][k]] for e, k in gb.energy_terms] == G['energy_terms']
    assert dict(gb.globals) == G['globals'] and gb.per_particle == G['per_particle']
    p = np.array(gb.particles)
    assert np.array_equal(p[:, 0], np.tile([1.0, -1.0], 70)) and np.array_equal(p[:, 1], np.tile([0.2, 0.1], 70))
    assert np.array_equal(p[:, 2], np.r_[np.full(70, 0.5), np.full(70, 0.8)])
    assert all(q == (p[i, 0], 0.335, 0.001603) for i, q in enumerate(nb.particles))
    assert s.positions.shape == (140, 3) and np.all((s.positions >= 0) & (s.positions < 10.0))
    d = system_to_desc(s.system)
    assert {k: d['gbsa'][k] for k in OBC2_MODEL} == dict(OBC2_MODEL, method=2, cutoff=2.0)
    assert (d['gbsa']['solute_dielectric'], d['gbsa']['solvent_dielectric'], d['gbsa']['surface_area']) == (1.0, 80.0, 1)


def _force(**changes):
    f = ts.CustomGBForceSystem().system.getForce(1)
    for k, v in changes.items():
        setattr(f, k, v)
    return f


def test_recognizer_accepts_shapes_a_and_b_plain_and_alchemical():
    a = _force()
    m = recognize_custom_gb(a)
    assert m['shape'] == 'A' and not m['alchemical'] and m['method'] == 2 and m['cutoff'] == 2.0
    alch = alchemically_modify_custom_gb(a, [0, 1, 2])
    m2 = recognize_custom_gb(alch)
    assert m2['shape'] == 'A' and m2['alchemical'] and {k: m2[k] for k in OBC2_MODEL} == {k: m[k] for k in OBC2_MODEL}
    back, atoms = unmodify_custom_gb(alch)
    assert atoms == [0, 1, 2] and recognize_custom_gb(back) == m
    # OBC1's constants in shape A
    obc1 = _force(computed=[a.computed[0], ('B', a.computed[1][1].replace('1*psi-0.8*psi^2+4.85*psi^3', '0.8*psi-0*psi^2+2.909125*psi^3'), 0)])
    assert {k: recognize_custom_gb(obc1)[k] for k in ('alpha', 'beta', 'gamma')} == OBC1
    # shape B: the factory's GBSA strings, with the lambda factors and without them
    b = CustomGBForce()
    for p in ('charge', 'radius', 'scale', 'alchemical'):
        b.addPerParticleParameter(p)
    for n, v in (('lambda_electrostatics', 1.0), ('solventDielectric', 78.5), ('soluteDielectric', 1.0), ('offset', 0.009)):
        b.addGlobalParameter(n, v)
    b.addComputedValue('I', ax._GB_I, 2); b.addComputedValue('B', ax._GB_B, 0)
    for t in (ax._GB_SELF, ax._GB_SURFACE):
        b.addEnergyTerm(t, 0)
    b.addEnergyTerm(ax._GB_PAIR, 2)
    mb = recognize_custom_gb(b)
    assert mb['shape'] == 'B' and mb['alchemical'] and mb['method'] == 0 and mb['solvent_dielectric'] == 78.5
    assert {k: mb[k] for k in OBC2_MODEL} == OBC2_MODEL
    plain = CustomGBForce()
    for p in ('charge', 'radius', 'scale'):
        plain.addPerParticleParameter(p)
    for n, v in (('solventDielectric', 78.5), ('soluteDielectric', 1.0), ('offset', 0.009)):
        plain.addGlobalParameter(n, v)
    strip = lambda s: s.replace('(lambda_electrostatics*alchemical2 + (1-alchemical2))*', '').replace('(lambda_electrostatics*alchemical+(1-alchemical))*', '') \
        .replace('(lambda_electrostatics*alchemical1+(1-alchemical1))*', '').replace('(lambda_electrostatics*alchemical2+(1-alchemical2))*', '')
    plain.addComputedValue('I', strip(ax._GB_I), 2); plain.addComputedValue('B', ax._GB_B, 0)
    plain.addEnergyTerm(strip(ax._GB_SELF), 0); plain.addEnergyTerm(strip(ax._GB_PAIR), 2)
    mp = recognize_custom_gb(plain)
    assert mp['shape'] == 'B' and not mp['alchemical'] and mp['surface_area'] == 0
    mpa = recognize_custom_gb(alchemically_modify_custom_gb(plain, [1]))
    assert mpa['shape'] == 'B' and mpa['alchemical']


def test_recognizer_refuses_by_name():
    a = _force()
    cases = [
        (_force(computed=[('I', a.computed[0][1].replace('0.5*log', '0.4*log'), 2), a.computed[1]]), "computed value 'I'"),
        (_force(computed=[a.computed[0], ('B', a.computed[1][1].replace('radius-0.009', 'radius-0.008'), 0)]), 'offset'),
        (_force(energy_terms=[a.energy_terms[0], (a.energy_terms[1][0].replace('-138.935485', '-138.9'), 2)]), 'energy term 1'),
        (_force(computed=[(a.computed[0][0], a.computed[0][1], 1), a.computed[1]]), 'ParticlePair'),
        (_force(energy_terms=[a.energy_terms[0], (a.energy_terms[1][0], 1)]), 'ParticlePair'),
        (_force(functions=[('tab', object())]), 'tabulated'),
        (_force(globals=a.globals + [['extra', 1.0]]), "global parameter 'extra'"),
        (_force(_method=1), 'CutoffNonPeriodic'),
    ]
    for f, what in cases:
        with pytest.raises(NotImplementedError, match='CustomGBForce') as e:
            recognize_custom_gb(f)
        assert what in str(e.value), (what, str(e.value))
    s = ts.CustomGBForceSystem()
    s.system.getForce(1).setCutoffDistance(5.5)
    with pytest.raises(NotImplementedError, match='CustomGBForce.*half the shortest box edge'):
        system_to_desc(s.system)
    s = ts.CustomGBForceSystem()
    s.system.getForce(0).setNonbondedMethod(NonbondedForce.NoCutoff)
    with pytest.raises(NotImplementedError, match='CustomGBForce.*not periodic'):
        system_to_desc(s.system)


def test_a_global_parameter_state_may_not_set_a_gb_global():
    class DielectricState(states.GlobalParameterState):
        testsystems_CustomGBForceSystem_solventDielectric = states.GlobalParameterState.GlobalParameter(
            'testsystems_CustomGBForceSystem_solventDielectric', standard_value=80.0)
    s = ts.CustomGBForceSystem()
    with pytest.raises(states.GlobalParameterError, match='CustomGBForce'):
        DielectricState(testsystems_CustomGBForceSystem_solventDielectric=40.0).apply_to_system(s.system)


def test_factory_writes_the_reference_strings_verbatim():
    s = ts.CustomGBForceSystem()
    asys = alchemy.AbsoluteAlchemicalFactory().create_alchemical_system(s.system, alchemy.AlchemicalRegion(alchemical_atoms=range(4)))
    gb = [f for f in asys.getForces() if isinstance(f, CustomGBForce)]
    assert len(gb) == 1
    gb = gb[0]
    want_values = [[n, e, k] for n, e, k in G['alchemical_computed_values']]
    assert [[n, e, ['SingleParticle', 'ParticlePair', 'ParticlePairNoExclusions'][k]] for n, e, k in gb.computed] == want_values
    assert [[e, ['SingleParticle', 'ParticlePair', 'ParticlePairNoExclusions'][k]] for e, k in gb.energy_terms] == G['alchemical_energy_terms']
    assert gb.per_particle == ['charge', 'radius', 'scale', 'alchemical'] and gb.globals[-1] == ['lambda_electrostatics', 1.0]
    assert [p[3] for p in gb.particles][:6] == [1.0] * 4 + [0.0] * 2
    two = [alchemy.AlchemicalRegion(alchemical_atoms=range(2), name='a'), alchemy.AlchemicalRegion(alchemical_atoms=range(2, 4), name='b')]
    with pytest.raises(NotImplementedError, match='Multiple regions does not work with CustomGBForce'):
        alchemy.AbsoluteAlchemicalFactory().create_alchemical_system(s.system, two)
    # written: in the lambda_electrostatics force group
    import xml.etree.ElementTree as ET
    forces = ET.fromstring(system_xml.to_xml(asys)).find('Forces').findall('Force')
    cgb = [f for f in forces if f.get('type') == 'CustomGBForce']
    elec = [f.get('forceGroup') for f in forces if 'U_electrostatics' in f.get('energy', '')]
    assert len(cgb) == 1 and elec and cgb[0].get('forceGroup') == elec[0]


def test_system_documents_round_trip():
    s = ts.CustomGBForceSystem()
    xml = system_xml.to_xml(s.system)
    back, _ = system_xml.from_xml(xml)
    assert back.fingerprint() == s.system.fingerprint()
    assert system_to_desc(back)['gbsa']['cutoff'] == 2.0
    asys = alchemy.AbsoluteAlchemicalFactory().create_alchemical_system(s.system, alchemy.AlchemicalRegion(alchemical_atoms=range(4)))
    back, _ = system_xml.from_xml(system_xml.to_xml(asys))
    assert back.fingerprint() == asys.fingerprint()
    assert np.array_equal(system_to_desc(back)['gbsa']['alchemical'], system_to_desc(asys)['gbsa']['alchemical'])
    with pytest.raises(NotImplementedError, match='CustomGBForce'):
        system_xml.from_xml(xml.replace('0.5*log(L/U)', '0.25*log(L/U)'))


def test_cpu_port_refuses_a_cutoff_model():
    if not os.path.exists(CPU_LIB):
        oracle.build()
    from openmmtools_amd._engine import HipEngine
    eng = HipEngine(lib_path=CPU_LIB)
    try:
        with pytest.raises(NotImplementedError, match='remd_hip_gb.h'):
            eng.set_system(system_to_desc(ts.CustomGBForceSystem().system))
    finally:
        eng.close()
