"""CPU: virtual sites on the host (openmmtools_amd/system.py, testsystems.py, alchemy.py, _engine.py) and the oracle the GPU tests
use (tests/virtual_sites_oracle.py): the oracle against finite differences and dual numbers, the descriptor's site table, every
refusal by its message, the conversion of OpenMM's site classes from stub objects, and the geometry of the water models."""
import math

import numpy as np
import pytest

import custom_dual_oracle as dual
import virtual_sites_oracle as oracle
from openmmtools_amd import alchemy, system_xml, testsystems, unit, virtual_sites
from openmmtools_amd.system import (System, NonbondedForce, HarmonicBondForce, TwoParticleAverageSite, ThreeParticleAverageSite,
                                    OutOfPlaneSite, system_to_desc, virtual_site_from_openmm)

CASES = [(oracle.TWO, (0.3, 0.7, 0.0)), (oracle.THREE, (0.5, 0.2, 0.3)), (oracle.PLANE, (-0.345, -0.345, 6.44)), (oracle.PLANE, (0.2, -0.4, -1.7))]


def _smooth_energy(rng):
    """A random smooth E of the site position and its gradient: a sum of six plane waves."""
    k, phase, amp = rng.normal(size=(6, 3)) * 2.0, rng.uniform(0, 2 * math.pi, 6), rng.normal(size=6)

    def energy(x):
        return float((amp * np.sin(k @ x + phase)).sum())

    def gradient(x):
        return (amp * np.cos(k @ x + phase)) @ k
    return energy, gradient


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,weights', CASES)
def test_oracle_redistribution_against_central_differences(kind, weights):
    """F_parent = - dE(site(parents)) / d parent: the oracle's chain rule against central differences of E o place, to 1e-7 of
    max|F| (the project's finite-difference bound)."""
    rng = np.random.RandomState(7 + kind)
    n = oracle.N_PARENTS[kind]
    for trial in range(5):
        parents = rng.normal(size=(n, 3)) * 0.1 + rng.normal(size=3)
        energy, gradient = _smooth_energy(rng)
        f_site = -gradient(oracle.place(kind, parents, weights))
        got = oracle.redistribute(kind, parents, weights, f_site)
        h = 1e-5
        ref = np.zeros((n, 3))
        for a in range(n):
            for c in range(3):
                up, dn = parents.copy(), parents.copy()
                up[a, c] += h; dn[a, c] -= h
                ref[a, c] = -(energy(oracle.place(kind, up, weights)) - energy(oracle.place(kind, dn, weights))) / (2 * h)
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print('kind', kind, 'trial', trial, 'relative error', err)
        assert err <= 1e-7
        assert np.allclose(got.sum(axis=0), f_site, rtol=0, atol=1e-12 * np.abs(f_site).max()) or kind != oracle.PLANE


def test_oracle_out_of_plane_against_dual_numbers():
    """The out-of-plane site through dual arithmetic (tests/custom_dual_oracle.py): a cubic polynomial of the site's coordinates,
    its exact gradient with respect to the nine parent coordinates, to 1e-13 of max|F|."""
    rng = np.random.RandomState(11)
    for weights in ((-0.345, -0.345, 6.44), (0.2, -0.4, -1.7), (0.0, 0.0, 3.0)):
        parents = rng.normal(size=(3, 3)) * 0.1 + rng.normal(size=3)
        coeff = rng.normal(size=(3, 3, 3))
        p = dual.seeds(parents)
        r12 = [p[1][c] - p[0][c] for c in range(3)]
        r13 = [p[2][c] - p[0][c] for c in range(3)]
        cr = dual._cross(r12, r13)
        x = [p[0][c] + weights[0] * r12[c] + weights[1] * r13[c] + weights[2] * cr[c] for c in range(3)]
        e = 0.0
        for i in range(3):
            for j in range(3):
                for k in range(3):
                    e = e + coeff[i, j, k] * x[0] ** i * x[1] ** j * x[2] ** k
        site = np.array([q.v for q in x])
        assert np.allclose(site, oracle.place(oracle.PLANE, parents, weights), rtol=0, atol=1e-15)
        grad_site = np.zeros(3)
        for i in range(3):
            for j in range(3):
                for k in range(3):
                    c = coeff[i, j, k]
                    grad_site += c * np.array([i * site[0] ** max(i - 1, 0) * site[1] ** j * site[2] ** k if i else 0.0,
                                               j * site[0] ** i * site[1] ** max(j - 1, 0) * site[2] ** k if j else 0.0,
                                               k * site[0] ** i * site[1] ** j * site[2] ** max(k - 1, 0) if k else 0.0])
        got = oracle.redistribute(oracle.PLANE, parents, weights, -grad_site)
        ref = -e.g.reshape(3, 3)
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print('weights', weights, 'relative error', err)
        assert err <= 1e-13


@pytest.mark.parametrize('kind,weights', CASES)
def test_the_package_places_as_the_oracle(kind, weights):
    rng = np.random.RandomState(3)
    parents = rng.normal(size=(4, oracle.N_PARENTS[kind], 3))
    got = virtual_sites.place(kind, parents, weights)
    for r in range(4):
        assert np.allclose(got[r], oracle.place(kind, parents[r], weights), rtol=0, atol=1e-15)


# ---- the classes and the System ------------------------------------------------------------------------------------------------
def test_site_classes_have_openmm_getters():
    a = TwoParticleAverageSite(4, 2, 0.25, 0.75)
    assert (a.getNumParticles(), a.getParticle(0), a.getParticle(1), a.getWeight(0), a.getWeight(1)) == (2, 4, 2, 0.25, 0.75)
    b = ThreeParticleAverageSite(0, 1, 2, 0.5, 0.25, 0.25)
    assert (b.getNumParticles(), [b.getParticle(k) for k in range(3)], [b.getWeight(k) for k in range(3)]) == (3, [0, 1, 2], [0.5, 0.25, 0.25])
    c = OutOfPlaneSite(0, 1, 2, -0.3, -0.4, 6.0)
    assert (c.getNumParticles(), c.getWeight12(), c.getWeight13(), c.getWeightCross()) == (3, -0.3, -0.4, 6.0)
    with pytest.raises(ValueError, match='not finite'):
        OutOfPlaneSite(0, 1, 2, float('nan'), 0.0, 0.0)


def _water(n_waters=2, periodic=True, site_mass=0.0):
    """n four-site waters (O, H, H, M) with the usual exceptions and constraints"""
    s = System()
    nb = NonbondedForce()
    nb.setNonbondedMethod(NonbondedForce.CutoffPeriodic if periodic else NonbondedForce.NoCutoff)
    nb.setCutoffDistance(0.9)
    s.setDefaultPeriodicBoxVectors([3, 0, 0], [0, 3, 0], [0, 0, 3])
    for w in range(n_waters):
        o = s.addParticle(15.99943); h1 = s.addParticle(1.007947); h2 = s.addParticle(1.007947); m = s.addParticle(site_mass)
        for q in (0.0, 0.52422, 0.52422, -1.04844):
            nb.addParticle(q, 0.316435 if q == 0.0 else 1.0, 0.680946 if q == 0.0 else 0.0)
        s.addConstraint(o, h1, 0.09572); s.addConstraint(o, h2, 0.09572); s.addConstraint(h1, h2, 0.15139)
        for a in range(o, o + 4):
            for b in range(a + 1, o + 4):
                nb.addException(a, b, 0.0, 1.0, 0.0)
        s.setVirtualSite(m, ThreeParticleAverageSite(o, h1, h2, 0.8, 0.1, 0.1))
    s.addForce(nb)
    return s


def test_system_methods():
    s = _water()
    assert s.isVirtualSite(3) and s.isVirtualSite(7) and not s.isVirtualSite(0)
    assert s.getVirtualSite(3) == ThreeParticleAverageSite(0, 1, 2, 0.8, 0.1, 0.1)
    with pytest.raises(ValueError, match='is not a virtual site'):
        s.getVirtualSite(0)
    with pytest.raises(ValueError, match='out of range'):
        s.setVirtualSite(99, TwoParticleAverageSite(0, 1, 0.5, 0.5))


def test_the_descriptor_table():
    d = system_to_desc(_water(3))
    t = d['virtual_sites']
    assert t['site'].tolist() == [3, 7, 11] and t['kind'].tolist() == [1, 1, 1]
    assert t['parent'].tolist() == [[0, 1, 2], [4, 5, 6], [8, 9, 10]]
    assert np.array_equal(t['weight'], np.tile([0.8, 0.1, 0.1], (3, 1)))
    assert t['molecule'].tolist() == [0, 4, 8]                    # each site counted into its parents' molecule
    # the constraint classification: three rigid waters, the sites in none of them
    assert d['settle_atoms'].tolist() == [[0, 1, 2], [4, 5, 6], [8, 9, 10]] and len(d['shake_atoms']) == 0
    assert d['mass'][[3, 7, 11]].tolist() == [0.0, 0.0, 0.0]
    assert 'virtual_sites' not in system_to_desc(testsystems.HarmonicOscillator().system)
    # a two-particle site takes two parents, the third slot is -1; the fingerprint sees the table
    s = _water(1, periodic=False)
    f0 = s.fingerprint()
    s.setVirtualSite(3, TwoParticleAverageSite(0, 1, 0.4, 0.6))
    t = system_to_desc(s)['virtual_sites']
    assert t['parent'].tolist() == [[0, 1, -1]] and t['kind'].tolist() == [0] and s.fingerprint() != f0


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_by_message():
    with pytest.raises(ValueError, match='virtual site 3 has mass 1: a virtual site must have mass 0'):
        system_to_desc(_water(1, site_mass=1.0))
    s = _water(1); s.virtual_sites.clear()
    with pytest.raises(ValueError, match='massless particles are not supported: particle 3'):
        system_to_desc(s)
    s = _water(2); s.setVirtualSite(7, ThreeParticleAverageSite(3, 5, 6, 0.8, 0.1, 0.1))
    with pytest.raises(NotImplementedError, match='parent 3 is itself a virtual site'):
        system_to_desc(s)
    s = _water(1); s.setVirtualSite(3, ThreeParticleAverageSite(0, 1, 9, 0.8, 0.1, 0.1))
    with pytest.raises(ValueError, match='parent index 9 out of range'):
        system_to_desc(s)
    s = _water(1); s.setVirtualSite(3, ThreeParticleAverageSite(0, 1, 1, 0.8, 0.1, 0.1))
    with pytest.raises(ValueError, match='a parent is named twice'):
        system_to_desc(s)
    s = _water(1); s.addConstraint(0, 3, 0.0125)
    with pytest.raises(ValueError, match='virtual site 3 takes part in a constraint'):
        system_to_desc(s)
    s = _water(2); s.setVirtualSite(7, ThreeParticleAverageSite(4, 5, 2, 0.8, 0.1, 0.1))
    with pytest.raises(ValueError, match='lie in different molecules of a periodic System'):
        system_to_desc(s)
    system_to_desc(_water(2, periodic=False))                      # (without a box nothing is wrapped: allowed)

    class LocalCoordinatesSite:
        pass
    with pytest.raises(NotImplementedError, match='LocalCoordinatesSite is not supported'):
        _water(1).setVirtualSite(3, LocalCoordinatesSite())
    with pytest.raises(NotImplementedError, match='virtual site class LocalCoordinatesSite is not supported'):
        virtual_site_from_openmm(LocalCoordinatesSite())
    s = _water(1); s.virtual_sites[3] = object()
    with pytest.raises(NotImplementedError, match='virtual site 3: object is not supported'):
        system_to_desc(s)


def test_stores_pools_and_the_cpu_port_refuse_by_name():
    from openmmtools_amd import _engine, states
    from openmmtools_amd.multistate._reference_store import ReferenceStoreWriter
    from openmmtools_amd.multistate._engine_pool import EnginePool
    s = _water(2)
    with pytest.raises(NotImplementedError, match='virtual sites in a System document'):
        system_xml.to_xml(s)
    ts = states.ThermodynamicState(s, 300.0)
    assert ReferenceStoreWriter.can_store([ts], [], []) == 'a System with virtual sites'
    d = system_to_desc(s)

    class Fake:
        def spawn(self):
            return Fake()
    pool = EnginePool(Fake(), [[0], [1]])
    with pytest.raises(NotImplementedError, match='virtual sites .* in more than one compatibility group'):
        pool.set_system([d, d])

    class NoSites:
        pass
    eng = _engine.HipEngine.__new__(_engine.HipEngine)
    eng.lib = NoSites()
    with pytest.raises(NotImplementedError, match='this build of the engine library has no virtual sites'):
        eng.set_virtual_sites(d['virtual_sites'])
    with pytest.raises(NotImplementedError, match='this build of the engine library has no virtual sites'):
        _engine.HipEngine.set_system(eng, d)
    eng.h = None


def test_from_openmm_site_classes_on_stub_objects():
    class TwoParticleAverageSite_:
        def getNumParticles(self): return 2
        def getParticle(self, k): return (5, 3)[k]
        def getWeight(self, k): return (0.25, 0.75)[k]
    stub = type('TwoParticleAverageSite', (TwoParticleAverageSite_,), {})()
    assert virtual_site_from_openmm(stub) == TwoParticleAverageSite(5, 3, 0.25, 0.75)

    class Three:
        def getNumParticles(self): return 3
        def getParticle(self, k): return (0, 1, 2)[k]
        def getWeight(self, k): return (0.5, 0.3, 0.2)[k]
    assert virtual_site_from_openmm(type('ThreeParticleAverageSite', (Three,), {})()) == ThreeParticleAverageSite(0, 1, 2, 0.5, 0.3, 0.2)

    class Plane:
        def getNumParticles(self): return 3
        def getParticle(self, k): return (0, 1, 2)[k]
        def getWeight12(self): return -0.3
        def getWeight13(self): return -0.4
        def getWeightCross(self): return 6.0
    assert virtual_site_from_openmm(type('OutOfPlaneSite', (Plane,), {})()) == OutOfPlaneSite(0, 1, 2, -0.3, -0.4, 6.0)


def test_from_openmm_converts_the_sites_of_a_stub_system():
    """A whole System through from_openmm: the stand-in OpenMM of the integration tests, given the two site accessors."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'stub_openmm'))
    import openmm
    from openmm import unit as u
    from openmmtools_amd.system import from_openmm
    src = _water(2, periodic=False)

    class WithSites(openmm.System):
        def isVirtualSite(self, index):
            return index in (3, 7)

        def getVirtualSite(self, index):
            o = index - 3
            stub = type('ThreeParticleAverageSite', (), dict(getNumParticles=lambda self: 3, getParticle=lambda self, k: o + k,
                                                             getWeight=lambda self, k: (0.8, 0.1, 0.1)[k]))
            return stub()
    s = WithSites()
    for i in range(src.getNumParticles()):
        s.addParticle(src.getParticleMass(i) * u.dalton)
    out = from_openmm(s)
    assert out.isVirtualSite(3) and out.isVirtualSite(7) and not out.isVirtualSite(4)
    assert out.getVirtualSite(7) == ThreeParticleAverageSite(4, 5, 6, 0.8, 0.1, 0.1)
    assert np.array_equal(system_to_desc(out)['virtual_sites']['parent'], [[0, 1, 2], [4, 5, 6]])


def test_the_alchemical_factory_refuses_a_site_in_a_region_and_passes_others_through():
    box = testsystems.FourSiteWaterBox(box_edge=1.25 * unit.nanometers, cutoff=0.6 * unit.nanometers)
    factory = alchemy.AbsoluteAlchemicalFactory()
    with pytest.raises(ValueError, match='Virtual atoms in region .*Alchemically modified virtual sites are not supported'):
        factory.create_alchemical_system(box.system, alchemy.AlchemicalRegion(alchemical_atoms=[0, 1, 2, 3]))
    out = factory.create_alchemical_system(box.system, alchemy.AlchemicalRegion(alchemical_atoms=[0, 1, 2]))
    assert out.isVirtualSite(3) and out.getVirtualSite(7) == box.system.getVirtualSite(7)


# ---- water geometry ----------------------------------------------------------------------------------------------------------------
def _one_water(model):
    m = testsystems.WATER_MODELS[model]
    half = 0.5 * math.radians(m['HOH'])
    return np.array([[0.0, 0.0, 0.0], [m['r_OH'] * math.cos(half), m['r_OH'] * math.sin(half), 0.0],
                     [m['r_OH'] * math.cos(half), -m['r_OH'] * math.sin(half), 0.0]])


def test_tip4pew_weights_reproduce_the_published_site():
    (cls, w), = testsystems.water_site_weights('tip4pew')
    assert cls == 'ThreeParticleAverageSite' and abs(w[1] - 0.10668) < 5e-6 and w[1] == w[2] and abs(sum(w) - 1.0) < 1e-15
    x = _one_water('tip4pew')
    site = oracle.place(oracle.THREE, x, w)
    assert abs(np.linalg.norm(site - x[0]) - 0.0125) <= 1e-9
    bis = (x[1] + x[2]) / np.linalg.norm(x[1] + x[2])
    assert abs(site @ bis - 0.0125) <= 1e-9                        # on the bisector, towards the hydrogens


def test_tip5p_weights_reproduce_the_lone_pair_geometry():
    (c1, w1), (c2, w2) = testsystems.water_site_weights('tip5p')
    assert c1 == c2 == 'OutOfPlaneSite'
    x = _one_water('tip5p')
    l1, l2 = oracle.place(oracle.PLANE, x, w1), oracle.place(oracle.PLANE, x, w2)
    assert abs(np.linalg.norm(l1) - 0.07) <= 1e-9 and abs(np.linalg.norm(l2) - 0.07) <= 1e-9
    ang = math.degrees(math.acos(l1 @ l2 / (np.linalg.norm(l1) * np.linalg.norm(l2))))
    assert abs(ang - 109.47) <= 1e-7
    assert (l1 + l2) @ (x[1] + x[2]) < 0 and abs(l1[2] + l2[2]) < 1e-15 and abs(l1[2]) > 0.05      # away from the hydrogens, off the plane


@pytest.mark.parametrize('cls,model,per', [(testsystems.FourSiteWaterBox, 'tip4pew', 4), (testsystems.FiveSiteWaterBox, 'tip5p', 5)])
def test_water_boxes(cls, model, per):
    box = cls(box_edge=1.25 * unit.nanometers, cutoff=0.6 * unit.nanometers)
    s, n = box.system, box.n_waters
    assert n == 65 and s.getNumParticles() == per * n and box.positions.shape == (per * n, 3)
    assert box.ndof == 6 * n                                       # the sites are no degrees of freedom
    assert sum(s.isVirtualSite(i) for i in range(per * n)) == (per - 3) * n
    nb = s.getForce(0)
    assert abs(sum(p[0] for p in nb.particles)) < 1e-12 and nb.getNonbondedMethod() == NonbondedForce.PME
    d = system_to_desc(s)
    assert len(d['settle_atoms']) == n and len(d['virtual_sites']['site']) == (per - 3) * n
    x = box.positions.reshape(n, per, 3)
    m = testsystems.WATER_MODELS[model]
    assert np.allclose(np.linalg.norm(x[:, 1] - x[:, 0], axis=1), m['r_OH'], rtol=0, atol=1e-12)
    assert np.array_equal(box.positions, oracle.place_table(d['virtual_sites'], box.positions)) or \
        np.allclose(box.positions, oracle.place_table(d['virtual_sites'], box.positions), rtol=0, atol=1e-15)
    same = testsystems.WaterBox(box_edge=1.25 * unit.nanometers, cutoff=0.6 * unit.nanometers, model=model)
    assert np.array_equal(same.positions, box.positions)
    # no two atoms of different molecules closer than 0.1 nm on the lattice
    real = x[:, :3].reshape(-1, 3)
    delta = real[:, None] - real[None]
    delta -= 1.25 * np.round(delta / 1.25)
    dist = np.sqrt((delta ** 2).sum(axis=2)) + 10.0 * np.kron(np.eye(n), np.ones((3, 3)))
    assert dist.min() > 0.1


def test_water_box_defaults_and_refusals():
    with pytest.raises(Exception, match="Specified water model 'tip9p' is not in list of supported models"):
        testsystems.WaterBox(model='tip9p')
    with pytest.raises(NotImplementedError, match='flexible water'):
        testsystems.WaterBox(constrained=False)
    three = testsystems.WaterBox(box_edge=1.25 * unit.nanometers, cutoff=0.6 * unit.nanometers)
    assert three.model == 'tip3p' and three.system.getNumParticles() == 3 * 65 and not three.system.virtual_sites
    nb = three.system.getForce(0)
    assert nb.getUseSwitchingFunction() and abs(nb.getSwitchingDistance() - 0.45) < 1e-12 and nb.getUseDispersionCorrection()
