"""GPU: virtual sites (include/remd_hip_vsites.h, csrc/virtual_sites.hip) against tests/virtual_sites_oracle.py.

Every comparison of forces and energies is against the TWIN System: the same particles, the sites given mass 1 and not declared,
at the positions the device holds (sites already placed).  The twin runs none of the new code, so its forces on the sites are what
the spread kernel has to hand to the parents; the oracle does that in f64.

Bounds.  Placement: the site is computed in f64 from f32 parents and rounded once, so each component lies within 2^-24 of the
largest coordinate magnitude involved.  Spread: a parent's component is the twin's plus one share per site it serves; each share is
rounded to f32 (2^-24 relative) and truncated to the 2^-32 fixed point, so n (2^-23 max|contribution| + 2^-31) with n = sites + 1.

The periodic box: 65 TIP4P-Ew waters in 1.25 nm, the smallest WaterBox edge above twice the 0.6 nm cutoff at which the lattice
holds liquid density (1.2 nm itself is the refused limit; the Ewald split stays the reference's so that the barostat may shrink it)."""
import math

import numpy as np
import pytest

import virtual_sites_oracle as oracle
from openmmtools_amd import testsystems, unit
from openmmtools_amd.system import (System, NonbondedForce, HarmonicBondForce, TwoParticleAverageSite, ThreeParticleAverageSite,
                                    OutOfPlaneSite, system_to_desc)

pytestmark = pytest.mark.gpu
KB = 0.008314462618153242
EDGE, CUTOFF = 1.25, 0.6


# ---- systems -----------------------------------------------------------------------------------------------------------------------
def _rotation(rng):
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    a, b, c, d = q
    return np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                     [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                     [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])


def _cluster(n_tip4p, sites=True):
    """NoCutoff: n TIP4P-Ew waters, one TIP5P water, one diatomic with a two-particle site off its midpoint -> (System, positions
    with garbage on the sites).  sites=False: the twin (sites with mass 1, none declared)."""
    rng = np.random.RandomState(1234)
    s, nb, bonds = System(), NonbondedForce(), HarmonicBondForce()
    nb.setNonbondedMethod(NonbondedForce.NoCutoff)
    x = []

    def molecule(masses, charges, lj, local, site_defs, centre):
        first = s.getNumParticles()
        rot = _rotation(rng)
        for k, (m, q) in enumerate(zip(masses, charges)):
            s.addParticle(m if (m > 0 or sites) else 1.0)
            nb.addParticle(q, lj[k][0], lj[k][1])
            x.append(centre + rot @ local[k] if m > 0 else rng.normal(size=3) * 50.0)       # garbage where a site goes
        for a in range(first, first + len(masses)):
            for b in range(a + 1, first + len(masses)):
                nb.addException(a, b, 0.0, 1.0, 0.0)
        if sites:
            for (k, site) in site_defs(first):
                s.setVirtualSite(first + k, site)
        return first

    def water(model, centre):
        m = testsystems.WATER_MODELS[model]
        half = 0.5 * math.radians(m['HOH'])
        w = testsystems.water_site_weights(model)
        local = [np.zeros(3), np.array([m['r_OH'] * math.cos(half), m['r_OH'] * math.sin(half), 0.0]),
                 np.array([m['r_OH'] * math.cos(half), -m['r_OH'] * math.sin(half), 0.0])] + [np.zeros(3)] * len(w)
        qs = -2.0 * m['q_H'] / len(w)
        first = molecule([15.99943, 1.007947, 1.007947] + [0.0] * len(w), [0.0, m['q_H'], m['q_H']] + [qs] * len(w),
                         [(m['sigma_O'], m['eps_O'])] + [(1.0, 0.0)] * (2 + len(w)), local,
                         lambda f: [(3 + k, ThreeParticleAverageSite(f, f + 1, f + 2, *wk) if cls == 'ThreeParticleAverageSite'
                                     else OutOfPlaneSite(f, f + 1, f + 2, *wk)) for k, (cls, wk) in enumerate(w)], centre)
        s.addConstraint(first, first + 1, m['r_OH']); s.addConstraint(first, first + 2, m['r_OH'])
        s.addConstraint(first + 1, first + 2, 2.0 * m['r_OH'] * math.sin(half))

    grid = [np.array([i, j, k]) * 0.36 for i in range(3) for j in range(3) for k in range(2)]
    for w in range(n_tip4p):
        water('tip4pew', grid[w])
    water('tip5p', grid[n_tip4p])
    first = molecule([12.011, 14.0067, 0.0], [0.3, -0.1, -0.2], [(0.34, 0.36), (0.325, 0.71), (1.0, 0.0)],
                     [np.array([-0.06, 0, 0]), np.array([0.06, 0, 0]), np.zeros(3)],
                     lambda f: [(2, TwoParticleAverageSite(f, f + 1, 0.3, 0.7))], grid[n_tip4p + 1])
    bonds.addBond(first, first + 1, 0.118, 2.0e5)
    s.addForce(nb); s.addForce(bonds)
    return s, np.array(x)


def _twin_of(system):
    """the same particles, the sites given mass 1 and none declared"""
    import copy
    t = copy.deepcopy(system)
    for i in t.virtual_sites:
        t.masses[i] = 1.0
    t.virtual_sites = {}
    return t


def _engine(factory, desc, x, box, T=(300.0,), labels=None, **kw):
    eng = factory()
    eng.set_system(desc)
    eng.set_states(1.0 / (KB * np.asarray(T, dtype=np.float64)))
    R = len(x)
    eng.set_replicas(R, 0, x, None, box, np.zeros(R, dtype=np.int64) if labels is None else labels)
    return eng


def _assert_placed(table, x, what):
    """every site within one f32 rounding of the oracle's f64 value from the parents the device holds"""
    ref = oracle.place_table(table, x)
    worst = 0.0
    for s, kind, par in zip(table['site'], table['kind'], table['parent']):
        idx = [s] + list(par[:oracle.N_PARENTS[int(kind)]])
        for r in range(len(x)):
            bound = 2.0 ** -24 * max(np.abs(x[r, idx]).max(), np.abs(ref[r, s]).max())
            err = np.abs(x[r, s] - ref[r, s]).max()
            worst = max(worst, err / bound)
            assert err <= bound, (what, r, int(s), err, bound)
    print(what, 'placement: worst error / bound', worst)


def _assert_spread(table, x, f_sites, f_twin, what):
    worst = 0.0
    for r in range(len(x)):
        ref, big, count = oracle.redistribute_table(table, x[r], f_twin[r])
        bound = (count + 1)[:, None] * (2.0 ** -23 * big + 2.0 ** -31)
        err = np.abs(f_sites[r] - ref)
        worst = max(worst, (err / bound).max())
        assert np.all(err <= bound), (what, r, np.argwhere(err > bound)[:4].tolist(), err.max())
        assert np.all(f_sites[r][table['site']] == 0.0), (what, 'forces on the sites must be exactly 0')
    print(what, 'spread: worst error / bound', worst)


# ---- placement, forces and energy of the NoCutoff cluster ------------------------------------------------------------------------------
# (sites x replicas = lanes of one launch.  The first cluster -- 6 TIP4P-Ew waters, one TIP5P water, the diatomic -- holds 9 sites:
# 8 replicas make 72 lanes, one wavefront and a partial one; 10 TIP4P-Ew waters hold 13 sites: 5 replicas make the 65 lanes, one
# wavefront plus one lane.)
@pytest.fixture(scope='module', params=[(6, 8), (10, 5)], ids=['6-waters-72-lanes', '10-waters-65-lanes'])
def cluster(request, hip_engine_factory):
    n_tip4p, R = request.param
    s, x0 = _cluster(n_tip4p)
    desc = system_to_desc(s)
    assert len(desc['virtual_sites']['site']) * R == (72 if n_tip4p == 6 else 65)
    rng = np.random.RandomState(5)
    x = np.stack([x0 + (r > 0) * np.array([0.3 * r, -0.2 * r, 0.1 * r]) for r in range(R)])
    real = np.array([not s.isVirtualSite(i) for i in range(len(x0))])
    x[:, real] += 0.002 * rng.normal(size=x[:, real].shape)
    box = np.array([[3.0, 3.0, 3.0] if r % 2 == 0 else [4.0, 3.5, 5.0] for r in range(R)])      # (one replica with a box, the next with another)
    eng = _engine(hip_engine_factory, desc, x, box)
    xd, vd = eng.get_replicas()[:2]
    twin = _engine(hip_engine_factory, system_to_desc(_twin_of(s)), xd, box)
    return s, desc, x, eng, twin, xd, vd


def test_garbage_on_the_sites_is_replaced_by_their_places(cluster):
    s, desc, x, eng, twin, xd, vd = cluster
    real = np.array([not s.isVirtualSite(i) for i in range(x.shape[1])])
    assert np.array_equal(xd[:, real], x[:, real].astype(np.float32).astype(np.float64))
    assert np.abs(x[:, ~real]).max() > 10.0 and np.abs(xd[:, ~real]).max() < 10.0
    _assert_placed(desc['virtual_sites'], xd, 'cluster')
    assert np.all(vd[:, ~real] == 0.0)


def test_cluster_energy_is_the_twins_and_forces_are_the_twins_redistributed(cluster):
    s, desc, x, eng, twin, xd, vd = cluster
    _, U = eng.compute_energies(want_potential=True)
    _, Ut = twin.compute_energies(want_potential=True)
    assert np.array_equal(U, Ut), (U, Ut)
    f, ft = eng.get_forces(), twin.get_forces()
    assert np.abs(ft[:, desc['virtual_sites']['site']]).max() > 1.0          # (the twin's sites do feel forces)
    _assert_spread(desc['virtual_sites'], xd, f, ft, 'cluster, all forces')
    for groups in (1, 0xffffffff):                                          # every class sits in force group 0
        _assert_spread(desc['virtual_sites'], xd, eng.get_forces(groups=groups), twin.get_forces(groups=groups), 'cluster, groups=%x' % groups)
    assert np.all(eng.get_forces(groups=2) == 0.0)


# ---- the periodic four-site box ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def pme_box(hip_engine_factory):
    """65 TIP4P-Ew waters in 1.25 nm under PME, relaxed once by 60 FIRE iterations (the lattice start is far from equilibrium)."""
    box = testsystems.FourSiteWaterBox(box_edge=EDGE * unit.nanometers, cutoff=CUTOFF * unit.nanometers)
    desc = system_to_desc(box.system, ewald_split='reference')
    R = 3
    edges = np.tile([EDGE] * 3, (R, 1))
    eng = _engine(hip_engine_factory, desc, np.tile(box.positions, (R, 1, 1)), edges, T=(300.0, 320.0, 340.0), labels=np.arange(R))
    eng.minimize(tolerance=1.0, max_iterations=60)
    x = eng.get_replicas()[0]
    return box, desc, x, edges


def test_pme_energy_forces_and_ukl_rows(pme_box, hip_engine_factory):
    from oracle.forcefield import ForceFieldOracle
    box, desc, x, edges = pme_box
    T = np.array([300.0, 320.0, 340.0])
    eng = _engine(hip_engine_factory, desc, x, edges, T=T, labels=np.arange(3))
    twin_desc = system_to_desc(_twin_of(box.system), ewald_split='reference')
    twin = _engine(hip_engine_factory, twin_desc, x, edges, T=T, labels=np.arange(3))
    xd = eng.get_replicas()[0]
    assert np.array_equal(xd, x)                                   # (already placed: placing again changes nothing)
    rows, U = eng.compute_energies(want_potential=True)
    rows_t, Ut = twin.compute_energies(want_potential=True)
    assert np.array_equal(U, Ut) and np.array_equal(rows, rows_t), (U, Ut)
    _assert_spread(desc['virtual_sites'], xd, eng.get_forces(), twin.get_forces(), 'PME box')
    _assert_spread(desc['virtual_sites'], xd, eng.get_forces(groups=1), twin.get_forces(groups=1), 'PME box, groups=1')
    ff = ForceFieldOracle(twin_desc)
    ref = np.array([ff.potential(xd[r], edges[r]) for r in range(3)])
    print('u_kl: device', rows.tolist(), 'oracle U', ref.tolist())
    assert np.allclose(rows, ref[:, None] / (KB * T)[None, :], rtol=1e-5, atol=0)


def _constraints_hold(box, x):
    n = box.n_waters
    w = x.reshape(len(x), n, 4, 3)
    m = testsystems.WATER_MODELS['tip4pew']
    d_hh = 2.0 * m['r_OH'] * math.sin(0.5 * math.radians(m['HOH']))
    err = max(np.abs(np.linalg.norm(w[:, :, 1] - w[:, :, 0], axis=-1) - m['r_OH']).max(),
              np.abs(np.linalg.norm(w[:, :, 2] - w[:, :, 0], axis=-1) - m['r_OH']).max(),
              np.abs(np.linalg.norm(w[:, :, 2] - w[:, :, 1], axis=-1) - d_hh).max())
    print('largest constraint error', err)
    assert err < 3e-6


def _propagated(factory, pme_box, phases):
    box, desc, x, edges = pme_box
    R = 4
    eng = factory()
    eng.set_phases(phases)
    eng.set_system(desc)
    eng.set_states(1.0 / (KB * np.linspace(300.0, 330.0, R)))
    eng.set_integrator('V R O R V', 0.001, 1.0, 50, True, 1e-8)
    eng.seed(17)
    eng.set_replicas(R, 0, np.tile(x[0], (R, 1, 1)), None, np.tile(edges[0], (R, 1)), np.arange(R))
    eng.compute_energies()
    assert not eng.propagate(0).any()
    xs, vs = eng.get_replicas()[:2]
    return xs, vs, eng.compute_energies(), eng.phases_active()


@pytest.fixture(scope='module')
def one_block(hip_engine_factory, pme_box):
    return _propagated(hip_engine_factory, pme_box, 1)


def test_after_50_langevin_steps_every_site_sits_at_its_place(pme_box, one_block):
    box, desc, x0, edges = pme_box
    x, v, u, phases = one_block
    assert phases == 1 and np.abs(x - x0[0]).max() > 1e-3
    _assert_placed(desc['virtual_sites'], x, 'after propagation')
    sites = desc['virtual_sites']['site']
    assert np.all(v[:, sites] == 0.0) and np.abs(v).max() > 0.1
    _constraints_hold(box, x)


def test_two_phases_are_the_one_block_propagation(hip_engine_factory, pme_box, one_block):
    x, v, u, phases = _propagated(hip_engine_factory, pme_box, 2)
    assert phases == 2
    assert np.array_equal(x, one_block[0]) and np.array_equal(v, one_block[1]) and np.array_equal(u, one_block[2])
    _assert_placed(pme_box[1]['virtual_sites'], x, 'two phases')


def test_after_an_accepted_barostat_move(hip_engine_factory, pme_box):
    box, desc, x, edges = pme_box
    eng = _engine(hip_engine_factory, desc, x, edges, T=(300.0, 320.0, 340.0), labels=np.arange(3))
    eng.set_barostat(np.full(3, 0.0602214076 * 1.01325), frequency=25)
    eng.seed(3)
    eng.barostat_attempts(12)
    _, attempted, accepted = eng.barostat_stats()
    boxes = eng.get_boxes()
    print('barostat: attempted', attempted.tolist(), 'accepted', accepted.tolist(), 'boxes', boxes.tolist())
    assert accepted.sum() > 0 and np.any(boxes != edges)
    xb = eng.get_replicas()[0]
    _assert_placed(desc['virtual_sites'], xb, 'after barostat moves')
    _constraints_hold(box, xb)


def test_after_20_fire_iterations(hip_engine_factory):
    box = testsystems.FourSiteWaterBox(box_edge=EDGE * unit.nanometers, cutoff=CUTOFF * unit.nanometers)
    desc = system_to_desc(box.system, ewald_split='reference')
    edges = np.tile([EDGE] * 3, (2, 1))
    eng = _engine(hip_engine_factory, desc, np.tile(box.positions, (2, 1, 1)), edges, T=(300.0, 300.0))
    _, U0 = eng.compute_energies(want_potential=True)
    eng.minimize(tolerance=1.0, max_iterations=20)
    x, v = eng.get_replicas()[:2]
    _, U1 = eng.compute_energies(want_potential=True)
    print('FIRE: U before', U0.tolist(), 'after', U1.tolist())
    assert np.all(U1 <= U0) and np.any(U1 < U0)
    _assert_placed(desc['virtual_sites'], x, 'after FIRE')
    assert np.all(v[:, desc['virtual_sites']['site']] == 0.0)
    _constraints_hold(box, x)


# ---- energy conservation ---------------------------------------------------------------------------------------------------------------
def _three_site_twin(box):
    """the same waters with the site's charge on the oxygen and no site: none of the virtual-site code runs"""
    s, nb = System(), NonbondedForce()
    src = box.system.getForce(0)
    nb.setNonbondedMethod(src.getNonbondedMethod()); nb.setCutoffDistance(src.getCutoffDistance())
    nb.setUseSwitchingFunction(src.getUseSwitchingFunction()); nb.setSwitchingDistance(src.getSwitchingDistance())
    nb.setUseDispersionCorrection(src.getUseDispersionCorrection()); nb.setEwaldErrorTolerance(src.getEwaldErrorTolerance())
    s.setDefaultPeriodicBoxVectors(*box.system.getDefaultPeriodicBoxVectors())
    m = testsystems.WATER_MODELS['tip4pew']
    for w in range(box.n_waters):
        o = s.addParticle(testsystems.WATER_MASS_O); h1 = s.addParticle(testsystems.WATER_MASS_H); h2 = s.addParticle(testsystems.WATER_MASS_H)
        nb.addParticle(-2.0 * m['q_H'], m['sigma_O'], m['eps_O']); nb.addParticle(m['q_H'], 1.0, 0.0); nb.addParticle(m['q_H'], 1.0, 0.0)
        for (a, b, d) in ((o, h1, m['r_OH']), (o, h2, m['r_OH']), (h1, h2, 2.0 * m['r_OH'] * math.sin(0.5 * math.radians(m['HOH'])))):
            s.addConstraint(a, b, d); nb.addException(a, b, 0.0, 1.0, 0.0)
    s.addForce(nb)
    return s


def _drift(factory, system, x, ndof):
    """|slope| of the total energy over 500 steps of V R V at 1 fs, per degree of freedom and kT, mean over 4 replicas"""
    R, T = 4, 300.0
    eng = factory()
    eng.set_system(system_to_desc(system, ewald_split='reference'))
    eng.set_states(np.full(R, 1.0 / (KB * T)))
    eng.seed(29)
    eng.set_replicas(R, 0, np.tile(x, (R, 1, 1)), None, np.tile([EDGE] * 3, (R, 1)), np.arange(R))
    eng.minimize(tolerance=1.0, max_iterations=100)
    eng.set_integrator('V R O R V', 0.001, 5.0, 200, True, 1e-8)
    assert not eng.propagate(0).any()                               # thermalise
    eng.set_integrator('V R V', 0.001, 0.0, 50, False, 1e-8)
    E = []
    for k in range(11):
        _, _, U, K = eng.get_replicas(positions=False, velocities=False, potential=True, kinetic=True)
        E.append(U + K)
        if k < 10:
            assert not eng.propagate(1 + k).any()
    E = np.array(E)                                                 # [11][R]
    t = np.arange(11) * 50.0
    slope = np.polyfit(t, E, 1)[0]                                  # per step
    return float(np.mean(np.abs(slope) * 500.0) / (ndof * KB * T))


def test_energy_drift_is_within_three_times_the_three_site_twins(hip_engine_factory):
    """500 steps of V R V at 1 fs on the PME box, drift of the total energy per degree of freedom and kT against the three-site twin.
    One f32 placement rounding and one f32 force rounding per site and step are added, and single runs of this length scatter by about
    a factor of 2: the four-site drift may be at most 3 times the twin's."""
    box = testsystems.FourSiteWaterBox(box_edge=EDGE * unit.nanometers, cutoff=CUTOFF * unit.nanometers)
    four = _drift(hip_engine_factory, box.system, box.positions, box.ndof)
    x3 = box.positions.reshape(box.n_waters, 4, 3)[:, :3].reshape(-1, 3)
    three = _drift(hip_engine_factory, _three_site_twin(box), x3, box.ndof)
    print('energy drift per dof and kT over 500 steps: four-site %.3e, three-site twin %.3e, ratio %.2f' % (four, three, four / three))
    assert four <= 3.0 * three
