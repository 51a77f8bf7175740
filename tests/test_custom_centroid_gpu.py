"""GPU: system.CustomCentroidBondForce (openmmtools_amd/custom_expr.py, csrc/custom_centroid.hip, include/remd_hip_custom.h) against the
independent f64 helper tests/centroid_expr_oracle.py.

Every check is a difference "with the force minus without it" at the same positions.  Bounds (the project's HIP-leg standard, those of
tests/test_custom_compound_gpu.py): forces within 1e-5 max|F_custom|, energies within 1e-5 sum|E_term|, u_kl differences within rtol
1e-5, atol 1e-5 max|want|.  Positions are rounded to f32 before they go to either side: that is what the engine stores.  The centroid
and spread kernels walk a group with a stride of 64 (one wavefront per group): group sizes 63, 64 and 65 are the edges."""
import copy
import math

import numpy as np
import pytest

import centroid_expr_oracle as oracle
import compound_expr_oracle as compound
import custom_expr_oracle as term_oracle
from openmmtools_amd import custom_expr as cx, forces, mcmc, states, testsystems, unit
from openmmtools_amd.system import (system_to_desc, CustomBondForce, CustomCompoundBondForce, CustomCentroidBondForce, HarmonicBondForce)

pytestmark = pytest.mark.gpu

KB = 0.008314462618153242
BETA = 1.0 / (KB * 300.0)
STRIDE = 64                             # atoms of a group per trip of the centroid and spread kernels


def _f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def _setup(engine, system, xs, boxes=None, global_table=None, labels=None, restraint_lambda=1.0):
    desc = system_to_desc(system, box=None if boxes is None else boxes[0])
    engine.set_system(desc)
    custom = desc.get('custom_terms')
    K = 1 if global_table is None else len(global_table)
    engine.set_states(np.full(K, BETA))
    if custom:
        engine.set_custom_globals(np.tile(custom['000']['global_defaults'], (K, 1)) if global_table is None else global_table)
    if desc.get('restraints'):
        engine.set_restraint_lambdas(np.full((K, len(desc['restraints'])), restraint_lambda))
    R = len(xs)
    engine.set_replicas(R, 0, xs, None, np.zeros((R, 3)) if boxes is None else boxes, np.zeros(R, dtype=np.int64) if labels is None else labels)
    return desc


def _device(engine, system, xs, boxes=None, global_table=None, labels=None, restraint_lambda=1.0):
    """forces [R][N][3], potentials [R], per-force energies [R][n] (None without custom forces)"""
    desc = _setup(engine, system, xs, boxes, global_table, labels, restraint_lambda)
    f = engine.get_forces()
    u = engine.get_replicas(positions=False, velocities=False, potential=True)[2]
    return f, u, engine.custom_energies() if desc.get('custom_terms') else None


def _helper(force, masses, x, box=None, global_values=None):
    """per-term energies and forces of one custom force from the helpers"""
    if isinstance(force, CustomCentroidBondForce):
        return oracle.evaluate_force(force, masses, x, box, global_values)
    atoms, params = force._term_arrays()
    g = {force.getGlobalParameterName(i): force.getGlobalParameterDefaultValue(i) for i in range(force.getNumGlobalParameters())}
    g.update(global_values or {})
    if isinstance(force, CustomCompoundBondForce):
        return compound.evaluate(force.getNumParticlesPerBond(), force.getEnergyFunction(), atoms, list(force._per_bond), params, g, x, box,
                                 force.usesPeriodicBoundaryConditions())
    return term_oracle.evaluate(cx.KIND_BOND, force.getEnergyFunction(), atoms, list(force._per_bond), params, g, x, box,
                                force.usesPeriodicBoundaryConditions())


def _check(factory, base, customs, xs, boxes=None):
    """the custom forces added to ``base`` against the helpers, at R positions (and boxes): forces, potential and per-force energies (in
    the forces' order); -> (force differences [R][N][3], per-force energies [R][n], helper forces [R][N][3])"""
    xs = _f32(xs)
    system = copy.deepcopy(base)
    for f in customs:
        system.addForce(f)
    f0, u0, _ = _device(factory(), base, xs, boxes)
    f1, u1, e1 = _device(factory(), system, xs, boxes)
    assert e1.shape == (len(xs), len(customs))
    wanted = []
    for r, x in enumerate(xs):
        per = [_helper(f, base.masses, x, None if boxes is None else boxes[r]) for f in customs]
        F = sum(p[1] for p in per)
        E = np.array([p[0].sum() for p in per])
        tol_E = 1e-5 * sum(np.abs(p[0]).sum() for p in per)
        print('replica %d: |dF| / max|F| = %.3g, |dE| / sum|E| = %.3g' % (r, np.abs(f1[r] - f0[r] - F).max() / np.abs(F).max(),
                                                                         np.abs(e1[r] - E).max() / (tol_E / 1e-5)))
        assert np.abs(f1[r] - f0[r] - F).max() <= 1e-5 * np.abs(F).max()
        assert np.abs(e1[r] - E).max() <= tol_E
        assert abs((u1[r] - u0[r]) - E.sum()) <= tol_E + 2e-7 * abs(u0[r])          # (the base potential is summed in f32 partials)
        wanted.append(F)
    return f1 - f0, e1, np.array(wanted)


def _alanine(R=3, seed=1):
    al = testsystems.AlanineDipeptideVacuum()
    rng = np.random.default_rng(seed)
    xs = np.array([np.asarray(al.positions, dtype=np.float64) + rng.normal(0.0, 0.004, (len(al.positions), 3)) for _ in range(R)])
    return al, xs


def _centroids_of(force, masses, x, box=None):
    masses = np.asarray(masses, dtype=np.float64)
    groups = []
    for g in range(force.getNumGroups()):
        atoms, w = force.getGroupParameters(g)
        groups.append((atoms, oracle.normalised(w if len(w) else masses[atoms])))
    return oracle.centroids(groups, x, box, force.usesPeriodicBoundaryConditions())


# ---- 1. the harmonic centroid restraint: the helper, and the restraint kernel on the device ---------------------------------------------
def test_harmonic_distance_against_the_helper_and_the_restraint_kernel(hip_engine_factory):
    al, xs = _alanine()
    xs = _f32(xs)
    K, lam, g1, g2 = 4000.0, 0.7, list(range(0, 6)), list(range(10, 22))
    f = CustomCentroidBondForce(2, 'lambda*(K/2)*distance(g1,g2)^2')
    f.addGlobalParameter('lambda', lam); f.addPerBondParameter('K')
    f.addGroup(g1); f.addGroup(g2); f.addBond([0, 1], [K])
    dF, e1, _ = _check(hip_engine_factory, al.system, [f], xs)
    # forces.HarmonicRestraintForce of the same groups runs csrc/restraints.hip: two independent kernels, one answer
    restrained = copy.deepcopy(al.system)
    restrained.addForce(forces.HarmonicRestraintForce(K, g1, g2))
    assert 'custom_terms' not in system_to_desc(restrained) and len(system_to_desc(restrained)['restraints']) == 1
    f0 = _device(hip_engine_factory(), al.system, xs)[0]
    eng = hip_engine_factory()
    f2 = _device(eng, restrained, xs, restraint_lambda=lam)[0]
    e2 = lam * eng.restraint_energies()[:, 0]
    print('|F_centroid - F_restraint| / max|F| = %.3g, |E - E_restraint| / |E| = %.3g'
          % (np.abs(dF - (f2 - f0)).max() / np.abs(dF).max(), np.abs(e1[:, 0] - e2).max() / np.abs(e2).max()))
    assert np.abs(dF - (f2 - f0)).max() <= 1e-5 * np.abs(dF).max()
    assert np.all(np.abs(e1[:, 0] - e2) <= 1e-5 * np.abs(e2))


# ---- 2. group sizes at the kernels' stride -------------------------------------------------------------------------------------------------
def test_group_size_edges_in_one_handle(hip_engine_factory):
    """groups of 1 atom, 2 atoms, one below / exactly / one above the stride of the centroid and spread kernels, and every atom of the
    system, in one force; explicit weights on the group of exactly one stride, masses on the rest"""
    hg = testsystems.HostGuestVacuum()
    N = len(hg.positions)
    rng = np.random.default_rng(2)
    xs = np.array([np.asarray(hg.positions, dtype=np.float64) + rng.normal(0.0, 0.003, (N, 3)) for _ in range(2)])
    f = CustomCentroidBondForce(2, 'k*(distance(g1,g2)-r0)^2')
    f.addPerBondParameter('k'); f.addPerBondParameter('r0')
    sizes = [1, 2, STRIDE - 1, STRIDE, STRIDE + 1, N]
    groups = [[126], [127, 128], list(range(0, STRIDE - 1)), list(range(STRIDE - 1, 2 * STRIDE - 1)), list(range(40, 40 + STRIDE + 1)), list(range(N))]
    assert [len(g) for g in groups] == sizes
    for g in groups:
        f.addGroup(g, rng.uniform(0.5, 2.0, len(g))) if len(g) == STRIDE else f.addGroup(g)
    for n, (a, b) in enumerate([(0, 1), (2, 3), (4, 5), (1, 5), (3, 0)]):
        f.addBond([a, b], [500.0 + 100.0 * n, 0.05])
    c = _centroids_of(f, hg.system.masses, _f32(xs[0]))
    for b in range(f.getNumBonds()):
        (a, bb), _ = f.getBondParameters(b)
        assert np.linalg.norm(c[a] - c[bb]) > 0.08                                 # (no bond near r = 0 or r = r0)
    t = system_to_desc(_with(hg.system, f))['custom_terms']['000']
    assert list(np.diff(t['group_offsets'])) == sizes
    dF, _, F = _check(hip_engine_factory, hg.system, [f], xs)
    assert np.all(np.abs(F).max(axis=2) > 0.0)                                     # (the last group holds every atom: each one is pulled)


def _with(base, *customs):
    system = copy.deepcopy(base)
    for f in customs:
        system.addForce(f)
    return system


# ---- 3. sharing --------------------------------------------------------------------------------------------------------------------------
def test_shared_groups_shared_atoms_and_groups_nothing_names(hip_engine_factory):
    """a group named by three bonds, an atom in two groups, a group no bond names, and a bond that ignores one of its groups: the atoms
    of the ignored and of the unnamed group get exactly zero force"""
    al, xs = _alanine(seed=3)
    f = CustomCentroidBondForce(3, 'k*(distance(g1,g2)-0.1)^2 + 0*k')              # (g3 is not in the expression)
    f.addPerBondParameter('k')
    for g in ([1, 4, 6], [6, 8, 14], [16, 18], [19], [20, 21]):                    # atom 6 sits in two groups; 19: ignored; 20, 21: unnamed
        f.addGroup(g)
    for n, b in enumerate(([0, 1, 3], [0, 2, 3], [2, 0, 3])):                      # group 0 in three bonds, at either end
        f.addBond(b, [300.0 + 50.0 * n])
    dF, _, F = _check(hip_engine_factory, al.system, [f], xs)
    assert not dF[:, [19, 20, 21]].any()                                           # exactly zero on the device
    assert np.abs(F[:, [19, 20, 21]]).max() <= 1e-8 * np.abs(F).max()              # (the helper's differences: zero within their step error)
    assert all(np.abs(dF[:, a]).max() > 0.0 for a in (1, 4, 6, 8, 14, 16, 18))


# ---- 4. launch shape ---------------------------------------------------------------------------------------------------------------------
def test_launch_shape_beside_compound_and_plain_forces(hip_engine_factory):
    """centroid forces of 1, 64 and 65 bonds (63 padding lanes; a full wavefront; one bond in a second wavefront) beside a compound force
    and a plain CustomBondForce, the per-force energies in descriptor order although the centroid forces' wavefronts lie last"""
    al, xs = _alanine(R=2, seed=4)
    bonds = [f for f in al.system.getForces() if isinstance(f, HarmonicBondForce)][0].bonds
    G = len(bonds)
    plain = CustomBondForce('0.5*K*(r-r0)^2'); plain.addPerBondParameter('K'); plain.addPerBondParameter('r0')
    for (i, j, r0, k) in bonds:
        plain.addBond(i, j, [k, r0 * 1.03])
    p2 = CustomCompoundBondForce(2, 'k*(distance(p1,p2)-0.2)^2 + k*(z2-z1)^2'); p2.addPerBondParameter('k'); p2.addBond([1, 8], [300.0])
    c1 = CustomCentroidBondForce(2, 'k*distance(g1,g2)^4'); c1.addGlobalParameter('k', 900.0)
    c1.addGroup([0, 1, 2, 3]); c1.addGroup([18, 19, 20, 21]); c1.addBond([0, 1])

    def many(n_bonds, energy):
        # one two-atom group per bond of the molecule; bond n joins two different ones
        f = CustomCentroidBondForce(2, energy); f.addPerBondParameter('K'); f.addPerBondParameter('r0')
        for (i, j, _, _) in bonds:
            f.addGroup([i, j])
        for n in range(n_bonds):
            f.addBond([n % G, (n % G + 1 + n // G) % G], [200.0 * (1.0 + 0.01 * n), 0.05])
        return f
    c64, c65 = many(64, '0.5*K*(distance(g2,g1)-r0)^2'), many(65, 'K*(pointdistance(x1,y1,z1,x2,y2,z2)-r0)^2 + 0.1*K*(z2-z1)')
    assert G > 1 + 64 // G
    customs = [c1, plain, p2, c64, c65]
    terms = system_to_desc(_with(al.system, *customs))['custom_terms']
    assert [len(terms[k]['atoms']) for k in sorted(terms)] == [1, G, 1, 64, 65]
    assert [terms[k]['kind'] for k in sorted(terms)] == [cx.KIND_CENTROID, cx.KIND_BOND, cx.KIND_COMPOUND, cx.KIND_CENTROID, cx.KIND_CENTROID]
    _check(hip_engine_factory, al.system, customs, xs)


# ---- 5. more than two centroids ----------------------------------------------------------------------------------------------------------
OFFSETS = (0.05, 0.4, -0.35, 0.45, -0.3, 0.5)
SPRINGS = (4000.0, 80.0, 90.0, 70.0, 60.0, 50.0)
HEAVY = [1, 4, 6, 8, 14, 16]


def _boresch(groups, masses, x, lam=1.0):
    """the Boresch string on six groups, the reference values OFFSETS off the geometry of the centroids at positions x"""
    f = CustomCentroidBondForce(6, compound.BORESCH.replace('(p', '(g').replace(',p', ',g'))
    f.addGlobalParameter('lambda_restraints', lam)
    for name in compound.BORESCH_PARAMETERS:
        f.addPerBondParameter(name)
    for g in groups:
        f.addGroup(g)
    v = compound.boresch_values(_centroids_of(f, masses, np.asarray(x, dtype=np.float64)))
    f.addBond(list(range(6)), [p for k, a, o in zip(SPRINGS, v, OFFSETS) for p in (k, a - o)])
    return f


def _assert_no_dihedral_near_its_wrap(f, masses, xs):
    p = f.getBondParameters(0)[1]
    for x in xs:
        v = compound.boresch_values(_centroids_of(f, masses, _f32(x)))
        for phi, ref in zip(v[3:], (p[7], p[9], p[11])):
            assert abs(abs(compound.wrap(phi - ref)) - math.pi) > 0.1


def test_angle_dihedral_and_boresch_of_group_centroids(hip_engine_factory):
    al, xs = _alanine(seed=5)
    m = al.system.masses
    a = CustomCentroidBondForce(3, 'ka*(angle(g1,g2,g3)-1.2)^2'); a.addGlobalParameter('ka', 70.0)
    for g in ([0, 1, 2, 3], [8, 9, 10], [16, 17, 18]):
        a.addGroup(g)
    a.addBond([0, 1, 2])
    d = CustomCentroidBondForce(4, 'kd*(1+cos(2*dihedral(g1,g2,g3,g4)-0.3)) + 5*y3'); d.addGlobalParameter('kd', 25.0)
    for g in ([1, 4, 5], [6, 7], [8, 10], [14, 15, 16]):
        d.addGroup(g)
    d.addBond([0, 1, 2, 3])
    b = _boresch([[1], [4, 5], [6], [8, 10], [14, 15], [16, 18, 15]], m, al.positions, lam=0.7)
    assert g_sizes(b) == [1, 2, 1, 2, 2, 3]
    assert 'g' in b.getEnergyFunction() and 'distance(g3,g4)' in b.getEnergyFunction() and '(p' not in b.getEnergyFunction()
    _assert_no_dihedral_near_its_wrap(b, m, xs)
    _check(hip_engine_factory, al.system, [a, d, b], xs)


def g_sizes(f):
    return [len(f.getGroupParameters(g)[0]) for g in range(f.getNumGroups())]


def test_boresch_on_single_atom_groups_agrees_with_the_compound_force(hip_engine_factory):
    al, xs = _alanine(seed=6)
    xs = _f32(xs)
    b = _boresch([[a] for a in HEAVY], al.system.masses, al.positions, lam=0.7)
    _assert_no_dihedral_near_its_wrap(b, al.system.masses, xs)
    c = CustomCompoundBondForce(6, compound.BORESCH)
    c.addGlobalParameter('lambda_restraints', 0.7)
    for name in compound.BORESCH_PARAMETERS:
        c.addPerBondParameter(name)
    c.addBond(HEAVY, b.getBondParameters(0)[1])
    dF, e1, _ = _check(hip_engine_factory, al.system, [b], xs)
    f0 = _device(hip_engine_factory(), al.system, xs)[0]
    f2, _, e2 = _device(hip_engine_factory(), _with(al.system, c), xs)
    print('|F_centroid - F_compound| / max|F| = %.3g' % (np.abs(dF - (f2 - f0)).max() / np.abs(dF).max()))
    assert np.abs(dF - (f2 - f0)).max() <= 1e-5 * np.abs(dF).max()
    assert np.all(np.abs(e1 - e2) <= 1e-5 * np.abs(e2))


# ---- 6. periodic -------------------------------------------------------------------------------------------------------------------------
def test_periodic_centroids_under_each_replicas_own_box(hip_engine_factory):
    """two water molecules on opposite faces of AlanineDipeptideExplicit's box as groups, three replicas with three boxes: the distance of
    the centroids is the minimum image under each replica's own box (the copy that is not periodic sees the raw one), and a group whose
    first atom sits one box vector away keeps its centroid"""
    al = testsystems.AlanineDipeptideExplicit()
    box = np.diag(al.system.getDefaultPeriodicBoxVectors())
    boxes = np.array([box, box * 1.01, box * 1.02])
    x = _f32(al.positions)
    xs = _f32(np.array([x, x + 0.001, x - 0.001]))
    oxygens = np.arange(22, len(x), 3)
    lo, hi = int(oxygens[np.argmin(x[oxygens, 0])]), int(oxygens[np.argmax(x[oxygens, 0])])
    for b in boxes:                                                                # (farther apart than half the box)
        assert abs(x[hi, 0] - x[lo, 0]) > 0.5 * b[0] + 0.01
    made = []
    for periodic in (True, False):
        f = CustomCentroidBondForce(2, 'k*(distance(g1,g2)-0.3)^2 + kp*pointdistance(x1,y1,z1,x2,y2,z2)^2')
        f.addGlobalParameter('k', 900.0); f.addGlobalParameter('kp', 40.0)
        f.addGroup([lo, lo + 1, lo + 2]); f.addGroup([hi, hi + 1, hi + 2])
        f.addBond([0, 1])
        f.setUsesPeriodicBoundaryConditions(periodic)
        made.append(f)
    m = al.system.masses
    e_periodic, e_raw = (_helper(f, m, xs[0], boxes[0])[0][0] for f in made)
    assert abs(e_raw - e_periodic) > 0.5 * abs(e_raw)                               # (two different results to tell apart)
    dF, e1, _ = _check(hip_engine_factory, al.system, [made[0]], xs, boxes)
    _check(hip_engine_factory, al.system, [made[1]], xs, boxes)
    # the first atom of group 1 one box vector away (each replica by its own box): the same energy and forces
    shifted = xs.copy()
    for r in range(3):
        shifted[r, lo] += [boxes[r][0], -boxes[r][1], 0.0]
    shifted = _f32(shifted)
    f0 = _device(hip_engine_factory(), al.system, shifted, boxes)[0]
    f1, _, e2 = _device(hip_engine_factory(), _with(al.system, made[0]), shifted, boxes)
    print('shifted first atom: |dF| / max|F| = %.3g, |dE| / |E| = %.3g' % (np.abs((f1 - f0) - dF).max() / np.abs(dF).max(), np.abs(e2 - e1).max() / np.abs(e1).max()))
    assert np.abs((f1 - f0) - dF).max() <= 1e-5 * np.abs(dF).max()
    assert np.all(np.abs(e2 - e1) <= 1e-5 * np.abs(e1))


# ---- 7. globals and u_kl -----------------------------------------------------------------------------------------------------------------
def _com_force():
    """lambda-scaled centre-of-mass wall with a second global in the exponent"""
    f = CustomCentroidBondForce(2, 'lambda*k*(distance(g1,g2)/0.3)^alpha')
    f.addGlobalParameter('lambda', 1.0); f.addGlobalParameter('alpha', 2.0); f.addPerBondParameter('k')
    f.addGroup([0, 1, 2, 3, 4, 5]); f.addGroup([14, 15, 16, 17, 18])
    f.addBond([0, 1], [35.0])
    return f


TABLE = np.array([[1.0, 2.0], [0.5, 2.5], [0.25, 3.5]])                             # (lambda, alpha) of three states


def test_ukl_rows_under_three_states_globals(hip_engine_factory):
    al, xs = _alanine(seed=7)
    xs = _f32(xs)
    f = _com_force()
    labels = np.array([2, 0, 1])
    e0 = hip_engine_factory(); _setup(e0, al.system, xs, global_table=TABLE, labels=labels)        # (three states, no custom force)
    u0 = e0.compute_energies()
    e1 = hip_engine_factory(); _setup(e1, _with(al.system, f), xs, global_table=TABLE, labels=labels)
    u1 = e1.compute_energies()
    E = np.array([[_helper(f, al.system.masses, x, global_values=dict(zip(('lambda', 'alpha'), g)))[0].sum() for g in TABLE] for x in xs])
    want = BETA * E                                                                # beta_l E_r(g_l)
    got = u1 - u0
    print('u_kl rows: max |got - want| / max|want| =', np.abs(got - want).max() / np.abs(want).max())
    assert np.allclose(got, want, rtol=1e-5, atol=1e-5 * np.abs(want).max())
    own = np.arange(3), labels
    share, wanted = (u1 - u1[own][:, None]) - (u0 - u0[own][:, None]), want - want[own][:, None]
    assert np.allclose(share, wanted, rtol=1e-5, atol=1e-5 * np.abs(want).max())
    # a state with the replica's own globals: its column is the own column to the bit (the kernel skips it, the share is exactly 0)
    e1.set_custom_globals(np.array([[1.0, 2.0], [0.5, 2.5], [0.5, 2.5]]))
    e1.set_labels(np.array([1, 2, 0]))
    u2 = e1.compute_energies()
    assert u2[0, 2] == u2[0, 1] and u2[1, 1] == u2[1, 2] and u2[0, 0] != u2[0, 1]


# ---- 8. determinism, and nothing moves without a centroid bond ---------------------------------------------------------------------------
def test_bit_identical_twice_and_beside_forces_that_name_nothing(hip_engine_factory):
    al, xs = _alanine(seed=8)
    xs = _f32(xs)
    f = _com_force()
    b = _boresch([[1], [4, 5], [6], [8, 10], [14, 15], [16, 18, 15]], al.system.masses, al.positions)
    out = []
    for _ in range(2):
        eng = hip_engine_factory()
        f1, u1, e1 = _device(eng, _with(al.system, f, b), xs)
        out.append((f1, u1, e1, eng.get_forces(), eng.custom_energies()))
    for q, name in enumerate(('forces', 'potential', 'custom energies', 'forces again', 'custom energies again')):
        assert np.array_equal(out[0][q], out[1][q]), name                           # two handles
    assert np.array_equal(out[0][0], out[0][3]) and np.array_equal(out[0][2], out[0][4])      # one handle, twice
    # a handle with a compound and a plain custom force: a centroid force without bonds, and one whose bond carries no energy, change
    # no bit of the forces or of the other forces' energies
    plain = CustomBondForce('0.5*K*(r-0.12)^2'); plain.addPerBondParameter('K'); plain.addBond(4, 6, [900.0]); plain.addBond(8, 14, [700.0])
    c = CustomCompoundBondForce(3, 'k*angle(p1,p2,p3)^2 + k*x2'); c.addGlobalParameter('k', 12.0); c.addBond([1, 4, 6]); c.addBond([8, 14, 16])
    unnamed = CustomCentroidBondForce(2, 'distance(g1,g2)^2'); unnamed.addGroup([0, 1]); unnamed.addGroup([2, 3])
    silent = CustomCentroidBondForce(2, 'q*distance(g1,g2)^2'); silent.addGlobalParameter('q', 0.0)
    silent.addGroup(list(range(0, 11))); silent.addGroup(list(range(11, 22))); silent.addGroup([5]); silent.addBond([0, 1])
    f_a, u_a, e_a = _device(hip_engine_factory(), _with(al.system, plain, c), xs)
    f_b, u_b, e_b = _device(hip_engine_factory(), _with(al.system, plain, c, unnamed), xs)
    f_c, u_c, e_c = _device(hip_engine_factory(), _with(al.system, plain, c, silent), xs)
    assert np.array_equal(f_a, f_b) and np.array_equal(e_a, e_b) and np.array_equal(u_a, u_b)
    assert np.array_equal(f_a, f_c) and np.array_equal(e_a, e_c[:, :2]) and not e_c[:, 2].any() and np.array_equal(u_a, u_c)


# ---- 9. end to end -----------------------------------------------------------------------------------------------------------------------
def test_minimisation_lowers_the_centroid_restraint(hip_engine_factory):
    al = testsystems.AlanineDipeptideVacuum()
    f = CustomCentroidBondForce(2, '0.5*K*distance(g1,g2)^2'); f.addPerBondParameter('K')
    f.addGroup([0, 1, 2, 3]); f.addGroup([18, 19, 20, 21]); f.addBond([0, 1], [2000.0])
    x = _f32(al.positions)
    eng = hip_engine_factory()
    _setup(eng, _with(al.system, f), np.tile(x, (2, 1, 1)))
    before = eng.custom_energies()[:, 0]
    eng.minimize(tolerance=1.0, max_iterations=200)
    after = eng.custom_energies()[:, 0]
    y = eng.get_replicas()[0]
    want = np.array([_helper(f, al.system.masses, _f32(yr))[0].sum() for yr in y])
    print('centroid restraint: %s -> %s kJ/mol' % (before, after))
    assert np.all(after < 0.5 * before) and np.all(np.abs(after - want) <= 1e-5 * np.abs(want))


def test_langevin_steps_keep_the_energy_the_helper_computes(hip_engine_factory):
    al, xs = _alanine(R=6, seed=9)
    f = _com_force()
    eng = hip_engine_factory()
    _setup(eng, _with(al.system, f), _f32(xs), global_table=TABLE, labels=np.array([0, 1, 2, 2, 1, 0]))
    eng.set_integrator('V R O R V', 0.001, 1.0, 20, True, 1e-8)
    eng.seed(5)
    eng.propagate(0)
    y = eng.get_replicas()[0]
    assert np.all(np.isfinite(y)) and np.abs(y - xs).max() > 1e-4
    got = eng.custom_energies()[:, 0]
    want = np.array([_helper(f, al.system.masses, _f32(yr), global_values=dict(zip(('lambda', 'alpha'), TABLE[l])))[0].sum()
                     for yr, l in zip(y, [0, 1, 2, 2, 1, 0])])
    assert np.all(np.isfinite(got)) and np.all(np.abs(got - want) <= 1e-5 * np.abs(want))


class ComState(states.GlobalParameterState):
    lambda_com = states.GlobalParameterState.GlobalParameter('lambda_com', standard_value=1.0)


def test_multistate_sampler_over_the_forces_global(hip_engine_factory):
    from openmmtools_amd.multistate import MultiStateSampler
    al = testsystems.AlanineDipeptideVacuum()
    f = CustomCentroidBondForce(2, 'lambda_com*k*distance(g1,g2)^4'); f.addGlobalParameter('lambda_com', 1.0); f.addPerBondParameter('k')
    f.addGroup([0, 1, 2, 3, 4, 5]); f.addGroup([14, 15, 16, 17, 18]); f.addBond([0, 1], [2500.0])
    al.system.addForce(f)
    lambdas = np.array([1.0, 0.5, 0.0])
    ts = states.ThermodynamicState(al.system, 300.0)
    sts = states.create_thermodynamic_state_protocol(ts, {'lambda_com': list(lambdas)}, composable_states=[ComState(lambda_com=1.0)])
    move = mcmc.LangevinSplittingDynamicsMove(timestep=1.0 * unit.femtosecond, collision_rate=1.0 / unit.picosecond, n_steps=20,
                                              reassign_velocities=True, splitting='V R O R V')
    engine = hip_engine_factory()
    s = MultiStateSampler(mcmc_moves=move, number_of_iterations=10 ** 9, engine=engine, seed=0xC0FFEE, online_analysis_interval=None)
    s.create(sts, [states.SamplerState(al.positions)], storage=None)
    s.run(2)
    u, x = np.array(s.energy_thermodynamic_states), engine.get_replicas()[0]
    E = np.array([_helper(f, al.system.masses, _f32(xr), global_values=dict(lambda_com=1.0))[0].sum() for xr in x])
    want = sts[0].beta * (lambdas[None, :] - lambdas[0]) * E[:, None]
    got = u - u[:, :1]
    print('sampler: E =', E, 'u_kl - u_k0 =', got.tolist())
    print('sampler u_kl: max |got - want| / max|want| =', np.abs(got - want).max() / np.abs(want).max())
    assert np.all(E > 0.0) and np.allclose(got, want, rtol=1e-5, atol=1e-5 * np.abs(want).max())
