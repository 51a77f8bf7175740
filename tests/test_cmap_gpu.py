"""GPU: system.CMAPTorsionForce (REMD_CUSTOM_CMAP, csrc/cmap.hip) against the exact-derivative f64 reference of tests/cmap_oracle.py
(the interpolant of tests/tabulated2d_oracle.py, the dihedrals by the dual numbers of tests/custom_dual_oracle.py) at the f32 positions
the engine holds.

Bounds, none of them new: |E_force - sum E_t| <= 1e-11 sum|E_t|; per atom and component |dF| <= n (2^-23 max|contribution| + 2^-31), n
the contributions the atom receives (custom_nonbonded_oracle.force_bound / energy_bound, the opcode tests).  Every comparison prints
measured / bound before it asserts.  Bare systems of the forces under test unless a test says otherwise."""
import copy
import math

import numpy as np
import pytest

import cmap_oracle as oracle
import custom_dual_oracle as dual
from test_custom_tabulated_gpu import BETA, _engine, _f32
from openmmtools_amd import custom_expr as cx, testsystems
from openmmtools_amd.system import (System, system_to_desc, CMAPTorsionForce, CustomBondForce, CustomCompoundBondForce, Continuous2DFunction,
                                    HarmonicBondForce, PeriodicTorsionForce)

pytestmark = pytest.mark.gpu
KB = 0.0083144626181532


def _force(maps, torsions, periodic=False, scale=1.0):
    f = CMAPTorsionForce()
    for size, energy in maps:
        f.addMap(size, scale * np.asarray(energy))
    for row in torsions:
        f.addTorsion(*[int(v) for v in row])
    f.setUsesPeriodicBoundaryConditions(periodic)
    return f


def _compare(name, ref, E_dev, F_dev):
    """one replica's energy and forces against the reference; prints measured / bound first"""
    eb, fb = oracle.energy_bound(ref), oracle.force_bound(ref)
    dE, dF = abs(E_dev - ref['E'].sum()), np.abs(F_dev - ref['F'])
    touched = ref['partners'] > 0
    print('%-22s |dE| / bound = %.3g, worst |dF| / bound = %.3g (%d terms, most contributions on an atom %d)'
          % (name, dE / eb, (dF[touched] / fb[touched]).max(), len(ref['E']), ref['partners'].max()))
    assert np.isfinite(ref['E']).all() and np.abs(ref['E']).sum() > 0.0
    assert dE <= eb
    assert np.all(dF <= fb), np.argwhere(dF > fb)[:5]
    assert not F_dev[~touched].any()


# ---- 1. the smallest map ------------------------------------------------------------------------------------------------------------------
def test_one_torsion_pair_on_the_smallest_map(hip_engine_factory):
    """size = 4: every patch touches the wrap.  One term of five atoms, three replicas at different geometries"""
    maps = [oracle.MAPS[0]]
    torsions = [(0, 0, 1, 2, 3, 1, 2, 3, 4)]
    xs = oracle.chain_positions(5, replicas=3, seed=3, special=False)
    eng, desc = _engine(hip_engine_factory, [_force(maps, torsions)], xs)
    t = desc['custom_terms']['000']
    assert t['kind'] == cx.KIND_CMAP and t['atoms'].shape == (1, 8) and len(t['consts']) == 8 + 4 * 25
    F, E = eng.get_forces(), eng.custom_energies()
    assert E.shape == (3, 1)
    for r in range(3):
        _compare('size 4, replica %d' % r, oracle.evaluate(maps, torsions, xs[r]), E[r, 0], F[r])
    assert np.abs(F).max() > 1.0


# ---- 2. map selection, padding lanes, shared atoms, the wrap --------------------------------------------------------------------------------
def test_seventy_pairs_over_three_maps(hip_engine_factory):
    """70 terms on a 74-atom chain (two wavefronts, 6 live lanes in the second), maps of sizes 4, 7 and 24 assigned in a scrambled order;
    consecutive terms share atoms, so an inner atom receives eight contributions.  Hand-placed segments put angles exactly on 0 (cis,
    planar), on +-pi (trans, planar), on +-pi/2 (a node of the sizes 4 and 24) and a hair either side of 0 (the last atom of the cis
    segment 1e-8 nm off the plane: +-1.07e-7 rad, above it in replica 0 and below it in replica 1)"""
    xs = oracle.XS70
    eng, _ = _engine(hip_engine_factory, [_force(oracle.MAPS, oracle.TORSIONS70)], xs)
    F, E = eng.get_forces(), eng.custom_energies()
    refs = [oracle.evaluate(oracle.MAPS, oracle.TORSIONS70, x) for x in xs]
    oracle.check_special_angles(refs)
    assert refs[0]['partners'].max() == 8 and sorted(set(oracle.TORSIONS70[:, 0].tolist())) == [0, 1, 2]
    for r, ref in enumerate(refs):
        _compare('70 terms, replica %d' % r, ref, E[r, 0], F[r])


# ---- 3. the compound-bond path: another kernel, the same numbers ----------------------------------------------------------------------------
def _compound_forces(maps, torsions):
    out = []
    for m, (size, energy) in enumerate(maps):
        f = CustomCompoundBondForce(8, 'm(dihedral(p1,p2,p3,p4), dihedral(p5,p6,p7,p8))')
        f.addTabulatedFunction('m', Continuous2DFunction(size + 1, size + 1, oracle.edge_repeated(size, energy), 0.0, oracle.TWO_PI, 0.0, oracle.TWO_PI,
                                                         periodic=True))
        for row in torsions:
            if row[0] == m:
                f.addBond([int(a) for a in row[1:]], [])
        out.append(f)
    return out


def test_the_compound_bond_path_gives_the_same_energies_and_forces(hip_engine_factory):
    """the 70 terms as one CustomCompoundBondForce of eight particles per map with the periodic Continuous2DFunction on the edge-repeated
    grid (custom_compound.hip: the stack machine, eight seeded passes): energies within the sum of both energy bounds, forces within the
    sum of both force bounds (each path rounds every contribution to f32 once)"""
    xs = oracle.XS70
    eng, _ = _engine(hip_engine_factory, [_force(oracle.MAPS, oracle.TORSIONS70)], xs)
    other, _ = _engine(hip_engine_factory, _compound_forces(oracle.MAPS, oracle.TORSIONS70), xs)
    F, E, Fo, Eo = eng.get_forces(), eng.custom_energies(), other.get_forces(), other.custom_energies()
    assert Eo.shape == (2, 3)
    for r, x in enumerate(xs):
        ref = oracle.evaluate(oracle.MAPS, oracle.TORSIONS70, x)
        eb, fb = 2.0 * oracle.energy_bound(ref), 2.0 * oracle.force_bound(ref)
        dE, dF = abs(E[r, 0] - Eo[r].sum()), np.abs(F[r] - Fo[r])
        print('replica %d: |E_cmap - E_compound| / bound = %.3g, worst |dF| / bound = %.3g' % (r, dE / eb, (dF / fb).max()))
        assert dE <= eb and np.all(dF <= fb)


# ---- 4, 5. the periodic flag ------------------------------------------------------------------------------------------------------------------
def test_the_periodic_flag_takes_minimum_images_and_its_absence_does_not(hip_engine_factory):
    """one term of eight distinct atoms wrapped into the box around a corner, so that its bonds cross every face: with the flag the
    reference takes minimum images, without it none, and the two energies differ"""
    boxes, xs = oracle.straddling_positions()
    maps, torsions = [oracle.MAPS[2]], [(0, 0, 1, 2, 3, 4, 5, 6, 7)]
    E = {}
    for periodic in (True, False):
        eng, _ = _engine(hip_engine_factory, [_force(maps, torsions, periodic=periodic)], xs, boxes)
        F, E[periodic] = eng.get_forces(), eng.custom_energies()
        for r in range(len(xs)):
            ref = oracle.evaluate(maps, torsions, xs[r], boxes[r], periodic)
            _compare('periodic %s, replica %d' % (periodic, r), ref, E[periodic][r, 0], F[r])
    print('energies with the flag', E[True][:, 0], 'without', E[False][:, 0])
    assert np.all(np.abs(E[True] - E[False]) > 1e-3)


# ---- 6. degenerate geometry -------------------------------------------------------------------------------------------------------------------
def test_a_collinear_quadruple_gives_a_finite_energy_and_no_nan(hip_engine_factory):
    """the first three atoms exactly collinear: b1 x b2 = 0, the first angle is atan2 of zeros (0 here); |b1 x b2|^2 is taken as 1e-24
    (the compound-bond convention), so the gradient on atom 0 vanishes and the others keep their formulas: the energy is the map at
    (0, psi) and the forces are those of oracle.convention_term"""
    x = np.array([[0.0, 0.0, 0.0], [0.125, 0.0, 0.0], [0.25, 0.0, 0.0], [0.25, 0.125, 0.0], [0.375, 0.125, 0.125]])
    xs = _f32([x, x])
    maps, torsions = [oracle.MAPS[1]], [(0, 0, 1, 2, 3, 1, 2, 3, 4)]
    eng, _ = _engine(hip_engine_factory, [_force(maps, torsions)], xs)
    F, E = eng.get_forces(), eng.custom_energies()
    slots = [0, 1, 2, 3, 1, 2, 3, 4]
    v, G, phi, psi = oracle.convention_term(oracle.table(*maps[0]), xs[0][slots])
    assert phi == 0.0 and abs(psi) > 0.1 and (phi, psi) == oracle.angles(xs[0][slots])
    want = np.zeros((5, 3))
    for a, i in enumerate(slots):
        want[i] += G[a]
    print('collinear: E = %r (map at (0, psi): %r), max |F - convention| = %.3g' % (E[0, 0], v, np.abs(F[0] - want).max()))
    assert np.isfinite(E).all() and np.isfinite(F).all()
    assert abs(E[0, 0] - v) <= 1e-11 * abs(v)
    assert np.all(np.abs(F[0] - want) <= 2.0 * (2.0 ** -23 * np.abs(want).max() + 2.0 ** -31))
    assert not F[0, 0].any() and np.abs(F[0, 1:]).min(axis=0).max() > 0.0       # (only the collinear dihedral names atom 0)


# ---- 7. repeatability -------------------------------------------------------------------------------------------------------------------------
def test_two_evaluations_are_bitwise_equal(hip_engine_factory):
    eng, _ = _engine(hip_engine_factory, [_force(oracle.MAPS, oracle.TORSIONS70)], oracle.XS70)
    F, E = eng.get_forces(), eng.custom_energies()
    again, _ = _engine(hip_engine_factory, [_force(oracle.MAPS, oracle.TORSIONS70)], oracle.XS70)
    assert np.array_equal(eng.get_forces(), F) and np.array_equal(eng.custom_energies(), E)
    assert np.array_equal(again.get_forces(), F) and np.array_equal(again.custom_energies(), E)


# ---- 8. phase clones ---------------------------------------------------------------------------------------------------------------------------
def test_phased_propagation_with_a_cmap_force_is_the_one_block_run(hip_engine_factory):
    """AlanineDipeptideExplicit with a periodic CMAP force on its phi / psi atoms and a second term, on two maps, 6 replicas, 20 steps
    per iteration: two blocks equal one block bit for bit, as tests/test_phases_gpu.py compares them (a clone that missed the maps, the
    map indices or the boundary of the CMAP wavefronts would differ or fault the descriptor check)"""
    al = testsystems.AlanineDipeptideExplicit()
    f = _force(oracle.MAPS[1:], [(1, 4, 6, 8, 14, 6, 8, 14, 16), (0, 1, 4, 6, 8, 4, 6, 8, 14)], periodic=True, scale=4.0)
    al.system.addForce(f)
    desc = system_to_desc(al.system, ewald_split='auto')
    box = np.diag(al.system.getDefaultPeriodicBoxVectors())
    R = 6
    out = []
    for phases in (1, 2):
        eng = hip_engine_factory()
        eng.set_phases(phases)
        eng.set_system(desc)
        eng.set_states(1.0 / (KB * np.linspace(300.0, 320.0, R)))
        eng.set_custom_globals(np.zeros((R, 0)))
        eng.set_integrator('V R R O R R V', 0.002, 1.0, 20, True, 1e-8)
        eng.seed(9)
        eng.set_replicas(R, 0, np.tile(al.positions, (R, 1, 1)), None, np.tile(box, (R, 1)), np.arange(R))
        for it in range(2):
            assert not eng.propagate(it).any()
            u = eng.compute_energies()
        x, v = eng.get_replicas()[:2]
        out.append((x.copy(), v.copy(), u.copy(), eng.custom_energies(), eng.phases_active()))
    assert out[0][4] == 1 and out[1][4] == 2
    for a, b in zip(out[0][:4], out[1][:4]):
        assert np.array_equal(a, b)
    assert np.abs(out[0][3]).min() > 0.0 and np.ptp(out[0][3][:, 0]) > 0.0


# ---- 9. force groups and per-force energies ---------------------------------------------------------------------------------------------------
def test_group_forces_and_custom_energies_separate_the_force(hip_engine_factory):
    """beside a built-in PeriodicTorsionForce on the same atoms (group 1) and a CustomBondForce (group 2, with the CMAP force: the custom
    forces of a handle share one group): custom_energies() has one column per custom force, get_forces(groups = the custom group) minus
    the bond reference is the CMAP force's share, and the groups add up to the total within 2^-30"""
    xs = oracle.XS70
    N = xs.shape[1]
    s = System()
    for _ in range(N):
        s.addParticle(12.0)
    tors = PeriodicTorsionForce()
    for row in oracle.TORSIONS70:
        tors.addTorsion(int(row[1]), int(row[2]), int(row[3]), int(row[4]), 2, 0.3, 5.0)
    tors.setForceGroup(1)
    bonds = CustomBondForce('0.5*k*(r-0.2)^2')
    bonds.addPerBondParameter('k')
    pairs = [(i, i + 1) for i in range(0, N - 1, 3)]
    for i, j in pairs:
        bonds.addBond(i, j, [300.0])
    bonds.setForceGroup(2)
    cmap = _force(oracle.MAPS, oracle.TORSIONS70)
    cmap.setForceGroup(2)
    for f in (tors, bonds, cmap):
        s.addForce(f)
    desc = system_to_desc(s)
    assert [t['kind'] for t in desc['custom_terms'].values()] == [cx.KIND_BOND, cx.KIND_CMAP]
    eng = hip_engine_factory()
    eng.set_system(desc)
    eng.set_states(np.full(1, BETA))
    eng.set_custom_globals(np.zeros((1, 0)))
    eng.set_replicas(2, 0, xs, None, np.zeros((2, 3)), np.zeros(2, dtype=np.int64))
    total, builtin, custom, E = eng.get_forces(), eng.get_forces(groups=1 << 1), eng.get_forces(groups=1 << 2), eng.custom_energies()
    assert E.shape == (2, 2)
    for r in range(2):
        ref = oracle.evaluate(oracle.MAPS, oracle.TORSIONS70, xs[r])
        Eb, Fb, Gb = dual.evaluate(dual.KIND_BOND, '0.5*k*(r-0.2)^2', pairs, ['k'], np.full((len(pairs), 1), 300.0), {}, xs[r], per_term=True)
        both = dict(E=ref['E'], F=ref['F'] + Fb, partners=ref['partners'].copy(), peak=ref['peak'].copy())
        for t, (i, j) in enumerate(pairs):
            for a, k in enumerate((i, j)):
                both['partners'][k] += 1
                both['peak'][k] = np.maximum(both['peak'][k], np.abs(Gb[t, a]))
        assert abs(E[r, 0] - Eb.sum()) <= 1e-11 * np.abs(Eb).sum()
        _compare('beside two forces, r %d' % r, both, E[r, 1], custom[r])
        print('replica %d: max |total - sum of the groups| = %.3g' % (r, np.abs(total[r] - builtin[r] - custom[r]).max()))
        assert np.abs(total[r] - builtin[r] - custom[r]).max() <= 2.0 ** -30
    assert np.abs(builtin).max() > 1.0 and not eng.get_forces(groups=1 << 3).any()


# ---- 10. minimisation --------------------------------------------------------------------------------------------------------------------------
def test_minimize_lowers_the_energy_of_a_chain_with_bonds_and_a_cmap_force(hip_engine_factory):
    """22 atoms, harmonic bonds along the chain and 18 CMAP terms on two maps: minimize() lowers the potential, and the force's energy at
    the final positions is the reference's"""
    N = 22
    xs = oracle.chain_positions(N, replicas=2, seed=10, special=False)
    torsions = np.array([(t % 2, t, t + 1, t + 2, t + 3, t + 1, t + 2, t + 3, t + 4) for t in range(N - 4)])
    maps = [oracle.MAPS[1], oracle.MAPS[2]]
    s = System()
    for _ in range(N):
        s.addParticle(12.0)
    hb = HarmonicBondForce()
    for i in range(N - 1):
        hb.addBond(i, i + 1, 0.15, 2.0e5)
    s.addForce(hb)
    s.addForce(_force(maps, torsions, scale=5.0))
    eng = hip_engine_factory()
    eng.set_system(system_to_desc(s))
    eng.set_states(np.full(1, BETA))
    eng.set_custom_globals(np.zeros((1, 0)))
    eng.set_replicas(2, 0, xs, None, np.zeros((2, 3)), np.zeros(2, dtype=np.int64))
    u0, E0 = eng.get_replicas(positions=False, velocities=False, potential=True)[2], eng.custom_energies()
    eng.minimize(tolerance=1.0, max_iterations=300)
    u1, E1 = eng.get_replicas(positions=False, velocities=False, potential=True)[2], eng.custom_energies()
    x1 = eng.get_replicas()[0]
    print('potential before', u0, 'after', u1, 'map', E0[:, 0], '->', E1[:, 0])
    assert np.all(u1 < u0 - 1.0)
    scaled = [(size, 5.0 * np.asarray(e)) for size, e in maps]
    for r in range(2):
        ref = oracle.evaluate(scaled, torsions, _f32(x1[r]))
        print('replica %d: final |dE| / bound = %.3g' % (r, abs(E1[r, 0] - ref['E'].sum()) / oracle.energy_bound(ref)))
        assert abs(E1[r, 0] - ref['E'].sum()) <= oracle.energy_bound(ref)


# ---- 11. the library's own checks -------------------------------------------------------------------------------------------------------------
def test_the_library_refuses_a_broken_descriptor_and_keeps_the_handle(hip_engine_factory):
    """what the host never lets through, handed to set_custom_terms directly: the library names the fault, and the force it held before
    the refused call still acts"""
    xs = oracle.XS70
    eng, desc = _engine(hip_engine_factory, [_force(oracle.MAPS, oracle.TORSIONS70)], xs)
    before, F_before = eng.custom_energies(), eng.get_forces()
    good = desc['custom_terms']['000']
    assert good['map_offsets'].tolist() == [0, 8 + 4 * 25, 16 + 4 * (25 + 64)]

    def broken(**changes):
        t = dict(good)
        t.update(changes)
        return t

    def consts_with(i, v):
        c = good['consts'].copy(); c[i] = v
        return c
    far_map = good['map_index'].copy(); far_map[69] = 3
    low_map = good['map_index'].copy(); low_map[0] = -1
    far_atom = good['atoms'].copy(); far_atom[5, 7] = xs.shape[1]
    second = int(good['map_offsets'][1])
    for t, message in ((broken(map_index=far_map), 'term 69: map index out of range'),
                       (broken(map_index=low_map), 'term 0: map index out of range'),
                       (broken(atoms=far_atom), 'atom index out of range'),
                       (broken(consts=consts_with(second + 1, 9.0)), 'map 1: a block whose sizes are not nx = ny, an integer 3 ... 256'),
                       (broken(consts=consts_with(0, 2.0)), 'map 0: a block whose sizes are not nx = ny'),
                       (broken(consts=consts_with(second + 6, 0.0)), 'map 1: a block that is not periodic'),
                       (broken(consts=consts_with(3, math.pi)), r'map 0: a block whose range is not \[0, 2 pi\] in both angles'),
                       (broken(consts=good['consts'][:-1].copy()), 'map 2: a block that runs past n_consts'),
                       (broken(map_offsets=np.array([0, second, len(good['consts']) - 4], dtype=np.int32)), 'map 2: a block that runs past n_consts'),
                       (broken(n_particles=5, atoms=good['atoms'][:, :5].copy()), 'n_particles is 8 for a CMAP force'),
                       (broken(program=np.array([[cx.CONST, 0]], dtype=np.int32)), 'a CMAP force has no per-term parameters and no program')):
        with pytest.raises(RuntimeError, match='remd_set_custom_terms.*force 0: .*' + message):
            eng.set_custom_terms([t])
        assert np.array_equal(eng.custom_energies(), before) and np.array_equal(eng.get_forces(), F_before)


# ---- 12. beside a centroid-bond force: the buffers of the parts in front keep their strides ----------------------------------------------------
def test_beside_a_centroid_bond_force_at_three_replicas(hip_engine_factory):
    """one wavefront of a CustomCentroidBondForce (two bonds between four groups of atoms 74 ... 89) in front of the two CMAP wavefronts,
    three replicas: the centroid force's per-replica gradient buffer spans every wavefront from its own on, so replicas 1 and 2 tell
    whether its size and its kernels' strides still agree.  The CMAP share (atoms 0 ... 73) at this file's bounds; the centroid share
    (the other atoms) at the bounds of tests/test_custom_centroid_gpu.py against its finite-difference reference: forces within 1e-5
    max|F|, energy within 1e-5 sum|E|"""
    import centroid_expr_oracle as centroid
    from openmmtools_amd.system import CustomCentroidBondForce
    xs = oracle.chain_positions(90, replicas=3, seed=12)
    c = CustomCentroidBondForce(2, '0.5*k*(distance(g1,g2)-d0)^2')
    c.addPerBondParameter('k'); c.addPerBondParameter('d0')
    for atoms in ([74, 75, 76, 77], [78, 79, 80], [81, 82, 83, 84, 85], [86, 87, 88, 89]):
        c.addGroup(atoms)
    c.addBond([0, 1], [400.0, 0.2]); c.addBond([2, 3], [250.0, 0.3])
    masses = 1.0 + np.arange(90) % 5
    eng, desc = _engine(hip_engine_factory, [c, _force(oracle.MAPS, oracle.TORSIONS70)], xs, masses=masses)
    assert [t['kind'] for t in desc['custom_terms'].values()] == [cx.KIND_CENTROID, cx.KIND_CMAP]
    F, E = eng.get_forces(), eng.custom_energies()
    assert E.shape == (3, 2)
    for r in range(3):
        ref = oracle.evaluate(oracle.MAPS, oracle.TORSIONS70, xs[r])
        Ec, Fc = centroid.evaluate_force(c, masses, xs[r])
        assert not Fc[:74].any() and not ref['F'][74:].any() and np.abs(Fc).max() > 1.0
        share = F[r].copy(); share[74:] = 0.0
        _compare('beside centroid, r %d' % r, ref, E[r, 1], share)
        dFc = np.abs(F[r, 74:] - Fc[74:]).max()
        print('replica %d: centroid |dF| / max|F| = %.3g, |dE| / sum|E| = %.3g' % (r, dFc / np.abs(Fc).max(), abs(E[r, 0] - Ec.sum()) / np.abs(Ec).sum()))
        assert dFc <= 1e-5 * np.abs(Fc).max() and abs(E[r, 0] - Ec.sum()) <= 1e-5 * np.abs(Ec).sum()


# ---- 13. u_kl rows beside forces whose globals differ between the states --------------------------------------------------------------------
def test_ukl_rows_beside_a_bond_and_a_cv_force_with_a_per_state_global(hip_engine_factory):
    """a CustomBondForce and a CustomCVForce that share the global lam, three states, beside the CMAP force (which has no globals and
    writes no u_kl partials: its columns of the partial array must stay zero, and the CV launch must end where the CMAP wavefronts
    begin).  All states share beta, so the CMAP energy drops out of a row relative to the replica's own state, and the rows are
    beta (lam_l - lam_own) (E_bond + E_cv) at lam = 1: rtol 1e-5, atol 1e-5 max|want|, the bounds of the u_kl rows in
    tests/test_custom_tabulated2d_gpu.py.  The CMAP energy itself is its column of custom_energies(), at this file's bound"""
    import custom_cv_oracle as cv_oracle
    from openmmtools_amd.system import CustomCVForce, RMSDForce
    xs = oracle.XS70
    N = xs.shape[1]
    bonds = CustomBondForce('lam*0.5*k*(r-0.2)^2')
    bonds.addGlobalParameter('lam', 1.0); bonds.addPerBondParameter('k')
    pairs = [(i, i + 1) for i in range(0, N - 1, 3)]
    for i, j in pairs:
        bonds.addBond(i, j, [300.0])
    rng = np.random.default_rng(13)
    cv = CustomCVForce('lam*200*v^2')
    cv.addGlobalParameter('lam', 1.0)
    cv.addCollectiveVariable('v', RMSDForce(xs[0] + rng.normal(0.0, 0.03, xs[0].shape), [50, 51, 52, 53, 54, 55, 56]))
    table = np.array([[1.0], [0.5], [0.0]])
    labels = np.array([2, 0])
    eng, desc = _engine(hip_engine_factory, [bonds, cv, _force(oracle.MAPS, oracle.TORSIONS70)], xs, global_table=table, labels=labels)
    assert [t['kind'] for t in desc['custom_terms'].values()] == [cx.KIND_BOND, cx.KIND_CV, cx.KIND_CMAP]
    u = eng.compute_energies()
    E1 = np.zeros(2)
    for r in range(2):
        Eb = dual.evaluate(dual.KIND_BOND, '0.5*k*(r-0.2)^2', pairs, ['k'], np.full((len(pairs), 1), 300.0), {}, xs[r])[0]
        E1[r] = Eb.sum() + cv_oracle.evaluate(cv, xs[r], dict(lam=1.0))[0]
    want = BETA * table[None, :, 0] * E1[:, None]
    own = np.arange(2), labels
    got, want = u - u[own][:, None], want - want[own][:, None]
    print('u_kl rows: max |got - want| / max|want| = %.3g' % (np.abs(got - want).max() / np.abs(want).max()))
    assert np.allclose(got, want, rtol=1e-5, atol=1e-5 * np.abs(want).max()) and np.abs(want).max() > 0.1
    again = eng.compute_energies()                                                 # (the partial array is allocated once: a second call reads it again)
    assert np.array_equal(again, u)
    E = eng.custom_energies()
    for r in range(2):
        ref = oracle.evaluate(oracle.MAPS, oracle.TORSIONS70, xs[r])
        print('replica %d: CMAP column |dE| / bound = %.3g' % (r, abs(E[r, 2] - ref['E'].sum()) / oracle.energy_bound(ref)))
        assert abs(E[r, 2] - ref['E'].sum()) <= oracle.energy_bound(ref)
