"""PME reciprocal space alone, per mesh path, box and placement edge (csrc/pme.hip), against the f64 oracle on the same mesh.

Cases, mesh paths, placements and helpers: tests/pme_edge_cases.py.  Reciprocal space sits in a force group of its own, so
get_forces(groups=...) is the mesh path alone; the ABI gives no per-class energy, so the total potential is compared with the oracle's total
and the bound is stated relative to the oracle's |E(classes={5})|.
  (a) forces and (b) potential of every mesh path x {bulk, faces, outside} and of every placement on mixed / p64 / slab;
  (c) replicas with their own boxes: each follows the oracle at its own box (a, b) and equals, bit for bit, a one-replica handle; the same
      with one box three times (the shared influence table);
  (d) a box change on a live handle gives the bits of a fresh handle (the table follows the box);
  (e) a permutation of the atoms does not change a bit of the forces; (f) periodic images; (g) charges scaled per replica.
Bounds: pme_edge_cases.bounds(), 4 x the largest error recorded in profiles/pme_edge_errors.txt per family."""
import numpy as np
import pytest

import pme_edge_cases as pc

pytestmark = pytest.mark.gpu


def _run(make, desc, x, box, lambda_electrostatics=None):
    eng = make()
    try:
        pc.setup_engine(eng, desc, x, box, lambda_electrostatics)
        return pc.evaluate(eng)
    finally:
        eng.close()


@pytest.fixture(scope='module')
def results(hip_engine_factory):
    """case -> (engine forces, potential, oracle class-5 forces, class-5 energy, total energy), evaluated once for (a), (b), (f)"""
    cache = {}

    def get(case):
        if case not in cache:
            desc, x, box = pc.build_case(case)
            f, U, xd = _run(hip_engine_factory, desc, x, box)
            cache[case] = (f, U) + pc.oracle_reference(desc, xd, box)
        return cache[case]
    return get


def _check_forces(case, f, f5):
    B = pc.bounds()
    small = case[1] in pc.SMALL
    for r in range(len(f)):
        w = pc.errors(f[r:r + 1], np.zeros(1), f5[r:r + 1], np.ones(1), np.zeros(1))[0]
        print('%s r%d max|df| %.4e rms %.4e max|f_ref| %.5e rel %.4e %.4e' % (pc.case_id(case), r, w['f_max'], w['f_rms'], w['f_ref'], w['f_max_rel'], w['f_rms_rel']))
        if small:
            assert w['f_max'] <= B['f_max_small'] and w['f_rms'] <= B['f_rms_small'], (case, r, w)
        else:
            assert w['f_ref'] > 1.0
            assert w['f_max_rel'] <= B['f_max_rel'] and w['f_rms_rel'] <= B['f_rms_rel'], (case, r, w)


@pytest.mark.parametrize('case', pc.MATRIX + pc.PER_REPLICA, ids=pc.case_id)
def test_reciprocal_forces_follow_the_oracle(results, case):
    """(a), (c): the reciprocal force group against the oracle's class 5, per replica"""
    f, U, f5, e5, et = results(case)
    assert np.all(np.isfinite(f))
    _check_forces(case, f, f5)


@pytest.mark.parametrize('case', pc.MATRIX + pc.PER_REPLICA, ids=pc.case_id)
def test_total_potential_follows_the_oracle(results, case):
    """(b), (c): the total potential against the oracle's, the bound relative to the oracle's reciprocal-space energy |E(classes={5})|
    (absolute for one and two atoms), and never looser than 1e-5 of the total"""
    f, U, f5, e5, et = results(case)
    B = pc.bounds()
    for r in range(len(U)):
        de = abs(U[r] - et[r])
        print('%s r%d U %.10e ref %.10e dE %.4e E_recip %.8e dE/|E_recip| %.4e' % (pc.case_id(case), r, U[r], et[r], de, e5[r], de / abs(e5[r])))
        bound = B['e_abs_small'] if case[1] in pc.SMALL else B['e_rel'] * abs(e5[r])
        assert de <= min(bound, 1e-5 * abs(et[r])), (case, r, U[r], et[r], e5[r])


@pytest.mark.parametrize('mesh', pc.PER_REPLICA_MESHES)
@pytest.mark.parametrize('boxes', ['own', 'shared'])
def test_replicas_equal_their_single_replica_handles(hip_engine_factory, mesh, boxes):
    """(c) exact: replica r of an R = 3 handle -- with its own box (one influence table per replica, infl_rep = nzc) or with the same box
    three times (one table for all, infl_rep = 0) -- gives the bits of an R = 1 handle with replica r's box and positions: the mesh is a
    32-bit fixed-point sum, the forces are 64-bit fixed-point sums, and the table values do not depend on r.  The potential is a sum of
    per-workgroup partial sums whose layout does not depend on R either, so it is held to the same bits."""
    desc, x, box = pc.build_case((mesh, 'bulk', 'per_replica'))
    if boxes == 'shared':
        box = np.tile(box[1], (3, 1))
    f3, U3, xd3 = _run(hip_engine_factory, desc, x, box)
    assert np.any(f3[0] != f3[1]) and np.any(f3[1] != f3[2])
    for r in range(3):
        f1, U1, xd1 = _run(hip_engine_factory, desc, x[r:r + 1], box[r:r + 1])
        assert np.array_equal(xd1[0], xd3[r])
        assert np.array_equal(f1[0], f3[r]), (mesh, boxes, r, np.abs(f1[0] - f3[r]).max())
        assert U1[0] == U3[r], (mesh, boxes, r, U1[0], U3[r])


@pytest.mark.parametrize('mesh', ['p64', 'slab'])
def test_a_box_change_on_a_live_handle_rebuilds_the_table(hip_engine_factory, mesh):
    """(d): evaluate, set_replicas again with another box and the positions scaled with it, evaluate again: the bits of a fresh handle built
    with the second box (the influence table follows box_version)"""
    desc, x, box = pc.build_case((mesh, 'bulk', 'ortho'))
    box2 = pc.SECOND_BOX[None]
    x2 = x * (box2 / box)[:, None, :]
    eng = hip_engine_factory()
    try:
        pc.setup_engine(eng, desc, x, box)
        f_a, U_a, _ = pc.evaluate(eng)
        eng.set_replicas(1, 0, x2, None, box2, np.zeros(1, dtype=np.int64))
        f_b, U_b, xd_b = pc.evaluate(eng)
    finally:
        eng.close()
    f_new, U_new, xd_new = _run(hip_engine_factory, desc, x2, box2)
    assert np.array_equal(xd_b, xd_new)
    assert np.any(f_a != f_b)
    assert np.array_equal(f_b, f_new), np.abs(f_b - f_new).max()
    assert U_b[0] == U_new[0], (U_b[0], U_new[0])
    # and the second result is right, not merely reproducible
    f5, e5, et = pc.oracle_reference(desc, xd_b, box2)
    _check_forces((mesh, 'bulk', 'second box'), f_b, f5)


@pytest.mark.parametrize('mesh,placement,boxid', [('mixed', 'bulk', 'ortho'), ('p64', 'many', 'big'), ('z64', 'faces', 'ortho'), ('slab', 'one_column', 'ortho')])
def test_a_permutation_of_the_atoms_changes_no_bit(hip_engine_factory, mesh, placement, boxid):
    """(e): the mesh is an integer sum and the gather is per atom, so the reciprocal forces of permuted (x, q), un-permuted, are the same
    bits (`many`: more atoms than one stride of pme_bin_kernel, in another order inside the bins)"""
    case = (mesh, placement, boxid)
    desc, x, box = pc.build_case(case)
    q = np.asarray(desc['charge'])
    perm = np.random.default_rng(pc.case_seed(*case) ^ 0x5a5a).permutation(len(q))
    f, U, xd = _run(hip_engine_factory, desc, x, box)
    fp, Up, xdp = _run(hip_engine_factory, pc.make_desc(q[perm], pc.MESHES[mesh][0]), x[:, perm], box)
    assert np.array_equal(xdp[0], xd[0][perm])
    back = np.empty_like(fp)
    back[:, perm] = fp
    assert np.any(f != 0) and np.array_equal(back, f), np.abs(back - f).max()


@pytest.mark.parametrize('mesh', list(pc.MESHES))
def test_periodic_images_give_the_same_forces(hip_engine_factory, results, mesh):
    """(f): atoms shifted by whole boxes against their wrapped parent: the two differ only by the fp32 rounding of x and of x / L, twice the
    bound of (a)"""
    case = (mesh, 'outside', 'ortho')
    f_out, U_out, f5, e5, et = results(case)
    desc, x, box = pc.build_case(case)
    xp = pc.wrapped_parent(x, box)
    assert np.all((xp >= 0) & (xp < box[:, None, :])) and np.abs(x - xp).max() >= 2.0 * box.min() and (x - xp).min() < 0
    f_par, U_par, xd = _run(hip_engine_factory, desc, xp, box)
    d = f_out[0] - f_par[0]
    scale = np.abs(f5).max()
    print('%s max|df| %.4e rms %.4e scale %.5e' % (mesh, np.abs(d).max(), np.sqrt((d * d).sum(axis=1).mean()), scale))
    assert np.abs(d).max() <= 2.0 * pc.bounds()['f_max_rel'] * scale
    assert np.sqrt((d * d).sum(axis=1).mean()) <= 2.0 * pc.bounds()['f_rms_rel'] * scale


@pytest.mark.parametrize('mesh', ['mixed', 'p64'])
def test_charges_scaled_per_replica(hip_engine_factory, mesh):
    """(g): one alchemical region of a third of the atoms under the exact PME treatment (its charges scale with lambda_electrostatics inside
    the whole Ewald sum); three states with lambda_electrostatics 1, 0.5, 0 and one replica in each: the reciprocal forces follow the oracle at
    each lambda, and at lambda 0 the scaled atoms get exactly zero (the q == 0 skip)"""
    grid = pc.MESHES[mesh][0]
    box = np.tile(pc.BOXES['ortho'], (3, 1))
    rng = np.random.default_rng(pc.case_seed(mesh, 'bulk', 'lambda'))
    x1, q = pc.bulk(rng, box[0], grid)
    x = np.stack([x1] + [pc.bulk(rng, box[0], grid)[0] for _ in range(2)])
    region = np.arange(len(q) // 3)
    lam = np.array([1.0, 0.5, 0.0])
    desc = pc.make_desc(q, grid, alch_atoms=region)
    f, U, xd = _run(hip_engine_factory, desc, x, box, lambda_electrostatics=lam)
    f5, e5, et = pc.oracle_reference(desc, xd, box, lambda_electrostatics=lam)
    _check_forces((mesh, 'bulk', 'lambda'), f, f5)
    assert np.array_equal(f[2][region], np.zeros((len(region), 3))) and np.all(f[1][region].any(axis=1))
    assert np.abs(f[2][len(region):]).max() > 1.0
