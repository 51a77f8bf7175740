"""The direct-space pair path of csrc/forces.hip (molecule order, gather, exclusion words, cluster-pair lists, nonbonded_sci_body in all its
instantiations, the scatter, and the 64-atom tile kernel) alone, against the f64 oracle on inputs built for its edges.

Cases, methods, placements and helpers: tests/pair_edge_cases.py.  Direct space sits in a force group of its own, so
get_forces(groups=...) is the pair path alone, compared with the oracle's classes={4} at the fp32 positions the engine holds; the ABI gives
no per-class energy, so the total potential is compared with the oracle's total, the bound stated relative to |E(classes={4})| and never
looser than 1e-5 of the total.
  (a) forces and (b) potential of every case: padding sizes per method, placements (faces, outside, minimal and thin boxes, blob,
      molecules), exclusion-window edges, non-zero exceptions, the LJ sub-system's own window, alchemical states, the tile kernel;
  (c) dimers: per-atom bounds inside the cutoff, exact zeros outside; (d) periodic images; (e) an exclusion span of 256 is refused;
  (f) replicas with their own boxes equal their one-replica handles bit for bit; (g) new positions and a smaller box on a live handle; an aged molecule order and a re-sort behind MD steps;
  (h) the u_kl rows of alchemical states, the soft core at 0.05 nm included.
Bounds: pair_edge_cases.bounds(family), 4 x the largest error recorded in profiles/pair_edge_errors.txt per family, capped by the suite's
bars (2e-4 of max |f_ref| for Lennard-Jones and the reaction field, 1e-3 under Ewald)."""
import numpy as np
import pytest

import pair_edge_cases as pc

pytestmark = pytest.mark.gpu


def _run(make, cid, case, x=None, box=None):
    eng = pc.make_engine(make, cid)
    try:
        pc.setup_engine(eng, case, x, box)
        return pc.evaluate(eng)
    finally:
        eng.close()


@pytest.fixture(scope='module')
def results(hip_engine_factory):
    """case id -> (case, engine forces, potential, u_kl rows, fp32 positions, oracle class-4 forces, class-4 energy, total), evaluated once"""
    cache = {}

    def get(cid):
        if cid not in cache:
            case = pc.build_case(cid)
            f, U, rows, xd = _run(hip_engine_factory, cid, case)
            cache[cid] = (case, f, U, rows, xd) + pc.oracle_reference(case, xd)
        return cache[cid]
    return get


def _check_forces(cid, case, f, f4, factor=1.0, what=''):
    B = pc.bounds(pc.case_family(cid))
    cid = cid + what
    assert np.all(np.isfinite(f))
    for r, w in enumerate(pc.errors(case, f, np.zeros(len(f)), f4, np.ones(len(f)), np.ones(len(f)))):
        print('%s r%d max|f_ref| %.5e max|df| rel %.4e rms rel %.4e (bounds %.3e %.3e)' % (cid, r, w['f_ref'], w['f_max_rel'], w['f_rms_rel'],
                                                                                       B['f_max_rel'], B['f_rms_rel']))
        assert w['f_ref'] > 1.0
        assert w['f_max_rel'] <= factor * B['f_max_rel'] and w['f_rms_rel'] <= factor * B['f_rms_rel'], (cid, r, w)


@pytest.mark.parametrize('cid', pc.ALL_CASES)
def test_direct_space_forces_follow_the_oracle(results, cid):
    """(a): the direct-space force group against the oracle's class 4, per replica"""
    case, f, U, rows, xd, f4, e4, et = results(cid)
    _check_forces(cid, case, f, f4)


@pytest.mark.parametrize('cid', pc.ALL_CASES)
def test_total_potential_follows_the_oracle(results, cid):
    """(b): the total potential against the oracle's, the bound relative to the oracle's direct-space energy |E(classes={4})| and never
    looser than 1e-5 of the total"""
    case, f, U, rows, xd, f4, e4, et = results(cid)
    B = pc.bounds(pc.case_family(cid))
    for r in range(len(U)):
        de = abs(U[r] - et[r])
        print('%s r%d U %.10e ref %.10e dE %.4e E_direct %.8e dE/|E_direct| %.4e' % (cid, r, U[r], et[r], de, e4[r], de / abs(e4[r])))
        assert np.isfinite(U[r])
        assert de <= min(B['e_rel'] * abs(e4[r]), B['e_tot_rel'] * abs(et[r])), (cid, r, U[r], et[r], e4[r])


@pytest.mark.parametrize('cid', pc.DIMER_CASES)
def test_dimers_per_atom(results, cid):
    """(c): every atom has exactly one partner.  Atoms of pairs inside the (method's longest) cutoff -- at 0.25, 0.4 and (1 - 1e-3) of each
    cutoff radius, half of them across a box face -- are held per atom to bound x |f_ref of that atom|; atoms of pairs at (1 + 1e-3) of the
    cutoff get exactly zero.  A list that drops a cluster pair at the rim of its bounding-box test, or a cutoff mask off by one comparison,
    shows here.  On the split methods two pairs in five carry Lennard-Jones on both atoms, at every separation, so the LJ sub-system's own
    list and rc2 mask are probed too."""
    case, f, U, rows, xd, f4, e4, et = results(cid)
    B = pc.bounds(pc.case_family(cid))
    ins, out = np.array(case['inside']).reshape(-1), np.array(case['outside']).reshape(-1)
    rel = np.linalg.norm(f[0][ins] - f4[0][ins], axis=1) / np.linalg.norm(f4[0][ins], axis=1)
    print('%s per-atom |df| / |f_ref,i|: max %.4e (bound %.3e); smallest |f_ref,i| %.4e' % (cid, rel.max(), B['f_atom_rel'],
                                                                                          np.linalg.norm(f4[0][ins], axis=1).min()))
    assert np.all(np.linalg.norm(f4[0][ins], axis=1) > 0)
    assert rel.max() <= B['f_atom_rel'], (cid, ins[rel.argmax()], rel.max())
    assert np.array_equal(f4[0][out], np.zeros((len(out), 3)))
    assert np.array_equal(f[0][out], np.zeros((len(out), 3))), (cid, out[np.abs(f[0][out]).max(axis=1) > 0])


@pytest.mark.parametrize('cid', pc.OUTSIDE_CASES)
def test_periodic_images_give_the_same_forces(hip_engine_factory, results, cid):
    """(d): atoms shifted by -3 ... +3 whole boxes against their wrapped parents: the same forces within twice the force bound (the fp32
    rounding of x differs, and the molecule order may: within the bound, not bit for bit)"""
    case, f_out, U, rows, xd, f4, e4, et = results(cid)
    xp = case['parent']
    assert np.abs(case['x'] - xp).max() >= 2.0 * case['box'].min() and (case['x'] - xp).min() < 0
    f_par = _run(hip_engine_factory, cid, case, x=xp)[0]
    B = pc.bounds(pc.case_family(cid))
    d = f_out[0] - f_par[0]
    scale = np.abs(f4).max()
    print('%s max|df| %.4e rms %.4e scale %.5e' % (cid, np.abs(d).max(), np.sqrt((d * d).sum(axis=1).mean()), scale))
    assert np.abs(d).max() <= 2.0 * B['f_max_rel'] * scale
    assert np.sqrt((d * d).sum(axis=1).mean()) <= 2.0 * B['f_rms_rel'] * scale


def test_an_exclusion_span_of_256_is_refused(hip_engine_factory):
    """(e): words = 9 > MAX_EXCL_WORDS"""
    q = np.zeros(300)
    desc = pc.make_desc('lj', q, np.array([2.5, 2.6, 2.7]), exceptions=[(0, 256, 0.0, 0.1, 0.0)])
    assert pc.build_rules(desc)['refused']
    eng = hip_engine_factory()
    try:
        with pytest.raises(RuntimeError, match='exclusions span more than 255 atom indices'):
            eng.set_system(desc)
    finally:
        eng.close()


@pytest.mark.parametrize('cid', pc.REPLICA_CASES)
def test_replicas_equal_their_single_replica_handles(hip_engine_factory, results, cid):
    """(f): replica r of the R = 3 handle with three different boxes equals, bit for bit in forces and potential, an R = 1 handle with its
    box and positions: the slices' fp32 partial sums are a property of the system (sci_split, remd_build_nonbonded), not of R, the
    forces are 64-bit fixed-point sums, and the cells of the molecule order come from the first replica's box in both (the three
    boxes' longest edges give the same number of Hilbert bits)"""
    case, f3, U3, rows, xd3, f4, e4, et = results(cid)
    assert np.any(f3[0] != f3[1]) and np.any(f3[1] != f3[2])
    for r in range(3):
        f1, U1, rows1, xd1 = _run(hip_engine_factory, cid, case, x=case['x'][r:r + 1], box=case['box'][r:r + 1])
        assert np.array_equal(xd1[0], xd3[r])
        assert np.array_equal(f1[0], f3[r]), (cid, r, np.abs(f1[0] - f3[r]).max())
        assert U1[0] == U3[r], (cid, r, U1[0], U3[r])


@pytest.mark.parametrize('method', ['lj', 'pme_split'])
@pytest.mark.parametrize('shrink', [1.0, 0.9])
def test_new_positions_on_a_live_handle_follow_the_oracle(hip_engine_factory, method, shrink):
    """(g): evaluate, then set_replicas with the same atoms placed anew (another seed; the same box, or one 10 % smaller with its own
    placement), then evaluate again.  set_replicas invalidates the molecule order (remd_nb_invalidate_sort), so this holds that a live
    handle sorts, lists and sizes everything again for new positions and a new box -- not a stale order; that is the next test"""
    cid = 'size-%s-200' % method if method == 'lj' else 'size-%s-129' % method
    case = pc.build_case(cid)
    n = case['x'].shape[1]
    box2 = case['box'] * shrink
    rng = np.random.default_rng(pc.case_seed(cid) ^ 0x77)
    assert n / box2[0].prod() < 32.0 and np.all(box2 > 2.0 * pc.longest_cutoff(method))
    x2 = pc.fresh_positions(case, rng, box2[0])[None]
    eng = pc.make_engine(hip_engine_factory, cid)
    try:
        pc.setup_engine(eng, case)
        f_a = pc.evaluate(eng)[0]
        eng.set_replicas(1, 0, x2, None, box2, np.zeros(1, dtype=np.int64))
        f_b, U_b, rows, xd = pc.evaluate(eng)
    finally:
        eng.close()
    assert np.any(f_a != f_b)
    f4, e4, et = pc.oracle_reference(case, xd, box2)
    _check_forces(cid, case, f_b, f4)
    B = pc.bounds(pc.case_family(cid))
    assert abs(U_b[0] - et[0]) <= min(B['e_rel'] * abs(e4[0]), B['e_tot_rel'] * abs(et[0])), (U_b[0], et[0], e4[0])


@pytest.mark.parametrize('cid', pc.LIVE_CASES)
@pytest.mark.parametrize('steps', pc.AGED_STEPS)
def test_an_aged_molecule_order_follows_the_oracle(hip_engine_factory, cid, steps):
    """(g): the atoms move by MD steps on the handle (pair_edge_cases.aged_order_run), not by set_replicas: a propagation sorts the
    molecules at its first force evaluation and then every 40th (resort_interval), and get_forces never invalidates the order.
      steps = 20: get_forces behind the run works on an order about 20 evaluations old -- lists, tile ranking and exclusion words of
        positions the atoms have left; 25 more get_forces calls at the same positions carry the evaluation count across the interval, so a
        re-sort falls among them; the first and the last follow the oracle;
      steps = 45: the re-sort fell inside the run, with atoms that had moved for 40 steps.
    The age is known from the counting rule in ensure_sorted, not observed: the ABI does not show it."""
    case = pc.build_case(cid)
    eng = pc.make_engine(hip_engine_factory, cid)
    try:
        got, moved = pc.aged_order_run(eng, case, steps)
    finally:
        eng.close()
    print(cid, steps, 'largest displacement %.4f nm' % moved)
    assert moved > 0.005
    for what, (f, xd) in got.items():
        _check_forces(cid, case, f, pc.oracle_reference(case, xd)[0], what=' %d steps, %s' % (steps, what))


@pytest.mark.parametrize('cid', pc.UKL_CASES)
def test_alchemical_rows_follow_the_oracle(results, cid):
    """(h): the u_kl rows of compute_energies against the oracle's potential of every replica's configuration at every state, at the
    suite's 1e-5 relative bar.  softcore-*: an alchemical atom 0.05 nm from a non-alchemical one at lambda_sterics 0.5 and 0 -- the soft
    core is finite where plain Lennard-Jones would overflow; forces and energies are finite and follow the oracle (a), (b)"""
    case, f, U, rows, xd, f4, e4, et = results(cid)
    ref = pc.oracle_rows(case, xd)
    assert rows.shape == ref.shape and np.all(np.isfinite(rows)) and np.all(np.isfinite(f))
    print(cid, np.abs(rows - ref).max(), np.abs(rows / ref - 1.0).max())
    assert np.allclose(rows, ref, rtol=1e-5, atol=0.0), (cid, rows, ref)
    if cid.startswith('softcore'):
        hub, partner = case['hub'], case['partner']
        assert abs(np.linalg.norm(xd[0][hub] - xd[0][partner]) - 0.05) < 1e-6
        assert np.abs(f4[:, [hub, partner]]).max() > 0
