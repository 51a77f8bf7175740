"""What test_pair_edges_gpu.py rests on, checked without a GPU (cases and helpers: tests/pair_edge_cases.py):
  * every method id is built into the kernel family it names by the rules of remd_build_nonbonded, and every case has what its id claims
    (sizes, NL, exclusion words, groups in the merged order, box, the dimers' pairs), keeps the minimum distance and stays out of the
    cutoff bands -- in f64 on the positions rounded to fp32, on the reference alone;
  * the bounds are 4 x the recorded maxima, capped by the suite's bars, and every case id of the GPU tests is recorded;
  * the bounds can see one wrong pair: on the oracle, a removed or an added exclusion moves some atom's force by more than 10 x the bound;
  * the same cases on the f64 C++ port of the ABI (libremd_cpu.so) at test_force_groups' f64 bars."""
import os

import numpy as np
import pytest

import oracle
import pair_edge_cases as pc
from oracle.forcefield import ForceFieldOracle

CPU_LIB = os.path.join(os.path.dirname(os.path.abspath(oracle.__file__)), '_build', 'libremd_cpu.so')


# ---- the case table -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('method', list(pc.METHODS))
def test_method_ids_take_the_paths_they_name(method):
    """t.method, lj_split (any_charge && NL > 0 && NL * 10 <= N * 6) and rcc2 as remd_build_nonbonded sets them, at every size of the method"""
    for n in pc.SIZES[method]:
        case = pc.build_case('size-%s-%d' % (method, n))
        got = pc.build_rules(case['desc'])
        want = dict(pc.EXPECTED_RULES[method], rcc=pc.longest_cutoff(method))
        assert {k: got[k] for k in want} == want, (method, n, got)
        pme, charges, every, switch, rcc, _ = pc.METHODS[method]
        d = case['desc']
        assert d['nb_method'] == (2 if pme else 1) and bool(np.any(d['charge'] != 0)) == charges
        assert d['switch_distance'] == (switch if switch is not None else -1.0) and d['cutoff'] == pc.CUTOFF
        assert got['NL'] == (n if every == 1 else (n + 2) // 3)
        assert ('coulomb_cutoff' in d) == (rcc is not None)


def test_the_sizes_are_the_padding_edges():
    for m in ('lj', 'pme_split'):
        assert set(pc.ALL_SIZES) <= set(pc.SIZES[m])
    for m in pc.METHODS:
        assert set(pc.FEW_SIZES) <= set(pc.SIZES[m])
    # one mixed real / padding cluster, none at all, a tile with one real atom and seven parked clusters
    assert {n % 8 for n in pc.ALL_SIZES} >= {0, 1, 7} and {n % 64 for n in pc.ALL_SIZES} >= {0, 1, 63}
    for m in ('rf_split', 'pme_split', 'pme_far'):
        assert {(n + 2) // 3 for n in pc.SIZES[m]} >= {1, 8, 9, 64, 65}
    assert max(c['x'].shape[1] for c in map(pc.build_case, pc.CASES)) <= 330 and max(len(c['x']) for c in map(pc.build_case, pc.CASES)) <= 3


@pytest.mark.parametrize('cid', list(pc.CASES))
def test_every_case_is_what_it_claims(cid):
    case = pc.build_case(cid)
    method, desc, claims = case['method'], case['desc'], case['claims']
    rules = pc.build_rules(desc)
    want = dict(pc.EXPECTED_RULES[method], rcc=pc.longest_cutoff(method))
    assert {k: rules[k] for k in want} == want and not rules['refused']
    for k in ('N', 'NL', 'words', 'excl_W', 'lj_words', 'groups'):
        if k in claims:
            assert rules[k] == claims[k], (cid, k, rules[k], claims[k])
    if 'n_mod_8' in claims:
        assert (rules['N'] % 8, rules['N'] % 64) == (claims['n_mod_8'], claims['n_mod_64'])
    assert 'excl_W' not in claims or claims['excl_W'] in (5, 9, 13, 17, 29, 33)
    excluded = {(min(i, j), max(i, j)) for i, j in np.asarray(desc['exception_atoms']).reshape(-1, 2)}
    rl = pc.longest_cutoff(method)
    for r in range(len(case['x'])):
        box = case['box'][r]
        assert np.all(box > 2.0 * rl), (cid, box)
        dist = pc.pair_distances(case['x'][r], box)
        iu = np.triu_indices(len(dist), 1)
        free = np.array([(i, j) not in excluded for i, j in zip(*iu)])
        if 'partner' in case and not excluded:
            free &= ~((iu[0] == case['hub']) & (iu[1] == case['partner']))          # softcore: the planted pair at 0.05 nm interacts
        # minimum distance of interacting pairs (chain neighbours and planted partners are excluded from each other)
        assert dist[iu][free].min() >= pc.DMIN - 1e-6, (cid, r, dist[iu][free].min())
        # no interacting pair within BAND x cutoff of a cutoff radius, but the planted dimers
        bad = pc.in_band(case['x'][r], box, sorted({pc.CUTOFF, rl}), exempt=case['exempt'])
        assert len(bad) == 0, (cid, r, bad)
    if cid.startswith('min_box'):
        assert int((case['box'][0] == 2.0 * pc.CUTOFF + 1e-3).sum()) == claims['min_edges']
    if cid.startswith('thin'):
        assert np.array_equal(case['box'][0], [1.25, 1.25, 6.0])
    if cid.startswith('outside'):
        s = np.rint((case['x'] - case['parent']) / case['box'][:, None, :])
        assert s.min() == -3 and s.max() == 3 and np.all((case['parent'] > -0.5) & (case['parent'] < case['box'][:, None, :]))
    if cid.startswith('faces'):
        x, box = case['x'][0], case['box'][0]
        x32, L32 = x.astype(np.float32), box.astype(np.float32)
        special = (x == 0) | (x32 == L32) | (x32 == np.nextafter(L32, np.float32(0))) | (x == -1e-7 * box) | (x == -1e-9 * box)
        assert special.any(axis=1).sum() >= len(x) // 3 and special.all(axis=1).sum() == 1 and (special.sum(axis=1) == 2).sum() >= 3
        for k in range(3):
            assert all((x[:, k] == v).any() or (x32[:, k] == np.float32(v)).any() for v in pc.face_values(box[k])), (cid, k)
        # frac() of gather_positions_body: v / L - floorf(v / L) in fp32 is 1.0 at -1e-9 L and stays below 1 at -1e-7 L
        f9, f7 = np.float32(-1e-9 * box[0]) / L32[0], np.float32(-1e-7 * box[0]) / L32[0]
        assert np.float32(f9 - np.floor(f9)) == np.float32(1.0) and np.float32(f7 - np.floor(f7)) < np.float32(1.0)
        # partners across the faces: pairs within the cutoff whose minimum image is not the direct one
        d = x[:, None, :] - x[None, :, :]
        assert ((np.abs(np.rint(d / box)).sum(-1) > 0) & (pc.pair_distances(x, box) < pc.CUTOFF)).sum() > 50
    if cid.startswith('blob'):
        dist = pc.pair_distances(case['x'][0], case['box'][0])
        n = len(dist)
        # (64 atoms at the minimum distance do not fit a ball of one cutoff: the ball is 1.55 nm wide, dense enough that every cluster has
        # neighbours in every other; the eight far atoms see each other only)
        assert dist[:n - 8, :n - 8].max() < 1.55 and dist[n - 8:, :n - 8].min() > pc.CUTOFF and dist[n - 8:, n - 8:].max() < pc.CUTOFF * 1.3
    if cid.startswith('molecules'):
        assert max(claims['groups']) > 64 and sorted(set(claims['groups'])) == [1, 3, 5, 9, 33, 65, 130]
        first = np.cumsum([0] + claims['groups'][:-1])
        assert any(a % 8 and (a + s - 1) // 8 > a // 8 for a, s in zip(first, claims['groups'])) and any((a + s - 1) // 64 > a // 64 for a, s in zip(first, claims['groups']))
    if cid.startswith('dimers'):
        dist = pc.pair_distances(case['x'][0], case['box'][0])
        pairs = case['inside'] + case['outside']
        assert len(case['inside']) == claims['pairs_inside'] and len(case['outside']) == claims['pairs_outside'] and len(case['outside']) >= 5
        near = (dist < rl + 0.3).sum(axis=1) - 1                          # partners within cutoff + 0.3 nm: exactly one
        assert np.all(near == 1) and all(dist[i, j] < rl + 0.3 for i, j in pairs)
        assert all(dist[i, j] < rl for i, j in case['inside']) and all(dist[i, j] > rl for i, j in case['outside'])
        seps = sorted({round(float(dist[i, j]), 5) for i, j in pairs})
        want = sorted({0.25, 0.4} | {round(rc * (1 + s * 1e-3), 5) for rc in {pc.CUTOFF, rl} for s in (-1, 1)})
        assert np.allclose(seps, want, atol=2e-5), (seps, want)
        x = case['x'][0]
        straddle = sum(1 for i, j in pairs if np.any(np.floor(x[i] / case['box'][0]) != np.floor(x[j] / case['box'][0])))
        assert straddle >= len(pairs) // 2
        if pc.METHODS[method][2] == 3:
            # both atoms with Lennard-Jones: pairs at every separation
            eps = np.asarray(desc['epsilon'])
            assert all((eps[i] != 0) == (eps[j] != 0) for i, j in pairs)
            assert {round(float(dist[i, j]), 5) for i, j in case['lj_pairs']} == {round(float(dist[i, j]), 5) for i, j in pairs}
    if 'plants' in case:
        # every excluded partner 0.1 nm from its hub; its neighbours (index, and LJ-ordinal where named) not excluded, 0.3 nm from the hub
        dist = pc.pair_distances(case['x'][0], case['box'][0])
        assert excluded == {(h, p) for h, p, nb in case['plants']}
        hubs_partners = {a for h, p, nb in case['plants'] for a in (h, p)}
        for h, p, nb in case['plants']:
            assert abs(dist[h, p] - 0.1) < 1e-6
            for k in nb:
                if 0 <= k < len(dist) and k not in hubs_partners:
                    assert abs(dist[h, k] - 0.3) < 1e-6 and (min(h, k), max(h, k)) not in excluded, (cid, h, k)
    if cid.startswith('ljord'):
        eps = np.asarray(desc['epsilon'])
        both = [(h, p) for h, p, nb in case['plants'] if eps[h] != 0 and eps[p] != 0]
        assert both and {(p - h) // 3 for h, p in both} == ({32} if cid.endswith('-a') else {20})
        assert all(eps[k] != 0 for h, p in both for k in (p - 3, p + 3))
    if cid.startswith('exc14'):
        dist = pc.pair_distances(case['x'][0], case['box'][0])
        x, box = case['x'][0], case['box'][0]
        for i, j in claims['exc14']:
            assert dist[i, j] > pc.CUTOFF + 0.1 and abs(i - j) in (3, 40)
            if claims['across']:
                assert np.floor(x[i][0] / box[0]) != np.floor(x[j][0] / box[0])
        assert np.all(np.asarray(desc['exception_params']).reshape(-1, 3)[:, [0, 2]] != 0)
    if case['lam'] is not None:
        assert len(case['lam'][0]) == len(case['x']) and list(desc['alch_atoms']) == list(range(claims['N'] // 3))


def test_the_lists_of_the_gpu_tests_are_cases_held_here():
    """test_pair_edges_gpu.py parametrizes over these lists alone; every id is a case of the table (held above) or its +tiles twin"""
    for ids in (pc.ALL_CASES, pc.DIMER_CASES, pc.OUTSIDE_CASES, pc.REPLICA_CASES, pc.LIVE_CASES, pc.UKL_CASES, pc.EXCL_CASES):
        assert ids and all(c.split('+')[0] in pc.CASES for c in ids)
    assert set(pc.DIMER_CASES + pc.OUTSIDE_CASES + pc.REPLICA_CASES + pc.LIVE_CASES + list(pc.UKL_CASES) + pc.EXCL_CASES) <= set(pc.ALL_CASES)
    for m in pc.METHODS:
        assert 'size-%s-129+tiles' % m in pc.ALL_CASES and 'outside-%s' % m in pc.OUTSIDE_CASES
    assert {pc.build_method(c) for c in pc.DIMER_CASES} == set(pc.DIMER_METHODS)
    assert 'size-lj-200' in pc.CASES and 'size-pme_split-129' in pc.CASES            # the live-handle test's systems
    # the propagated cases stay off the resident small-system kernel (it takes Lennard-Jones systems without exceptions only)
    assert all(len(pc.build_case(c)['desc']['exception_atoms']) > 0 for c in pc.LIVE_CASES) and min(pc.AGED_STEPS) < 40 < max(pc.AGED_STEPS)
    # the exclusion family: 1, 2, 3, 7 and 8 words, the window's start on every lane offset
    for m in ('lj', 'pme_split'):
        assert {pc.build_case('excl-%s-d%d' % (m, d))['claims']['excl_W'] for d in pc.EXCL_D} == {5, 9, 13, 29, 33}
        assert all('excl-%s-d65-o%d' % (m, o) in pc.CASES for o in range(1, 8))


def test_the_bounds_are_four_times_the_recorded_maxima():
    rows = pc.read_error_table()
    recorded = {(w['case'], w['r']) for w in rows}
    expected = {(c, r) for c in pc.ALL_CASES for r in range(len(pc.build_case(c)['x']))}
    assert recorded == expected
    mx = pc.family_maxima(rows)
    assert set(mx) == set(pc.BARS)
    for fam, bar in pc.BARS.items():
        B = pc.bounds(fam)
        for k in ('f_max_rel', 'f_rms_rel', 'f_atom_rel'):
            assert B[k] == min(4.0 * mx[fam][k], bar) and 0 < mx[fam][k] <= bar, (fam, k, mx[fam][k])
        assert B['e_rel'] == 4.0 * mx[fam]['e_rel'] and B['e_tot_rel'] == 1e-5 and mx[fam]['e_tot_rel'] <= 1e-5


# ---- sensitivity --------------------------------------------------------------------------------------------------------------
def _class4(desc, x, box):
    return ForceFieldOracle(desc).energy_forces(x, box, classes={4})[1]


def _with_exceptions(desc, pairs):
    d = dict(desc)
    d['exception_atoms'] = np.array([p[:2] for p in pairs], dtype=np.int32).reshape(-1, 2)
    d['exception_params'] = np.array([p[2:] for p in pairs], dtype=np.float64).reshape(-1, 3)
    return d


@pytest.mark.parametrize('cid', pc.EXCL_CASES + ['dimers-%s' % m for m in pc.DIMER_METHODS])
def test_one_wrong_pair_misses_the_force_bound_tenfold(cid):
    """on the oracle alone, for every case of the exclusion family: each exception removed in turn (a missed exclusion: a pair at 0.1 nm
    interacts; a lost 1-4 term), and one exclusion added per plant (a spurious one: a neighbour of the partner at 0.3 nm loses its pair;
    without plants, the closest interacting pair) each move some atom's force by more than 10 x the force bound.  For the dimers: an
    exclusion added to any pair inside the cutoff moves its atoms by more than 10 x the per-atom bound"""
    case = pc.build_case(cid)
    desc, x, box = case['desc'], case['x'][0], case['box'][0]
    B = pc.bounds(pc.case_family(cid))
    f0 = _class4(desc, x, box)
    scale = np.abs(f0).max()
    have = [tuple(a) + tuple(p) for a, p in zip(np.asarray(desc['exception_atoms']).reshape(-1, 2).tolist(),
                                                np.asarray(desc['exception_params']).reshape(-1, 3).tolist())]
    if cid.startswith('dimers'):
        for i, j in case['inside']:
            f1 = _class4(_with_exceptions(desc, [(i, j, 0.0, 0.1, 0.0)]), x, box)
            assert np.linalg.norm(f1[i] - f0[i]) > 10.0 * B['f_atom_rel'] * np.linalg.norm(f0[i]), (cid, i, j)
        return
    for k in range(len(have)):
        missed = _class4(_with_exceptions(desc, have[:k] + have[k + 1:]), x, box)
        assert np.abs(missed - f0).max() > (1000.0 if 'plants' in case else 10.0) * B['f_max_rel'] * scale, (cid, have[k])
    if 'plants' in case:
        n = len(x)
        taken = {a for h, p, nb in case['plants'] for a in (h, p)}
        free = [(h, [k for k in nb if 0 <= k < n and k not in taken]) for h, p, nb in case['plants']]
        added = [(h, ks[0]) for h, ks in free if ks]          # (interleaved: both neighbours of partner 2 are planted atoms themselves)
        assert len(added) >= len(free) - 1
    else:
        dist = pc.pair_distances(x, box) + 10.0 * np.eye(len(x))
        for i, j in np.asarray(desc['exception_atoms']).reshape(-1, 2):
            dist[i, j] = dist[j, i] = 10.0
        added = [np.unravel_index(dist.argmin(), dist.shape)]
    for h, k in added:
        spurious = _class4(_with_exceptions(desc, have + [(int(h), int(k), 0.0, 0.1, 0.0)]), x, box)
        assert np.abs(spurious - f0).max() > 10.0 * B['f_max_rel'] * scale, (cid, h, k, np.abs(spurious - f0).max() / scale)


# ---- the C++ port of the ABI --------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def cpu_lib():
    if not os.path.exists(CPU_LIB):
        oracle.build()
    return CPU_LIB


@pytest.mark.parametrize('cid', pc.ALL_CASES)
def test_cpu_port_follows_the_oracle(cpu_lib, cid):
    """every case on libremd_cpu.so: two f64 implementations of the same sums agree to 1e-10 of max |f_ref| and of |E(classes={4})|, per atom
    on the dimers, with exact zeros outside the cutoff; the u_kl rows to 1e-10"""
    from openmmtools_amd._engine import HipEngine
    case = pc.build_case(cid)
    eng = pc.make_engine(lambda: HipEngine(lib_path=cpu_lib), cid)
    try:
        pc.setup_engine(eng, case)
        f, U, rows, xd = pc.evaluate(eng)
    finally:
        eng.close()
    assert np.array_equal(xd, case['x'])
    for w in pc.errors(case, f, U, *pc.oracle_reference(case, xd)):
        assert w['f_max_rel'] <= 1e-10 and w['f_atom_rel'] <= 1e-10 and w['e_rel'] <= 1e-10, (cid, w)
    if case.get('outside'):
        out = np.array(case['outside']).reshape(-1)
        assert np.array_equal(f[0][out], np.zeros((len(out), 3)))
    if cid in pc.UKL_CASES:
        assert np.allclose(rows, pc.oracle_rows(case, xd), rtol=1e-10, atol=0.0)


@pytest.mark.parametrize('cid', pc.LIVE_CASES)
@pytest.mark.parametrize('steps', pc.AGED_STEPS)
def test_cpu_port_behind_md_steps(cpu_lib, cid, steps):
    """the live-handle run of test_an_aged_molecule_order_follows_the_oracle on the f64 port: the atoms move, and the group's forces at the
    positions they reach follow the oracle"""
    from openmmtools_amd._engine import HipEngine
    case = pc.build_case(cid)
    eng = HipEngine(lib_path=cpu_lib)
    try:
        got, moved = pc.aged_order_run(eng, case, steps)
    finally:
        eng.close()
    assert moved > 0.005
    for f, xd in got.values():
        f4 = pc.oracle_reference(case, xd)[0]
        assert np.abs(f - f4).max() <= 1e-10 * np.abs(f4).max()
