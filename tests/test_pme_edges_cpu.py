"""What test_pme_edges_gpu.py rests on, checked without a GPU (cases and helpers: tests/pme_edge_cases.py):
  * every mesh id takes the path it names by the rules of pme_setup_impl / remd_pme_forces, and the placements are what they claim;
  * the reference itself: the oracle's smooth PME against a direct f64 reciprocal Ewald sum over m vectors on `faces`, `outside` and
    `corner`, and under shifts by whole boxes;
  * the bounds can fail: deliberately wrong variants of the oracle's arithmetic miss the recorded force bound by at least 10 x on a named
    case of the matrix;
  * the same matrix on the f64 C++ port of the ABI (libremd_cpu.so) at test_force_groups' f64 bars."""
import math
import os

import numpy as np
import pytest
import torch

import oracle
import pme_edge_cases as pc
from oracle.forcefield import ForceFieldOracle, _bspline_moduli

CPU_LIB = os.path.join(os.path.dirname(os.path.abspath(oracle.__file__)), '_build', 'libremd_cpu.so')


# ---- the case table -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mesh', list(pc.MESHES))
def test_mesh_ids_take_the_paths_they_name(mesh):
    got = pc.mesh_path(pc.MESHES[mesh][0])
    want = pc.EXPECTED_PATH[mesh]
    assert {k: got.get(k) for k in want} == want, (mesh, got)


def test_the_matrix_walks_every_path_and_placement():
    for m in pc.MESHES:
        assert all((m, p, 'ortho') in pc.MATRIX for p in ('bulk', 'faces', 'outside'))
    for m in ('mixed', 'p64', 'slab'):
        assert {p for mm, p, b in pc.MATRIX if mm == m} == set(pc.PLACEMENTS)
    assert len(set(pc.MATRIX)) == len(pc.MATRIX) and {m for m, p, b in pc.PER_REPLICA} == {'mixed', 'p64', 'p128', 'z64', 'slab'}
    assert np.all(np.concatenate(list(pc.BOXES.values())) >= 2.1) and np.all(pc.SECOND_BOX >= 2.1)
    assert len(np.unique(pc.BOXES['per_replica'], axis=0)) == 3


def test_the_placements_are_what_they_claim():
    grid = np.array(pc.MESHES['p64'][0])
    box = pc.BOXES['ortho'][0]
    w = box / grid
    for name, fn in pc.PLACEMENTS.items():
        b = pc.BOXES['big'][0] if name == 'many' else box
        x, q = fn(np.random.default_rng(3), b, grid)
        assert len(x) == len(q) and np.all((np.abs(q) >= 0.2) & (np.abs(q) <= 0.8) | (q == 0))
        if name != 'corner' and len(x) > 1:
            d = np.concatenate([pc._min_image_dist(x[i + 1:], x[i][None], b) for i in range(len(x) - 1)])
            assert d.min() >= pc.DMIN
        x32 = x.astype(np.float32)
        if name == 'faces':
            L32 = box.astype(np.float32)
            u = x / box * grid
            on_plane = np.abs(u - np.rint(u)) < 1e-5                   # (0, L in fp32, -1e-9 and the last fp32 below L are on a plane to 1e-5 of a cell)
            mid = np.abs(u - np.floor(u) - 0.5) < 1e-9
            assert np.all((on_plane | mid).any(axis=1))
            assert (x32 == L32).any() and (x == -1e-9).any() and (x == 0).any() and (x32 == np.nextafter(L32, np.float32(0))).any()
            # what remd_pme_scaled1 makes of a tiny negative coordinate: f = 1.0f, so k = n before the callers' patch
            f = np.float32(-1e-9) / L32[0]
            assert np.float32(f - np.floor(f)) == np.float32(1.0)
        if name == 'outside':
            s = np.floor(x / box)
            assert s.min() == -3 and s.max() == 4
        if name == 'one_column':
            k = np.floor((x[:, 0] / box[0] - np.floor(x[:, 0] / box[0])) * grid[0]).astype(int)
            assert set(k) == {0, grid[0] - 1}
        if name == 'corner':
            assert np.all(np.abs(x) <= 2 * w) and (x < 0).any(axis=0).all() and (x > 0).any(axis=0).all()
        if name == 'sparse_q':
            assert np.all(q[1::2] == 0) and np.all(q[0::2] != 0)
        if name == 'pair':
            assert len(q) == 2 and q[0] == -q[1]
        if name == 'single':
            assert len(q) == 1 and q[0] != 0
        if name == 'many':
            assert len(q) > 1024


def test_the_bounds_are_four_times_the_recorded_maxima():
    rows = pc.read_error_table()
    recorded = {(w['case'], w['r']) for w in rows}
    expected = {(pc.case_id(c), r) for c in pc.MATRIX + pc.PER_REPLICA for r in range(len(pc.BOXES[c[2]]))}
    assert recorded == expected
    mx, B = pc.family_maxima(rows), pc.bounds()
    assert set(B) == {'f_max_rel', 'f_rms_rel', 'f_max_small', 'f_rms_small', 'e_abs_small', 'e_rel'}
    assert all(B[k] == 4.0 * mx[k] for k in B) and B['f_max_rel'] <= 1e-3
    assert all(v > 0 for v in mx.values())


# ---- the reference itself -----------------------------------------------------------------------------------------------------
def _direct_reciprocal(x, q, box, alpha, mmax):
    """E = 1 / (2 pi V) sum_{m != 0} exp(-pi^2 m^2 / alpha^2) / m^2 |S(m)|^2 in f64, every m with |m_k| <= mmax[k]"""
    rng = [np.arange(-k, k + 1) for k in mmax]
    m = np.stack(np.meshgrid(*rng, indexing='ij'), axis=-1).reshape(-1, 3)
    m = m[(m != 0).any(axis=1)] / box
    msq = (m * m).sum(axis=1)
    S = (q[None, :] * np.exp(2j * np.pi * (m @ x.T))).sum(axis=1)
    return pc.ONE_4PI_EPS0 / (2.0 * np.pi * box.prod()) * float((np.exp(-np.pi ** 2 * msq / alpha ** 2) / msq * np.abs(S) ** 2).sum())


@pytest.mark.parametrize('placement', ['faces', 'outside', 'corner'])
def test_the_oracle_agrees_with_a_direct_reciprocal_ewald_sum(placement):
    """order-5 smooth PME converges to the Ewald sum as the mesh gets finer: at alpha = 1.2 / nm on 72 x 96 x 125 the two agree to 1e-6"""
    box = pc.BOXES['ortho'][0]
    grid = (72, 96, 125)
    n = 6 if placement == 'corner' else 12
    x, q = pc.PLACEMENTS[placement](np.random.default_rng(5), box, np.array(pc.MESHES['mixed'][0]), n)
    desc = pc.make_desc(q, grid)
    desc['ewald_alpha'] = 1.2
    ff = ForceFieldOracle(desc)
    e_pme = float(ff.pme_reciprocal(torch.tensor(x), torch.tensor(box), torch.tensor(q)))
    # exp(-pi^2 m^2 / alpha^2) < 1e-30 beyond |m| = 3.2 / nm
    e_dir = _direct_reciprocal(x, q, box, 1.2, [int(math.ceil(3.2 * L)) for L in box])
    assert abs(e_pme - e_dir) <= 1e-6 * abs(e_dir), (e_pme, e_dir)
    # whole-box shifts, negative ones included
    s = pc.outside_shifts(np.random.default_rng(6), n)
    e_shift = float(ff.pme_reciprocal(torch.tensor(x + s * box), torch.tensor(box), torch.tensor(q)))
    assert abs(e_shift - e_pme) <= 1e-10 * abs(e_pme)
    f0 = ForceFieldOracle(pc.make_desc(q, pc.MESHES['mixed'][0])).energy_forces(x, box, classes={5})[1]
    f1 = ForceFieldOracle(pc.make_desc(q, pc.MESHES['mixed'][0])).energy_forces(x + s * box, box, classes={5})[1]
    assert np.abs(f1 - f0).max() <= 1e-10 * np.abs(f0).max()


# ---- mutants ------------------------------------------------------------------------------------------------------------------
def _bspline5(f):
    """w[j] = M5(f + j), dw[j] = M5'(f + j) for mesh index k0 - j (the recursion of oracle/forcefield._bspline_weights)"""
    a = [f, 1.0 - f] + [np.zeros_like(f)] * 3
    dw = None
    for m in range(3, 6):
        if m == 5:
            dw = [a[j] - (a[j - 1] if j > 0 else 0.0) for j in range(5)]
        a = [(((f + j) * (a[j] if j < m - 1 else 0.0) + (m - f - j) * (a[j - 1] if j > 0 else 0.0)) / (m - 1)) if j < m else np.zeros_like(f)
             for j in range(5)]
    return np.stack(a, axis=-1), np.stack(dw, axis=-1)


def _table_position(kx, ky, nx, ny, perm_r1):
    """where pme_influence_table_kernel stores G(kx, ky) for pme_xy_pow2_kernel"""
    j, hi, mm = ky & 7, ky >> 3, perm_r1 >> 3
    m, k2 = hi % mm, hi // mm
    return (m * 8 + k2) * (nx * ny // perm_r1) + kx * 8 + j


def pme_numpy(x, q, box, grid, alpha, mutant=None, table_box=None):
    """Smooth PME reciprocal forces in f64 numpy organised like the device path -- bins by mesh column, a half spectrum in z with weights
    1 / 2 / 1 on the planes, a tabulated influence function -- with one deliberate mistake when `mutant` names it."""
    n = np.array(grid)
    nx, ny, nz = grid
    nzc = nz // 2 + 1
    fr = x / box - np.floor(x / box)
    u = fr * n
    k0 = np.floor(u).astype(int)
    keep = np.ones(len(q), dtype=bool)
    if mutant == 'bin_dropped':
        keep = (k0[:, 0] % nx) != (k0[0, 0] % nx)                     # the x bin of atom 0 never reaches a workgroup
    w, dw = zip(*[_bspline5(u[:, k] - k0[:, k]) for k in range(3)])
    off = np.arange(5)
    raw = [k0[:, k, None] - off[None, :] for k in range(3)]
    idx = [np.mod(raw[k], n[k]) for k in range(3)]
    ok = np.ones((len(q), 5), dtype=bool)
    if mutant == 'stencil_not_wrapped':
        ok = raw[2] >= 0                                              # a z index that leaves the mesh is not brought back: its share is lost
    lin = (idx[0][:, :, None, None] * ny + idx[1][:, None, :, None]) * nz + idx[2][:, None, None, :]
    sel = (keep[:, None] & ok)[:, None, None, :] * np.ones((1, 5, 5, 1))
    val = q[:, None, None, None] * w[0][:, :, None, None] * w[1][:, None, :, None] * w[2][:, None, None, :] * sel
    Q = np.bincount(lin.reshape(-1), weights=val.reshape(-1), minlength=nx * ny * nz).reshape(nx, ny, nz)
    S = np.fft.fftn(Q)[:, :, :nzc]
    # the table
    tb = box if table_box is None else table_box
    fold = lambda k, nk: np.where(k <= nk // 2, k, k - nk)
    kx, ky, kz = np.arange(nx), np.arange(ny), np.arange(nzc)
    mx = (kx if mutant == 'm_not_folded' else fold(kx, nx)) / tb[0]
    my, mz = fold(ky, ny) / tb[1], kz / tb[2]
    msq = mx[:, None, None] ** 2 + my[None, :, None] ** 2 + mz[None, None, :] ** 2
    bm = [_bspline_moduli(int(nk)) for nk in grid]
    B = bm[0][:, None, None] * bm[1][None, :, None] * bm[2][None, None, :nzc]
    safe = np.where(msq > 0, msq, 1.0)
    G = np.where(msq > 0, pc.ONE_4PI_EPS0 * np.exp(-np.pi ** 2 * safe / alpha ** 2) / (np.pi * tb.prod() * safe * B), 0.0)
    if mutant == 'table_transposed':
        assert nx == ny
        G = G.transpose(1, 0, 2).copy()
    if mutant == 'table_unpermuted':
        assert nx == ny and nx in (64, 128)
        pos = _table_position(kx[:, None], ky[None, :], nx, ny, 8 if nx == 64 else 16)
        stored = np.empty((nx * ny, nzc))
        stored[pos.reshape(-1)] = G.reshape(nx * ny, nzc)
        G = stored.reshape(nx, ny, nzc)                               # read in natural order
    wt = np.full(nzc, 2.0)
    wt[0] = 1.0
    if nz % 2 == 0:
        wt[nz // 2] = 1.0
    if mutant == 'mirror_weight_1':
        wt[1] = 1.0
    if mutant == 'nyquist_weight_2':
        assert nz % 2 == 0
        wt[nz // 2] = 2.0
    A = np.fft.ifft2(G * S, axes=(0, 1)) * (nx * ny)                 # [x][y][kz]
    ph = np.exp(2j * np.pi * np.outer(kz, np.arange(nz)) / nz) * wt[:, None]
    phi = (A @ ph).real                                              # potential mesh: sum over the half spectrum with its weights
    p = phi.reshape(-1)[lin] * sel
    f = np.zeros((len(q), 3))
    wd = [[dw[0], w[1], w[2]], [w[0], dw[1], w[2]], [w[0], w[1], dw[2]]]
    for k in range(3):
        a, b, c = wd[k]
        f[:, k] = -q * keep * n[k] / box[k] * (a[:, :, None, None] * b[:, None, :, None] * c[:, None, None, :] * p).sum(axis=(1, 2, 3))
    return f


# mutant -> the case of the matrix that catches it (and the replica)
MUTANTS = {
    'other_box_table':     (('p64', 'bulk', 'per_replica'), 1),       # replica 0's box used for replica 1's influence function
    'mirror_weight_1':     (('mixed', 'bulk', 'ortho'), 0),           # weight 1 instead of 2 on a mirrored plane
    'nyquist_weight_2':    (('p64', 'bulk', 'ortho'), 0),             # the plane 2 kz == nz weighted 2
    'stencil_not_wrapped': (('mixed', 'corner', 'ortho'), 0),         # one stencil index not wrapped at the face
    'table_unpermuted':    (('p64', 'faces', 'ortho'), 0),            # the permuted table of the 64 x 64 plane read in natural order
    'table_transposed':    (('p128', 'bulk', 'ortho'), 0),            # ... or transposed in (kx, ky)
    'm_not_folded':        (('odd_z', 'outside', 'ortho'), 0),        # m1 not folded to negative frequencies
    'bin_dropped':         (('slab', 'one_column', 'ortho'), 0),      # the atoms of one x bin dropped
}


@pytest.fixture(scope='module')
def mutant_case():
    cache = {}

    def get(case, r):
        if (case, r) not in cache:
            desc, x, box = pc.build_case(case)
            f5 = ForceFieldOracle(desc).energy_forces(x[r], box[r], classes={5})[1]
            cache[case, r] = (desc, x, box, f5)
        return cache[case, r]
    return get


@pytest.mark.parametrize('mutant', [None] + list(MUTANTS))
def test_a_wrong_variant_misses_the_force_bound_tenfold(mutant_case, mutant):
    """None: the unmutated numpy path is the oracle (1e-10); every mutant is caught on its named case of the matrix"""
    case, r = MUTANTS[mutant] if mutant else (('mixed', 'faces', 'ortho'), 0)
    assert case in pc.MATRIX + pc.PER_REPLICA
    desc, x, box, f5 = mutant_case(case, r)
    f = pme_numpy(x[r], np.asarray(desc['charge']), box[r], pc.MESHES[case[0]][0], float(desc['ewald_alpha']), mutant,
                  table_box=box[0] if mutant == 'other_box_table' else None)
    scale = np.abs(f5).max()
    d = f - f5
    err, rms = np.abs(d).max() / scale, math.sqrt((d * d).sum(axis=1).mean()) / scale
    print(mutant, pc.case_id(case), err, rms)
    if mutant is None:
        assert err <= 1e-10
        for c, rr in set(MUTANTS.values()):                         # ... on every case a mutant is judged on
            dd, xx, bb, ff = mutant_case(c, rr)
            g = pme_numpy(xx[rr], np.asarray(dd['charge']), bb[rr], pc.MESHES[c[0]][0], float(dd['ewald_alpha']))
            assert np.abs(g - ff).max() <= 1e-10 * np.abs(ff).max(), c
    else:
        B = pc.bounds()
        assert err >= 10.0 * B['f_max_rel'] and rms >= 10.0 * B['f_rms_rel'], (mutant, err, rms)


# ---- the C++ port of the ABI --------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def cpu_lib():
    if not os.path.exists(CPU_LIB):
        oracle.build()
    return CPU_LIB


@pytest.mark.parametrize('case', pc.MATRIX + pc.PER_REPLICA, ids=pc.case_id)
def test_cpu_port_follows_the_oracle_on_the_matrix(cpu_lib, case):
    """(a), (b), (c) on libremd_cpu.so at test_force_groups' f64 bars: two f64 implementations of the same mesh sum (different FFTs and
    summation orders) agree to 1e-10 of max |f_ref|, and in the potential to 1e-10 of |E(classes={5})|"""
    from openmmtools_amd._engine import HipEngine
    desc, x, box = pc.build_case(case)
    eng = HipEngine(lib_path=cpu_lib)
    try:
        pc.setup_engine(eng, desc, x, box)
        f, U, xd = pc.evaluate(eng)
    finally:
        eng.close()
    assert np.array_equal(xd, x)
    for w in pc.errors(f, U, *pc.oracle_reference(desc, xd, box)):
        assert w['f_max'] <= 1e-10 * w['f_ref'] and w['f_rms'] < 1e-8 and w['e_abs'] <= 1e-10 * abs(w['e_recip']), (case, w)
