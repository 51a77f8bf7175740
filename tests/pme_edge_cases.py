"""Cases and helpers of the PME reciprocal-space edge tests (test_pme_edges_gpu.py, test_pme_edges_cpu.py).

Systems: N point charges (epsilon = 0, no bonded terms, no constraints, no exceptions) in an orthorhombic periodic box under PME, built
with the package's own System / NonbondedForce / system_to_desc; the mesh of the description is then overwritten (any mesh is a legal
choice because the f64 oracle, oracle/forcefield.py, runs on the same mesh).  Cutoff 1 nm and the Ewald alpha that follows from it are
the same everywhere, as is the minimum pair distance of 0.25 nm that keeps the direct-space part tame (not under test).

MESHES: one id per code path of csrc/pme.hip; `mesh_path` restates the rules of pme_setup_impl / remd_pme_forces that choose the path,
and test_pme_edges_cpu.py holds every id to the path it names.
PLACEMENTS: functions (rng, box, grid) -> (x [N][3], q [N]).
bounds(): 4 x the largest error recorded on the MI355X in each family (profiles/pme_edge_errors.txt, tools/record_pme_edge_errors.py).
"""
import math
import os
import zlib

import numpy as np

from openmmtools_amd.system import System, NonbondedForce, system_to_desc
from oracle.md_oracle import ONE_4PI_EPS0

KB = 0.008314462618153242
BETA = 1.0 / (KB * 300.0)
CUTOFF = 1.0
DMIN = 0.25
RECIP_GROUP = 1                         # reciprocal space in force group 1, everything else in group 0
FORCE_GROUPS = [0, 0, 0, 0, 0, RECIP_GROUP]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERROR_TABLE = os.path.join(ROOT, 'profiles', 'pme_edge_errors.txt')

# ---- mesh paths -------------------------------------------------------------------------------------------------------------
# id -> (mesh, the path meant).  long_y: the issue's 6 x 256 x 7 keeps a whole row in one workgroup (nl = ny = 256), so nz = 25 replaces
# it: 256 lines of 25 points outgrow 12 points x 512 threads and the row splits into two workgroups of nl = 128 lines.
MESHES = {
    'min':      ((6, 6, 6),      'pme_xy_fused_kernel; five of the six x bins per row, every stencil wraps; z packed, M = 3'),
    'mixed':    ((30, 36, 10),   'pme_xy_fused_kernel, radices 2 3 5 and 4 3 3; z packed, M = 5'),
    'odd_z':    ((45, 20, 9),    'pme_xy_fused_kernel; odd nz: full-length z transform'),
    'long_y':   ((6, 256, 25),   'pme_xy_fused_kernel with the longest line; full-length z at 512 threads, nl = 128 < ny (REPLACES 6 x 256 x 7)'),
    'p64':      ((64, 64, 6),    'pme_xy_pow2_kernel<64> (512 threads, table permuted by 8); z packed, M = 3'),
    'p64_odd':  ((64, 64, 9),    'pme_xy_pow2_kernel<64> behind odd nz'),
    'p128':     ((128, 128, 8),  'pme_xy_pow2_kernel<128> (1024 threads, table permuted by 16); z packed, M = 4'),
    'z64':      ((6, 64, 64),    'pme_spread_zfwd_pow2_kernel<32, 4> / pme_zinv_gather_pow2_kernel<32, 4> (256 threads) behind a scheduled plane'),
    'z128':     ((6, 128, 128),  'pme_spread_zfwd_pow2_kernel<64, 8> / pme_zinv_gather_pow2_kernel<64, 8> (512 threads), two workgroups per mesh row'),
    'slab':     ((144, 144, 6),  'pme_y_slab_kernel + pme_x_fused_kernel (slabs of 24)'),
    'slab_ns':  ((160, 135, 9),  'pme_y_slab_kernel + pme_x_fused_kernel, non-square (slabs of 20 rows / 15 columns), odd nz'),
    'slab_max': ((256, 256, 6),  'pme_y_slab_kernel + pme_x_fused_kernel on the largest plane the setup accepts (slabs of 8)'),
}
# what mesh_path must say of each id
EXPECTED_PATH = {
    'min':      dict(plane='sched', z='packed', M=3),
    'mixed':    dict(plane='sched', z='packed', M=5, radix_x=[2, 3, 5], radix_y=[4, 3, 3]),
    'odd_z':    dict(plane='sched', z='full', M=9),
    'long_y':   dict(plane='sched', z='full', M=25, nl=128, zt=512),
    'p64':      dict(plane='pow2_64', z='packed', M=3),
    'p64_odd':  dict(plane='pow2_64', z='full', M=9),
    'p128':     dict(plane='pow2_128', z='packed', M=4),
    'z64':      dict(plane='sched', z='pow2_64', M=32, nl=64, zt=256, z_groups_per_row=1),
    'z128':     dict(plane='sched', z='pow2_128', M=64, nl=64, zt=512, z_groups_per_row=2),
    'slab':     dict(plane='slab', z='packed', M=3, xs_sw=24, ys_sh=24),
    'slab_ns':  dict(plane='slab', z='full', M=9, xs_sw=15, ys_sh=20),
    'slab_max': dict(plane='slab', z='packed', M=3, xs_sw=8, ys_sh=8),
}
XY_PPT, XS_THREADS, Z_PPT = 15, 256, 12         # csrc/pme.hip


def _factorize(n):
    """pme.hip factorize: the power of two in ceil(e / 3) stages of radix 8 / 4 / 2, then 3s, then 5s"""
    radix, m, e = [], n, 0
    while m % 2 == 0:
        e, m = e + 1, m // 2
    st, left = (e + 2) // 3, e
    for k in range(st):
        b = (left + (st - k) - 1) // (st - k)
        radix.append(1 << b)
        left -= b
    for p in (3, 5):
        while m % p == 0:
            radix.append(p)
            m //= p
    return radix if m == 1 and len(radix) <= 8 else None


def mesh_path(grid):
    """The kernels a mesh runs on, from the rules of pme_setup_impl and remd_pme_forces (default switches)."""
    nx, ny, nz = (int(g) for g in grid)
    rad = [_factorize(n) for n in (nx, ny, nz)]
    assert all(6 <= n <= 256 for n in (nx, ny, nz)) and all(r is not None for r in rad), 'PME mesh sizes must be products of 2, 3, 5 between 6 and 256'
    half = nz % 2 == 0 and nz // 2 >= 3 and _factorize(nz // 2) is not None
    out = dict(radix_x=rad[0], radix_y=rad[1])
    # plane pass
    npl = nx * ny
    xy_lds = 8 * (nx * (ny | 1) + nx + ny) + 128
    best = None
    for t in (512, 256, 768, 1024):
        cost, ok = 0, True
        for ax in (0, 1):
            for rx in rad[ax]:
                slots = (npl // rx + t - 1) // t
                ok = ok and slots <= (XY_PPT + rx - 1) // rx
                cost += slots * t * rx
        if ok and (best is None or cost < best[0]):
            best = (cost, t)
    fused = best is not None and xy_lds <= 160 * 1024
    if fused and nx == ny and nx in (64, 128):
        out['plane'] = 'pow2_%d' % nx
    elif fused:
        out['plane'] = 'sched'
    else:
        def slab(n_line, n_other):
            return max([c for c in range(1, n_other + 1)
                        if n_other % c == 0 and n_line * c <= XY_PPT * XS_THREADS and n_line * (c | 1) * 8 <= 40 * 1024] or [0])
        out['xs_sw'] = slab(nx, ny)
        out['ys_sh'] = max([c for c in range(1, nx + 1) if nx % c == 0 and ny * c <= XY_PPT * XS_THREADS and c * (ny | 1) * 8 <= 40 * 1024] or [0])
        out['plane'] = 'slab' if out['xs_sw'] > 0 and out['ys_sh'] > 0 else 'strided'
    # z pass
    M = nz // 2 if half else nz
    zt = 256 if ny * M <= Z_PPT * 256 else 512
    nl = max([c for c in range(1, ny + 1) if ny % c == 0 and c * M <= Z_PPT * zt] or [1])
    out.update(M=M, zt=zt, nl=nl, z_groups_per_row=(ny + nl - 1) // nl)
    if half and nz in (64, 128) and ny % 64 == 0 and nl == 64 and zt == 64 * (nz // 16):
        out['z'] = 'pow2_%d' % nz
    else:
        out['z'] = 'packed' if half else 'full'
    return out


# ---- boxes ------------------------------------------------------------------------------------------------------------------
ORTHO = np.array([2.2, 3.1, 4.3])
BOXES = {
    'cubic': np.array([[2.4, 2.4, 2.4]]),
    'ortho': ORTHO[None].copy(),
    'big': 1.5 * ORTHO[None],                  # room for the 1100 atoms of `many` at the minimum distance
    'per_replica': ORTHO[None] * np.array([[1.0, 1.0, 1.0], [1.04, 0.97, 1.02], [0.98, 1.05, 0.99]]),
}
SECOND_BOX = ORTHO * np.array([1.03, 0.98, 1.05])      # (d): the box a live handle changes to


# ---- placements -------------------------------------------------------------------------------------------------------------
def _charges(rng, n):
    return rng.uniform(0.2, 0.8, n) * rng.choice([-1.0, 1.0], n)


def _min_image_dist(a, b, box):
    d = a - b
    d -= box * np.rint(d / box)
    return np.sqrt((d * d).sum(-1))


def _place(rng, n, box, draw, dmin=DMIN):
    """n positions from draw() by sequential rejection: each at least dmin (minimum image) from those before it"""
    x = np.zeros((0, 3))
    tries = 0
    while len(x) < n:
        c = np.asarray(draw(), dtype=np.float64)
        tries += 1
        assert tries < 200000, 'placement does not fit the minimum distance'
        if len(x) == 0 or _min_image_dist(x, c[None], box).min() >= dmin:
            x = np.vstack([x, c[None]])
    return x


def bulk(rng, box, grid, n=120):
    return _place(rng, n, box, lambda: rng.uniform(0.0, 1.0, 3) * box), _charges(rng, n)


def faces(rng, box, grid, n=96):
    """every atom has at least one coordinate from {0, L as fp32, -1e-9, nextafter(L, 0) in fp32, a mesh plane k L / n, the middle of a
    cell}; a third of the atoms have two such coordinates, a sixth all three"""
    def special(k):
        L, nk = box[k], int(grid[k])
        j = int(rng.integers(0, nk))
        return [0.0, float(np.float32(L)), -1e-9, float(np.nextafter(np.float32(L), np.float32(0.0))), j * L / nk, (j + 0.5) * L / nk][int(rng.integers(0, 6))]

    def draw():
        c = rng.uniform(0.0, 1.0, 3) * box
        ns = [1, 1, 1, 2, 2, 3][int(rng.integers(0, 6))]
        for k in rng.permutation(3)[:ns]:
            c[k] = special(k)
        return c
    return _place(rng, n, box, draw), _charges(rng, n)


def outside_shifts(rng, n):
    s = rng.integers(-3, 5, size=(n, 3))
    s[0] = (-3, 4, -1)                      # the ends of the range and a negative shift are always there
    s[1] = (4, -3, -2)
    return s


def outside(rng, box, grid, n=120):
    """`bulk` (the same atoms: the same generator state) shifted per atom by integer multiples of the box edges in [-3, 4]"""
    x, q = bulk(rng, box, grid, n)
    return x + outside_shifts(rng, n) * box, q


def one_column(rng, box, grid, n=40):
    """all atoms inside one mesh cell width in x, straddling x = 0: their x bins are the last and the first one"""
    w = box[0] / int(grid[0])

    def draw():
        c = rng.uniform(0.0, 1.0, 3) * box
        c[0] = rng.uniform(-0.5, 0.5) * w
        return c
    x = _place(rng, n, box, draw)
    x[0, 0], x[1, 0] = -0.25 * w, 0.25 * w   # (both sides are occupied whatever the draws)
    return x, _charges(rng, n)


def corner(rng, box, grid, n=6):
    """all atoms within two mesh cells of the box corner (the eight corners are one point), so every stencil wraps in x, y and z at once.
    The cube of four cells is narrower than the minimum distance on all but the coarsest meshes: the atoms keep 0.25 nm where it fits and
    otherwise 0.45 of the cube's shortest edge."""
    w = 2.0 * box / np.asarray(grid, dtype=np.float64)
    dmin = min(DMIN, 0.45 * float(2.0 * w.min()))
    x = _place(rng, n, box, lambda: rng.uniform(-1.0, 1.0, 3) * w, dmin)
    return x, _charges(rng, n)


def sparse_q(rng, box, grid, n=120):
    x, q = bulk(rng, box, grid, n)
    q[1::2] = 0.0
    return x, q


def pair(rng, box, grid):
    x = _place(rng, 2, box, lambda: rng.uniform(0.0, 1.0, 3) * box)
    q0 = float(rng.uniform(0.2, 0.8))
    return x, np.array([q0, -q0])


def single(rng, box, grid):
    return (rng.uniform(0.0, 1.0, 3) * box)[None], np.array([float(rng.uniform(0.2, 0.8))])


def many(rng, box, grid, n=1100):
    return bulk(rng, box, grid, n)


PLACEMENTS = dict(bulk=bulk, faces=faces, outside=outside, one_column=one_column, corner=corner, sparse_q=sparse_q, pair=pair,
                  single=single, many=many)
SMALL = ('pair', 'single')                   # no other charge to set a force scale: held to absolute bounds


def case_seed(mesh, placement, box):
    return zlib.crc32(('%s/%s/%s' % (mesh, placement, box)).encode()) & 0x7fffffff


# ---- the matrix -------------------------------------------------------------------------------------------------------------
# (a), (b): every mesh path x {bulk, faces, outside} on ortho, R = 1; every placement on mixed, p64, slab (`many` in its larger box)
def _matrix():
    cases = [(m, p, 'ortho') for m in MESHES for p in ('bulk', 'faces', 'outside')]
    for m in ('mixed', 'p64', 'slab'):
        cases += [(m, p, 'big' if p == 'many' else 'ortho') for p in PLACEMENTS if p not in ('bulk', 'faces', 'outside')]
    return cases


MATRIX = _matrix()
PER_REPLICA_MESHES = ('mixed', 'p64', 'p128', 'z64', 'slab')
PER_REPLICA = [(m, 'bulk', 'per_replica') for m in PER_REPLICA_MESHES]


def case_id(case):
    return '-'.join(case)


def make_system(q, box):
    s = System()
    nb = NonbondedForce()
    nb.setNonbondedMethod(NonbondedForce.PME)
    nb.setCutoffDistance(CUTOFF)
    nb.setUseDispersionCorrection(False)
    for qi in q:
        s.addParticle(12.0)
        nb.addParticle(float(qi), 0.3, 0.0)
    s.addForce(nb)
    s.setDefaultPeriodicBoxVectors((box[0], 0, 0), (0, box[1], 0), (0, 0, box[2]))
    return s


_ALPHA = []


def make_desc(q, grid, alch_atoms=None):
    """the description of N point charges on the given mesh; alpha is what the 1 nm cutoff gives in the reference 2.4 nm box (fixed)"""
    desc = system_to_desc(make_system(q, BOXES['cubic'][0]))
    assert desc['nb_method'] == 2 and 'coulomb_cutoff' not in desc
    if not _ALPHA:
        _ALPHA.append(float(desc['ewald_alpha']))
    assert float(desc['ewald_alpha']) == _ALPHA[0]
    desc['pme_grid'] = np.array(grid, dtype=np.int32)
    if alch_atoms is not None:
        desc['alch_atoms'] = np.array(sorted(alch_atoms), dtype=np.int32)
    return desc


def self_energy(q, alpha):
    return -ONE_4PI_EPS0 * alpha / math.sqrt(math.pi) * float(np.sum(np.asarray(q) ** 2))


_CASES = {}


def build_case(case):
    """(desc, x [R][N][3], box [R][3]) of a case (mesh id, placement, box id); replica r of a per-replica box has its own positions.

    Random charges that do not add up to zero give totals anywhere between a few percent and a half of the Ewald self energy: the
    reciprocal sum, the self term and the direct sum cancel.  The suite's demand of 1e-5 of the total potential (bounds()) would then measure
    that cancellation and not the kernels, so a configuration whose f64 reference total is below 5 % of the self energy is drawn again (from
    the reference alone; the generator goes on where it was)."""
    if case not in _CASES:
        from oracle.forcefield import ForceFieldOracle
        mesh, placement, boxid = case
        grid = MESHES[mesh][0]
        box = BOXES[boxid]
        rng = np.random.default_rng(case_seed(*case))
        xs, desc = [], None
        for r in range(len(box)):
            for attempt in range(16):
                x, q = PLACEMENTS[placement](rng, box[r], grid)
                d = make_desc(q, grid) if desc is None else desc
                if r > 0:
                    assert len(x) == len(desc['charge'])
                e = ForceFieldOracle(d).energy_forces(x, box[r], forces=False)[0]
                if abs(e) >= 0.05 * abs(self_energy(d['charge'], d['ewald_alpha'])):
                    break
            else:
                raise AssertionError('no configuration of %s with a total that does not cancel' % case_id(case))
            desc = d
            xs.append(x)
        _CASES[case] = (desc, np.stack(xs), box.copy())
    desc, x, box = _CASES[case]
    return dict(desc), x.copy(), box.copy()


def wrapped_parent(x, box):
    """(f): the image inside the box of every atom of an `outside` case"""
    return x - np.floor(x / box[:, None, :]) * box[:, None, :]


# ---- engines and the oracle -------------------------------------------------------------------------------------------------
def setup_engine(eng, desc, x, box, lambda_electrostatics=None):
    """one state per replica when lambda_electrostatics [R] is given (replica r in state r), else one state for all"""
    R = len(x)
    eng.set_system(desc)
    if lambda_electrostatics is None:
        eng.set_states(np.full(1, BETA))
        labels = np.zeros(R, dtype=np.int64)
    else:
        assert len(lambda_electrostatics) == R
        eng.set_states(np.full(R, BETA), np.ones(R), np.asarray(lambda_electrostatics, dtype=np.float64))
        labels = np.arange(R, dtype=np.int64)
    eng.set_integrator('V R O R V', 0.001, 1.0, 1, True, 1e-8)
    eng.set_replicas(R, 0, x, None, box, labels)
    eng.set_force_groups(FORCE_GROUPS)
    return eng


def evaluate(eng):
    """(reciprocal-group forces [R][N][3], total potential [R], the fp32-rounded positions the engine holds [R][N][3])"""
    U = eng.compute_energies(want_potential=True)[1]
    f = eng.get_forces(groups=1 << RECIP_GROUP)
    return f, U.copy(), eng.get_replicas()[0]


def oracle_reference(desc, xd, box, lambda_electrostatics=None):
    """f64 smooth PME on the same mesh: (class-5 forces [R][N][3], class-5 energy [R], total energy [R])"""
    from oracle.forcefield import ForceFieldOracle
    ff = ForceFieldOracle(desc)
    f5, e5, et = [], [], []
    for r in range(len(xd)):
        le = 1.0 if lambda_electrostatics is None else float(lambda_electrostatics[r])
        e, f = ff.energy_forces(xd[r], box[r], lambda_electrostatics=le, classes={5})
        f5.append(f)
        e5.append(e)
        et.append(ff.energy_forces(xd[r], box[r], lambda_electrostatics=le, forces=False)[0])
    return np.stack(f5), np.array(e5), np.array(et)


def errors(f, U, f5, e5, et):
    """per replica: max |df|, RMS of the per-atom error vector, both over max |f_ref| of the reciprocal group, |dE|, |dE| / |E_recip|"""
    rows = []
    for r in range(len(f)):
        d = f[r] - f5[r]
        fmax = np.abs(f5[r]).max()
        amax, rms = np.abs(d).max(), math.sqrt((d * d).sum(axis=1).mean())
        de = abs(U[r] - et[r])
        rows.append(dict(f_max=amax, f_rms=rms, f_ref=fmax, f_max_rel=amax / fmax if fmax > 0 else 0.0, f_rms_rel=rms / fmax if fmax > 0 else 0.0,
                         e_abs=de, e_rel=de / abs(e5[r]), e_recip=e5[r], e_total=et[r]))
    return rows


# ---- bounds -----------------------------------------------------------------------------------------------------------------
FAMILIES = ('f_max', 'f_rms', 'f_max_rel', 'f_rms_rel', 'e_abs', 'e_rel')


def read_error_table(path=ERROR_TABLE):
    """rows of profiles/pme_edge_errors.txt: dicts with case, replica and one float per family"""
    rows = []
    with open(path) as fh:
        for line in fh:
            t = line.split('|')[0].split()
            if len(t) == 4 + len(FAMILIES) and t[0] == 'row':
                rows.append(dict(case=t[1], r=int(t[2]), n=int(t[3]), **{k: float(v) for k, v in zip(FAMILIES, t[4:])}))
    return rows


def family_maxima(rows):
    """the largest recorded value per family; the relative force families over the cases with other charges to set a scale (not SMALL), the
    absolute ones over the SMALL cases, the energy families over all"""
    small = [w for w in rows if w['case'].split('-')[1] in SMALL]
    rest = [w for w in rows if w['case'].split('-')[1] not in SMALL]
    out = {k: max(w[k] for w in rest) for k in ('f_max_rel', 'f_rms_rel')}
    out.update({k + '_small': max(w[k] for w in small) for k in ('f_max', 'f_rms', 'e_abs')})
    out['e_rel'] = max(w['e_rel'] for w in rows)
    return out


_BOUNDS = {}


def bounds():
    """4 x the largest value recorded in each family: the factor covers other seeds and another atomic order in the rounding of the
    __float2int_rn sums of other inputs.  Never looser than what the suite already demands of this force group: 1e-3 of max |f_ref|
    (test_force_groups._follows); the 1e-5 of the total potential is applied where the potential is compared.
    e_rel: two recorded values stand out from the rest of their family (2e-8 ... 1.8e-6): z128-outside (8.1e-6) and p64_odd-bulk (5.2e-6).
    Their |dE| (1.8e-3 and 1.0e-3 kJ/mol) is as ordinary as any; their denominator E(classes={5}) is 220 and 186 kJ/mol instead of
    thousands because the reciprocal sum and the self term happen to cancel there."""
    if not _BOUNDS:
        _BOUNDS.update({k: 4.0 * v for k, v in family_maxima(read_error_table()).items()})
        _BOUNDS['f_max_rel'] = min(_BOUNDS['f_max_rel'], 1e-3)
    return _BOUNDS
