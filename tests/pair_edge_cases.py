"""Cases and helpers of the direct-space pair path edge tests (test_pair_edges_gpu.py, test_pair_edges_cpu.py).

Systems: N point particles (no bonded terms, no constraints) in an orthorhombic periodic box, built from seeds with the package's own
System / NonbondedForce / system_to_desc.  Cutoff 0.6 nm (the shortest the suite uses), argon-like sigma and epsilon, charges drawn as in
pme_edge_cases._charges, minimum distance of interacting pairs 0.25 nm unless a placement says otherwise.  Direct space sits in force
group 1 (FORCE_GROUPS), so get_forces(groups=2) is the pair path alone: the pairs, the non-zero exceptions and the Ewald exclusion
correction -- the oracle's class 4 (oracle/forcefield.py).

METHODS: one id per instantiation family of nonbonded_sci_body; `build_rules` restates the rules of remd_build_nonbonded (csrc/forces.hip)
that pick the kernel, the LJ sub-system, the exclusion window and the molecule groups, and test_pair_edges_cpu.py holds every case to the
`claims` it makes.
CASES: id -> builder; build_case(id) gives a dict with desc, x [R][N][3], box [R][3], the states' lambdas, claims, and for `dimers` the
atoms of the pairs inside and outside the cutoff.
bounds(): 4 x the largest error recorded on the MI355X per family (profiles/pair_edge_errors.txt, tools/record_pair_edge_errors.py), never
looser than the bars the suite already sets; before the table exists, those bars.
"""
import contextlib
import math
import os
import zlib

import numpy as np

from openmmtools_amd.system import System, NonbondedForce, system_to_desc
from oracle.md_oracle import ONE_4PI_EPS0
from pme_edge_cases import _charges, _min_image_dist, BOXES as PME_BOXES

KB = 0.008314462618153242
BETA = 1.0 / (KB * 300.0)
CUTOFF = 0.6
SWITCH = 0.5
RCC_FAR = 0.75                          # pme_far: the explicit Coulomb range handed to system_to_desc(ewald_split=...)
DMIN = 0.25
SIGMA, EPSILON = 0.3405, 0.996          # argon
BAND = 2e-4                             # no interacting pair within BAND x cutoff of a cutoff radius
DIRECT_GROUP = 1
FORCE_GROUPS = [0, 0, 0, 0, DIRECT_GROUP, 0]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERROR_TABLE = os.path.join(ROOT, 'profiles', 'pair_edge_errors.txt')
MAX_EXCL_WORDS = 8                      # csrc/forces.hip

# id -> (PME, charges, every how-manieth atom has epsilon != 0, switch distance or None, Coulomb range or None, the path meant)
METHODS = {
    'lj':          (False, False, 1, SWITCH, None,    'NB_LJ_ONLY, one-system launch, switched'),
    'lj_noswitch': (False, False, 1, None,   None,    'NB_LJ_ONLY, one-system launch, no switch'),
    'rf':          (False, True,  1, None,   None,    'NB_RF, no split (NL * 10 > N * 6)'),
    'rf_split':    (False, True,  3, SWITCH, None,    'NB_RF_NOLJ + the LJ sub-system in nonbonded_sci2_kernel'),
    'pme':         (True,  True,  1, None,   None,    'NB_EWALD: force table in the force-only launch, polynomial erfc with energies'),
    'pme_split':   (True,  True,  3, SWITCH, None,    'NB_EWALD_NOLJ on the early-table path + the LJ sub-system'),
    'pme_far':     (True,  True,  3, SWITCH, RCC_FAR, 'as pme_split; the main list runs to rcc2, the LJ list to rc2'),
}
# what build_rules must say of a system of each method
EXPECTED_RULES = {
    'lj': dict(method='NB_LJ_ONLY', split=False), 'lj_noswitch': dict(method='NB_LJ_ONLY', split=False),
    'rf': dict(method='NB_RF', split=False), 'rf_split': dict(method='NB_RF', split=True),
    'pme': dict(method='NB_EWALD', split=False), 'pme_split': dict(method='NB_EWALD', split=True),
    'pme_far': dict(method='NB_EWALD', split=True, rcc=RCC_FAR),
}
FAMILY = {'lj': 'lj', 'lj_noswitch': 'lj', 'rf': 'rf', 'rf_split': 'rf', 'pme': 'ewald', 'pme_split': 'ewald', 'pme_far': 'ewald'}


def longest_cutoff(method):
    return METHODS[method][4] or CUTOFF


def build_rules(desc):
    """What remd_build_nonbonded makes of a description: kernel family, LJ sub-system, exclusion windows, molecule groups."""
    N = int(desc['n_atoms'])
    q, eps = np.asarray(desc['charge']), np.asarray(desc['epsilon'])
    exc = np.asarray(desc['exception_atoms']).reshape(-1, 2)
    any_charge = bool(np.any(q != 0))
    out = dict(N=N, method='NB_LJ_ONLY' if not any_charge else ('NB_EWALD' if desc['nb_method'] == 2 else 'NB_RF'))
    maxd = int(np.abs(exc[:, 0] - exc[:, 1]).max()) if len(exc) else 0
    out['words'] = max(1, (maxd + 32) // 32)
    out['refused'] = out['words'] > MAX_EXCL_WORDS
    out['excl_W'] = 4 * out['words'] + 1
    ordn = np.full(N, -1)
    ordn[eps != 0] = np.arange(int((eps != 0).sum()))
    NL = int((eps != 0).sum())
    out['NL'] = NL
    out['split'] = any_charge and NL > 0 and NL * 10 <= N * 6
    if out['split']:
        lj = [(ordn[i], ordn[j]) for i, j in exc if ordn[i] >= 0 and ordn[j] >= 0]
        out['lj_words'] = max(1, (max([abs(a - b) for a, b in lj] or [0]) + 32) // 32)
        out['split'] = out['lj_words'] <= MAX_EXCL_WORDS
    out['rcc'] = max(float(desc['cutoff']), float(desc.get('coulomb_cutoff', 0.0))) if out['method'] == 'NB_EWALD' else float(desc['cutoff'])
    # groups: connected components of the exceptions, extended to their index span, interleaved ones merged
    parent = list(range(N))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for i, j in exc:
        a, b = find(int(i)), find(int(j))
        if a != b:
            parent[max(a, b)] = min(a, b)
    hi = list(range(N))
    for i in range(N):
        hi[find(i)] = max(hi[find(i)], i)
    sizes, i = [], 0
    while i < N:
        end, k = hi[find(i)], i
        while k <= end:
            end = max(end, hi[find(k)])
            k += 1
        sizes.append(end - i + 1)
        i = end + 1
    out['groups'] = sizes
    return out


# ---- systems ----------------------------------------------------------------------------------------------------------------
def make_system(method, q, box, exceptions=(), eps_on=None):
    pme, charges, every, switch, rcc, _ = METHODS[method]
    n = len(q)
    s = System()
    nb = NonbondedForce()
    nb.setNonbondedMethod(NonbondedForce.PME if pme else NonbondedForce.CutoffPeriodic)
    nb.setCutoffDistance(CUTOFF)
    if switch is not None:
        nb.setUseSwitchingFunction(True)
        nb.setSwitchingDistance(switch)
    nb.setUseDispersionCorrection(True)
    for i in range(n):
        s.addParticle(39.9)
        on = (i % every == 0) if eps_on is None else bool(eps_on[i])
        nb.addParticle(float(q[i]) if charges else 0.0, SIGMA, EPSILON if on else 0.0)
    for e in exceptions:
        nb.addException(int(e[0]), int(e[1]), float(e[2]), float(e[3]), float(e[4]))
    s.addForce(nb)
    s.setDefaultPeriodicBoxVectors((box[0], 0, 0), (0, box[1], 0), (0, 0, box[2]))
    return s


def make_desc(method, q, box, exceptions=(), eps_on=None, alch_atoms=None, annihilate=False):
    desc = system_to_desc(make_system(method, q, box, exceptions, eps_on), box=np.asarray(box, dtype=np.float64),
                          ewald_split=METHODS[method][4])
    if alch_atoms is not None:
        desc['alch_atoms'] = np.array(sorted(alch_atoms), dtype=np.int32)
        desc['annihilate_sterics'] = bool(annihilate)
    return desc


def self_energy(desc):
    return -ONE_4PI_EPS0 * float(desc['ewald_alpha']) / math.sqrt(math.pi) * float(np.sum(np.asarray(desc['charge']) ** 2))


def box_for(n, method, density=20.0):
    """an orthorhombic box a little over two of the method's longest cutoff, or wide enough for n atoms at the minimum distance"""
    e = max(2.0 * longest_cutoff(method) + 0.05, (n / density) ** (1.0 / 3.0))
    return e * np.array([1.0, 1.08, 1.17])


# ---- placements: (rng, box, n) -> x ---------------------------------------------------------------------------------------------
PAD = 4e-3                              # the placements keep DMIN + PAD, so that the nudges out of the cutoff bands (below) keep DMIN


def _place(rng, n, box, draw, dmin=DMIN + PAD, x0=None):
    """n more positions from draw(i) by sequential rejection: each at least dmin (minimum image) from those before it (x0 included)"""
    x = np.zeros((0, 3)) if x0 is None else np.asarray(x0, dtype=np.float64)
    n0, tries = len(x), 0
    while len(x) < n0 + n:
        c = np.asarray(draw(len(x)), dtype=np.float64)
        tries += 1
        assert tries < 400000, 'placement does not fit the minimum distance'
        if len(x) == 0 or _min_image_dist(x, c[None], box).min() >= dmin:
            x = np.vstack([x, c[None]])
    return x


def pair_distances(x, box):
    """f64 minimum-image distances [N][N] of the positions as fp32 holds them"""
    xf = np.asarray(x, dtype=np.float32).astype(np.float64)
    d = xf[:, None, :] - xf[None, :, :]
    d -= box * np.rint(d / box)
    return np.sqrt((d * d).sum(-1))


def in_band(x, box, radii, exempt=()):
    """pairs (i < j) within BAND x radius of one of the radii"""
    r = pair_distances(x, box)
    bad = np.zeros_like(r, dtype=bool)
    for rc in radii:
        bad |= np.abs(r - rc) < BAND * rc
    bad = np.triu(bad, 1)
    for i, j in exempt:
        bad[min(i, j), max(i, j)] = False
    return np.argwhere(bad)


def out_of_bands(rng, x, box, radii, pinned=(), exempt=()):
    """moves one atom of every pair that sits within 1.5 BAND of a cutoff radius by 1e-3 nm, until none is left (the unswitched terms are
    discontinuous there: an fp32 and an f64 verdict that differ are not a kernel error).  pinned: atom indices that stay, or a mask
    [N][3] of the coordinates that stay"""
    x = x.copy()
    frozen = np.zeros(x.shape, dtype=bool)
    if isinstance(pinned, np.ndarray) and pinned.dtype == bool:
        frozen = pinned
    else:
        frozen[[int(p) for p in pinned]] = True
    for it in range(400):
        r = pair_distances(x, box)
        bad = np.zeros_like(r, dtype=bool)
        for rc in radii:
            bad |= np.abs(r - rc) < 1.5 * BAND * rc
        bad = np.triu(bad, 1)
        for i, j in exempt:
            bad[min(i, j), max(i, j)] = False
        pairs = np.argwhere(bad)
        if len(pairs) == 0:
            return x
        for i, j in pairs:
            k = j if not frozen[j].all() else i
            assert not frozen[k].all(), 'two pinned atoms at a cutoff radius'
            v = rng.normal(size=3) * ~frozen[k]
            x[k] += 1e-3 * v / np.linalg.norm(v)
    raise AssertionError('atoms stay in a cutoff band')


def bulk(rng, box, n):
    """uniform at the minimum distance; fewer than 40 atoms sit in a cube around the box corner (they see each other, across the faces)"""
    if n < 40:
        e = max(0.45, (n / 20.0) ** (1.0 / 3.0))
        return _place(rng, n, box, lambda i: rng.uniform(-0.5, 0.5, 3) * e)
    return _place(rng, n, box, lambda i: rng.uniform(0.0, 1.0, 3) * box)


def face_values(L):
    """0, L, the float just below L, -1e-7 L (v / L - floorf(v / L) is 1 - 2^-23 there) and -1e-9 L (which does round
    frac() of gather_positions_body to 1.0 before its cast)"""
    L32 = np.float32(L)
    return [0.0, float(L32), float(np.nextafter(L32, np.float32(0.0))), -1e-7 * L, -1e-9 * L]


def faces(rng, box, n):
    """a third of the atoms on faces, edges and corners; a third within 0.5 nm of a face on either side (their partners); the rest anywhere"""
    ns = n // 3
    frozen = np.zeros((n, 3), dtype=bool)

    def draw(i):
        c = rng.uniform(0.0, 1.0, 3) * box
        if i < ns:
            # (one corner atom, the first: the eight corners are one point; then five on edges; the values cycle per axis)
            for k in ((0, 1, 2) if i == 0 else (i % 3, (i + 1) % 3) if i < 6 else (i % 3,)):
                v = face_values(box[k])
                c[k] = v[(i + int(k)) % len(v)]
                frozen[i, k] = True
        elif i < 2 * ns:
            k = int(rng.integers(0, 3))
            c[k] = rng.uniform(-0.5, 0.5)
        return c
    return _place(rng, n, box, draw), frozen


def outside_shifts(rng, n):
    s = rng.integers(-3, 4, size=(n, 3))
    s[0] = (-3, 3, -1)
    if n > 1:
        s[1] = (3, -3, -2)
    return s


def blob(rng, box, n):
    """all atoms but eight within one cutoff of each other (a ball of diameter 0.6 nm would not hold them at the minimum distance: the
    ball's diameter is the cutoff for up to 20 atoms, beyond that the atoms sit within a ball whose tiles all list each other), the last
    eight more than a cutoff away from the ball and within 0.45 nm of each other"""
    rad = max(0.3, 0.5 * (max(n - 8, 1) / 18.0) ** (1.0 / 3.0))
    c0 = 0.3 * box

    def ball(i):
        v = rng.normal(size=3)
        return c0 + v / np.linalg.norm(v) * rad * rng.uniform() ** (1.0 / 3.0)
    x = _place(rng, n - 8, box, ball)
    c1 = c0 + 0.5 * box
    return _place(rng, 8, box, lambda i: c1 + rng.uniform(-0.225, 0.225, 3), x0=x)


MOLECULE_SIZES = (1, 3, 5, 9, 33, 65, 130, 1, 3, 5, 9, 33, 3, 1, 9, 5, 3, 1)     # 319 atoms; 130 > a tile of 64


def chain_exclusions(sizes, reach=3):
    exc, first = [], 0
    for s in sizes:
        exc += [(first + a, first + b) for a in range(s) for b in range(a + 1, min(s, a + reach + 1))]
        first += s
    return exc


def molecules(rng, box, n=None):
    """chains laid out as self-avoiding walks with 0.26 nm steps: index neighbours up to distance 3 are excluded, everything else keeps the
    minimum distance.  In sorted order the groups of 1, 3, 5 ... atoms start wherever the ones before them end, so they straddle cluster
    (8) and tile (64) boundaries whatever the order of the molecules"""
    x = np.zeros((0, 3))
    for s in MOLECULE_SIZES:
        for attempt in range(400):
            m = []
            for k in range(s):
                for t in range(200):
                    v = rng.normal(size=3)
                    c = rng.uniform(0.0, 1.0, 3) * box if k == 0 else m[-1] + 0.26 * v / np.linalg.norm(v)
                    far = np.vstack([x] + [p[None] for p in m[:max(0, k - 3)]])          # everything that is not excluded from it
                    if len(far) and _min_image_dist(far, c[None], box).min() < DMIN + PAD:
                        continue
                    if k >= 2 and _min_image_dist(np.array(m[max(0, k - 3):k - 1]), c[None], box).min() < 0.2:
                        continue
                    m.append(c)
                    break
                else:
                    break
            if len(m) == s:
                x = np.vstack([x, np.array(m)])
                break
        else:
            raise AssertionError('molecule does not fit')
    return x


# ---- dimers -----------------------------------------------------------------------------------------------------------------
DIMER_SPACING = 1.8                      # > longest cutoff + 0.3 nm + the longest separation


def dimers(rng, method):
    """(x, box, inside pairs, outside pairs, separations): isolated pairs on a 2 x 4 x 4 lattice of spacing 1.8 nm.  The layer i = 0 is
    centred on the face x = 0 with its pairs along x (they straddle it); of the layer i = 1 the row j = 0 is centred on the face y = 0 with
    its pairs along y; the rest point anywhere.  Separations cycle through 0.25, 0.4, rc (1 - 1e-3) inside and rc (1 + 1e-3) outside;
    on pme_far rcc (1 -+ 1e-3) too, and there only pairs beyond rcc are outside"""
    rl = longest_cutoff(method)
    seps = [0.25, 0.4, CUTOFF * (1 - 1e-3), CUTOFF * (1 + 1e-3)]
    if rl > CUTOFF:
        seps += [rl * (1 - 1e-3), rl * (1 + 1e-3)]
    s = DIMER_SPACING
    box = np.array([2 * s, 4 * s, 4 * s])
    x, inside, outside, sep_of = [], [], [], []
    p = 0
    for i in range(2):
        for j in range(4):
            for k in range(4):
                c = np.array([i * s, j * s, k * s + 0.37])
                if i == 0:
                    u = np.array([1.0, 0.0, 0.0])
                elif j == 0:
                    u = np.array([0.0, 1.0, 0.0])
                else:
                    u = rng.normal(size=3)
                    u /= np.linalg.norm(u)
                d = seps[p % len(seps)]
                x += [c - 0.5 * d * u, c + 0.5 * d * u]
                (inside if d < rl else outside).append((2 * p, 2 * p + 1))
                sep_of.append(d)
                p += 1
    return np.array(x), box, inside, outside, sep_of


# ---- the cases --------------------------------------------------------------------------------------------------------------
CASES = {}


def case_seed(cid):
    return zlib.crc32(cid.encode()) & 0x7fffffff


def _case(cid, fn, **kw):
    assert cid not in CASES
    CASES[cid] = (fn, kw)


def _finish(cid, method, x, box, exceptions=(), eps_on=None, lam=None, alch=None, annihilate=False, claims=None, exempt=(), q=None, **extra):
    """x [N][3] or [R][N][3], box [3] or [R][3] -> the case"""
    x = np.asarray(x, dtype=np.float64)
    x = x[None] if x.ndim == 2 else x
    box = np.asarray(box, dtype=np.float64)
    box = np.tile(box, (len(x), 1)) if box.ndim == 1 else box
    desc = make_desc(method, q, box[0], exceptions, eps_on, alch, annihilate)
    c = dict(id=cid, method=method, desc=desc, x=x, box=box, lam=lam, claims=dict(claims or {}), exempt=list(exempt), **extra)
    return c


def _drawn(cid, method, n, place, exceptions=(), box=None, radii=None, **kw):
    """the common builder: charges, a placement inside its box, atoms nudged out of the cutoff bands.  A PME configuration whose f64 total
    is below 5 % of the Ewald self energy is drawn again: the suite's 1e-5 of the total would measure the cancellation, as in
    pme_edge_cases"""
    from oracle.forcefield import ForceFieldOracle
    rng = np.random.default_rng(case_seed(cid))
    box = box_for(n, method) if box is None else np.asarray(box, dtype=np.float64)
    radii = sorted({CUTOFF, longest_cutoff(method)}) if radii is None else radii
    for attempt in range(16):
        q = _charges(rng, n)
        got = place(rng, box, n)
        x, pinned = got if isinstance(got, tuple) else (got, ())
        x = out_of_bands(rng, x, box, radii, pinned=pinned)
        c = _finish(cid, method, x, box, exceptions, q=q, **kw)
        ff = ForceFieldOracle(c['desc'])
        e = ff.energy_forces(x, box, forces=False)[0]
        if METHODS[method][0] and abs(e) < 0.05 * abs(self_energy(c['desc'])):
            continue
        # ... and the direct-space energy, the denominator of the energy bound, is not a cancellation either (from the reference alone)
        if abs(ff.energy_forces(x, box, forces=False, classes={4})[0]) < 0.02 * abs(e):
            continue
        return c
    raise AssertionError('no configuration of %s with a total that does not cancel' % cid)


# sizes: padding edges of the main system (and NL of the LJ sub-system on the split methods)
ALL_SIZES = (2, 7, 8, 9, 63, 64, 65, 72, 127, 128, 129, 200)
FEW_SIZES = (9, 64, 65, 129)
NL_SIZES = {2: 1, 23: 8, 26: 9, 191: 64, 194: 65}        # N -> NL = ceil(N / 3)
SIZES = {m: (ALL_SIZES if m in ('lj', 'pme_split') else FEW_SIZES) for m in METHODS}
for _m in ('rf_split', 'pme_split', 'pme_far'):
    SIZES[_m] = tuple(sorted(set(SIZES[_m]) | set(NL_SIZES)))


def _size(cid, method, n):
    claims = dict(N=n, n_mod_8=n % 8, n_mod_64=n % 64)
    if METHODS[method][2] == 3:
        claims['NL'] = (n + 2) // 3
    return _drawn(cid, method, n, bulk, claims=claims)


for _m in METHODS:
    for _n in SIZES[_m]:
        _case('size-%s-%d' % (_m, _n), _size, method=_m, n=_n)


def _faces(cid, method):
    return _drawn(cid, method, 96, faces, box=np.array([1.7, 1.85, 2.0]), claims=dict(N=96))


def _outside(cid, method):
    c = _drawn(cid, method, 100, bulk, claims=dict(N=100))
    c['parent'] = c['x'].copy()
    c['x'] = c['x'] + outside_shifts(np.random.default_rng(case_seed(cid) ^ 0x33), 100)[None] * c['box'][:, None, :]
    return c


def _min_box(cid, method, dims):
    e = 2.0 * CUTOFF + 1e-3
    box = np.array([e if k < dims else 1.9 for k in range(3)])
    n = int(20.0 * box.prod())
    return _drawn(cid, method, n, bulk if n >= 40 else (lambda rng, b, m: _place(rng, m, b, lambda i: rng.uniform(0.0, 1.0, 3) * b)),
                  box=box, claims=dict(N=n, min_edges=dims))


def _thin(cid, method):
    return _drawn(cid, method, 150, bulk, box=np.array([1.25, 1.25, 6.0]), claims=dict(N=150))


def _blob(cid, method):
    return _drawn(cid, method, 72, blob, box=np.array([3.0, 3.2, 3.4]), claims=dict(N=72, blob=True))


def _molecules(cid, method):
    n = sum(MOLECULE_SIZES)
    return _drawn(cid, method, n, molecules, exceptions=[(i, j, 0.0, 0.1, 0.0) for i, j in chain_exclusions(MOLECULE_SIZES)],
                  box=np.array([2.6, 2.8, 3.0]), claims=dict(N=n, groups=list(MOLECULE_SIZES), words=1))


def _dimers(cid, method):
    rng = np.random.default_rng(case_seed(cid))
    x, box, inside, outside, seps = dimers(rng, method)
    q = _charges(rng, len(x))
    q[1::2] = -q[0::2]                                   # opposite charges in a pair
    claims = dict(N=len(x), pairs_inside=len(inside), pairs_outside=len(outside))
    eps_on = None
    if METHODS[method][2] == 3:
        # the split methods: both atoms of two pairs in five carry Lennard-Jones (every separation among them), the others none, so the
        # LJ sub-system's own list and rc2 mask see pairs at every radius
        eps_on = np.repeat(np.arange(len(x) // 2) % 5 < 2, 2)
        claims['NL'] = int(eps_on.sum())
    return _finish(cid, method, x, box, q=q, eps_on=eps_on, claims=claims, exempt=inside + outside, inside=inside, outside=outside, seps=seps,
                   lj_pairs=[] if eps_on is None else [pr for pr in inside + outside if eps_on[pr[0]]])


for _m in METHODS:
    _case('faces-%s' % _m, _faces, method=_m)
    _case('outside-%s' % _m, _outside, method=_m)
for _m in ('lj', 'rf_split', 'pme_split'):
    for _d in (1, 2, 3):
        _case('min_box%d-%s' % (_d, _m), _min_box, method=_m, dims=_d)
    _case('thin-%s' % _m, _thin, method=_m)
    _case('blob-%s' % _m, _blob, method=_m)
    _case('molecules-%s' % _m, _molecules, method=_m)
DIMER_METHODS = ('lj_noswitch', 'rf', 'rf_split', 'pme', 'pme_far')
for _m in DIMER_METHODS:
    _case('dimers-%s' % _m, _dimers, method=_m)


# ---- exclusion-window edges ---------------------------------------------------------------------------------------------------
EXCL_D = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 223, 224, 255)
EXCL_N = 258


def words_of(d):
    return max(1, (d + 32) // 32)


def _around(rng, box, n, fixed):
    """(x, the planted indices): the atoms of `fixed` (index -> position) where they are, the others uniform at the minimum distance from
    them and from each other"""
    keys = sorted(fixed)
    x0 = np.array([fixed[k] for k in keys])
    rest = _place(rng, n - len(keys), box, lambda i: rng.uniform(0.0, 1.0, 3) * box, x0=x0)[len(keys):]
    x = np.zeros((n, 3))
    x[keys] = x0
    x[[k for k in range(n) if k not in fixed]] = rest
    return x, keys


def _planted_many(rng, box, n, plants, near=0.1, neighbours=0.3):
    """bulk, with every (hub, partner, neighbour indices) of `plants` planted: the partner `near` from its hub, the neighbours (atoms next
    to the partner in the index or LJ-ordinal order, not excluded from the hub) `neighbours` from it; the hubs sit on the box diagonal"""
    fixed = {}
    taken = {a for hub, partner, nbrs in plants for a in (hub, partner)}
    at_frac = [0.5] if len(plants) == 1 else [0.2 + 0.6 * k / (len(plants) - 1) for k in range(len(plants))]
    for (hub, partner, nbrs), fr in zip(plants, at_frac):
        assert hub not in fixed
        fixed[hub] = fr * box
    for hub, partner, nbrs in plants:
        c0 = fixed[hub]

        def at(r):
            for t in range(100000):
                v = rng.normal(size=3)
                c = c0 + r * v / np.linalg.norm(v)
                others = [p for k, p in fixed.items() if k != hub]
                if not others or _min_image_dist(np.array(others), c[None], box).min() >= DMIN + PAD:
                    return c
            raise AssertionError('no room around the hub')
        assert partner not in fixed
        fixed[partner] = at(near)
        for k in nbrs:
            if 0 <= k < n and k not in fixed and k not in taken:
                fixed[k] = at(neighbours)
    return _around(rng, box, n, fixed)


def _planted(rng, box, n, hub, partner, near=0.1, neighbours=0.3):
    """one plant: the partner's index neighbours are the neighbours"""
    return _planted_many(rng, box, n, [(hub, partner, (partner - 1, partner + 1))], near, neighbours)


def _excl(cid, method, d, off):
    """one exclusion (off, off + d): the partner 0.1 nm from the hub, the partner's index neighbours (not excluded) at 0.3 nm.  The
    component {off, off + d} spans unrelated free atoms, which the build rules take into its group; `off` free atoms come first"""
    n = EXCL_N + off
    ex = [(off, off + d, 0.0, 0.1, 0.0)]
    groups = [1] * off + [d + 1] + [1] * (n - off - d - 1)
    return _drawn(cid, method, n, lambda rng, box, m: _planted(rng, box, m, off, off + d), exceptions=ex, box=np.array([2.35, 2.5, 2.7]),
                  claims=dict(N=n, words=words_of(d), excl_W=4 * words_of(d) + 1, groups=groups), hub=off, partner=off + d,
                  plants=[(off, off + d, (off + d - 1, off + d + 1))])


for _m in ('lj', 'pme_split'):
    for _d in EXCL_D:
        _case('excl-%s-d%d' % (_m, _d), _excl, method=_m, d=_d, off=0)
    for _o in range(1, 8):
        _case('excl-%s-d65-o%d' % (_m, _o), _excl, method=_m, d=65, off=_o)
for _d in (31, 64, 255):
    _case('excl-rf_split-d%d' % _d, _excl, method='rf_split', d=_d, off=0)


def _exc14(cid, method, across):
    """exceptions with non-zero parameters (1-4 style) at index distances 3 and 40, their atoms farther apart than the cutoff (0.8 nm):
    no cutoff, no switch, the minimum image -- `across`: the pair straddles a box face"""
    n = 72
    box = box_for(n, method) * 1.25

    def place(rng, b, m):
        fixed = {}
        for k, (a, p) in enumerate(((0, 3), (10, 50))):
            if across:
                fixed[a] = np.array([0.15, (0.3 + 0.4 * k) * b[1], (0.3 + 0.4 * k) * b[2]])
                fixed[p] = fixed[a] - np.array([0.8, 0.0, 0.0])          # at x = -0.65: the other side of the face x = 0
            else:
                v = rng.normal(size=3)
                fixed[a] = (0.3 + 0.4 * k) * b
                fixed[p] = fixed[a] + 0.8 * v / np.linalg.norm(v)
        return _around(rng, b, m, fixed)
    ex = [(0, 3, 0.05, 0.3, 0.4), (10, 50, -0.04, 0.32, 0.5)]
    return _drawn(cid, method, n, place, exceptions=ex, box=box, claims=dict(N=n, words=2, exc14=[(0, 3), (10, 50)], across=across))


def _lj_ordinal(cid, method, variant):
    """the LJ sub-system's window lives in LJ-ordinal space (LJ atoms are every third atom).  a: exclusions between LJ atoms 96 indices =
    32 ordinals apart: 4 words in the main system, 2 in the LJ sub-system.  b: exclusions 64 indices apart between an LJ atom and one
    without (3 words) and 60 indices = 20 ordinals apart between LJ atoms: 3 words in the main system, 1 in the LJ sub-system.  Every
    excluded partner sits 0.1 nm from its hub; the partner's neighbours -- the next LJ atoms on either side (+-3 indices, +-1 ordinal)
    and the next atoms on either side (+-1 index) -- are not excluded and sit 0.3 nm from the hub"""
    n = 200
    if variant == 'a':
        pairs = [(3 * k, 3 * k + 96) for k in (0, 5, 11)]
        claims = dict(N=n, words=4, lj_words=2)
    else:
        pairs = [(0, 64), (9, 73), (30, 90)]
        claims = dict(N=n, words=3, lj_words=1)
    plants = [(h, p, (p - 3, p + 3, p - 1, p + 1)) for h, p in pairs]
    return _drawn(cid, method, n, lambda rng, box, m: _planted_many(rng, box, m, plants), exceptions=[(h, p, 0.0, 0.1, 0.0) for h, p in pairs],
                  claims=claims, plants=plants)


def _interleaved(cid, method):
    """exceptions (0, 2) and (1, 3) -- two components the build merges into one group of four -- and (10, 20): a component whose span
    holds nine free atoms.  Planted as above: partners at 0.1 nm, their index neighbours at 0.3 nm"""
    n = 65
    pairs = [(0, 2), (1, 3), (10, 20)]
    plants = [(h, p, (p - 1, p + 1)) for h, p in pairs]
    return _drawn(cid, method, n, lambda rng, box, m: _planted_many(rng, box, m, plants), exceptions=[(h, p, 0.0, 0.1, 0.0) for h, p in pairs],
                  claims=dict(N=n, words=1, groups=[4] + [1] * 6 + [11] + [1] * 44), plants=plants)


for _m in ('lj', 'pme_split'):
    _case('exc14-%s-inside' % _m, _exc14, method=_m, across=False)
    _case('exc14-%s-across' % _m, _exc14, method=_m, across=True)
    _case('interleaved-%s' % _m, _interleaved, method=_m)
for _m in ('rf_split', 'pme_split'):
    _case('ljord-%s-a' % _m, _lj_ordinal, method=_m, variant='a')
    _case('ljord-%s-b' % _m, _lj_ordinal, method=_m, variant='b')


# the exclusion family: every case whose exceptions are what it is about
EXCL_CASES = [c for c in CASES if c.split('-')[0] in ('excl', 'exc14', 'ljord', 'interleaved')]


# ---- replicas -----------------------------------------------------------------------------------------------------------------
def _replicas3(cid, method):
    """R = 3 with three different boxes (the factors of pme_edge_cases.BOXES['per_replica']), each replica with its own positions"""
    from oracle.forcefield import ForceFieldOracle
    n = 129
    f = PME_BOXES['per_replica'] / PME_BOXES['per_replica'][0]
    box = box_for(n, method)[None] * f
    rng = np.random.default_rng(case_seed(cid))
    q = _charges(rng, n)
    c = _finish(cid, method, np.zeros((1, n, 3)), box[0], q=q)
    xs = [fresh_positions(c, rng, box[r]) for r in range(3)]
    return _finish(cid, method, np.stack(xs), box, q=q, claims=dict(N=n, R=3))


for _m in ('rf_split', 'pme_split'):
    _case('rep3-%s' % _m, _replicas3, method=_m)


# ---- alchemical ---------------------------------------------------------------------------------------------------------------
LAMBDAS = np.array([1.0, 0.5, 0.0])


def _alch(cid, method, what, annihilate=False):
    """the first third of the atoms is the region; three states and one replica in each (the same positions): `s` steps lambda_sterics
    through 1, 0.5, 0 at lambda_electrostatics 1 (0 where lambda_sterics is 0: a charge without a core), `e` lambda_electrostatics at
    lambda_sterics 1"""
    n = 65
    c = _drawn(cid, method, n, bulk, alch=range(n // 3), annihilate=annihilate, claims=dict(N=n, n_alch=n // 3))
    ls = LAMBDAS if what == 's' else np.ones(3)
    le = np.ones(3) if what == 's' else LAMBDAS
    if what == 's' and METHODS[method][1]:
        le = np.array([1.0, 1.0, 0.0])
    c['x'], c['box'], c['lam'] = np.tile(c['x'], (3, 1, 1)), np.tile(c['box'], (3, 1)), (ls, le)
    return c


def _softcore(cid, method):
    """states lambda_sterics 0.5 and 0 (lambda_electrostatics 0); an alchemical atom 0.05 nm from a non-alchemical one that carries
    Lennard-Jones: the soft core is finite there, plain Lennard-Jones is 4 eps (sigma / r)^12 = 4e10 kJ/mol"""
    n = 65
    c = _drawn(cid, method, n, lambda rng, box, m: _planted(rng, box, m, 0, 30, near=0.05, neighbours=0.3), alch=range(n // 3),
               claims=dict(N=n, n_alch=n // 3), hub=0, partner=30)
    c['x'], c['box'] = np.tile(c['x'], (2, 1, 1)), np.tile(c['box'], (2, 1))
    c['lam'] = (np.array([0.5, 0.0]), np.zeros(2) if METHODS[method][1] else np.ones(2))
    return c


for _m in METHODS:
    _case('alch_s-%s' % _m, _alch, method=_m, what='s')
    if METHODS[_m][1]:
        _case('alch_e-%s' % _m, _alch, method=_m, what='e')
_case('alch_s-lj-annihilate', _alch, method='lj', what='s', annihilate=True)
for _m in ('lj', 'pme_split'):
    _case('softcore-%s' % _m, _softcore, method=_m)
UKL_CASES = ('alch_s-lj', 'alch_s-pme_split', 'alch_e-pme_split', 'softcore-lj', 'softcore-pme_split')

# the same cases on the 64-atom tile kernel (REMD_NB_TILES=1): id + '+tiles'
TILE_CASES = ['size-%s-129' % m for m in METHODS] + ['faces-lj', 'faces-pme_split', 'molecules-rf_split', 'excl-lj-d255', 'excl-pme_split-d65',
                                                      'alch_s-lj', 'alch_s-pme_split', 'dimers-pme_far']
ALL_CASES = list(CASES) + [c + '+tiles' for c in TILE_CASES]
# the other lists test_pair_edges_gpu.py parametrizes over
DIMER_CASES = ['dimers-%s' % m for m in DIMER_METHODS] + ['dimers-pme_far+tiles']
OUTSIDE_CASES = ['outside-%s' % m for m in METHODS]
REPLICA_CASES = ['rep3-rf_split', 'rep3-pme_split']
LIVE_CASES = ['molecules-lj', 'molecules-pme_split']     # (exceptions keep the Lennard-Jones one off the resident small-system kernel)

_BUILT = {}


def build_case(cid):
    cid = cid.split('+')[0]
    if cid not in _BUILT:
        fn, kw = CASES[cid]
        _BUILT[cid] = fn(cid, **kw)
    c = _BUILT[cid]
    return dict(c, desc=dict(c['desc']), x=c['x'].copy(), box=c['box'].copy())


def fresh_positions(case, rng, box):
    """the case's atoms placed anew in `box` [3] (bulk, out of the cutoff bands, totals that do not cancel: the rules of _drawn)"""
    from oracle.forcefield import ForceFieldOracle
    ff = ForceFieldOracle(case['desc'])
    n, method = case['x'].shape[1], case['method']
    for attempt in range(16):
        x = out_of_bands(rng, bulk(rng, box, n), box, sorted({CUTOFF, longest_cutoff(method)}))
        e = ff.energy_forces(x, box, forces=False)[0]
        if METHODS[method][0] and abs(e) < 0.05 * abs(self_energy(case['desc'])):
            continue
        if abs(ff.energy_forces(x, box, forces=False, classes={4})[0]) >= 0.02 * abs(e):
            return x
    raise AssertionError('no configuration with a total that does not cancel')


# ---- engines and the oracle -------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def switches(**kw):
    """the engine's switches are read when a handle is made"""
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def make_engine(make, cid):
    if cid.endswith('+tiles'):
        with switches(REMD_NB_TILES='1'):
            return make()
    return make()


def setup_engine(eng, case, x=None, box=None):
    """one state per replica when the case has lambdas (replica r in state r), else one state for all"""
    x = case['x'] if x is None else x
    box = case['box'] if box is None else box
    R = len(x)
    eng.set_system(case['desc'])
    if case['lam'] is None:
        eng.set_states(np.full(1, BETA))
        labels = np.zeros(R, dtype=np.int64)
    else:
        ls, le = case['lam']
        assert len(ls) == R
        eng.set_states(np.full(R, BETA), np.asarray(ls, dtype=np.float64), np.asarray(le, dtype=np.float64))
        labels = np.arange(R, dtype=np.int64)
    eng.set_integrator('V R O R V', 0.001, 1.0, 1, True, 1e-8)
    eng.set_replicas(R, 0, x, None, box, labels)
    eng.set_force_groups(FORCE_GROUPS)
    return eng


def evaluate(eng):
    """(direct-space group forces [R][N][3], total potential [R], u_kl rows [R][K], the fp32-rounded positions the engine holds)"""
    rows, U = eng.compute_energies(want_potential=True)
    f = eng.get_forces(groups=1 << DIRECT_GROUP)
    return f, U.copy(), np.array(rows, dtype=np.float64).copy(), eng.get_replicas()[0]


AGED_STEPS = (20, 45)


def aged_order_run(eng, case, steps, more=25):
    """`steps` MD steps of 1 fs on the handle (V R O R V: one force evaluation per step), then get_forces of the direct-space group behind
    them; after 20 steps `more` further get_forces calls, which move no atom but count as evaluations.
    -> ({label: (forces, fp32 positions)}, the largest displacement of an atom)"""
    setup_engine(eng, case)
    eng.set_integrator('V R O R V', 0.001, 1.0, int(steps), True, 1e-8)
    x0 = eng.get_replicas()[0]
    assert not np.any(eng.propagate(0))
    got = {'behind the run': (eng.get_forces(groups=1 << DIRECT_GROUP), eng.get_replicas()[0])}
    if steps < 40:
        for k in range(more):
            f = eng.get_forces(groups=1 << DIRECT_GROUP)
        got['%d evaluations later' % more] = (f, eng.get_replicas()[0])
        assert np.array_equal(got['behind the run'][1], got['%d evaluations later' % more][1])
    d = got['behind the run'][1] - x0
    d -= case['box'][:, None, :] * np.rint(d / case['box'][:, None, :])
    return got, float(np.abs(d).max())


def oracle_reference(case, xd, box=None):
    """f64: (class-4 forces [R][N][3], class-4 energy [R], total energy [R])"""
    from oracle.forcefield import ForceFieldOracle
    ff = ForceFieldOracle(case['desc'])
    box = case['box'] if box is None else box
    f4, e4, et = [], [], []
    for r in range(len(xd)):
        ls, le = (1.0, 1.0) if case['lam'] is None else (float(case['lam'][0][r]), float(case['lam'][1][r]))
        e, f = ff.energy_forces(xd[r], box[r], lambda_sterics=ls, lambda_electrostatics=le, classes={4})
        f4.append(f)
        e4.append(e)
        et.append(ff.energy_forces(xd[r], box[r], lambda_sterics=ls, lambda_electrostatics=le, forces=False)[0])
    return np.stack(f4), np.array(e4), np.array(et)


def oracle_rows(case, xd):
    """beta x the potential of replica r's configuration at every state: the u_kl rows"""
    from oracle.forcefield import ForceFieldOracle
    ff = ForceFieldOracle(case['desc'])
    ls, le = case['lam']
    return np.stack([BETA * np.array([ff.potential(xd[r], case['box'][r], float(a), float(b)) for a, b in zip(ls, le)]) for r in range(len(xd))])


def dimer_atom_error(case, f, f4):
    """the largest per-atom |df| / |f_ref,i| over the atoms of the pairs inside the cutoff (0 where the case has none)"""
    if not case.get('inside'):
        return 0.0
    at = np.array(case['inside']).reshape(-1)
    return float((np.linalg.norm(f[at] - f4[at], axis=1) / np.linalg.norm(f4[at], axis=1)).max())


def errors(case, f, U, f4, e4, et):
    """per replica: max |df| and the RMS of the per-atom error vector over max |f_ref| of the group, the dimers' per-atom error,
    |dE| / |E(classes={4})|, |dE| / |E_total|"""
    rows = []
    for r in range(len(f)):
        d = f[r] - f4[r]
        fmax = np.abs(f4[r]).max()
        de = abs(U[r] - et[r])
        rows.append(dict(f_max_rel=np.abs(d).max() / fmax, f_rms_rel=math.sqrt((d * d).sum(axis=1).mean()) / fmax,
                         f_atom_rel=dimer_atom_error(case, f[r], f4[r]), e_rel=de / abs(e4[r]), e_tot_rel=de / abs(et[r]),
                         f_ref=fmax, e_direct=e4[r], e_total=et[r]))
    return rows


# ---- bounds -----------------------------------------------------------------------------------------------------------------
COLUMNS = ('f_max_rel', 'f_rms_rel', 'f_atom_rel', 'e_rel', 'e_tot_rel')
# the bars the suite already sets: 2e-4 of max |f_ref| for Lennard-Jones and the reaction field (test_lj_fluid_energy_and_forces), 1e-3 under
# Ewald (test_force_groups._follows), 1e-5 of the total potential
BARS = {'lj': 2e-4, 'rf': 2e-4, 'ewald': 1e-3}
E_TOTAL_BAR = 1e-5


def read_error_table(path=ERROR_TABLE):
    rows = []
    if not os.path.exists(path):
        return rows
    with open(path) as fh:
        for line in fh:
            t = line.split('|')[0].split()
            if len(t) == 4 + len(COLUMNS) and t[0] == 'row':
                rows.append(dict(case=t[1], r=int(t[2]), n=int(t[3]), **{k: float(v) for k, v in zip(COLUMNS, t[4:])}))
    return rows


def case_family(cid):
    return FAMILY[build_method(cid)]


def build_method(cid):
    return CASES[cid.split('+')[0]][1]['method']


def family_maxima(rows):
    """family -> column -> the largest recorded value, families lj, rf and ewald.  Under Ewald the force columns hold the force-only launch
    (the force table) and the energy columns the evaluation with energies (the polynomial erfc).  NOT covered: the forces that the
    evaluation with energies computes with the polynomial erfc.  The ABI has no way to read them -- get_forces always evaluates again,
    force-only -- so only that launch's energies are compared."""
    out = {}
    for w in rows:
        m = out.setdefault(case_family(w['case']), {k: 0.0 for k in COLUMNS})
        for k in COLUMNS:
            m[k] = max(m[k], w[k])
    return out


_BOUNDS = {}


def bounds(family):
    """4 x the largest recorded value per family and column (the factor of the PME edge tests, for other seeds and summation orders), the
    force columns never looser than BARS; without a table the bars themselves (f_rms_rel then has the bar of f_max_rel).  e_tot_rel is
    the suite's 1e-5 of the total potential whatever was recorded."""
    if not _BOUNDS:
        mx = family_maxima(read_error_table())
        for fam, bar in BARS.items():
            m = mx.get(fam)
            b = {k: (min(4.0 * m[k], bar) if m else bar) for k in ('f_max_rel', 'f_rms_rel', 'f_atom_rel')}
            b['e_rel'] = 4.0 * m['e_rel'] if m else float('inf')
            b['e_tot_rel'] = E_TOTAL_BAR
            _BOUNDS[fam] = b
    return _BOUNDS[family]
