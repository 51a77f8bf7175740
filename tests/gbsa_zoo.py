"""Shared by tests/test_gbsa_zoo_cpu.py and tests/test_gbsa_zoo_gpu.py: implicit-solvent cases that reach every branch of the pair
function H(r; or_i, sr_j) of the Born-radius sum (csrc/gbsa.hip gb_H, oracle/cpu/remd_cpu.cpp gb_H), at the atom counts where the
kernels change path.  An ORDERED pair (i, j) -- atom j seen from atom i -- is in one of four regimes:

  zero      r + sr_j < or_i                       j lies inside i's own sphere, H = 0
  engulfed  sr_j - r >= or_i                      i lies inside j's scaled sphere: the C term, L = sr_j - r, dL/dr = -1
  partial   |r - sr_j| <= or_i  (and not zero)    the spheres intersect, L = or_i
  far       |r - sr_j| >  or_i  (not engulfed)    L = |r - sr_j|

(or = radius - offset, sr = scale * or).  Every case pins, by assertions in the CPU file, which regimes it reaches.

The nonbonded parameters of every case are zero, so that GB is the only term and a bound relative to the largest force component is a
bound on GB.  Pairs closer than MIN_DISTANCE are never built: below it log(L/U)/r^2 loses digits in f32 that f64 keeps.

Bounds.  Every case is held to the project's GB tolerances (tests/test_gbsa.py): energy rtol 5e-6 with atol 100 rtol, force error below
2e-4 of the largest reference force component, alchemical rows 1e-5.  None had to be widened: on the MI355X the worst figures were
4e-6 (energy, the two-atom scan), 4e-5 (force, the two-atom scan; 2e-5 in the zoos) and 4e-7 (rows).  Should a case ever need more
room, its bound is 4 x f32_error of that case -- the oracle's expressions in numpy float32 against the f64 oracle, measured without
any kernel -- recorded here next to the case; never a figure taken from a kernel's output.
"""
import numpy as np

from openmmtools_amd.system import System, NonbondedForce, GBSAOBCForce, CustomGBForce

OFFSET = 0.009
RADII = (0.05, 0.12, 0.2, 0.45)
SCALES = (0.5, 0.85, 1.2)
MIN_DISTANCE = 0.02
CELL, CELL_ATOMS = 0.9, 96                 # the cube of the recipe and the atom count it was tried at: the density of the larger cases
JITTER = 0.001                             # replica r is moved by JITTER (r + 1) N(0, 1) per coordinate
BORDER_GUARD = 1e-4                        # pair_scan: no point this close to a regime border (dH has kinks there)
ZOO_BORDER_GUARD = 1e-6                    # the zoos: no pair this close to one (f32 positions put r on the other side: ulp(1 nm) = 1.2e-7)
CUTOFF_GUARD = 1e-3                        # periodic_zoo: no pair this close to the cutoff (the energy jumps there)

ENERGY_RTOL, FORCE_TOL, ROWS_RTOL = 5e-6, 2e-4, 1e-5          # tests/test_gbsa.py


def _pairs(x, box=None):
    d = x[None, :, :] - x[:, None, :]
    if box is not None:
        d = d - box * np.round(d / box)
    r = np.sqrt((d * d).sum(-1))
    return d, r


def regime_masks(x, radius, scale, offset=OFFSET, box=None, cutoff=None):
    """[n, n] boolean masks of the ordered pairs (i, j) by regime; the diagonal and (with a cutoff) the pairs out of range are in none"""
    x = np.asarray(x, dtype=np.float64)
    orr = np.asarray(radius, dtype=np.float64) - offset
    sr = np.asarray(scale, dtype=np.float64) * orr
    _, r = _pairs(x, box)
    live = ~np.eye(len(x), dtype=bool)
    if cutoff is not None:
        live &= r < cutoff
    or1, sr2 = orr[:, None], sr[None, :]
    zero = live & (r + sr2 < or1)
    engulfed = live & (sr2 - r >= or1)
    partial = live & ~zero & ~engulfed & (np.abs(r - sr2) <= or1)
    far = live & ~zero & ~engulfed & ~partial
    return dict(zero=zero, partial=partial, far=far, engulfed=engulfed)


def regimes(x, radius, scale, offset=OFFSET, box=None, cutoff=None):
    """the number of ordered pairs in each regime"""
    return {k: int(m.sum()) for k, m in regime_masks(x, radius, scale, offset, box, cutoff).items()}


def border_margin(x, radius, scale, offset=OFFSET, box=None):
    """the smallest distance (nm) of any ordered pair's r from a regime border of that pair: r = or_i - sr_j, sr_j - or_i, sr_j + or_i, sr_j"""
    x = np.asarray(x, dtype=np.float64)
    orr = np.asarray(radius, dtype=np.float64) - offset
    sr = np.asarray(scale, dtype=np.float64) * orr
    _, r = _pairs(x, box)
    or1, sr2 = orr[:, None], sr[None, :]
    off = np.eye(len(x)) * 1e9
    return float(min(np.abs(r - b + off).min() for b in (or1 - sr2, sr2 - or1, sr2 + or1, sr2 + 0.0 * or1))) if len(x) > 1 else np.inf


def jitters(n, R):
    return [JITTER * (r + 1) * np.random.default_rng(1000 + r).normal(size=(n, 3)) for r in range(R)]


def replica_positions(x0, R):
    """R replicas at different jitters (the builders keep MIN_DISTANCE in every one of up to MAX_REPLICAS of them)"""
    return np.stack([x0 + j for j in jitters(len(x0), R)])


MAX_REPLICAS = 3


def _place(n, edge, rng, radius, scale, fixed=None, box=None, cutoff=None):
    """uniform positions in a cube, drawn one atom at a time.  An atom is drawn again if, in any jittered replica, it is closer than
    MIN_DISTANCE to an earlier one, within ZOO_BORDER_GUARD of a regime border with it or -- with a cutoff -- within twice CUTOFF_GUARD
    of the cutoff (twice: the device rounds positions to f32).  fixed: positions of the first atoms, taken as they are."""
    orr = np.asarray(radius) - OFFSET
    sr = np.asarray(scale) * orr
    jit = jitters(n, MAX_REPLICAS)
    x = np.zeros((n, 3))
    n_fixed = 0 if fixed is None else len(fixed)
    redrawn = 0
    for i in range(n):
        while True:
            p = fixed[i] if i < n_fixed else rng.random(3) * edge
            ok = True
            for r in range(MAX_REPLICAS):
                d = (x[:i] + jit[r][:i]) - (p + jit[r][i])
                if box is not None:
                    d = d - box * np.round(d / box)
                dist = np.sqrt((d * d).sum(-1))
                if np.any(dist < MIN_DISTANCE) or (cutoff is not None and np.any(np.abs(dist - cutoff) < 2.0 * CUTOFF_GUARD)):
                    ok = False
                for o, t in ((orr[i], sr[:i]), (orr[:i], sr[i])):
                    for b in (o - t, t - o, t + o, t + 0.0 * o):
                        if np.any(np.abs(dist - b) < 2.0 * ZOO_BORDER_GUARD):
                            ok = False
            if ok:
                break
            assert i >= n_fixed, 'the hand-placed atoms must satisfy the guards themselves'
            redrawn += 1
        x[i] = p
    return x, redrawn


def zoo_parameters(n, rng):
    radius = np.array(RADII)[rng.integers(0, len(RADII), n)]
    scale = np.array(SCALES)[rng.integers(0, len(SCALES), n)]
    charge = rng.normal(0.0, 0.4, n)
    return charge, radius, scale


def zoo_edge(n):
    """the cube of the recipe; beyond 200 atoms a larger cube at the density of CELL_ATOMS atoms per CELL^3"""
    return CELL if n <= 200 else CELL * (n / CELL_ATOMS) ** (1.0 / 3.0)


def _nocutoff_system(charge, radius, scale):
    s = System()
    nb = NonbondedForce(); nb.setNonbondedMethod(NonbondedForce.NoCutoff)
    gb = GBSAOBCForce()
    for q, rad, sc in zip(charge, radius, scale):
        s.addParticle(39.9)
        nb.addParticle(0.0, 0.3, 0.0)
        gb.addParticle(float(q), float(rad), float(sc))
    s.addForce(nb); s.addForce(gb)
    return s


_ZOO = {}


DILUTE = 2.0


def overlap_zoo(n, seed=1, spread=1.0):
    """(System, positions [n, 3], (charge, radius, scale)): a NoCutoff System of a GBSAOBCForce and a NonbondedForce without charges or
    wells, radii from RADII and scales from SCALES, charges N(0, 0.4), positions uniform in a cube of spread x zoo_edge(n).
    spread = 1 is the dense recipe: from 96 atoms on every atom is buried (psi > 1), tanh is 1 to five digits or more and dB/dI, with
    it the whole force through the Born radii, all but vanishes -- a case for the saturated end and for the pair sums, blind to H and
    dH.  spread = DILUTE keeps all four regimes and leaves about half of the atoms on the slope of the tanh (born_saturation)."""
    if (n, seed, spread) not in _ZOO:
        rng = np.random.default_rng(seed)
        charge, radius, scale = zoo_parameters(n, rng)
        x, _ = _place(n, spread * zoo_edge(n), rng, radius, scale)
        _ZOO[n, seed, spread] = (_nocutoff_system(charge, radius, scale), x, (charge, radius, scale))
    return _ZOO[n, seed, spread]


def born_saturation(x, radius, scale, box=None, cutoff=None):
    """(psi, 1 - tanh^2) of every atom at lambda = 1, in f64: dB/dI is proportional to the second"""
    orr = np.asarray(radius) - OFFSET
    sr = np.asarray(scale) * orr
    _, r = _pairs(np.asarray(x, dtype=np.float64), box)
    r = r + np.eye(len(orr))
    or1, sr2 = orr[:, None], sr[None, :]
    U, L = r + sr2, np.maximum(or1, np.abs(r - sr2))
    H = (r + sr2 - or1 >= 0) * 0.5 * (1 / L - 1 / U + 0.25 * (r - sr2 ** 2 / r) * (1 / U ** 2 - 1 / L ** 2) + 0.5 * np.log(L / U) / r
                                      + 2.0 * (1 / or1 - 1 / L) * (sr2 - r - or1 >= 0))
    live = ~np.eye(len(orr), dtype=bool) if cutoff is None else (~np.eye(len(orr), dtype=bool)) & (r < cutoff)
    psi = np.where(live, H, 0.0).sum(1) * orr
    return psi, 1.0 - np.tanh(psi - 0.8 * psi ** 2 + 4.85 * psi ** 3) ** 2


# ---- the two-atom scan ---------------------------------------------------------------------------------------------------------------
# (radius_0, scale_0, radius_1, scale_1); in each, one atom can engulf the other (or_i < sr_j) and be hidden by it the other way round (or_j > sr_i)
PAIR_SETS = ((0.12, 0.85, 0.45, 1.2), (0.2, 1.2, 0.12, 0.5), (0.05, 1.2, 0.2, 1.2))
PAIR_CHARGES = (0.7, -0.5)
PAIR_DIRECTION = np.array([0.36, -0.48, 0.8])              # unit length, oblique to every axis
BORDER_STEP = 1e-3


def pair_borders(p):
    """the regime borders (nm) of both ordered pairs of a parameter set that lie above MIN_DISTANCE"""
    r0, s0, r1, s1 = p
    out = []
    for or_i, sr_j in ((r0 - OFFSET, s1 * (r1 - OFFSET)), (r1 - OFFSET, s0 * (r0 - OFFSET))):
        out += [or_i - sr_j, sr_j - or_i, sr_j + or_i, sr_j]
    return sorted(b for b in out if b > MIN_DISTANCE)


def pair_scan(k):
    """(System, positions [R, 2, 3], r [R], dropped): parameter set k of PAIR_SETS, one replica per distance: 40 distances from 0.02 to
    1.5 nm and the two points at BORDER_STEP on either side of every regime border.  dropped counts the points that had to go because
    they lay within BORDER_GUARD of a border: the grid is built so that it is 0, and the tests assert that."""
    p = PAIR_SETS[k]
    borders = np.array(pair_borders(p))
    grid = np.concatenate([np.geomspace(MIN_DISTANCE, 1.5, 40)] + [[b - BORDER_STEP, b + BORDER_STEP] for b in borders])
    grid = np.sort(grid)
    keep = np.array([np.abs(r - borders).min() >= BORDER_GUARD and r >= MIN_DISTANCE for r in grid])
    r = grid[keep]
    system = _nocutoff_system(PAIR_CHARGES, (p[0], p[2]), (p[1], p[3]))
    x = np.zeros((len(r), 2, 3))
    x[:, 1, :] = r[:, None] * PAIR_DIRECTION
    return system, x, r, int((~keep).sum())


# ---- the periodic case ---------------------------------------------------------------------------------------------------------------
def _obc_custom_gb(cutoff):
    """the OBC2 strings of testsystems.CustomGBForceSystem on a new CutoffPeriodic CustomGBForce (as test_custom_gb_gpu._small_periodic)"""
    from openmmtools_amd import testsystems as ts
    gb0 = ts.CustomGBForceSystem().system.getForce(1)
    gb = CustomGBForce(); gb.setNonbondedMethod(CustomGBForce.CutoffPeriodic); gb.setCutoffDistance(cutoff)
    for p in gb0.per_particle:
        gb.addPerParticleParameter(p)
    for name, v in gb0.globals:
        gb.addGlobalParameter(name, v)
    for c in gb0.computed:
        gb.addComputedValue(*c)
    for t in gb0.energy_terms:
        gb.addEnergyTerm(*t)
    return gb


# pairs joined only by the minimum image, one through each face: (radius, scale) of both atoms, their distance, the axis of the face
#   x: a small atom inside a large one -- (small, large) engulfed, (large, small) zero;  y: two intersecting spheres, both partial;
#   z: a large atom that hides a mid-sized one -- (large, mid) zero, (mid, large) partial
_FACE_PAIRS = (((0.05, 0.85), (0.45, 1.2), 0.10, 0), ((0.2, 0.85), (0.2, 0.85), 0.15, 1), ((0.45, 0.5), (0.12, 0.85), 0.21, 2))


def periodic_shifts(R):
    return [0.37 * r for r in range(R)]


def periodic_replicas(x0, R, edge):
    """R replicas at different jitters, the later ones shifted through the periodic boundary (as test_custom_gb_gpu._replica_positions,
    with this file's jitter: the hand-placed pairs keep their regimes)"""
    return np.stack([np.mod(x0 + j + s, edge) for j, s in zip(jitters(len(x0), R), periodic_shifts(R))])


def periodic_zoo(n=130, edge=3.0, cutoff=1.4, seed=3):
    """(System, positions, box [3], (charge, radius, scale), redrawn): a CutoffPeriodic System of an OBC2-shaped CustomGBForce with the zoo's
    radii and scales and a NonbondedForce without charges or wells.  The first six atoms are three pairs that straddle the x, y and z
    faces of the box (_FACE_PAIRS), the others are uniform in the box.  No pair lies within CUTOFF_GUARD of the cutoff in any of
    MAX_REPLICAS replicas: an atom that would put one there is drawn again (redrawn counts them; what remains is asserted to be none)."""
    key = ('periodic', n, edge, cutoff, seed)
    if key in _ZOO:
        return _ZOO[key]
    rng = np.random.default_rng(seed)
    charge, radius, scale = zoo_parameters(n, rng)
    fixed = np.zeros((6, 3))
    for k, (a, b, dist, axis) in enumerate(_FACE_PAIRS):
        base = np.array([0.9, 1.7, 2.3])[[(k + c) % 3 for c in range(3)]]
        pa, pb = base.copy(), base.copy()
        pa[axis], pb[axis] = 0.4 * dist, edge - 0.6 * dist             # through the face: the minimum image is dist long
        fixed[2 * k], fixed[2 * k + 1] = pa, pb
        radius[2 * k], scale[2 * k] = a
        radius[2 * k + 1], scale[2 * k + 1] = b
    box = np.full(3, edge)
    x, redrawn = _place(n, edge, rng, radius, scale, fixed=fixed, box=box, cutoff=cutoff)
    s = System()
    s.setDefaultPeriodicBoxVectors([edge, 0, 0], [0, edge, 0], [0, 0, edge])
    nb = NonbondedForce(); nb.setNonbondedMethod(NonbondedForce.CutoffPeriodic); nb.setCutoffDistance(cutoff)
    gb = _obc_custom_gb(cutoff)
    for q, rad, sc in zip(charge, radius, scale):
        s.addParticle(39.9)
        nb.addParticle(0.0, 0.3, 0.0)
        gb.addParticle([float(q), float(rad), float(sc)])
    s.addForce(nb); s.addForce(gb)
    _ZOO[key] = (s, x, box, (charge, radius, scale), redrawn)
    return _ZOO[key]


def straddling(x, box):
    """[n, n] mask of the pairs whose minimum image is not the vector inside the box"""
    d = x[None, :, :] - x[:, None, :]
    return np.any(np.round(d / box) != 0.0, axis=-1)


def cutoff_margin(x, box, cutoff):
    """the smallest | r - cutoff | over all pairs (minimum image)"""
    _, r = _pairs(np.asarray(x, dtype=np.float64), box)
    return float(np.abs(r - cutoff)[~np.eye(len(x), dtype=bool)].min())


# ---- the oracle's expressions in f32 -------------------------------------------------------------------------------------------------
def f32_energy_forces(x, charge, radius, scale, alchemical=None, lam=1.0, solute_dielectric=1.0, solvent_dielectric=78.5, sasa=True,
                      box=None, cutoff=None, ke=138.935485, surface=28.3919551, probe=0.14):
    """oracle/gbsa.py (tests/custom_gb_oracle.py with a box and a cutoff) in numpy float32 throughout: a plain loop over the atoms i, every
    expression of the pairs (i, j) as the oracle writes it, the force as the derivative of those expressions (the step functions and
    max() are constants under it).  It measures what f32 costs on a case; no kernel is involved."""
    f = np.float32
    x = np.asarray(x, dtype=np.float32)
    n = len(x)
    q, R, sc = (np.asarray(a, dtype=np.float32) for a in (charge, radius, scale))
    a = np.zeros(n, dtype=np.float32) if alchemical is None else np.asarray(alchemical, dtype=np.float32)
    s = f(lam) * a + (f(1) - a)
    orr = R - f(OFFSET)
    sr = sc * orr
    tau = f(f(1) / f(solute_dielectric) - f(1) / f(solvent_dielectric))
    ke, surface, probe = f(ke), f(surface), f(probe)
    L3 = None if box is None else np.asarray(box, dtype=np.float32)
    cut = None if cutoff is None else f(cutoff)

    def row(i):
        d = x - x[i]
        if L3 is not None:
            d = d - L3 * np.round(d / L3)
        r = np.sqrt((d * d).sum(-1, dtype=np.float32))
        m = np.arange(n) != i
        if cut is not None:
            m &= r < cut
        return d[m], r[m], np.nonzero(m)[0]

    def H_dH(r, or1, sr2):
        U = r + sr2
        D = np.abs(r - sr2)
        moving = D > or1
        L = np.where(moving, D, or1).astype(np.float32)
        dL = np.where(moving, np.where(r > sr2, f(1), f(-1)), f(0)).astype(np.float32)
        inside = sr2 - r - or1 >= 0
        C = np.where(inside, f(2) * (f(1) / or1 - f(1) / L), f(0)).astype(np.float32)
        dC = np.where(inside, f(2) * dL / L ** 2, f(0)).astype(np.float32)
        on = (r + sr2 - or1 >= 0).astype(np.float32)
        lg = np.log(L / U)
        H = on * f(0.5) * (f(1) / L - f(1) / U + f(0.25) * (r - sr2 ** 2 / r) * (f(1) / U ** 2 - f(1) / L ** 2) + f(0.5) * lg / r + C)
        dH = on * f(0.5) * (-dL / L ** 2 + f(1) / U ** 2 + f(0.25) * (f(1) + sr2 ** 2 / r ** 2) * (f(1) / U ** 2 - f(1) / L ** 2)
                            + f(0.25) * (r - sr2 ** 2 / r) * (f(-2) / U ** 3 + f(2) * dL / L ** 3) + f(0.5) * ((dL / L - f(1) / U) / r - lg / r ** 2) + dC)
        return H.astype(np.float32), dH.astype(np.float32)

    B = np.zeros(n, dtype=np.float32); dBdI = np.zeros(n, dtype=np.float32)
    for i in range(n):
        _, r, j = row(i)
        H, _ = H_dH(r, orr[i], sr[j])
        I = (s[j] * H).sum(dtype=np.float32)
        psi = I * orr[i]
        th = np.tanh(psi - f(0.8) * psi ** 2 + f(4.85) * psi ** 3)
        B[i] = f(1) / (f(1) / orr[i] - th / R[i])
        dBdI[i] = B[i] ** 2 * (f(1) - th ** 2) * (f(1) - f(1.6) * psi + f(14.55) * psi ** 2) * orr[i] / R[i]
    E = f(0)
    F = np.zeros((n, 3), dtype=np.float32)
    dEdB = np.zeros(n, dtype=np.float32)
    for i in range(n):
        E += f(-0.5) * ke * tau * s[i] * q[i] ** 2 / B[i]
        dEdB[i] += f(0.5) * ke * tau * s[i] * q[i] ** 2 / B[i] ** 2
        if sasa:
            pre = s[i] * surface * (R[i] + probe) ** 2
            E += pre * (R[i] / B[i]) ** 6
            dEdB[i] -= f(6) * pre * (R[i] / B[i]) ** 6 / B[i]
        d, r, j = row(i)
        BB = B[i] * B[j]
        ex = np.exp(-r ** 2 / (f(4) * BB))
        f2 = r ** 2 + BB * ex
        ff = np.sqrt(f2)
        QQ = ke * tau * (s[i] * q[i]) * (s[j] * q[j])
        E += f(0.5) * (-QQ / ff).sum(dtype=np.float32)
        dEdB[i] += (QQ / f2 * ex * (f(1) + r ** 2 / (f(4) * BB)) / (f(2) * ff) * B[j]).sum(dtype=np.float32)
        F[i] += ((QQ / f2 * (f(1) - f(0.25) * ex) / ff)[:, None] * d).sum(0, dtype=np.float32)
    c = dEdB * dBdI
    for i in range(n):
        d, r, j = row(i)
        _, dH1 = H_dH(r, orr[i], sr[j])
        _, dH2 = H_dH(r, orr[j], sr[i])
        F[i] += (((c[i] * s[j] * dH1 + c[j] * s[i] * dH2) / r)[:, None] * d).sum(0, dtype=np.float32)
    return float(E), F.astype(np.float64)


# ---- running a case on an engine and checking it against the f64 oracle ---------------------------------------------------------------
KB = 0.008314462618153242
BETA = 1.0 / (KB * 300.0)
LADDER_S = np.array([[1.0], [1.0], [0.5], [0.0]])
LADDER_E = np.array([[1.0], [0.4], [0.0], [0.0]])
LADDER_LABELS = np.array([1, 2, 3])


def alchemical_zoo(n, seed=1, spread=1.0):
    """the overlap zoo with every third atom alchemical, by the factory (as test_gbsa._check_alchemical): (System, positions, parameters)"""
    from openmmtools_amd import alchemy
    system, x, par = overlap_zoo(n, seed, spread)
    return alchemy.AbsoluteAlchemicalFactory().create_alchemical_system(system, alchemy.AlchemicalRegion(alchemical_atoms=range(0, n, 3))), x, par


def gb_reference(gb, x, lam=1.0, box=None, forces=True):
    """the f64 oracle of a descriptor's GB part: oracle/gbsa.py without a cutoff, tests/custom_gb_oracle.py with one"""
    if int(gb.get('method', 0)) == 2:
        from custom_gb_oracle import custom_gb_energy_forces
        return custom_gb_energy_forces(x, gb, lam, box, forces=forces)
    from oracle.gbsa import gbsa_energy_forces
    return gbsa_energy_forces(x, gb['charge'], gb['radius'], gb['scale'], gb['alchemical'], lam, gb['solute_dielectric'], gb['solvent_dielectric'],
                              sasa=bool(gb['surface_area']), forces=forces)


def gb_is_the_only_term(desc):
    """every zoo System: no bonded term, no charge and no well outside GB (tests/test_gbsa_zoo_cpu.py also evaluates the other oracles: 0)"""
    assert not np.any(desc['charge']) and not np.any(desc['epsilon']) and desc['n_ext'] == 0
    assert len(desc['bond_atoms']) == len(desc['angle_atoms']) == len(desc['torsion_atoms']) == len(desc['exception_atoms']) == 0
    ar = desc.get('alch_regions')
    assert ar is None or (not np.any(ar['charge']) and not np.any(ar['epsilon']) and len(ar['exception_atoms']) == 0)


def evaluate(eng, desc, X, box=None, ladder=False):
    """potentials, u_kl rows, the positions the engine holds and its forces: R replicas of one state, or (ladder) LADDER_LABELS on the
    four alchemical states of LADDER_S, LADDER_E"""
    R = len(X)
    eng.set_system(desc)
    eng.set_states(np.full(4 if ladder else 1, BETA))
    if ladder:
        eng.set_region_lambdas(LADDER_S, LADDER_E)
    eng.set_integrator('V R O R V', 0.001, 1.0, 1, True, 1e-8)
    eng.seed(6)
    labels = LADDER_LABELS[:R] if ladder else np.zeros(R, dtype=int)
    eng.set_replicas(R, 0, X, None, np.zeros((R, 3)) if box is None else np.tile(box, (R, 1)), labels)
    rows, U = eng.compute_energies(want_potential=True)
    return rows, U, eng.get_replicas()[0], eng.get_forces(), labels


def check_against_oracle(eng, desc, X, rtol, ftol, box=None, ladder=False, rows_rtol=None, name=''):
    """energy and forces of every replica (and, on the ladder, the u_kl row at every state's lambda) against the f64 oracle at the
    positions the engine holds.  Every figure is printed before it is asserted.  Returns (U, forces)."""
    gb_is_the_only_term(desc)
    gb = desc['gbsa']
    rows, U, xd, f, labels = evaluate(eng, desc, X, box, ladder)
    for r in range(len(X)):
        lam = float(LADDER_E[labels[r], 0]) if ladder else 1.0
        if box is not None:                                          # the guard, at the positions the engine holds
            assert cutoff_margin(xd[r], box, float(gb['cutoff'])) >= CUTOFF_GUARD, (name, r)
        e, f_ref = gb_reference(gb, xd[r], lam, box)
        fmax = np.abs(f_ref).max()
        f_err = np.abs(f[r] - f_ref).max()
        print('%s replica %d: E %.10g ref %.10g rel %.3g | force err %.3g of max %.6g (%.3g)' %
              (name, r, U[r], e, abs(U[r] - e) / abs(e), f_err, fmax, f_err / fmax if fmax else 0.0))
        if ladder:
            ref = np.array([gb_reference(gb, xd[r], float(le), box, forces=False)[0] for le in LADDER_E[:, 0]])
            print('%s replica %d: u_kl rows err %.3g of max %.6g' % (name, r, np.abs(rows[r] - BETA * ref).max(), np.abs(BETA * ref).max()))
            assert np.ptp(ref) > 10.0
            assert np.allclose(rows[r], BETA * ref, rtol=rows_rtol, atol=rows_rtol * np.abs(BETA * ref).max()), (name, r)
            assert np.isclose(U[r], ref[labels[r]], rtol=rows_rtol, atol=rows_rtol * np.abs(ref).max()), (name, r)
        else:
            assert np.isclose(U[r], e, rtol=rtol, atol=rtol * 100.0), (name, r, U[r], e)
            assert np.allclose(rows[r], BETA * e, rtol=rtol, atol=rtol * 100.0), (name, r)
        if fmax == 0.0:
            assert not np.any(f[r]), (name, r)                       # (one atom: no pair, no force)
        else:
            assert f_err < ftol * fmax, (name, r, f_err / fmax)
    return U, f


def f32_error(gb, x, lam=1.0, box=None):
    """(relative energy error, force error over the largest reference force component) of f32_energy_forces against the f64 oracle"""
    e, f_ref = gb_reference(gb, x, lam, box)
    cut = float(gb['cutoff']) if int(gb.get('method', 0)) == 2 else None
    e32, f32 = f32_energy_forces(x, gb['charge'], gb['radius'], gb['scale'], gb['alchemical'], lam, gb['solute_dielectric'], gb['solvent_dielectric'],
                                 bool(gb['surface_area']), box if cut else None, cut)
    return abs(e32 - e) / abs(e), float(np.abs(f32 - f_ref).max() / np.abs(f_ref).max())
