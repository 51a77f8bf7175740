"""A "constraint zoo": a handful of atoms holding every kind of constraint unit the engine integrates (csrc/constraint_units.h) --
rigid three-site waters (SETTLE), X-H star clusters with one, two and three hydrogens (SHAKE<2>, <3>, <4>) and unconstrained
atoms (FREE<4> / FREE<1>) -- in any counts, so that the packing rules of remd_build_constraints and every instance of the unit
arithmetic can be held to the f64 oracle one unit at a time.  TEST INFRASTRUCTURE ONLY.

Atom indices of the kinds are INTERLEAVED: the atoms are numbered round-robin over the units (first atom of every unit, then the
second of every unit that has one, ...), and every other cluster lists a hydrogen before its heavy atom, so no unit's atoms are
contiguous and a cluster's centre is not always its lowest index.

Forces are weak on purpose: a harmonic spring from every atom to an atom of the next unit and a NonbondedForce with small charges
and Lennard-Jones sites on the heavy atoms, so that a V substep carries a non-zero force of varied direction.
"""
import numpy as np

from openmmtools_amd.system import System, NonbondedForce, HarmonicBondForce

KINDS = ('water', 'xh1', 'xh2', 'xh3', 'free')
SPACING = 0.45                                   # nm between the units' sites
D_OH, ANGLE_HOH = 0.09572, np.deg2rad(104.52)    # TIP3P
D_HH = 2.0 * D_OH * np.sin(0.5 * ANGLE_HOH)
M_O, M_H, M_H_HMR = 15.9994, 1.008, 4.032
HEAVY = ((12.011, 0.109), (14.007, 0.101))       # (mass, X-H length) of the clusters' heavy atoms, alternating C / N
FREE_MASS = (39.948, 22.98977, 35.453, 12.011)
CUTOFF = 0.8


def _snake_sites(n):
    """n lattice sites in boustrophedon order: consecutive sites are nearest neighbours"""
    side = max(1, int(np.ceil(n ** (1.0 / 3.0) - 1e-9)))
    out = []
    for z in range(side):
        ys = range(side) if z % 2 == 0 else range(side - 1, -1, -1)
        for yi, y in enumerate(ys):
            xs = range(side) if (z * side + yi) % 2 == 0 else range(side - 1, -1, -1)
            for x in xs:
                out.append((x, y, z))
    return np.array(out[:n], dtype=np.float64), side


def _rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    a, b, c, d = q
    return np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                     [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                     [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])


# hydrogens of a star cluster: tetrahedral directions
_TET = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0]]) / np.sqrt(3.0)


class Zoo:
    """system, positions [N, 3], kind_of_atom [N] (index into KINDS), units: list of (kind, [atom indices, centre first]),
    constraints as (i, j, d) arrays, masses"""

    def atoms_of(self, kind):
        return np.flatnonzero(self.kind_of_atom == KINDS.index(kind))


def build(n_water=2, n_xh1=2, n_xh2=2, n_xh3=2, n_free=5, hmr=False, periodic=False, charges=True, water_masses=None, seed=0):
    """water_masses: {water instance: (mO, mH)} for waters that are not H2O (the mixed-mass cases)"""
    rng = np.random.default_rng(1000 + seed)
    counts = dict(water=n_water, xh1=n_xh1, xh2=n_xh2, xh3=n_xh3, free=n_free)
    # the units in interleaved order: one of every kind in turn while they last
    order, left = [], dict(counts)
    while any(left.values()):
        for k in KINDS:
            if left[k] > 0:
                order.append((k, counts[k] - left[k]))
                left[k] -= 1
    sites, side = _snake_sites(len(order))
    # local geometry, masses and nonbonded parameters of every unit; atom 0 of a unit is its centre
    local = []
    for u, (kind, inst) in enumerate(order):
        rot = _rotation(rng)
        origin = 0.2 + SPACING * sites[u] + 0.02 * rng.normal(size=3)
        if kind == 'water':
            mo, mh = (water_masses or {}).get(inst, (M_O, M_H))
            geo = np.array([[0, 0, 0], [D_OH, 0, 0], [D_OH * np.cos(ANGLE_HOH), D_OH * np.sin(ANGLE_HOH), 0]])
            m = [mo, mh, mh]
            nbp = [(-0.10, 0.315, 0.6), (0.05, 0.1, 0.0), (0.05, 0.1, 0.0)]
            cons = [(0, 1, D_OH), (0, 2, D_OH), (1, 2, D_HH)]
        elif kind == 'free':
            geo = np.zeros((1, 3))
            m = [FREE_MASS[inst % len(FREE_MASS)]]
            nbp = [(0.08 if inst % 2 else -0.08, 0.33, 0.5)]
            cons = []
        else:
            nh = int(kind[2])
            mx, d = HEAVY[inst % 2]
            mh = M_H_HMR if hmr else M_H
            if hmr:
                mx -= nh * (M_H_HMR - M_H)
            geo = np.concatenate([np.zeros((1, 3)), d * _TET[:nh]])
            m = [mx] + [mh] * nh
            nbp = [(-0.03 * nh, 0.34, 0.4)] + [(0.03, 0.1, 0.0)] * nh
            cons = [(0, k + 1, d) for k in range(nh)]
        local.append(dict(kind=kind, inst=inst, x=origin + geo @ rot.T, m=m, nb=nbp, cons=cons))
    # atom numbering: round-robin over the units; every other cluster hands out a hydrogen before its centre
    for u, L in enumerate(local):
        n = len(L['m'])
        L['give'] = list(range(n))
        if L['kind'] in ('xh1', 'xh2', 'xh3') and L['inst'] % 2 == 1:
            L['give'] = [1, 0] + list(range(2, n))
        L['index'] = [None] * n
    nxt, rank = 0, 0
    while True:
        gave = False
        for L in local:
            if rank < len(L['give']):
                L['index'][L['give'][rank]] = nxt
                nxt += 1
                gave = True
        if not gave:
            break
        rank += 1
    N = nxt
    z = Zoo()
    mass, pos, kind_of = np.zeros(N), np.zeros((N, 3)), np.zeros(N, dtype=np.int64)
    nbpar = [None] * N
    for L in local:
        for k, a in enumerate(L['index']):
            mass[a], pos[a], kind_of[a], nbpar[a] = L['m'][k], L['x'][k], KINDS.index(L['kind']), L['nb'][k]
    if not charges:
        nbpar = [(0.0, s, e) for (_, s, e) in nbpar]
    s = System()
    for a in range(N):
        s.addParticle(float(mass[a]))
    nb = NonbondedForce()
    if periodic:
        nb.setNonbondedMethod(NonbondedForce.CutoffPeriodic)
        nb.setCutoffDistance(CUTOFF)
        nb.setUseSwitchingFunction(False)
        nb.setUseDispersionCorrection(False)
        edge = max(side * SPACING + 0.2, 3.0)
        s.setDefaultPeriodicBoxVectors([edge, 0, 0], [0, edge, 0], [0, 0, edge])
    else:
        nb.setNonbondedMethod(NonbondedForce.NoCutoff)
    for a in range(N):
        nb.addParticle(*nbpar[a])
    bonds = HarmonicBondForce()
    cons_i, cons_j, cons_d = [], [], []
    for u, L in enumerate(local):
        idx = L['index']
        for (i, j, d) in L['cons']:
            s.addConstraint(idx[i], idx[j], d)
            cons_i.append(idx[i]); cons_j.append(idx[j]); cons_d.append(d)
        for i in range(len(idx)):
            for j in range(i + 1, len(idx)):
                nb.addException(idx[i], idx[j], 0.0, 1.0, 0.0)
        # a weak spring from every atom to the centre of the next unit (the last unit: of the one before it), stretched by 10 %
        other = local[u + 1] if u + 1 < len(local) else (local[u - 1] if u > 0 else None)
        if other is not None:
            b = other['index'][0]
            for a in idx:
                bonds.addBond(a, b, 0.9 * float(np.linalg.norm(pos[a] - pos[b])), 400.0)
    s.addForce(nb)
    if bonds.getNumBonds():
        s.addForce(bonds)
    z.system, z.positions, z.kind_of_atom, z.mass = s, pos, kind_of, mass
    z.units = [(L['kind'], list(L['index'])) for L in local]
    z.cons = (np.array(cons_i, dtype=int), np.array(cons_j, dtype=int), np.array(cons_d))
    z.box = np.diag(s.getDefaultPeriodicBoxVectors()) if periodic else np.zeros(3)
    z.n_constraints = len(cons_d)
    return z


# (n_water, n_xh1, n_xh2, n_xh3, n_free) of the tests (tests/test_constraint_units_gpu.py; the oracle side of each is checked on the
# CPU in tests/test_oracle_md.py)
MAIN = (2, 2, 2, 2, 5)
# packing edges of remd_build_constraints: free atoms modulo four next to one water and one CH2; 0 / 63 / 64 / 65 waters (none, one
# short of a wavefront of SETTLE units, exactly one, one more) without and with one cluster -- no water and no cluster is ONE free atom:
# both paddings run on empty tables and the handle holds a single one-atom unit; clusters only
PACKING = ([(1, 0, 1, 0, f) for f in (0, 1, 2, 3, 4, 5, 7)]
           + [(w, 0, c, 0, 1) for w in (0, 63, 64, 65) for c in (0, 1)]
           + [(0, 0, 0, 3, 0)])
MIXED_WATERS = {'d2o': {1: (M_O, 2.014)}, 'o18': {1: (17.999, M_H)}}


def unit_momenta(zoo, v):
    """sum(m v) [..., n_units, 3] and sum(|m v|) [..., n_units] of every unit"""
    p = zoo.mass[:, None] * v
    P = np.stack([p[..., idx, :].sum(axis=-2) for _, idx in zoo.units], axis=-2)
    S = np.stack([np.linalg.norm(p[..., idx, :], axis=-1).sum(axis=-1) for _, idx in zoo.units], axis=-1)
    return P, S
