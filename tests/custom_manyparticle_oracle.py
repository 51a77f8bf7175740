"""f64 reference for CustomManyParticleForce with three particles per set (openmmtools_amd/custom_expr.py kind 11,
csrc/custom_manyparticle.hip), independent of the package (it imports nothing from it) and of the engine's enumeration: no neighbour
rows, no central particles.  It goes over ALL N^3 ordered candidates (p1, p2, p3) and applies the definition directly: an assignment is
admissible when the three particles differ, no pair among them is excluded, the cutoff holds (SinglePermutation: all three distances
below it; UniqueCentralParticle: the two distances to p1; minimum image under CutoffPeriodic) and the particle in slot s has a type the
filter of slot s admits.  The admissible assignments of one set -- the unordered {i, j, k} in SinglePermutation, (p1, {p2, p3}) in
UniqueCentralParticle -- are ordered lexicographically by atom indices, and the first is evaluated.  Positions are the f32-rounded ones
the device holds (the caller rounds them).  Every set is evaluated through the dual numbers of tests/custom_dual_oracle.py, so the
derivatives are exact."""
import keyword
import re

import numpy as np

import custom_dual_oracle as dual

NO_CUTOFF, CUTOFF_NON_PERIODIC, CUTOFF_PERIODIC = 0, 1, 2
SINGLE_PERMUTATION, UNIQUE_CENTRAL_PARTICLE = 0, 1
SLOTS = dict(p1=0, p2=1, p3=2)


def _rename(name):
    """(the dual oracle evaluates the string as Python: a name that is a Python keyword -- a global called lambda -- gets a trailing _)"""
    return name + '_' if keyword.iskeyword(name) else name


def named_slots(energy):
    """the particle slots the expression names (every occurrence of p1 p2 p3 as a whole word)"""
    return sorted({SLOTS[w] for w in re.findall(r'[A-Za-z_][A-Za-z_0-9]*', energy) if w in SLOTS})


def distances(x, box=None, method=NO_CUTOFF):
    """[N][N]: the distance of every pair, the image where the method is CutoffPeriodic"""
    x = np.asarray(x, dtype=np.float64)
    d = x[None, :, :] - x[:, None, :]
    if method == CUTOFF_PERIODIC:
        L = np.asarray(box, dtype=np.float64)
        d = d - L * np.rint(d / L)
    return np.sqrt((d * d).sum(axis=2))


def set_energy(expression, x3, box, periodic, values, functions, gradients=True):
    """(energy, dE/dx [3][3]) of one set at the positions of p1 p2 p3"""
    p = dual.seeds(np.asarray(x3, dtype=np.float64), gradients)
    pbox = box if periodic else None
    v = dict(distance=lambda i, j: dual.distance(p, i, j, pbox), angle=lambda i, j, k: dual.angle(p, i, j, k, pbox),
             dihedral=lambda i, j, k, l: dual.dihedral(p, i, j, k, l, pbox))
    v.update(SLOTS)
    v.update(values)
    e = expression(v, dict(dual.FUNCTIONS, **functions))
    if not isinstance(e, dual.Dual):
        return float(e), np.zeros((3, 3))
    return e.v, (e.g.reshape(3, 3) if gradients and e.g.size else np.zeros((3, 3)))


def enumerate_sets(x, types, filters, box=None, method=NO_CUTOFF, cutoff=0.0, exclusions=(), mode=SINGLE_PERMUTATION):
    """([S][3] the evaluated assignments (p1, p2, p3), r_all the distances of all non-excluded pairs): the brute-force cube"""
    N = len(x)
    r = distances(x, box, method)
    pair_ok = ~np.eye(N, dtype=bool)
    for a, b in exclusions:
        pair_ok[int(a), int(b)] = pair_ok[int(b), int(a)] = False
    near = np.ones((N, N), dtype=bool) if method == NO_CUTOFF else r < cutoff
    types = np.asarray(types, dtype=np.int64)
    admits = [np.ones(N, dtype=bool) if not f else np.isin(types, list(f)) for f in (filters or ((), (), ()))]
    ok = pair_ok[:, :, None] & pair_ok[:, None, :] & pair_ok[None, :, :]                       # [p1][p2][p3]: every pair differs and is not excluded
    ok &= near[:, :, None] & near[:, None, :]                                                    # p1-p2 and p1-p3
    if mode == SINGLE_PERMUTATION:
        ok &= near[None, :, :]                                                                   # and p2-p3
    ok &= admits[0][:, None, None] & admits[1][None, :, None] & admits[2][None, None, :]
    chosen, seen = [], set()
    for a, b, c in np.argwhere(ok).tolist():                                                     # (lexicographic in (p1, p2, p3))
        key = frozenset((a, b, c)) if mode == SINGLE_PERMUTATION else (a, frozenset((b, c)))
        if key not in seen:
            seen.add(key)
            chosen.append((a, b, c))
    iu = np.triu_indices(N, 1)
    return np.array(chosen, dtype=np.int64).reshape(-1, 3), r[iu][pair_ok[iu]]


def evaluate(energy, names, params, types, filters, global_values, x, box=None, method=NO_CUTOFF, cutoff=0.0, exclusions=(),
             mode=SINGLE_PERMUTATION, functions=None):
    """dict(E [S] set energies, F [N][3], sets [S][3] the atoms of p1 p2 p3 of every evaluated set, r_all the distances of ALL
    non-excluded pairs, count [N] contributions per atom (one per set and named particle slot that is this atom), peak [N] the largest
    |component| any one contribution has) of one force.  params [N][len(names)]; parameter q of the particle in slot s is names[q] + str(s + 1)."""
    x = np.asarray(x, dtype=np.float64)
    params = np.asarray(params, dtype=np.float64).reshape(len(x), -1)
    expression = dual.Expression(re.sub(r'[A-Za-z_][A-Za-z_0-9]*', lambda m: _rename(m.group(0)), energy))
    slots = named_slots(energy)
    g = {_rename(n): float(v) for n, v in global_values.items()}
    sets, r_all = enumerate_sets(x, types, filters, box, method, cutoff, exclusions, mode)
    E, F = np.zeros(len(sets)), np.zeros_like(x)
    count, peak = np.zeros(len(x), dtype=np.int64), np.zeros(len(x))
    periodic = method == CUTOFF_PERIODIC
    for p, atoms in enumerate(sets):
        values = dict(g)
        for s in range(3):
            values.update(('%s%d' % (n, s + 1), float(v)) for n, v in zip(names, params[atoms[s]]))
        E[p], grad = set_energy(expression, x[atoms], box, periodic, values, functions or {})
        for s in slots:
            F[atoms[s]] -= grad[s]
            count[atoms[s]] += 1
            peak[atoms[s]] = max(peak[atoms[s]], np.abs(grad[s]).max())
    return dict(E=E, F=F, sets=sets, r_all=r_all, count=count, peak=peak)


def force_bound(result):
    """[N][1]: n (2^-23 max|contribution| + 2^-31), n the atom's contributions (every contribution is rounded to f32 once, then added in
    fixed point)"""
    return (result['count'] * (2.0 ** -23 * result['peak'] + 2.0 ** -31))[:, None]


def energy_bound(result):
    return 1e-11 * np.abs(result['E']).sum()


def clear_of_cutoff(result, cutoff, margin=1e-6):
    """the membership condition of every test with a cutoff: no non-excluded pair's distance within ``margin`` nm of the cutoff (every
    distance that can decide membership: i-j, i-k and, in SinglePermutation, j-k)"""
    return len(result['r_all']) == 0 or float(np.abs(result['r_all'] - cutoff).min()) > margin
