"""CustomGBForce by its definition, in f64 over the dual numbers of tests/custom_dual_oracle.py.  It imports nothing from the package.

A force is a plain dict: per_particle (names), params [N][n], globals {name: value}, computed [(name, expression, type)], terms
[(expression, type)], method (0 NoCutoff, 1 CutoffNonPeriodic, 2 CutoffPeriodic), cutoff, exclusions [(i, j)], functions {name:
callable over duals} (tests/tabulated_oracle.py, tests/tabulated2d_oracle.py).  Types: 0 SingleParticle, 1 ParticlePair,
2 ParticlePairNoExclusions.

Every coordinate is a dual whose gradient runs over all 3N coordinates.  V_0,i is the dual sum over j != i of the first value's
expression at r_ij (particle 1 = i, particle 2 = j; inside the cutoff; the ParticlePair type leaves out excluded j); the expression
is evaluated over the six coordinates of the pair and its gradient is put into its place among the 3N (an embedding, not a chain
rule).  Later values and all energy terms are composed from those duals, a pair term once per unordered pair with particle 1 the
lower index.  The forces are minus the gradient of the sum: no chain-rule code of its own.  r = 0 between distinct particles is
refused (the callers choose positions with r > 0).

For the callers' bounds it returns `abs_energy`, the sum of |summand| (every single-particle term of a particle and every pair term
of a pair is a summand), and the scale of the pair pieces of the force on every atom.  The force on atom i is a sum over its partners
j of pieces along x_j - x_i: the piece of the pair terms, (sum_t de_t/dr) u_ij, and the piece of the values' dependence on r_ij,
(dE/dV_0,i df(i,j)/dr + dE/dV_0,j df(j,i)/dr) u_ij.  `count` [N] is the number of nonzero pieces of atom i (at most two per partner)
and `peak` [N] the largest |component| among them.  These three factors are formed for the SCALE only (pair_pieces, below: dE/dV_0
as the gradient of a second dual evaluation seeded on the V_0, the derivatives with respect to r from duals seeded on r); no force
comes from them.  It also returns the distances of all pairs (r_all) for the borderline check.
"""
import keyword
import re

import numpy as np

import custom_dual_oracle as dual

SINGLE, PAIR, PAIR_NO_EXCLUSIONS = 0, 1, 2


def _expression(text):
    """(the dual oracle evaluates the string as Python: a name that is a Python keyword -- OBC's ``or`` -- gets a trailing _)"""
    return dual.Expression(re.sub(r'[A-Za-z_][A-Za-z_0-9]*', lambda m: m.group(0) + '_' if keyword.iskeyword(m.group(0)) else m.group(0), text))


def _image(d, box):
    return d - box * np.rint(d / box) if box is not None else d


def pair_distances(x, box=None):
    """[N][N] minimum-image distances (plain f64)"""
    x = np.asarray(x, dtype=np.float64)
    d = x[None, :, :] - x[:, None, :]
    return np.sqrt((_image(d, None if box is None else np.asarray(box, dtype=np.float64)) ** 2).sum(axis=2))


def evaluate(force, x, box=None):
    x = np.asarray(x, dtype=np.float64)
    N = len(x)
    box = None if box is None or force['method'] != 2 else [float(b) for b in box]
    params = np.asarray(force['params'], dtype=np.float64).reshape(N, -1)
    names = list(force['per_particle'])
    functions = dict(dual.FUNCTIONS, **force.get('functions', {}))
    base = {n: float(v) for n, v in force.get('globals', {}).items()}
    excluded = set()
    for i, j in force.get('exclusions', ()):
        excluded.add((i, j)); excluded.add((j, i))
    r_all = pair_distances(x, box)
    cutoff = float(force['cutoff']) if force['method'] else np.inf
    near = (r_all < cutoff) & ~np.eye(N, dtype=bool)
    if np.any(r_all[near] == 0.0):
        raise ValueError('two distinct particles at r = 0')
    P = dual.seeds(x)
    computed, terms = list(force['computed']), list(force['terms'])
    values = [dict() for _ in range(N)]                         # per particle: value name -> dual

    def single_names(i):
        v = dict(base)
        v.update({n: float(params[i, k]) for k, n in enumerate(names)})
        v.update(values[i])
        return v

    def pair_names(a, b, r):
        v = dict(base, r=r)
        for k, n in enumerate(names):
            v[n + '1'], v[n + '2'] = float(params[a, k]), float(params[b, k])
        for n, d in values[a].items():
            v[n + '1'] = d
        for n, d in values[b].items():
            v[n + '2'] = d
        return v

    def as_dual(e):
        return e if isinstance(e, dual.Dual) else dual.Dual(float(e), np.zeros(3 * N))

    zero = dual.Dual(0.0, np.zeros(3 * N))
    if computed:
        name, text, kind = computed[0]
        expression = _expression(text)
        for i in range(N):
            total = zero
            for j in range(N):
                if not near[i, j] or (kind == PAIR and (i, j) in excluded):
                    continue
                # the pair's own six coordinates as the gradient's space, then embedded among the 3N
                six = dual.seeds([x[i], x[j]])
                e = expression(pair_names(i, j, dual.distance(six, 0, 1, box)), functions)
                if isinstance(e, dual.Dual) and e.g.size:
                    g = np.zeros(3 * N)
                    g[3 * i:3 * i + 3], g[3 * j:3 * j + 3] = e.g[:3], e.g[3:]
                    e = dual.Dual(e.v, g)
                total = total + as_dual(e)
            values[i][name] = total
        for name, text, kind in computed[1:]:
            expression = _expression(text)
            for i in range(N):
                values[i][name] = as_dual(expression(single_names(i), functions))
    E_terms = np.zeros(len(terms))
    gradient = np.zeros(3 * N)
    abs_energy = 0.0

    def summand(t, e):
        nonlocal gradient, abs_energy
        e = as_dual(e)
        E_terms[t] += e.v
        abs_energy += abs(e.v)
        gradient = gradient + e.g

    for t, (text, kind) in enumerate(terms):
        expression = _expression(text)
        if kind == SINGLE:
            for i in range(N):
                summand(t, expression(single_names(i), functions))
        else:
            for a in range(N):
                for b in range(a + 1, N):
                    if near[a, b] and not (kind == PAIR and (a, b) in excluded):
                        summand(t, expression(pair_names(a, b, dual.distance(P, a, b, box)), functions))
    plain = [{n: d.v for n, d in v.items()} for v in values]
    count, peak = pair_pieces(force, x, box, near, excluded, r_all, plain)
    return dict(E=float(E_terms.sum()), E_terms=E_terms, F=-gradient.reshape(N, 3), r_all=r_all, count=count, peak=peak, abs_energy=abs_energy,
                values=plain)


def pair_pieces(force, x, box, near, excluded, r_all, plain):
    """(count [N], peak [N]) of the pair pieces of the force on every atom (the module's docstring): the scale of the force bound"""
    N = len(x)
    params = np.asarray(force['params'], dtype=np.float64).reshape(N, -1)
    names = list(force['per_particle'])
    functions = dict(dual.FUNCTIONS, **force.get('functions', {}))
    base = {n: float(v) for n, v in force.get('globals', {}).items()}
    computed, terms = list(force['computed']), list(force['terms'])

    def single_names(i, values):
        v = dict(base)
        v.update({n: float(params[i, k]) for k, n in enumerate(names)})
        v.update(values[i])
        return v

    def pair_names(a, b, r, values):
        v = dict(base, r=r)
        for k, n in enumerate(names):
            v[n + '1'], v[n + '2'] = float(params[a, k]), float(params[b, k])
        for n, d in values[a].items():
            v[n + '1'] = d
        for n, d in values[b].items():
            v[n + '2'] = d
        return v

    def slope(e):
        return float(e.g[0]) if isinstance(e, dual.Dual) and e.g.size else 0.0

    def counted(kind, a, b):
        return near[a, b] and not (kind == PAIR and (a, b) in excluded)

    # dE/dV_0: the energy over duals seeded on the V_0, every r a plain number
    g0 = np.zeros(N)
    if computed:
        unit = np.eye(N)
        seeded = [{computed[0][0]: dual.Dual(plain[i][computed[0][0]], unit[i])} for i in range(N)]
        for name, text, kind in computed[1:]:
            expression = _expression(text)
            for i in range(N):
                seeded[i][name] = expression(single_names(i, seeded), functions)
        for text, kind in terms:
            expression = _expression(text)
            if kind == SINGLE:
                es = [expression(single_names(i, seeded), functions) for i in range(N)]
            else:
                es = [expression(pair_names(a, b, float(r_all[a, b]), seeded), functions)
                      for a in range(N) for b in range(a + 1, N) if counted(kind, a, b)]
            for e in es:
                if isinstance(e, dual.Dual) and e.g.size:
                    g0 = g0 + e.g
    one = np.ones(1)
    chain = np.zeros((N, N))                                   # dE/dr_ij through the values
    if computed:
        name, text, kind = computed[0]
        expression = _expression(text)
        none = [dict() for _ in range(N)]
        for i in range(N):
            for j in range(N):
                if i != j and counted(kind, i, j):
                    d = g0[i] * slope(expression(pair_names(i, j, dual.Dual(r_all[i, j], one), none), functions))
                    chain[i, j] += d; chain[j, i] += d
    direct = np.zeros((N, N))                                  # dE/dr_ij of the pair terms
    for text, kind in terms:
        if kind == SINGLE:
            continue
        expression = _expression(text)
        for a in range(N):
            for b in range(a + 1, N):
                if counted(kind, a, b):
                    d = slope(expression(pair_names(a, b, dual.Dual(r_all[a, b], one), plain), functions))
                    direct[a, b] += d; direct[b, a] += d
    d = x[None, :, :] - x[:, None, :]
    if box is not None:
        d = d - np.asarray(box) * np.rint(d / np.asarray(box))
    with np.errstate(invalid='ignore', divide='ignore'):
        u = np.where(r_all[:, :, None] > 0.0, np.abs(d) / r_all[:, :, None], 0.0).max(axis=2)
    pieces = np.stack([np.abs(chain) * u, np.abs(direct) * u])
    return (pieces > 0.0).sum(axis=(0, 2)).astype(np.int64), pieces.max(axis=(0, 2))


def energy_bound(result):
    return 1e-11 * result['abs_energy']


def force_bound(result):
    """[N][1]: n (2^-23 max|contribution| + 2^-31), n the atom's nonzero pair pieces (two per partner: the pair terms' and the
    values'); each launch and column slice hands the fixed-point accumulators one f32-rounded partial sum of them"""
    return (result['count'] * (2.0 ** -23 * result['peak'] + 2.0 ** -31))[:, None]


def borderline(result, cutoff, margin=1e-6):
    """True where some pair lies within `margin` of the cutoff"""
    r = result['r_all'][~np.eye(len(result['r_all']), dtype=bool)]
    return bool(np.any(np.abs(r - cutoff) < margin))
