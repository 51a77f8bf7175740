"""Exact f64 reference for the energy parameter derivatives of the custom forces (dE/dglobal), independent of the package: the dual
numbers of tests/custom_dual_oracle.py with the chosen global a Dual of unit gradient and everything else -- positions, per-term
parameters, the other globals -- carrying a zero gradient of the same length (one component).  Geometry, functions and the piecewise
rules are that module's, so min / max / select differentiate as the branch the machine states it takes.

Every evaluate_* returns dict(dE [n] per-term dE_t/dglobal, total their sum, E [n] the term energies, scale sum_t |dE_t/dglobal|: the
tests' error scale, bound = 1e-11 scale).  Tabulated functions are given as callables over duals (continuous1d, discrete1d and
separable2d below, fitted here from the samples: natural cubic splines solved densely with numpy).
"""
import keyword
import math
import re

import numpy as np

import custom_dual_oracle as dual
from custom_dual_oracle import Dual

ZERO, ONE = np.zeros(1), np.ones(1)
HB_SLOTS = dict(d1=0, d2=1, d3=2, a1=3, a2=4, a3=5)
MP_SLOTS = dict(p1=0, p2=1, p3=2)


def _rename(name):
    """(the string is evaluated as Python: a name that is a keyword -- a global called lambda -- gets a trailing _)"""
    return name + '_' if keyword.iskeyword(name) else name


def expression_of(energy):
    return dual.Expression(re.sub(r'[A-Za-z_][A-Za-z_0-9]*', lambda m: _rename(m.group(0)), energy))


def _const(v):
    return Dual(float(v), ZERO)


def _points(x):
    return [[_const(c) for c in row] for row in np.asarray(x, dtype=np.float64)]


def _globals(global_values, wrt):
    if wrt not in global_values:
        raise KeyError('the global %r is not among %s' % (wrt, sorted(global_values)))
    return {_rename(n): Dual(float(v), ONE if n == wrt else ZERO) for n, v in global_values.items()}


def _geometry(kind, x, box, periodic, slots=None):
    """the names an expression of this kind may use at the term's positions x [W][3], every coordinate a constant"""
    p = _points(x)
    pbox = box if periodic else None
    if kind == dual.KIND_EXTERNAL:
        v = dict(x=p[0][0], y=p[0][1], z=p[0][2])
        if periodic:
            v['periodicdistance'] = dual.point_distance(box)
        return v
    if kind == dual.KIND_BOND:
        return dict(r=dual.distance(p, 0, 1, pbox))
    if kind == dual.KIND_ANGLE:
        return dict(theta=dual.angle(p, 0, 1, 2, pbox))
    if kind == dual.KIND_TORSION:
        return dict(theta=dual.dihedral(p, 0, 1, 2, 3, pbox))
    v = dict(distance=lambda i, j: dual.distance(p, i, j, pbox), angle=lambda i, j, k: dual.angle(p, i, j, k, pbox),
             dihedral=lambda i, j, k, l: dual.dihedral(p, i, j, k, l, pbox), pointdistance=dual.point_distance(pbox))
    if slots is not None:
        v.update(slots)
        return v
    for i in range(len(p)):
        v['p%d' % (i + 1)] = v['g%d' % (i + 1)] = i
        v.update({'x%d' % (i + 1): p[i][0], 'y%d' % (i + 1): p[i][1], 'z%d' % (i + 1): p[i][2]})
    return v


def _term(expression, values, functions):
    e = expression(values, dict(dual.FUNCTIONS, **(functions or {})))
    if not isinstance(e, Dual):
        return float(e), 0.0
    return e.v, float(e.g[0]) if e.g.size else 0.0


def _result(E, dE):
    E, dE = np.asarray(E, dtype=np.float64), np.asarray(dE, dtype=np.float64)
    scale = float(np.abs(dE).sum())
    return dict(E=E, dE=dE, total=float(dE.sum()), scale=scale, bound=1e-11 * scale)


def evaluate(kind, energy, atoms, names, params, global_values, wrt, positions, box=None, periodic=False, functions=None, n_particles=None):
    """a bond / angle / torsion / external force (kind of custom_dual_oracle) or, with n_particles, a compound-bond force: atoms
    [n][W], params [n][len(names)], positions [N][3] (nm, as the device holds them), box the three edges"""
    width = n_particles if n_particles else dual.WIDTH[kind]
    kind = dual.KIND_COMPOUND if n_particles else kind
    expression = expression_of(energy)
    positions = np.asarray(positions, dtype=np.float64)
    atoms = np.asarray(atoms, dtype=np.int64).reshape(-1, width)
    params = np.asarray(params, dtype=np.float64).reshape(len(atoms), -1)
    g = _globals(global_values, wrt)
    E, dE = [], []
    for idx, p in zip(atoms, params):
        v = _geometry(kind, positions[idx], box, periodic)
        v.update((_rename(n), _const(q)) for n, q in zip(names, p))
        v.update(g)
        e, d = _term(expression, v, functions)
        E.append(e); dE.append(d)
    return _result(E, dE)


def centroids(groups, positions, box=None, periodic=False):
    """[G][3]: x_first + sum_i w_i img(x_i - x_first) of every group (atoms, weights summing to 1)"""
    positions = np.asarray(positions, dtype=np.float64)
    out = []
    for atoms, weights in groups:
        d = positions[list(atoms)] - positions[atoms[0]]
        if periodic:
            L = np.asarray(box, dtype=np.float64)
            d = d - L * np.rint(d / L)
        out.append(positions[atoms[0]] + (np.asarray(weights, dtype=np.float64)[:, None] * d).sum(axis=0))
    return np.array(out)


def evaluate_centroid(n_groups_per_bond, energy, groups, bonds, names, params, global_values, wrt, positions, box=None, periodic=False,
                      functions=None):
    """a centroid-bond force: groups a list of (atoms, weights summing to 1), bonds [n][P] group numbers"""
    return evaluate(None, energy, bonds, names, params, global_values, wrt, centroids(groups, positions, box, periodic), box, periodic,
                    functions, n_particles=n_groups_per_bond)


def evaluate_hbond(energy, donor_names, acceptor_names, donors, acceptors, donor_params, acceptor_params, global_values, wrt, pairs,
                   positions, box=None, periodic=False, functions=None):
    """a donor-acceptor force over the (donor, acceptor) pairs given (custom_hbond_oracle.evaluate's i, j: the membership is that
    oracle's business)"""
    expression = expression_of(energy)
    positions = np.asarray(positions, dtype=np.float64)
    donors, acceptors = np.asarray(donors, dtype=np.int64).reshape(-1, 3), np.asarray(acceptors, dtype=np.int64).reshape(-1, 3)
    donor_params = np.asarray(donor_params, dtype=np.float64).reshape(len(donors), -1)
    acceptor_params = np.asarray(acceptor_params, dtype=np.float64).reshape(len(acceptors), -1)
    g = _globals(global_values, wrt)
    E, dE = [], []
    for i, j in pairs:
        at = np.concatenate([donors[i], acceptors[j]])
        v = _geometry(dual.KIND_COMPOUND, positions[np.where(at >= 0, at, at[0])], box, periodic, HB_SLOTS)
        v.update((_rename(n), _const(q)) for n, q in zip(donor_names, donor_params[i]))
        v.update((_rename(n), _const(q)) for n, q in zip(acceptor_names, acceptor_params[j]))
        v.update(g)
        e, d = _term(expression, v, functions)
        E.append(e); dE.append(d)
    return _result(E, dE)


def evaluate_manyparticle(energy, names, params, global_values, wrt, sets, positions, box=None, periodic=False, functions=None):
    """a many-particle force over the assignments (p1, p2, p3) given (custom_manyparticle_oracle.evaluate's sets)"""
    expression = expression_of(energy)
    positions = np.asarray(positions, dtype=np.float64)
    params = np.asarray(params, dtype=np.float64).reshape(len(positions), -1)
    g = _globals(global_values, wrt)
    E, dE = [], []
    for at in np.asarray(sets, dtype=np.int64).reshape(-1, 3):
        v = _geometry(dual.KIND_COMPOUND, positions[at], box, periodic, MP_SLOTS)
        for s in range(3):
            v.update(('%s%d' % (n, s + 1), _const(q)) for n, q in zip(names, params[at[s]]))
        v.update(g)
        e, d = _term(expression, v, functions)
        E.append(e); dE.append(d)
    return _result(E, dE)


# ---- tabulated functions over duals -----------------------------------------------------------------------------------------------
def natural_spline(values, lo, hi):
    """(h, y, M): the second derivatives M of the natural cubic spline through `values` at uniform points over [lo, hi], solved densely"""
    y = np.asarray(values, dtype=np.float64)
    n = len(y)
    h = (hi - lo) / (n - 1)
    A, b = np.zeros((n, n)), np.zeros(n)
    A[0, 0] = A[-1, -1] = 1.0
    for i in range(1, n - 1):
        A[i, i - 1], A[i, i], A[i, i + 1] = 1.0, 4.0, 1.0
        b[i] = 6.0 * (y[i - 1] - 2.0 * y[i] + y[i + 1]) / (h * h)
    return h, y, np.linalg.solve(A, b)


def continuous1d(values, lo, hi):
    """a Continuous1DFunction that is not periodic: the natural spline inside [lo, hi], 0 with derivative 0 outside"""
    h, y, M = natural_spline(values, lo, hi)
    n = len(y)

    def value_slope(t):
        if not lo <= t <= hi:
            return 0.0, 0.0
        i = min(max(int((t - lo) / h), 0), n - 2)
        b = (t - lo) / h - i
        a = 1.0 - b
        return (a * y[i] + b * y[i + 1] + ((a ** 3 - a) * M[i] + (b ** 3 - b) * M[i + 1]) * h * h / 6.0,
                (y[i + 1] - y[i]) / h + ((1.0 - 3.0 * a * a) * M[i] + (3.0 * b * b - 1.0) * M[i + 1]) * h / 6.0)

    def call(x):
        if not isinstance(x, Dual):
            return value_slope(float(x))[0]
        v, k = value_slope(x.v)
        return Dual(v, k * x.g)
    call.value_slope = value_slope
    return call


def discrete1d(values):
    """a Discrete1DFunction: values[round(x)], halves away from zero, derivative 0"""
    values = [float(v) for v in values]

    def call(x):
        xv = x.v if isinstance(x, Dual) else float(x)
        v = values[int(math.floor(abs(xv) + 0.5) * (1 if xv >= 0 else -1))]
        return Dual(v, np.zeros_like(x.g)) if isinstance(x, Dual) else v
    return call


def separable2d(gx, xlo, xhi, hy, ylo, yhi):
    """a Continuous2DFunction (not periodic) whose samples are gx[i] hy[j]: its bicubic interpolant is the product of the two natural
    splines (include/remd_hip_custom.h, REMD_CX_TABLE2D), which is what this returns; 0 where either argument is out of range"""
    fx, fy = continuous1d(gx, xlo, xhi), continuous1d(hy, ylo, yhi)

    def call(x, y):
        xv, yv = (x.v if isinstance(x, Dual) else float(x)), (y.v if isinstance(y, Dual) else float(y))
        if not (xlo <= xv <= xhi and ylo <= yv <= yhi):
            z = [a for a in (x, y) if isinstance(a, Dual)]
            return Dual(0.0, np.zeros_like(z[0].g)) if z else 0.0
        return fx(x) * fy(y)
    return call
