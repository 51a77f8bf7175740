"""f64 reference for CustomNonbondedForce (openmmtools_amd/custom_expr.py kind 6, csrc/custom_nonbonded.hip), independent of the package
(it imports nothing from it): all pairs i < j in numpy, the minimum image, cutoff, OpenMM's switch and exclusions, and the energy string
evaluated through the dual numbers of tests/custom_dual_oracle.py (value and dE/dr, the dual's one coordinate being r itself).  The
long-range correction goes an independent route: the closed form for Lennard-Jones classes and numpy's trapezoid on a fine grid for
the switched part.  Positions are the f32-rounded ones the device holds (the caller rounds them)."""
import keyword
import math
import re

import numpy as np

import custom_dual_oracle as dual

NO_CUTOFF, CUTOFF_NON_PERIODIC, CUTOFF_PERIODIC = 0, 1, 2


def switch(r, rs, rc):
    """OpenMM's switching function and its derivative at r (arrays allowed)"""
    t = np.clip((np.asarray(r, dtype=np.float64) - rs) / (rc - rs), 0.0, 1.0)
    return 1.0 - 10.0 * t ** 3 + 15.0 * t ** 4 - 6.0 * t ** 5, (-30.0 * t ** 2 + 60.0 * t ** 3 - 30.0 * t ** 4) / (rc - rs)


def pair_list(x, box=None, method=NO_CUTOFF, cutoff=0.0, exclusions=()):
    """(i [P], j [P], d [P][3] = the image of x_j - x_i, r [P]) of every pair i < j no exclusion names, inside the cutoff where there is
    one; also the distances of ALL non-excluded pairs (for the callers' borderline assertion)"""
    x = np.asarray(x, dtype=np.float64)
    i, j = np.triu_indices(len(x), 1)
    if len(exclusions):
        ex = {(min(a, b), max(a, b)) for a, b in exclusions}
        keep = np.array([(a, b) not in ex for a, b in zip(i.tolist(), j.tolist())])
        i, j = i[keep], j[keep]
    d = x[j] - x[i]
    if method == CUTOFF_PERIODIC:
        d = d - np.asarray(box, dtype=np.float64) * np.rint(d / np.asarray(box, dtype=np.float64))
    r = np.sqrt((d * d).sum(axis=1))
    r_all = r
    if method != NO_CUTOFF:
        inside = r < cutoff
        i, j, d, r = i[inside], j[inside], d[inside], r[inside]
    return i, j, d, r, r_all


def evaluate(energy, names, params, global_values, x, box=None, method=NO_CUTOFF, cutoff=0.0, switch_distance=-1.0, exclusions=()):
    """dict(E [P] pair energies (switched), F [N][3], i, j, r, r_all, partners [N] pairs per atom, peak [N] the largest |component| any
    pair contributes to the atom's force) of one force.  names: the per-particle parameter names (p -> p1, p2); params [N][n]."""
    x = np.asarray(x, dtype=np.float64)
    params = np.asarray(params, dtype=np.float64).reshape(len(x), -1)
    # (the dual oracle evaluates the string as Python: a name that is a Python keyword -- a global called lambda -- gets a trailing _)
    rename = lambda name: name + '_' if keyword.iskeyword(name) else name
    expression = dual.Expression(re.sub(r'[A-Za-z_][A-Za-z_0-9]*', lambda m: rename(m.group(0)), energy))
    global_values = {rename(n): g for n, g in global_values.items()}
    names = [rename(n) for n in names]
    i, j, d, r, r_all = pair_list(x, box, method, cutoff, exclusions)
    E, F = np.zeros(len(i)), np.zeros_like(x)
    partners, peak = np.zeros(len(x), dtype=np.int64), np.zeros(len(x))
    for p, (a, b) in enumerate(zip(i.tolist(), j.tolist())):
        values = {n: float(g) for n, g in global_values.items()}
        for k, n in enumerate(names):
            values[n + '1'], values[n + '2'] = float(params[a, k]), float(params[b, k])
        zero = r[p] == 0.0                              # (r = 0: an energy and no force, the convention of the other kinds)
        values['r'] = dual.Dual(r[p], np.zeros(0) if zero else np.ones(1))
        e = expression(values)
        ev, de = (e.v, 0.0 if zero or e.g.size == 0 else float(e.g[0])) if isinstance(e, dual.Dual) else (float(e), 0.0)
        if switch_distance >= 0.0:
            s, ds = switch(r[p], switch_distance, cutoff)
            ev, de = ev * s, de * s + ev * ds
        E[p] = ev
        if not zero:
            f = de * d[p] / r[p]                        # the force on i; j gets the opposite
            F[a] += f; F[b] -= f
            partners[a] += 1; partners[b] += 1
            peak[a] = max(peak[a], np.abs(f).max()); peak[b] = max(peak[b], np.abs(f).max())
        else:
            partners[a] += 1; partners[b] += 1
    return dict(E=E, F=F, i=i, j=j, r=r, r_all=r_all, partners=partners, peak=peak)


def force_bound(result):
    """[N][1]: n (2^-23 max|contribution| + 2^-31), n the atom's partners (the f32 rounding of every contribution handed to the
    fixed-point accumulator, and the accumulator's own step)"""
    return (result['partners'] * (2.0 ** -23 * result['peak'] + 2.0 ** -31))[:, None]


def energy_bound(result):
    return 1e-11 * np.abs(result['E']).sum()


def class_counts(params):
    """[(parameter tuple, count)] of the distinct parameter rows"""
    classes = {}
    for row in np.asarray(params, dtype=np.float64).reshape(len(params), -1):
        classes[tuple(row.tolist())] = classes.get(tuple(row.tolist()), 0) + 1
    return sorted(classes.items())


def long_range_coefficient(n, classes, integral):
    """2 pi N^2 sum count I / (N (N + 1) / 2) over the pairs of classes, integral(pa, pb) -> I (OpenMM's convention); the energy is
    this over the volume"""
    total = 0.0
    for a, (pa, na) in enumerate(classes):
        for pb, nb in classes[a:]:
            total += (na * (na + 1) // 2 if pa == pb else na * nb) * integral(pa, pb)
    return 2.0 * math.pi * n * n * total / (n * (n + 1) / 2.0)


def lj_tail(sigma, epsilon, rc):
    """int_rc^inf 4 eps ((s/r)^12 - (s/r)^6) r^2 dr in closed form: 4 eps (s^12 / (9 rc^9) - s^6 / (3 rc^3))"""
    return 4.0 * epsilon * (sigma ** 12 / (9.0 * rc ** 9) - sigma ** 6 / (3.0 * rc ** 3))


def switched_part(energy_of_r, rs, rc, points):
    """int_rs^rc (1 - S) E r^2 dr by numpy's trapezoid on ``points`` equal steps"""
    r = np.linspace(rs, rc, points + 1)
    s, _ = switch(r, rs, rc)
    y = (1.0 - s) * energy_of_r(r) * r * r
    return float(np.sum(0.5 * (y[1:] + y[:-1]) * np.diff(r)))
