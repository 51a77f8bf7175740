"""CPU: the exact-derivative reference tests/custom_dual_oracle.py held to three other things over the case table of
tests/custom_opcode_cases.py (every row, every lane, both replicas): mpmath at 50 digits, the finite-difference helpers
(tests/custom_expr_oracle.py, tests/compound_expr_oracle.py) on the smooth rows, and the compiler's program through the Python
interpreter of the machine.

The GPU bound of tests/test_custom_opcodes_gpu.py is 2^-23 of a contribution per force component and 1e-11 of sum|E| per energy; the
reference alone sits at 1e-13 of (|want| + the largest intermediate) here, i.e. the stated intervals are well conditioned."""
import math

import numpy as np
import pytest

import compound_expr_oracle
import custom_dual_oracle as dual
import custom_expr_oracle
import custom_opcode_cases as cases
from openmmtools_amd import custom_expr as cx

ROWS = cases.all_rows()
IDS = [r['name'] for r in ROWS]
KIND = {'ext': dual.KIND_EXTERNAL, 'bond': dual.KIND_BOND, 'angle': dual.KIND_ANGLE, 'torsion': dual.KIND_TORSION}


def _box(row, r):
    return cases.BOXES[r] if row['periodic'] else None


def _own_variables(row, x, box):
    """(names, values) of the force's own variables at the term's atoms x [W][3]"""
    if row['place'] in ('bond', 'angle', 'torsion'):
        name, value = next(iter(custom_expr_oracle.variables(KIND[row['place']], x, box, row['periodic']).items()))
        return [name], [value]
    if row['place'] == 'ext':
        return ['x', 'y', 'z'], list(x[0])
    return ['%s%d' % (c, i + 1) for i in range(len(x)) for c in 'xyz'], list(x.reshape(-1))


def _dual_own(row, expression, x, params, box):
    """the dual reference's value and partials with respect to the own variables, and the largest intermediate"""
    names, values = _own_variables(row, x, box)
    dual.peak[0] = 0.0
    if row['place'] in ('bond', 'angle', 'torsion'):
        v = {names[0]: dual.Dual(values[0], np.ones(1))}
    else:
        v = dual.term_values(KIND.get(row['place'], dual.KIND_COMPOUND), x, box, row['periodic'])
    v.update(zip(row['names'], (float(p) for p in params)))
    v.update(row['globals'])
    e = expression(v)
    return e.v, e.g, dual.peak[0]


def _mp_functions(mp, box):
    tie = mp.mpf(10) ** -15                   # (an exact tie stays a tie under the difference step of 1e-20)

    def image(d, L):
        return d - L * mp.nint(d / L) if L else d

    def pointdistance(x1, y1, z1, x2, y2, z2):
        L = box if box is not None else (0, 0, 0)
        return mp.sqrt(sum(image(b - a, mp.mpf(float(l))) ** 2 for a, b, l in zip((x1, y1, z1), (x2, y2, z2), L)))
    f = dict(sqrt=mp.sqrt, exp=mp.exp, log=mp.log, sin=mp.sin, cos=mp.cos, tan=mp.tan, asin=mp.asin, acos=mp.acos, atan=mp.atan, atan2=mp.atan2,
             sinh=mp.sinh, cosh=mp.cosh, tanh=mp.tanh, erf=mp.erf, erfc=mp.erfc, abs=abs, min=lambda x, y: x if x < y else y,
             max=lambda x, y: x if x > y else y, step=lambda x: mp.mpf(1 if x >= 0 else 0), delta=lambda x: mp.mpf(1 if abs(x) < tie else 0),
             select=lambda x, y, z: y if abs(x) >= tie else z, floor=mp.floor, ceil=mp.ceil, periodicdistance=pointdistance,
             pointdistance=pointdistance)
    return f


def _mp_geometry(mp, p):
    """distance / angle / dihedral over the mp particle coordinates p [P][3]"""
    def sub(a, b): return [a[k] - b[k] for k in range(3)]
    def dot(a, b): return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    def cross(a, b): return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

    def angle(i, j, k):
        v0, v1 = sub(p[i], p[j]), sub(p[k], p[j])
        return mp.acos(dot(v0, v1) / mp.sqrt(dot(v0, v0) * dot(v1, v1)))

    def dihedral(i, j, k, l):
        b1, b2, b3 = sub(p[j], p[i]), sub(p[k], p[j]), sub(p[l], p[k])
        m, n = cross(b1, b2), cross(b2, b3)
        return mp.atan2(mp.sqrt(dot(b2, b2)) * dot(b1, n), dot(m, n))
    return dict(distance=lambda i, j: mp.sqrt(dot(sub(p[j], p[i]), sub(p[j], p[i]))), angle=angle, dihedral=dihedral)


@pytest.mark.parametrize('row', ROWS, ids=IDS)
def test_the_dual_reference_against_mpmath(row):
    mpmath = pytest.importorskip('mpmath')
    mp = mpmath.mp
    mp.dps = 50
    expression = dual.Expression(row['energy'])
    h = mp.mpf(10) ** -20
    worst = 0.0
    for r in (0, 1):
        box = _box(row, r)
        functions = _mp_functions(mp, box)
        for t in range(cases.N_TERMS):
            x = cases.XS[r][row['atoms'][t]]
            names, values = _own_variables(row, x, box)
            got_E, got_g, scale = _dual_own(row, expression, x, row['params'][t], box)
            fixed = dict(zip(row['names'], (mp.mpf(float(p)) for p in row['params'][t])))
            fixed.update({n: mp.mpf(float(g)) for n, g in row['globals'].items()})

            def f(*args):
                v = dict(fixed, **dict(zip(names, args)))
                if row['place'] in ('compound', 'c1', 'c3'):
                    v.update(_mp_geometry(mp, [args[3 * i:3 * i + 3] for i in range(len(args) // 3)]))
                    v.update({'p%d' % (i + 1): i for i in range(len(args) // 3)})
                return expression(v, functions)
            at = [mp.mpf(float(v)) for v in values]
            want_E = f(*at)
            tol = 1e-13 * (abs(float(want_E)) + scale)
            assert abs(got_E - float(want_E)) <= tol, (row['name'], r, t, got_E, want_E)
            for k in range(len(names)):
                if len(names) == 1:
                    want = mp.diff(f, at[0], 1, h=h, direction=0)
                else:
                    want = mp.diff(f, tuple(at), tuple(int(j == k) for j in range(len(names))), h=h, direction=0)
                tol = 1e-13 * (abs(float(want)) + scale)
                worst = max(worst, abs(got_g[k] - float(want)) / tol)
                assert abs(got_g[k] - float(want)) <= tol, (row['name'], r, t, names[k], got_g[k], want)
    print('%s: worst |dual - mpmath| / bound = %.3g' % (row['name'], worst))


@pytest.mark.parametrize('row', [r for r in ROWS if r['interval'] is not None], ids=[r['name'] for r in ROWS if r['interval'] is not None])
def test_every_operand_lies_in_its_interval_and_off_its_kinks(row):
    lo, hi = row['interval']
    p = row['params']
    assert len(set(np.abs(p[:, 0]))) == cases.N_TERMS and np.all(np.abs(p[:, 0]) != np.abs(p[:, 1])) and np.all(p[:, :2] != 0.0)
    for r in (0, 1):
        u = cases.u_values(row, r)
        assert np.all((u >= lo) & (u <= hi))
        assert u.max() - u.min() > 0.6 * (hi - lo)                                 # (spread over the interval)
        if row['kink'] is not None:
            assert min(row['kink'](v) for v in u) >= 1e-3
            if row['kink'] is abs:
                assert (u > 0).sum() >= 10 and (u < 0).sum() >= 10                 # both sides of the jump


def test_the_branches_and_quadrants_the_table_promises():
    by = {r['name']: r for r in ROWS}
    for place, P in cases.PLACES.items():
        for r in (0, 1):
            row = by['%s/min' % place]
            x, y, z = cases._xyz(place, row['atoms'], r)
            assert (x * y < z).sum() >= 20 and (x * y > z).sum() >= 20 and np.abs(x * y - z).min() >= 1e-3
            assert {(a > 0, b > 0) for a, b in zip(x * y, z - 1.0)} == {(True, True), (True, False), (False, True), (False, False)}
            row = by['%s/select(x-x0)' % place]
            c = cases._xyz(place, row['atoms'], r)[0] - row['params'][:, 1]
            assert (c == 0.0).sum() == 10 and (c > 0.0).sum() >= 10 and (c < 0.0).sum() >= 10
            row = by['%s/(x+1)^(y*z)' % place]
            x = cases._xyz(place, row['atoms'], r)[0]
            assert np.all((x + 1.0 >= 1.0) & (x + 1.0 <= 3.0))
    row = by['ext/periodicdistance']
    for r in (0, 1):
        x, y, z = cases._xyz('ext', row['atoms'], r)
        d = np.column_stack([row['params'][:, 1] - x * y, row['params'][:, 2] + z - y, row['params'][:, 3] - (z + x)]) / cases.BOXES[r]
        assert (np.abs(d) > 0.5).any(axis=1).sum() >= 10                           # lanes that image across a face
        assert np.abs(np.abs(d - np.rint(d)) - 0.5).min() >= 1e-3                  # none on the face itself
    assert np.array_equal(cases.BOXES, cases.BOXES.astype(np.float32)) and not np.array_equal(cases.BOXES[0], cases.BOXES[1])
    assert np.array_equal(cases.XS, cases.XS.astype(np.float32))
    # the one-variable kinds and the particle rows stay off their kinks and degenerate geometries
    for name, kind, kinks in (('angle', dual.KIND_ANGLE, lambda th, c: (abs(th - c), math.sin(th) - 0.05)),
                              ('torsion', dual.KIND_TORSION, lambda th, c: (abs(th), abs(th - round(th)), math.pi - abs(th)))):
        row = by[name]
        for r in (0, 1):
            for t in range(cases.N_TERMS):
                th = custom_expr_oracle.variables(kind, cases.XS[r][row['atoms'][t]])['theta']
                assert min(kinks(th, row['params'][t][-1])) >= 1e-3, (name, r, t, th)


SMOOTH = [r for r in ROWS if not any(w in r['energy'] for w in ('abs', 'min', 'max', 'select', 'step', 'floor', 'ceil', 'delta', 'periodicdistance'))
          and 'erfc tail' not in r['name'] and '^64' not in r['energy'] and '^-64' not in r['energy']
          and 'u^0' not in r['energy']]            # (u^0: no force at all, and the helpers' own check divides by max|F|)


@pytest.mark.parametrize('row', SMOOTH, ids=lambda r: r['name'])
def test_the_dual_reference_against_the_finite_difference_helpers(row):
    """Cartesian forces: the geometry composition of the dual reference.  The helpers guarantee their own truncation error to 1e-8 of
    max|F| (their halving check); 1e-7 leaves an order of magnitude over it."""
    x = cases.XS[0]
    if row['P']:
        E, F = compound_expr_oracle.evaluate(row['P'], row['energy'], row['atoms'], row['names'], row['params'], row['globals'], x)
        E2, F2 = dual.evaluate_compound(row['P'], row['energy'], row['atoms'], row['names'], row['params'], row['globals'], x)
    else:
        E, F = custom_expr_oracle.evaluate(KIND[row['place']], row['energy'], row['atoms'], row['names'], row['params'], row['globals'], x)
        E2, F2 = dual.evaluate(KIND[row['place']], row['energy'], row['atoms'], row['names'], row['params'], row['globals'], x)
    print('%s: |dF| / max|F| = %.3g' % (row['name'], np.abs(F - F2).max() / np.abs(F).max()))
    assert np.allclose(E, E2, rtol=1e-13, atol=0.0)
    assert np.abs(F - F2).max() <= 1e-7 * np.abs(F).max()


def _variables_of(row):
    if row['place'] in ('bond', 'angle', 'torsion', 'ext'):
        return cx.VARIABLES[KIND[row['place']]]
    return cx.compound_variables(row['P'])


@pytest.mark.parametrize('row', ROWS, ids=IDS)
def test_the_compiled_program_gives_the_dual_references_value_and_partials(row):
    columns = {n: i for i, n in enumerate(row['globals'])}
    prog = cx.compile_expression(row['energy'], list(_variables_of(row)), row['names'], columns, periodic_distance=row['periodic'],
                                 n_particles=row['P'])
    assert len(prog['program']) <= cx.MAX_PROGRAM and prog['stack_depth'] <= cx.MAX_STACK and len(row['names']) <= cx.MAX_PARAMS
    expression = dual.Expression(row['energy'])
    g = list(row['globals'].values())
    for r in (0, 1):
        box = _box(row, r)
        for t in range(cases.N_TERMS):
            x = cases.XS[r][row['atoms'][t]]
            want_E, want_g, scale = _dual_own(row, expression, x, row['params'][t], box)
            tol = 1e-13 * (abs(want_E) + scale)
            if row['P']:
                for seed in range(row['P']):
                    E, dE, _ = cases.run_pass(prog, x, row['params'][t], g, seed, box)
                    assert abs(E - want_E) <= tol and np.abs(dE - want_g[3 * seed:3 * seed + 3]).max() <= tol, (row['name'], r, t, seed)
            else:
                values = _own_variables(row, x, box)[1]
                E, dE, _ = cases.run_program(prog, values, row['params'][t], g, box)
                assert abs(E - want_E) <= tol and np.abs(dE[:len(values)] - want_g).max() <= tol, (row['name'], r, t)
