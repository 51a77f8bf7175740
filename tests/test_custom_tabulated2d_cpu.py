"""CPU: the tabulated functions of two and three arguments of the custom forces (system.Continuous2DFunction, Discrete2DFunction,
Discrete3DFunction).  The definition of include/remd_hip_custom.h is pinned on the reference tests/tabulated2d_oracle.py (properties that
hold for the construction whatever the code: interpolation, bilinear reproduction, separable tables against two 1D splines, commuting
node derivatives, C1 across patch edges, periodicity), then the compiler's blocks and the host interpreter (custom_expr.run_values, the
device's formulas) are held against the reference; the classes, every refusal by name, and the descriptor of each of the seven kinds.

Scales of the relative bounds: a value is a combination of samples, its error relative to max|f|; a partial along x is a difference
of samples over hx, relative to max|f| / hx (fy: / hy, fxy: / (hx hy)) -- the scales of tests/test_custom_tabulated_cpu.py."""
import copy
import math

import numpy as np
import pytest

import custom_dual_oracle as dual
import tabulated2d_cases as cases
import tabulated2d_oracle as tab2
import tabulated_oracle as tab
from openmmtools_amd import custom_expr as cx
from openmmtools_amd.system import (System, system_to_desc, CustomBondForce, CustomAngleForce, CustomTorsionForce, CustomExternalForce,
                                    CustomCompoundBondForce, CustomCentroidBondForce, CustomNonbondedForce, CustomGBForce,
                                    Continuous1DFunction, Discrete1DFunction, Continuous2DFunction, Discrete2DFunction, Discrete3DFunction)

NAMES = ('t2x2', 't2x3', 't3x2', 't5x7', 'p4x6', 'p3x4')
GENERAL = ('t5x7', 'p4x6')


def _grid(t):
    return t.xmin + t.hx * np.arange(t.nx), t.ymin + t.hy * np.arange(t.ny)


def _scales(t):
    top = np.abs(t.f).max()
    return top, top / t.hx, top / t.hy, top / (t.hx * t.hy)


def _random_arguments(t, n, seed, margin=0.0):
    rng = np.random.default_rng(seed)
    Lx, Ly = t.xmax - t.xmin, t.ymax - t.ymin
    return rng.uniform(t.xmin - margin * Lx, t.xmax + margin * Lx, n), rng.uniform(t.ymin - margin * Ly, t.ymax + margin * Ly, n)


# ---- the definition, on the reference -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_interpolation_at_every_node(name):
    t = cases.table(name)
    xs, ys = _grid(t)
    xs[-1], ys[-1] = t.xmax, t.ymax                                # (the last nodes are the bounds themselves)
    for j, y in enumerate(ys):
        for i, x in enumerate(xs):
            v, kx, ky = t.value_and_gradient(float(x), float(y))
            assert abs(v - t.f[j, i]) <= 1e-14 * abs(t.f[j, i]), (i, j)
            assert abs(kx - t.fx[j, i]) <= 1e-12 * _scales(t)[1] and abs(ky - t.fy[j, i]) <= 1e-12 * _scales(t)[2], (i, j)


@pytest.mark.parametrize('nx,ny', [(2, 2), (2, 3), (3, 2), (5, 7)])
def test_a_bilinear_function_is_reproduced_with_its_gradient(nx, ny):
    a, b, c, d = 0.7, -1.3, 2.1, 0.9
    xmin, xmax, ymin, ymax = -0.5, 1.75, 0.25, 1.5
    x, y = np.linspace(xmin, xmax, nx)[None, :], np.linspace(ymin, ymax, ny)[:, None]
    t = tab2.Table2D(nx, ny, (a + b * x + c * y + d * x * y).reshape(-1), xmin, xmax, ymin, ymax)
    px, py = _random_arguments(t, 200, nx + ny)
    worst = 0.0
    for p, q in zip(px, py):
        v, kx, ky = t.value_and_gradient(float(p), float(q))
        worst = max(worst, abs(v - (a + b * p + c * q + d * p * q)), abs(kx - (b + d * q)), abs(ky - (c + d * p)))
    print('%d x %d: %.3g' % (nx, ny, worst))
    assert worst <= 1e-12 * 10.0                                   # (|f|, |fx|, |fy| stay below 10)


@pytest.mark.parametrize('nx,ny,periodic', [(2, 3, False), (3, 2, False), (5, 7, False), (4, 6, True), (9, 5, True)])
def test_a_separable_table_is_the_product_of_two_1d_splines(nx, ny, periodic):
    xmin, xmax, ymin, ymax = -1.0, 2.0, 0.5, 1.75
    s, u = 2.0 * math.pi * np.arange(nx) / (nx - 1), 2.0 * math.pi * np.arange(ny) / (ny - 1)
    g, h = 2.0 + np.sin(s + 0.4) + 0.3 * np.cos(2.0 * s), 1.5 + np.cos(u - 0.2) + 0.25 * np.sin(2.0 * u)
    if periodic:
        g[-1], h[-1] = g[0], h[0]
    t = tab2.Table2D(nx, ny, (h[:, None] * g[None, :]).reshape(-1), xmin, xmax, ymin, ymax, periodic)
    sg, sh = tab.Spline(g, xmin, xmax, periodic), tab.Spline(h, ymin, ymax, periodic)
    px, py = _random_arguments(t, 300, nx * ny, margin=1.5 if periodic else 0.0)
    top, topx, topy, _ = _scales(t)
    worst = np.zeros(3)
    for p, q in zip(px, py):
        v, kx, ky = t.value_and_gradient(float(p), float(q))
        (gv, gk), (hv, hk) = sg.value_and_slope(float(p)), sh.value_and_slope(float(q))
        worst = np.maximum(worst, [abs(v - gv * hv) / top, abs(kx - gk * hv) / topx, abs(ky - gv * hk) / topy])
    print('%d x %d periodic = %s: %s' % (nx, ny, periodic, worst))
    assert np.all(worst <= 1e-12)


@pytest.mark.parametrize('name', NAMES)
def test_the_node_derivatives_commute(name):
    """fxy = D_y D_x f equals D_x D_y f: D_x and D_y are linear maps that act on different indices"""
    t = cases.table(name)
    other = np.array([tab2.node_derivatives(t.fy[j], t.xmin, t.xmax, t.periodic) for j in range(t.ny)])
    assert np.abs(t.fxy - other).max() <= 1e-12 * _scales(t)[3]


@pytest.mark.parametrize('name', NAMES)
def test_value_and_partials_are_continuous_across_every_interior_patch_edge(name):
    """from the node's coordinate (the patch to the right) and the f64 number below it (the patch to the left); the step itself moves a
    value by |slope| ulp, far inside the bound"""
    t = cases.table(name)
    xs, ys = _grid(t)
    top, topx, topy, _ = _scales(t)
    rng = np.random.default_rng(7)
    worst, edges = 0.0, 0
    for x in xs[1:-1]:
        for y in rng.uniform(t.ymin, t.ymax, 12):
            a, b = t.value_and_gradient(float(np.nextafter(x, -np.inf)), float(y)), t.value_and_gradient(float(x), float(y))
            worst = max(worst, abs(a[0] - b[0]) / top, abs(a[1] - b[1]) / topx, abs(a[2] - b[2]) / topy)
            edges += 1
    for y in ys[1:-1]:
        for x in rng.uniform(t.xmin, t.xmax, 12):
            a, b = t.value_and_gradient(float(x), float(np.nextafter(y, -np.inf))), t.value_and_gradient(float(x), float(y))
            worst = max(worst, abs(a[0] - b[0]) / top, abs(a[1] - b[1]) / topx, abs(a[2] - b[2]) / topy)
            edges += 1
    print('%s: %d edge points, %.3g' % (name, edges, worst))
    assert worst <= 1e-9 and (edges > 0 or t.nx == 2 == t.ny)


@pytest.mark.parametrize('name', ('p4x6', 'p3x4'))
def test_a_periodic_function_repeats(name):
    """F(x, y) = F(x + Lx, y) = F(x, y - 2 Ly), gradients included; the seam itself joins C1 (value and partials from both sides).
    Bound: the wrap rounds the argument by a few ulp of a number up to 3 L, which moves a value by that times the slope -- 1e-12 of
    the scales leaves three orders of room."""
    t = cases.table(name)
    Lx, Ly = t.xmax - t.xmin, t.ymax - t.ymin
    top, topx, topy, _ = _scales(t)
    scale = np.array([top, topx, topy])
    px, py = _random_arguments(t, 200, 11)
    for p, q in zip(px, py):
        a = np.array(t.value_and_gradient(float(p), float(q)))
        for b in (t.value_and_gradient(float(p + Lx), float(q)), t.value_and_gradient(float(p), float(q - 2.0 * Ly)),
                  t.value_and_gradient(float(p - Lx), float(q + Ly))):
            assert np.all(np.abs(a - np.array(b)) <= 1e-12 * scale)
    for q in py[:20]:
        a, b = np.array(t.value_and_gradient(t.xmin, float(q))), np.array(t.value_and_gradient(t.xmax, float(q)))
        assert np.all(np.abs(a - b) <= 1e-12 * scale)
    for p in px[:20]:
        a, b = np.array(t.value_and_gradient(float(p), t.ymin)), np.array(t.value_and_gradient(float(p), t.ymax))
        assert np.all(np.abs(a - b) <= 1e-12 * scale)


def test_the_reference_is_a_function_of_duals_in_both_arguments():
    t = cases.table('t5x7')
    g = np.array([[1.0, 0.0, 0.5], [0.0, 2.0, -1.0]])
    v, kx, ky = t.value_and_gradient(1.1, 0.3)
    both = t(dual.Dual(1.1, g[0]), dual.Dual(0.3, g[1]))
    assert both.v == v and np.allclose(both.g, kx * g[0] + ky * g[1], rtol=1e-15)
    assert np.array_equal(t(dual.Dual(1.1, g[0]), 0.3).g, kx * g[0]) and np.array_equal(t(1.1, dual.Dual(0.3, g[1])).g, ky * g[1])
    assert t(1.1, 0.3) == v and t(dual.Dual(1.1, np.zeros(0)), 0.3).g.size == 0
    with tab.registered(tab=t):
        e = dual.Expression('2*tab(x, y*y)')(dict(x=dual.Dual(1.1, np.array([1.0, 0.0])), y=dual.Dual(0.5, np.array([0.0, 1.0]))))
    v, kx, ky = t.value_and_gradient(1.1, 0.25)
    assert e.v == 2.0 * v and np.allclose(e.g, [2.0 * kx, 2.0 * ky * 2.0 * 0.5], rtol=1e-15)
    eps = 1e-6                                                     # (and the partials are the function's: central differences)
    assert abs((t(1.1 + eps, 0.3) - t(1.1 - eps, 0.3)) / (2 * eps) - t.value_and_gradient(1.1, 0.3)[1]) <= 1e-7 * _scales(t)[1]
    assert abs((t(1.1, 0.3 + eps) - t(1.1, 0.3 - eps)) / (2 * eps) - t.value_and_gradient(1.1, 0.3)[2]) <= 1e-7 * _scales(t)[2]


# ---- the compiler's blocks and the interpreter against the reference ----------------------------------------------------------------------
def _bond(energy, names=(), params=(), **functions):
    f = CustomBondForce(energy)
    for n in names:
        f.addPerBondParameter(n)
    for name, fn in functions.items():
        f.addTabulatedFunction(name, fn)
    f.addBond(0, 1, list(params))
    return f


def _system(n, forces, box=None):
    s = System()
    for _ in range(n):
        s.addParticle(12.0)
    if box is not None:
        s.setDefaultPeriodicBoxVectors([box[0], 0, 0], [0, box[1], 0], [0, 0, box[2]])
    for f in forces:
        s.addForce(f)
    return s


@pytest.mark.parametrize('name', NAMES + ('cmap',))
def test_the_compilers_block_against_the_reference(name):
    t = cases.table(name)
    term = system_to_desc(_system(2, [_bond('3 + tab(r, k)', ('k',), (0.5,), tab=cases.function(name))]))['custom_terms']['000']
    assert term['program'].tolist() == [[cx.CONST, 0], [cx.VAR, 0], [cx.PARAM, 0], [cx.TABLE2D, 1], [cx.ADD, 0]] and term['stack_depth'] == 3
    block = term['consts'][1:]
    assert len(block) == 8 + 4 * t.nx * t.ny
    assert block[:8].tolist() == [t.nx, t.ny, t.xmin, t.xmax, t.ymin, t.ymax, float(t.periodic), 0.0]
    got = block[8:].reshape(t.ny, t.nx, 4)
    err = np.abs(got - t.nodes()).max(axis=(0, 1)) / np.array(_scales(t))
    print('%s: f %.3g, fx %.3g, fy %.3g, fxy %.3g (relative)' % ((name,) + tuple(err)))
    assert np.array_equal(got[..., 0], t.f) and np.all(err <= 1e-12)
    if t.periodic:                                                # the last row and column of node data repeat the first
        assert np.array_equal(got[-1], got[0]) and np.array_equal(got[:, -1], got[:, 0])


def test_the_blocks_of_the_lookups_and_the_operands():
    f = _bond('two(r, a) + three(a, r, 1) + two(a, r) + one(r)', ('a',), (1.0,), two=cases.lookup2_function(), three=cases.lookup3_function(),
              one=Discrete1DFunction([1.0, 2.0]))
    term = system_to_desc(_system(2, [f]))['custom_terms']['000']
    ops = [(o, a) for o, a in term['program'].tolist() if o in (cx.LOOKUP1D, cx.LOOKUP2D, cx.LOOKUP3D)]
    assert ops == [(cx.LOOKUP2D, 1), (cx.LOOKUP3D, 9), (cx.LOOKUP2D, 1), (cx.LOOKUP1D, 25)]       # one block per function, in the order first called
    c = term['consts']
    assert c[0] == 1.0 and c[1:9].tolist() == [2.0, 3.0] + cases.LOOKUP2.tolist()
    assert c[9:25].tolist() == [2.0, 3.0, 2.0, 0.0] + cases.LOOKUP3.tolist() and c[25:].tolist() == [2.0, 1.0, 2.0]
    assert term['stack_depth'] == 4


@pytest.mark.parametrize('name', NAMES)
def test_the_interpreter_against_the_reference(name):
    """custom_expr.table2d_values (the device's formulas, the sum over the four corners) on random arguments inside and around the
    range, and run_values through a compiled program of one variable.  Bound 1e-12 max|f|: both routes carry a few dozen roundings of
    numbers no larger than max|f|."""
    t = cases.table(name)
    term = system_to_desc(_system(2, [_bond('tab(a*r + b, r) + 0.5*tab(r, c)', ('a', 'b', 'c'), (0.0, 0.0, 0.0), tab=cases.function(name))]))['custom_terms']['000']
    offset = int(term['program'][term['program'][:, 0] == cx.TABLE2D][0, 1])
    px, py = _random_arguments(t, 400, 3, margin=1.2 if t.periodic else 0.25)
    want = np.array([t(float(p), float(q)) for p, q in zip(px, py)])
    got = cx.table2d_values(term['consts'], offset, px, py)
    inside = (px >= t.xmin) & (px <= t.xmax) & (py >= t.ymin) & (py <= t.ymax)
    assert t.periodic or (np.all(want[~inside] == 0.0) and (~inside).sum() > 50 and inside.sum() > 50)
    assert want[inside].min() > 1.0                                # (the tables of the GPU cases stay positive between their nodes)
    print('%s: %.3g' % (name, np.abs(got - want).max() / _scales(t)[0]))
    assert np.all(np.abs(got - want) <= 1e-12 * _scales(t)[0]) and np.all(got[want == 0.0] == 0.0)
    a, b, c = 0.8, t.xmin - 0.1, 0.5 * (t.ymin + t.ymax)
    r = np.random.default_rng(4).uniform(t.ymin - 0.2, t.ymax + 0.2, 300)
    want = np.array([t(a * v + b, v) + 0.5 * t(v, c) for v in r.tolist()])
    assert np.all(np.abs(cx.run_values(term, r, [a, b, c], []) - want) <= 1.5e-12 * _scales(t)[0])


@pytest.mark.parametrize('name', GENERAL)
def test_out_of_range_arguments(name):
    """exactly min and max belong to the end patches; one ulp outside, 1e300 and an infinity are 0 where the function is not periodic;
    a periodic function wraps them (an infinity: NaN); a NaN in either argument is NaN whatever the other is"""
    t = cases.table(name)
    term = system_to_desc(_system(2, [_bond('tab(r, k)', ('k',), (0.0,), tab=cases.function(name))]))['custom_terms']['000']
    y_in = 0.5 * (t.ymin + t.ymax) + 0.1
    x_in = 0.5 * (t.xmin + t.xmax) + 0.1
    up, down = lambda v: float(np.nextafter(v, np.inf)), lambda v: float(np.nextafter(v, -np.inf))
    points = [(t.xmin, y_in), (t.xmax, y_in), (x_in, t.ymin), (x_in, t.ymax), (t.xmin, t.ymin), (t.xmax, t.ymax),
              (down(t.xmin), y_in), (up(t.xmax), y_in), (x_in, down(t.ymin)), (x_in, up(t.ymax)), (1e300, y_in), (x_in, -1e300),
              (math.inf, y_in), (x_in, -math.inf), (math.nan, y_in), (x_in, math.nan), (math.nan, 1e300), (1e300, math.nan),
              (math.nan, math.inf)]
    got = cx.table2d_values(term['consts'], 0, [p[0] for p in points], [p[1] for p in points])
    want = np.array([t(*p) for p in points])
    print(name, got.tolist())
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[14:]).all()
    ok = ~np.isnan(want)
    assert np.all(np.abs(got[ok] - want[ok]) <= 1e-12 * _scales(t)[0])
    assert np.all(got[:6] > 1.0)                                   # the bounds themselves are inside
    if t.periodic:
        assert np.isnan(got[12:14]).all() and np.all(got[6:12] > 1.0)
        assert abs(got[0] - got[1]) <= 1e-12 * _scales(t)[0]        # min and max are one point
    else:
        assert np.all(got[6:14] == 0.0) and np.all(want[6:14] == 0.0)
        for p in points[6:14]:
            assert t.value_and_gradient(*p) == (0.0, 0.0, 0.0)
    # through a compiled program
    r = np.array([t.xmin, t.xmax, down(t.xmin), up(t.xmax), 1e300, math.nan])
    out = cx.run_values(term, r, [y_in], [])
    assert np.array_equal(np.isnan(out), [False] * 5 + [True]) and (t.periodic or np.all(out[2:5] == 0.0)) and np.all(out[:2] > 1.0)


def test_the_lookups_round_halves_away_from_zero_and_give_nan_outside():
    two, three = cases.lookup2(), cases.lookup3()
    term = system_to_desc(_system(2, [_bond('two(r, a) + 0*three(r, a, b)', ('a', 'b'), (0.0, 0.0), two=cases.lookup2_function(),
                                            three=cases.lookup3_function())]))['custom_terms']['000']
    at = {int(o): int(a) for o, a in term['program'].tolist() if o in (cx.LOOKUP2D, cx.LOOKUP3D)}       # (behind the scalar constants)
    x = np.array([0.0, 1.0, 0.49, 0.5, -0.49, -0.5, 1.49, 1.5, math.nan, math.inf, 0.0, 1.0, 0.0, 0.0, 1.0])
    y = np.array([0.0, 2.0, 1.49, 1.5, 2.49, 1.0, 0.5, 0.0, 1.0, 1.0, 2.5, -0.5, math.nan, -0.49, 1e300])
    want = [4.0, 3.0, 6.5, 3.0, 2.0, math.nan, 7.25, math.nan, math.nan, math.nan, math.nan, math.nan, math.nan, 4.0, math.nan]
    got = cx.lookup_grid_values(term['consts'], at[cx.LOOKUP2D], x, y)
    ref = np.array([two(float(p), float(q)) for p, q in zip(x, y)])
    assert np.array_equal(got, want, equal_nan=True) and np.array_equal(ref, want, equal_nan=True)
    assert [two(i, j) for j in range(3) for i in range(2)] == cases.LOOKUP2.tolist()          # values[i + xsize*j]
    assert [three(i, j, k) for k in range(2) for j in range(3) for i in range(2)] == cases.LOOKUP3.tolist()
    z = np.array([0.0, 1.0, 0.5, 1.49, 1.5, -0.5, math.nan])
    got = cx.lookup_grid_values(term['consts'], at[cx.LOOKUP3D], 1.0, 2.0, z)
    assert np.array_equal(got, [3.0, 3.5, 3.5, 3.5, math.nan, math.nan, math.nan], equal_nan=True)
    assert np.array_equal(got, [three(1.0, 2.0, float(v)) for v in z], equal_nan=True)
    grad = three(dual.Dual(1.0, np.ones(2)), 2.0, dual.Dual(0.2, np.ones(2)))
    assert grad.v == 3.0 and not grad.g.any()
    out = cx.run_values(term, np.array([0.0, 1.0, 1.5, -0.5]), [2.0, 1.0], [])
    assert np.array_equal(out, [2.0, 3.0, math.nan, math.nan], equal_nan=True)


# ---- the classes ------------------------------------------------------------------------------------------------------------------------
def test_accessors_and_copy():
    f = Continuous2DFunction(3, 2, (1, 2, 4, 3, 5, 6), -1, 3, 0, 2)
    assert f.getFunctionParameters() == (3, 2, [1.0, 2.0, 4.0, 3.0, 5.0, 6.0], -1.0, 3.0, 0.0, 2.0) and f.getPeriodic() is False
    g = f.Copy()
    f.setFunctionParameters(2, 2, [3.0, 3.0, 1.0, 1.0], 0.0, 1.0, 0.0, 1.0)
    assert g.getFunctionParameters() == (3, 2, [1.0, 2.0, 4.0, 3.0, 5.0, 6.0], -1.0, 3.0, 0.0, 2.0)
    assert f.getFunctionParameters() == (2, 2, [3.0, 3.0, 1.0, 1.0], 0.0, 1.0, 0.0, 1.0)
    p = Continuous2DFunction(3, 2, [1.0, 2.0, 1.0, 1.0, 2.0, 1.0], 0.0, 1.0, 0.0, 1.0, periodic=True)
    assert p.Copy().getPeriodic() is True and p.Copy().getFunctionParameters() == p.getFunctionParameters()
    d = Discrete2DFunction(2, 1, [1, 2])
    e = d.Copy()
    d.setFunctionParameters(1, 1, [5.0])
    assert e.getFunctionParameters() == (2, 1, [1.0, 2.0]) and d.getFunctionParameters() == (1, 1, [5.0]) and not hasattr(d, 'getPeriodic')
    d3 = Discrete3DFunction(1, 2, 2, [1, 2, 3, 4])
    e3 = d3.Copy()
    d3.setFunctionParameters(1, 1, 1, [7.0])
    assert e3.getFunctionParameters() == (1, 2, 2, [1.0, 2.0, 3.0, 4.0]) and d3.getFunctionParameters() == (1, 1, 1, [7.0])
    b = CustomBondForce('tab(r, 1)')
    assert b.addTabulatedFunction('tab', g) == 0 and b.getTabulatedFunction(0) is g and b.getTabulatedFunctionName(0) == 'tab'
    assert copy.deepcopy(b).getTabulatedFunction(0).getFunctionParameters() == g.getFunctionParameters()
    # a function changed after the descriptor was made does not reach it: the blocks are copies
    desc = system_to_desc(_system(2, [_bond('tab(r, 1)', tab=g)]))
    before = desc['custom_terms']['000']['consts'].copy()
    g.setFunctionParameters(2, 2, [9.0, 9.0, 9.0, 9.0], 0.0, 1.0, 0.0, 1.0)
    assert np.array_equal(desc['custom_terms']['000']['consts'], before)


def test_the_constructors_refuse_by_name():
    ok = [1.0, 2.0, 3.0, 4.0]
    for args, match in (((2, 2, ok[:3], 0.0, 1.0, 0.0, 1.0), '3 values for a grid of 2 x 2'), ((2, 3, ok, 0.0, 1.0, 0.0, 1.0), '4 values for a grid of 2 x 3'),
                        ((1, 4, ok, 0.0, 1.0, 0.0, 1.0), 'xsize = 1'), ((4, 1, ok, 0.0, 1.0, 0.0, 1.0), 'ysize = 1'),
                        ((2, 2, ok, 1.0, 1.0, 0.0, 1.0), 'xmin = 1.0 is not below xmax'), ((2, 2, ok, 0.0, 1.0, 2.0, 1.0), 'ymin = 2.0 is not below ymax'),
                        ((2, 2, ok, 0.0, math.inf, 0.0, 1.0), 'xmin = 0.0, xmax = inf are not finite'),
                        ((2, 2, ok, 0.0, 1.0, math.nan, 1.0), 'ymin = nan, ymax = 1.0 are not finite'),
                        ((2, 2, [1.0, math.nan, 1.0, 1.0], 0.0, 1.0, 0.0, 1.0), 'value 1 is not finite'),
                        ((3, 2, [1.0, 2.0, 1.5, 1.0, 2.0, 1.5], 0.0, 1.0, 0.0, 1.0, True), 'last row and column equal to the first'),
                        ((3, 2, [1.0, 2.0, 1.0, 1.0, 2.5, 1.0], 0.0, 1.0, 0.0, 1.0, True), 'last row and column equal to the first')):
        with pytest.raises(ValueError, match='Continuous2DFunction.*' + match):
            Continuous2DFunction(*args)
    with pytest.raises(ValueError, match='Discrete2DFunction: 3 values for a grid of 2 x 2'):
        Discrete2DFunction(2, 2, ok[:3])
    with pytest.raises(ValueError, match='Discrete2DFunction: ysize = 0'):
        Discrete2DFunction(2, 0, [])
    with pytest.raises(ValueError, match='Discrete2DFunction: value 0 is not finite'):
        Discrete2DFunction(1, 1, [math.inf])
    with pytest.raises(ValueError, match='Discrete3DFunction: 4 values for a grid of 2 x 2 x 2'):
        Discrete3DFunction(2, 2, 2, ok)
    with pytest.raises(ValueError, match='Discrete3DFunction: zsize = 0'):
        Discrete3DFunction(2, 2, 0, [])
    f = Continuous2DFunction(2, 2, ok, 0.0, 1.0, 0.0, 1.0)
    with pytest.raises(ValueError, match='not below'):
        f.setFunctionParameters(2, 2, ok, 0.0, 0.0, 0.0, 1.0)
    assert f.getFunctionParameters() == (2, 2, ok, 0.0, 1.0, 0.0, 1.0)              # a refused change changes nothing


# ---- what is refused by name --------------------------------------------------------------------------------------------------------------
def test_what_is_refused_by_name():
    flat = Continuous2DFunction(2, 2, [1.0, 2.0, 3.0, 4.0], 0.0, 1.0, 0.0, 1.0)
    two, three = cases.lookup2_function(), cases.lookup3_function()
    line = Continuous1DFunction([1.0, 2.0], 0.0, 1.0)
    for energy, sentence in (('tab(r)', "tabulated function 'tab' takes 2 arguments, not 1"), ('tab(r, r, r)', "tabulated function 'tab' takes 2 arguments, not 3"),
                             ('two(r)', "tabulated function 'two' takes 2 arguments, not 1"), ('three(r, r)', "tabulated function 'three' takes 3 arguments, not 2"),
                             ('line(r, r)', "tabulated function 'line' takes 1 argument, not 2"), ('look(r, 1)', "tabulated function 'look' takes 1 argument, not 2")):
        with pytest.raises(NotImplementedError, match='CustomBondForce.*' + sentence):
            system_to_desc(_system(2, [_bond(energy, tab=flat, two=two, three=three, line=line, look=Discrete1DFunction([1.0]))]))
    # the cell cap: 65536 values pass, one row more does not
    assert cx.MAX_TABLE_CELLS == 65536
    system_to_desc(_system(2, [_bond('tab(r, 1)', tab=Continuous2DFunction(256, 256, np.ones(65536), 0.0, 1.0, 0.0, 1.0))]))
    with pytest.raises(NotImplementedError, match=r"tabulated function 'tab' has 65792 values \(256 x 257; the engine takes 65536\)"):
        system_to_desc(_system(2, [_bond('tab(r, 1)', tab=Continuous2DFunction(256, 257, np.ones(65792), 0.0, 1.0, 0.0, 1.0))]))
    with pytest.raises(NotImplementedError, match="tabulated function 'two' has 65537 values"):
        system_to_desc(_system(2, [_bond('two(r, 1)', two=Discrete2DFunction(65537, 1, np.ones(65537)))]))
    with pytest.raises(NotImplementedError, match="tabulated function 'three' has 65600 values"):
        system_to_desc(_system(2, [_bond('three(r, 1, 1)', three=Discrete3DFunction(41, 40, 40, np.ones(65600)))]))
    system_to_desc(_system(2, [_bond('three(r, 1, 1)', three=Discrete3DFunction(64, 32, 32, np.ones(65536)))]))

    class Continuous3DFunction:                                   # the kind that stays out, and a plain foreign object
        pass
    for foreign in (object(), Continuous3DFunction()):
        with pytest.raises(NotImplementedError, match="CustomBondForce.*tabulated function 'tab'.*only Continuous1DFunction.*Discrete3DFunction are supported"):
            system_to_desc(_system(2, [_bond('tab(r)', tab=foreign)]))
    with pytest.raises(NotImplementedError, match="a Continuous3DFunction"):
        system_to_desc(_system(2, [_bond('tab(r)', tab=Continuous3DFunction())]))
    # the long-range correction of a pair energy that calls any of the three
    box = (3.0, 3.0, 3.0)
    for energy, fn in (('tab(r, t1 + t2)', flat), ('tab(t1, t2)*r^-6', cases.lookup2_function()), ('tab(t1, t2, 0)*r^-6', cases.lookup3_function())):
        nb = CustomNonbondedForce(energy)
        nb.addPerParticleParameter('t')
        nb.addTabulatedFunction('tab', fn)
        for _ in range(3):
            nb.addParticle([0.0])
        nb.setNonbondedMethod(CustomNonbondedForce.CutoffPeriodic)
        nb.setCutoffDistance(0.9)
        assert len(system_to_desc(_system(3, [nb], box))['custom_terms']) == 1
        nb.setUseLongRangeCorrection(True)
        with pytest.raises(NotImplementedError, match="CustomNonbondedForce.*long-range correction.*tabulated function.*'tab'"):
            system_to_desc(_system(3, [nb], box))
    # CustomGBForce keeps refusing every tabulated function
    gb = CustomGBForce()
    gb.addTabulatedFunction('tab', flat)
    gb.addParticle([])
    with pytest.raises(NotImplementedError, match='tabulated'):
        system_to_desc(_system(1, [gb]))


# ---- the descriptor of every kind ---------------------------------------------------------------------------------------------------------
def _force_of_kind(kind):
    fn = dict(tab=cases.function('t3x2'), two=cases.lookup2_function(), three=cases.lookup3_function())
    if kind == 'bond':
        f = CustomBondForce('tab(r, k) + two(k, 1) + three(k, 1, 0)'); f.addPerBondParameter('k'); f.addBond(0, 1, [1.0])
    elif kind == 'angle':
        f = CustomAngleForce('tab(theta, k) + two(k, 1) + three(k, 1, 0)'); f.addPerAngleParameter('k'); f.addAngle(0, 1, 2, [1.0])
    elif kind == 'torsion':
        f = CustomTorsionForce('tab(theta, k) + two(k, 1) + three(k, 1, 0)'); f.addPerTorsionParameter('k'); f.addTorsion(0, 1, 2, 3, [1.0])
    elif kind == 'external':
        f = CustomExternalForce('tab(x, y) + two(k, 1) + three(k, 1, 0) + z'); f.addPerParticleParameter('k'); f.addParticle(0, [1.0])
    elif kind == 'compound':
        f = CustomCompoundBondForce(3, 'tab(distance(p1,p2), angle(p1,p2,p3)) + two(k, 1) + three(k, 1, 0)'); f.addPerBondParameter('k')
        f.addBond([0, 1, 2], [1.0])
    elif kind == 'centroid':
        f = CustomCentroidBondForce(2, 'tab(distance(g1,g2), k) + two(k, 1) + three(k, 1, 0)'); f.addPerBondParameter('k')
        f.addGroup([0, 1]); f.addGroup([2, 3]); f.addBond([0, 1], [1.0])
    else:
        f = CustomNonbondedForce('tab(r, k1 + k2) + two(k1, k2) + three(k1, k2, 0)'); f.addPerParticleParameter('k')
        for _ in range(4):
            f.addParticle([1.0])
    for name, function in fn.items():
        f.addTabulatedFunction(name, function)
    return f


@pytest.mark.parametrize('kind', ['bond', 'angle', 'torsion', 'external', 'compound', 'centroid', 'nonbonded'])
def test_the_descriptor_of_every_kind(kind):
    term = system_to_desc(_system(4, [_force_of_kind(kind)]))['custom_terms']['000']
    ops = term['program'][:, 0].tolist()
    assert ops.count(cx.TABLE2D) == 1 and ops.count(cx.LOOKUP2D) == 1 and ops.count(cx.LOOKUP3D) == 1
    offsets = {int(o): int(a) for o, a in term['program'].tolist() if o in (cx.TABLE2D, cx.LOOKUP2D, cx.LOOKUP3D)}
    c = term['consts']
    n_scalars = offsets[cx.TABLE2D]
    assert offsets[cx.LOOKUP2D] == n_scalars + 8 + 24 and offsets[cx.LOOKUP3D] == n_scalars + 8 + 24 + 8 and len(c) == n_scalars + 8 + 24 + 8 + 16
    assert c[n_scalars:n_scalars + 8].tolist() == [3.0, 2.0, -1.5, 1.5, -1.25, 1.5, 0.0, 0.0]
    assert np.abs(c[n_scalars + 8:n_scalars + 32].reshape(2, 3, 4) - cases.table('t3x2').nodes()).max() <= 1e-12 * _scales(cases.table('t3x2'))[0]
    assert c[offsets[cx.LOOKUP2D]:offsets[cx.LOOKUP2D] + 8].tolist() == [2.0, 3.0] + cases.LOOKUP2.tolist()
    assert c[offsets[cx.LOOKUP3D]:].tolist() == [2.0, 3.0, 2.0, 0.0] + cases.LOOKUP3.tolist()
    # the stack effect: the compiler's depth is what the opcodes' pops give
    sp = top = 0
    for o, _ in term['program'].tolist():
        sp += 1 - cx.POPS.get(o, 1)
        top = max(top, sp)
    assert sp == 1 and top == term['stack_depth']
