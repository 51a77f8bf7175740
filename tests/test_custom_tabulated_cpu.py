"""CPU: tabulated functions of the custom forces (system.Continuous1DFunction, system.Discrete1DFunction): the test helper
tests/tabulated_oracle.py against scipy, the compiler's blocks and second derivatives against the helper, the host interpreter
(custom_expr.run_values) against the helper, the constructors and everything that is refused by name.

Scales of the relative bounds.  A spline value is a combination of samples: its error is relative to max|y|.  A first derivative
is a difference of samples over h, (y[i+1] - y[i]) / h + ..., so every way of computing it carries eps max|y| / h: its error (and that
of y'', a second difference: max|y| / h^2) is relative to that."""
import copy
import math

import numpy as np
import pytest

import tabulated_cases as cases
import tabulated_oracle as tab
from openmmtools_amd import alchemy, custom_expr as cx, states, system_xml, testsystems, unit
from openmmtools_amd.system import (System, system_to_desc, CustomBondForce, CustomNonbondedForce, CustomGBForce, Continuous1DFunction,
                                    Discrete1DFunction)

SIZES = (2, 3, 4, 65, 8192)
SHAPES = [(n, False) for n in SIZES] + [(n, True) for n in SIZES if n >= 3]       # (a periodic function has at least 3 points)


def _samples(n, lo, hi, periodic):
    x = np.linspace(lo, hi, n)
    if periodic:
        s = 2.0 * math.pi * (x - lo) / (hi - lo)
        y = 2.0 + np.sin(s) + 0.5 * np.cos(3.0 * s + 0.3)
        y[-1] = y[0]
        return y
    return 2.0 + np.sin(3.0 * x) + 0.5 * np.cos(7.0 * x + 0.3)


def _arguments(n, lo, hi):
    """interior points, every node (of at most 65; else a stride), both ends"""
    h = (hi - lo) / (n - 1)
    nodes = lo + np.arange(n)[::max(1, n // 64)] * h
    rng = np.random.default_rng(n)
    return np.unique(np.concatenate([[lo, hi], nodes[(nodes >= lo) & (nodes <= hi)], rng.uniform(lo, hi, 200)]))


@pytest.mark.parametrize('n,periodic', SHAPES)
def test_the_helper_against_scipy(n, periodic):
    interpolate = pytest.importorskip('scipy.interpolate')
    lo, hi = -0.7, 2.3
    y = _samples(n, lo, hi, periodic)
    s = tab.Spline(y, lo, hi, periodic)
    x = _arguments(n, lo, hi)
    if n == 2:                                                   # (scipy takes a natural spline of two points as the line it is)
        want_v, want_k = y[0] + (y[1] - y[0]) * (x - lo) / (hi - lo), np.full_like(x, (y[1] - y[0]) / (hi - lo))
    else:
        ref = interpolate.CubicSpline(np.linspace(lo, hi, n), y, bc_type='periodic' if periodic else 'natural')
        want_v, want_k = ref(x), ref(x, 1)
    got = np.array([s.value_and_slope(float(v)) for v in x])
    scale = np.abs(y).max()
    ev, ek = np.abs(got[:, 0] - want_v).max() / scale, np.abs(got[:, 1] - want_k).max() / (scale / s.h)
    print('n = %d periodic = %s: value %.3g, derivative %.3g (relative)' % (n, periodic, ev, ek))
    assert ev <= 1e-12 and ek <= 1e-12


@pytest.mark.parametrize('n,periodic', SHAPES)
def test_the_compilers_second_derivatives_against_the_dense_solve(n, periodic):
    lo, hi = -0.7, 2.3
    y = _samples(n, lo, hi, periodic)
    got, want = cx.spline_second_derivatives(y, lo, hi, periodic), tab.second_derivatives(y, lo, hi, periodic)
    h = (hi - lo) / (n - 1)
    err = np.abs(got - want).max() / (np.abs(y).max() / h ** 2)
    print('n = %d periodic = %s: %.3g' % (n, periodic, err))
    assert err <= 1e-12
    assert got[-1] == got[0] if periodic else (got[0] == 0.0 and got[-1] == 0.0)


def _compile(energy, functions, variables=('r',), parameters=()):
    return cx.compile_expression(energy, variables, parameters, {}, where='test', tabulated=list(functions.items()))


def test_the_block_layout_and_the_operands():
    y, z = _samples(5, 0.0, 2.0, False), _samples(7, -1.0, 1.0, True)
    f, g, d = Continuous1DFunction(y, 0.0, 2.0), Continuous1DFunction(z, -1.0, 1.0, periodic=True), Discrete1DFunction([4.0, 5.0, 6.0])
    # one function called twice: one block, behind the two scalars; the scalars deduplicate among themselves only
    prog = _compile('2*tab(r) + tab(5*r) + 5', dict(tab=f, unused=g))
    ops = prog['program'].tolist()
    assert [o for o in ops if o[0] == cx.TABLE1D] == [[cx.TABLE1D, 2], [cx.TABLE1D, 2]]
    assert prog['consts'][:2].tolist() == [2.0, 5.0] and len(prog['consts']) == 2 + 4 + 2 * 5
    assert prog['consts'][2:6].tolist() == [5.0, 0.0, 2.0, 0.0]
    assert np.array_equal(prog['consts'][6:11], y)
    assert np.abs(prog['consts'][11:16] - tab.second_derivatives(y, 0.0, 2.0)).max() <= 1e-12 * np.abs(y).max() / 0.5 ** 2
    assert prog['stack_depth'] == 3
    # a scalar equal to a table's header value is a constant of its own (5.0 = n above); a table value is never taken for a scalar
    assert [o for o in ops if o[0] == cx.CONST] == [[cx.CONST, 0], [cx.CONST, 1], [cx.CONST, 1]]
    # two functions and a lookup in one expression, one of them inside a definition: blocks in the order first called
    prog = _compile('a*look(r) + per(r); a = tab(r) + 1', dict(tab=f, per=g, look=d))
    ops = prog['program'].tolist()
    assert [o for o in ops if o[0] in (cx.TABLE1D, cx.LOOKUP1D)] == [[cx.TABLE1D, 1], [cx.LOOKUP1D, 15], [cx.TABLE1D, 19]]
    c = prog['consts']
    assert len(c) == 1 + 14 + 4 + 18
    assert c[15:19].tolist() == [3.0, 4.0, 5.0, 6.0] and c[19:23].tolist() == [7.0, -1.0, 1.0, 1.0] and np.array_equal(c[23:30], z)


def _grid(s):
    """min, max, every node, one f64 ulp outside each end, negative arguments and (periodic) multiples of the period"""
    nodes = s.lo + np.arange(s.n) * s.h
    L = s.hi - s.lo
    x = [s.lo, s.hi, np.nextafter(s.lo, -np.inf), np.nextafter(s.hi, np.inf), -3.7, -0.1, -1e30, 1e30, np.inf, -np.inf, np.nan]
    x += list(nodes) + list(np.random.default_rng(s.n).uniform(s.lo - 0.5 * L, s.hi + 0.5 * L, 300))
    if s.periodic:
        x += [s.lo + k * L for k in (-3, -1, 1, 2, 7)] + [s.lo + 0.3 * L + k * L for k in (-3, -1, 1, 2, 7)]
    return np.array(x)


@pytest.mark.parametrize('n,periodic', [(2, False), (3, False), (65, False), (8192, False), (3, True), (4, True), (65, True)])
def test_run_values_against_the_helper(n, periodic):
    lo, hi = (-math.pi, math.pi) if periodic else (0.25, 2.75)
    y = _samples(n, lo, hi, periodic)
    s = tab.Spline(y, lo, hi, periodic)
    prog = _compile('tab(r)', dict(tab=Continuous1DFunction(y, lo, hi, periodic)))
    x = _grid(s)
    got, want = cx.run_values(prog, x, [], []), np.array([s(float(v)) for v in x])
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok]).max() / np.abs(y).max()
    print('n = %d periodic = %s: %.3g' % (n, periodic, err))
    assert err <= 1e-14
    if not periodic:
        outside = (x < lo) | (x > hi)
        assert outside.sum() >= 6 and np.all(got[outside] == 0.0)                  # one ulp outside, 1e30, inf: exactly 0
        assert got[0] != 0.0 and got[1] != 0.0                                     # exactly min and max: the end intervals
        assert abs(got[0] - y[0]) <= 1e-14 * np.abs(y).max() and abs(got[1] - y[-1]) <= 1e-14 * np.abs(y).max()
        assert np.isnan(got[10]) and not np.isnan(got[:10]).any()
    else:
        assert np.isnan(got[8:11]).all()                                           # +-inf cannot be wrapped; NaN stays NaN
        near = np.abs(x) < 100.0                                                   # (1e30 has lost its place in the period: 0 or on the curve)
        assert np.all(got[near] >= y.min() - 0.5)                                  # every moderate argument lands on the curve
        k = len(x) - 10                                                            # min + k L is min again, min + 0.3 L + k L is min + 0.3 L
        # (the argument min + k L is rounded by at most 8 L 2^-52, the slope of these samples is below 10 max|y| / L: 2e-14 max|y|)
        assert np.abs(got[k:k + 5] - y[0]).max() <= 1e-13 * np.abs(y).max() and np.ptp(got[k + 5:]) <= 1e-13 * np.abs(y).max()


def test_run_values_lookup():
    values = np.array([4.0, -5.0, 6.5, 7.25])
    prog = _compile('look(r)', dict(look=Discrete1DFunction(values)))
    helper = tab.Lookup(values)
    x = np.array([k + d for k in range(4) for d in (0.0, 0.49, -0.49)] + [0.5, 1.5, 2.5, -0.5, 3.5, -0.51, 3.51, 4.0, -1.0, 1e30, -1e30,
                                                                         np.inf, np.nan, 0.49999999999999994])
    got, want = cx.run_values(prog, x, [], []), np.array([helper(float(v)) for v in x])
    assert np.array_equal(got, want, equal_nan=True)
    assert got[:12].tolist() == [v for v in values for _ in range(3)]
    assert got[12:15].tolist() == [-5.0, 6.5, 7.25]                                # halves away from zero
    assert np.isnan(got[15:25]).all() and got[25] == 4.0                          # -0.5 rounds to -1: out of range


def test_the_constructors_refuse_by_name():
    for args, match in ((([1.0], 0.0, 1.0), 'at least 2'), (([1.0, 2.0], 0.0, 1.0, True), 'at least 3'), (([1.0, 2.0], 1.0, 1.0), 'not below'),
                        (([1.0, 2.0], 2.0, 1.0), 'not below'), (([1.0, 2.0], 0.0, math.inf), 'not finite'),
                        (([1.0, 2.0], math.nan, 1.0), 'not finite'), (([1.0, math.nan], 0.0, 1.0), 'value 1 is not finite'),
                        (([1.0, math.inf, 1.0], 0.0, 1.0), 'value 1 is not finite'), (([1.0, 2.0, 1.5], 0.0, 1.0, True), r'values\[0\] == values\[-1\]')):
        with pytest.raises(ValueError, match='Continuous1DFunction.*' + match):
            Continuous1DFunction(*args)
    with pytest.raises(ValueError, match='Discrete1DFunction: no values'):
        Discrete1DFunction([])
    with pytest.raises(ValueError, match='Discrete1DFunction: value 0 is not finite'):
        Discrete1DFunction([math.nan])
    f = Continuous1DFunction([1.0, 2.0, 1.0], 0.0, 1.0, True)
    with pytest.raises(ValueError, match='at least 3'):
        f.setFunctionParameters([1.0, 1.0], 0.0, 1.0)
    assert f.getFunctionParameters() == ([1.0, 2.0, 1.0], 0.0, 1.0)                # a refused change changes nothing


def test_accessors_and_copy():
    f = Continuous1DFunction((1, 2, 4), -1, 3)
    assert f.getFunctionParameters() == ([1.0, 2.0, 4.0], -1.0, 3.0) and f.getPeriodic() is False
    g = f.Copy()
    f.setFunctionParameters([3.0, 3.0], 0.0, 1.0)
    assert g.getFunctionParameters() == ([1.0, 2.0, 4.0], -1.0, 3.0) and f.getFunctionParameters() == ([3.0, 3.0], 0.0, 1.0)
    assert Continuous1DFunction([1.0, 2.0, 1.0], 0.0, 1.0, periodic=True).Copy().getPeriodic() is True
    d = Discrete1DFunction([1, 2])
    e = d.Copy()
    d.setFunctionParameters([5.0])
    assert e.getFunctionParameters() == [1.0, 2.0] and d.getFunctionParameters() == [5.0]
    b = CustomBondForce('tab(r)')
    assert b.addTabulatedFunction('tab', g) == 0 and b.getTabulatedFunction(0) is g and b.getTabulatedFunctionName(0) == 'tab'
    assert copy.deepcopy(b).getTabulatedFunction(0).getFunctionParameters() == g.getFunctionParameters()


def _bond(energy, **functions):
    f = CustomBondForce(energy)
    for name, fn in functions.items():
        f.addTabulatedFunction(name, fn)
    f.addBond(0, 1, [])
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


def test_what_is_refused_by_name():
    line = Continuous1DFunction([1.0, 2.0], 0.0, 1.0)
    with pytest.raises(NotImplementedError, match="CustomBondForce.*tabulated function 'tab' takes 1 argument, not 2"):
        system_to_desc(_system(2, [_bond('tab(r, r)', tab=line)]))
    big = Continuous1DFunction(np.ones(cx.MAX_TABLE_POINTS + 1), 0.0, 1.0)
    with pytest.raises(NotImplementedError, match="tabulated function 'tab' has 8193 points"):
        system_to_desc(_system(2, [_bond('tab(r)', tab=big)]))
    with pytest.raises(NotImplementedError, match="tabulated function 'look' has 8193 points"):
        system_to_desc(_system(2, [_bond('look(r)', look=Discrete1DFunction(np.ones(cx.MAX_TABLE_POINTS + 1)))]))
    system_to_desc(_system(2, [_bond('tab(r)', tab=Continuous1DFunction(np.ones(cx.MAX_TABLE_POINTS), 0.0, 1.0))]))

    class Continuous2DFunction:                                   # a kind this engine does not have, and a plain foreign object
        pass
    for foreign in (object(), Continuous2DFunction()):
        with pytest.raises(NotImplementedError, match="CustomBondForce.*tabulated function 'tab'"):
            system_to_desc(_system(2, [_bond('tab(r)', tab=foreign)]))
    # the long-range correction of a tabulated pair energy
    nb = CustomNonbondedForce('tab(r)')
    nb.addTabulatedFunction('tab', Continuous1DFunction([1.0, 0.5, 0.0], 0.0, 1.0))
    for _ in range(3):
        nb.addParticle([])
    nb.setNonbondedMethod(CustomNonbondedForce.CutoffPeriodic)
    nb.setCutoffDistance(0.9)
    box = (3.0, 3.0, 3.0)
    assert len(system_to_desc(_system(3, [nb], box))['custom_terms']) == 1
    nb.setUseLongRangeCorrection(True)
    with pytest.raises(NotImplementedError, match="CustomNonbondedForce.*long-range correction.*tabulated function.*'tab'"):
        system_to_desc(_system(3, [nb], box))
    # CustomGBForce keeps refusing every tabulated function
    gb = CustomGBForce()
    gb.addTabulatedFunction('tab', line)
    gb.addParticle([])
    with pytest.raises(NotImplementedError, match='tabulated'):
        system_to_desc(_system(1, [gb]))
    # System XML and the netCDF4 store layout: the sentences of every custom force
    s = _system(2, [_bond('tab(r)', tab=line)])
    with pytest.raises(NotImplementedError, match='CustomBondForce'):
        system_xml.to_xml(s)
    from openmmtools_amd.multistate import _reference_store
    st = states.ThermodynamicState(s, 300.0 * unit.kelvin)
    assert _reference_store.ReferenceStoreWriter.can_store([st], [], []) == "a System with a CustomBondForce (energy 'tab(r)')"


def test_the_alchemical_factory_passes_the_functions_through():
    al = testsystems.AlanineDipeptideVacuum()
    fn = Continuous1DFunction([1.0, 2.0, 4.0], 0.0, 1.0)
    f = _bond('tab(r)', tab=fn)
    al.system.addForce(f)
    system = alchemy.AbsoluteAlchemicalFactory().create_alchemical_system(al.system, alchemy.AlchemicalRegion(alchemical_atoms=list(range(0, 6))))
    kept = [g for g in system.getForces() if isinstance(g, CustomBondForce)]
    assert len(kept) == 1 and kept[0].getNumTabulatedFunctions() == 1 and kept[0].getTabulatedFunctionName(0) == 'tab'
    assert kept[0].getTabulatedFunction(0).getFunctionParameters() == fn.getFunctionParameters()
    terms = system_to_desc(system)['custom_terms']
    assert len(terms) == 1 and terms['000']['program'].tolist() == [[cx.VAR, 0], [cx.TABLE1D, 0]] and len(terms['000']['consts']) == 10


def test_the_gpu_cases_tables_do_not_amplify_argument_rounding():
    """the GPU file's energy bound, 1e-11 sum|E_t|, with the tables it uses: the helper evaluated with its argument moved by one f64 ulp
    stays inside the bound term by term (the tables are positive, >= 1, so nothing cancels in a term)"""
    for name, s in cases.splines().items():
        L = s.hi - s.lo
        x = np.random.default_rng(5).uniform(s.lo - (L if s.periodic else 0.0), s.hi + (3.0 * L if s.periodic else 0.0), 2000)
        x = x[np.abs((x - s.lo) / L - np.rint((x - s.lo) / L)) > 1e-9] if s.periodic else x      # (not on the seam of the wrap itself)
        a, b = np.array([s(float(v)) for v in x]), np.array([s(float(np.nextafter(v, np.inf))) for v in x])
        worst = (np.abs(a - b) / np.abs(a)).max()
        print('%-10s %.3g' % (name, worst))
        assert a.min() >= 1.0 and worst <= 1e-13
