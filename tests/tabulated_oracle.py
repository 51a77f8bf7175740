"""f64 reference for the tabulated functions of the custom forces (system.Continuous1DFunction, system.Discrete1DFunction), independent of
openmmtools_amd/custom_expr.py (it imports nothing from the package).

The second derivatives of the spline come from a dense ``np.linalg.solve`` of the natural and of the periodic system (the compiler
solves the same systems by the Thomas algorithm); the spline and its first derivative are a function of a ``custom_dual_oracle.Dual``, so
that the existing ``Expression`` evaluates ``tab(...)`` with exact chain-rule partials; the lookup has a zero gradient.

``registered(tab=..., ...)`` puts such functions among the names every expression of tests/custom_dual_oracle.py knows, for the
duration of a ``with`` block: custom_dual_oracle, custom_nonbonded_oracle and centroid_expr_oracle then evaluate an energy string that
calls them, unchanged.

The stated conventions (include/remd_hip_custom.h): outside [min, max] a function that is not periodic is 0 with the derivative 0;
exactly min and max belong to the end intervals; a periodic function wraps its argument, t = x - (max - min) floor((x - min) / (max -
min)); the lookup rounds halves away from zero and is NaN outside 0 ... n - 1.
"""
import contextlib
import math

import numpy as np

import custom_dual_oracle as dual


def second_derivatives(values, lo, hi, periodic=False):
    """y'' [n] by a dense solve: natural (y''[0] = y''[n-1] = 0) or periodic (y''[n-1] = y''[0], the rows cyclic over the n - 1 points)"""
    y = np.asarray(values, dtype=np.float64)
    n = len(y)
    h = (hi - lo) / (n - 1)
    out = np.zeros(n)
    if not periodic:
        if n > 2:
            m = n - 2
            A = 4.0 * np.eye(m) + np.eye(m, k=1) + np.eye(m, k=-1)
            out[1:-1] = np.linalg.solve(A, 6.0 * (y[2:] - 2.0 * y[1:-1] + y[:-2]) / h ** 2)
        return out
    m = n - 1
    A, rhs = np.zeros((m, m)), np.zeros(m)
    for i in range(m):
        A[i, i] += 4.0
        A[i, (i - 1) % m] += 1.0
        A[i, (i + 1) % m] += 1.0
        rhs[i] = 6.0 * (y[(i + 1) % m] - 2.0 * y[i] + y[(i - 1) % m]) / h ** 2
    out[:m] = np.linalg.solve(A, rhs)
    out[-1] = out[0]
    return out


class Spline:
    """the cubic spline of a Continuous1DFunction: spline(x) for a float or a Dual"""

    def __init__(self, values, lo, hi, periodic=False):
        self.y, self.lo, self.hi, self.periodic = np.asarray(values, dtype=np.float64), float(lo), float(hi), bool(periodic)
        self.n = len(self.y)
        self.h = (self.hi - self.lo) / (self.n - 1)
        self.y2 = second_derivatives(self.y, self.lo, self.hi, self.periodic)

    def value_and_slope(self, x):
        """(y, dy/dx) at the float x"""
        if math.isnan(x):
            return math.nan, 0.0
        L = self.hi - self.lo
        if self.periodic:
            if math.isinf(x):
                return math.nan, 0.0
            t = min(max(x - L * math.floor((x - self.lo) / L), self.lo), self.hi)      # (rounding may leave the wrap an ulp outside)
        else:
            t = x
        if not self.lo <= t <= self.hi:
            return 0.0, 0.0
        h = self.h
        s = (t - self.lo) / h
        i = min(max(int(s), 0), self.n - 2)
        b = s - i                                   # (t - x_i) / h; a = (x_{i+1} - t) / h as 1 - b, so that a + b is exactly 1
        a = 1.0 - b
        y, y2 = self.y, self.y2
        v = a * y[i] + b * y[i + 1] + ((a ** 3 - a) * y2[i] + (b ** 3 - b) * y2[i + 1]) * h * h / 6.0
        k = (y[i + 1] - y[i]) / h + ((1.0 - 3.0 * a * a) * y2[i] + (3.0 * b * b - 1.0) * y2[i + 1]) * h / 6.0
        return float(v), float(k)

    def __call__(self, x):
        if not isinstance(x, dual.Dual):
            return self.value_and_slope(float(x))[0]
        v, k = self.value_and_slope(x.v)
        return dual.Dual(v, x.g * k if x.g.size else x.g)


class Lookup:
    """a Discrete1DFunction: values[round(x)], halves away from zero; NaN outside 0 ... n - 1; zero gradient"""

    def __init__(self, values):
        self.values = np.asarray(values, dtype=np.float64)

    def value(self, x):
        if math.isnan(x) or math.isinf(x):
            return math.nan
        whole = math.trunc(x)
        k = whole + (int(math.copysign(1, x)) if abs(x - whole) >= 0.5 else 0)
        return float(self.values[k]) if 0 <= k < len(self.values) else math.nan

    def __call__(self, x):
        if not isinstance(x, dual.Dual):
            return self.value(float(x))
        return dual.Dual(self.value(x.v), np.zeros_like(x.g))


@contextlib.contextmanager
def registered(**functions):
    """the names ``functions`` known to every dual.Expression inside the block (dual.FUNCTIONS is the default table of its call)"""
    clash = set(functions) & set(dual.FUNCTIONS)
    assert not clash, clash
    dual.FUNCTIONS.update(functions)
    try:
        yield
    finally:
        for name in functions:
            del dual.FUNCTIONS[name]
