"""f64 reference for the tabulated functions of two and three arguments of the custom forces (system.Continuous2DFunction,
system.Discrete2DFunction, system.Discrete3DFunction), independent of openmmtools_amd/custom_expr.py (it imports nothing from the package).

The definition is the one of include/remd_hip_custom.h.  Node data: with D the map "samples of a row -> first derivatives at the nodes
of the 1D cubic spline through them" (natural, or periodic), f, fx = D_x f, fy = D_y f and fxy = D_y fx.  Here D takes the spline's second
derivatives from the dense solves of tests/tabulated_oracle.py (the compiler uses the Thomas algorithm).  Evaluation goes another route
than the device's sum over the four corners: the 1D cubic Hermite interpolant along x of (f, fx) and of (fy, fxy) on the rows j and
j + 1 gives f and fy at (x, y_j) and (x, y_{j+1}); the 1D Hermite interpolant along y of those gives the value.  The partial along x is
the same construction on the x-derivatives of the row interpolants.

``Table2D`` is a callable of floats or ``custom_dual_oracle.Dual``s with exact chain-rule partials in both arguments, so that through
``tabulated_oracle.registered(name=Table2D(...))`` the bond, compound, centroid and nonbonded oracles evaluate an energy string that
calls it, unchanged.  ``Lookup2D`` and ``Lookup3D`` have zero gradients.

Conventions: a function that is not periodic is 0 with both partials 0 where either argument lies outside its range (exactly min and
max belong to the end patches); a periodic one wraps each argument, t = x - L floor((x - min) / L), clamped into [min, max]; a NaN
argument (an infinite one of a periodic function) gives NaN, whatever the other argument is; the lookups round halves away from zero
and are NaN where an index lies outside its range.
"""
import math

import numpy as np

import custom_dual_oracle as dual
import tabulated_oracle as tab


def node_derivatives(values, lo, hi, periodic=False):
    """s'(x_i) [n] of the 1D spline through ``values``: (y[i+1] - y[i]) / h - h (2 M[i] + M[i+1]) / 6, and at the last node
    (y[n-1] - y[n-2]) / h + h (M[n-2] + 2 M[n-1]) / 6 (a periodic spline's last node repeats its first)"""
    y = np.asarray(values, dtype=np.float64)
    n = len(y)
    h = (hi - lo) / (n - 1)
    M = tab.second_derivatives(y, lo, hi, periodic)
    d = np.empty(n)
    for i in range(n - 1):
        d[i] = (y[i + 1] - y[i]) / h - h * (2.0 * M[i] + M[i + 1]) / 6.0
    d[n - 1] = d[0] if periodic else (y[n - 1] - y[n - 2]) / h + h * (M[n - 2] + 2.0 * M[n - 1]) / 6.0
    return d


def _hermite(t, h, p0, p1, m0, m1):
    """(value, derivative with respect to the coordinate) of the cubic through p0, p1 with the slopes m0, m1 over an interval h, at t in [0, 1]"""
    v = (2 * t ** 3 - 3 * t ** 2 + 1) * p0 + (3 * t ** 2 - 2 * t ** 3) * p1 + h * ((t ** 3 - 2 * t ** 2 + t) * m0 + (t ** 3 - t ** 2) * m1)
    k = (6 * t ** 2 - 6 * t) * (p0 - p1) / h + (3 * t ** 2 - 4 * t + 1) * m0 + (3 * t ** 2 - 2 * t) * m1
    return v, k


class Table2D:
    """a Continuous2DFunction: values[i + xsize*j] = f(x_i, y_j); table(x, y) for floats or Duals"""

    def __init__(self, xsize, ysize, values, xmin, xmax, ymin, ymax, periodic=False):
        self.nx, self.ny, self.periodic = int(xsize), int(ysize), bool(periodic)
        self.xmin, self.xmax, self.ymin, self.ymax = float(xmin), float(xmax), float(ymin), float(ymax)
        self.hx, self.hy = (self.xmax - self.xmin) / (self.nx - 1), (self.ymax - self.ymin) / (self.ny - 1)
        f = np.asarray(values, dtype=np.float64).reshape(self.ny, self.nx)          # [j][i]
        self.f = f
        self.fx = np.array([node_derivatives(f[j], self.xmin, self.xmax, periodic) for j in range(self.ny)])
        self.fy = np.array([node_derivatives(f[:, i], self.ymin, self.ymax, periodic) for i in range(self.nx)]).T
        self.fxy = np.array([node_derivatives(self.fx[:, i], self.ymin, self.ymax, periodic) for i in range(self.nx)]).T

    def nodes(self):
        """[ny][nx][4]: (f, fx, fy, fxy)"""
        return np.stack([self.f, self.fx, self.fy, self.fxy], axis=-1)

    def _place(self, x, lo, hi, n):
        """(status, patch, offset): status 'nan', 'outside' or 'inside'"""
        if math.isnan(x):
            return 'nan', 0, 0.0
        L = hi - lo
        if self.periodic:
            if math.isinf(x):
                return 'nan', 0, 0.0
            x = min(max(x - L * math.floor((x - lo) / L), lo), hi)
        if not lo <= x <= hi:
            return 'outside', 0, 0.0
        s = (x - lo) / ((hi - lo) / (n - 1))
        i = min(max(int(s), 0), n - 2)
        return 'inside', i, s - i

    def value_and_gradient(self, x, y):
        """(F, dF/dx, dF/dy) at the floats x, y"""
        sx, i, u = self._place(x, self.xmin, self.xmax, self.nx)
        sy, j, w = self._place(y, self.ymin, self.ymax, self.ny)
        if 'nan' in (sx, sy):
            return math.nan, 0.0, 0.0
        if 'outside' in (sx, sy):
            return 0.0, 0.0, 0.0
        rows = []
        for jj in (j, j + 1):
            g, gx = _hermite(u, self.hx, self.f[jj, i], self.f[jj, i + 1], self.fx[jj, i], self.fx[jj, i + 1])          # f, df/dx at (x, y_jj)
            gy, gxy = _hermite(u, self.hx, self.fy[jj, i], self.fy[jj, i + 1], self.fxy[jj, i], self.fxy[jj, i + 1])    # fy, dfy/dx
            rows.append((g, gx, gy, gxy))
        F, Fy = _hermite(w, self.hy, rows[0][0], rows[1][0], rows[0][2], rows[1][2])
        Fx, _ = _hermite(w, self.hy, rows[0][1], rows[1][1], rows[0][3], rows[1][3])
        return float(F), float(Fx), float(Fy)

    def __call__(self, x, y):
        if not isinstance(x, dual.Dual) and not isinstance(y, dual.Dual):
            return self.value_and_gradient(float(x), float(y))[0]
        v, kx, ky = self.value_and_gradient(dual._val(x), dual._val(y))
        like = x.g if isinstance(x, dual.Dual) else y.g
        g = np.zeros_like(like)
        if g.size:
            if isinstance(x, dual.Dual):
                g = g + kx * x.g
            if isinstance(y, dual.Dual):
                g = g + ky * y.g
        return dual.Dual(v, g)


class _Lookup:
    def __init__(self, sizes, values):
        self.sizes = tuple(int(n) for n in sizes)
        self.values = np.asarray(values, dtype=np.float64).reshape(-1)
        assert len(self.values) == int(np.prod(self.sizes))

    def value(self, *args):
        flat, stride = 0, 1
        for n, x in zip(self.sizes, args):
            if math.isnan(x) or math.isinf(x):
                return math.nan
            whole = math.trunc(x)
            k = whole + (int(math.copysign(1, x)) if abs(x - whole) >= 0.5 else 0)
            if not 0 <= k < n:
                return math.nan
            flat, stride = flat + stride * k, stride * n
        return float(self.values[flat])

    def __call__(self, *args):
        assert len(args) == len(self.sizes)
        v = self.value(*[dual._val(a) for a in args])
        duals = [a for a in args if isinstance(a, dual.Dual)]
        return dual.Dual(v, np.zeros_like(duals[0].g)) if duals else v


class Lookup2D(_Lookup):
    """a Discrete2DFunction: values[round(x) + xsize*round(y)]"""

    def __init__(self, xsize, ysize, values):
        super().__init__((xsize, ysize), values)


class Lookup3D(_Lookup):
    """a Discrete3DFunction: values[round(x) + xsize*round(y) + xsize*ysize*round(z)]"""

    def __init__(self, xsize, ysize, zsize, values):
        super().__init__((xsize, ysize, zsize), values)
