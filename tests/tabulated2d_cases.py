"""Shared by tests/test_custom_tabulated2d_cpu.py and tests/test_custom_tabulated2d_gpu.py: the tables of two arguments the cases use, as
the package's functions and as the reference's (tests/tabulated2d_oracle.py).  nx != ny and hx != hy in every one, so that a transposed
index or a swapped spacing shows.  Every table is positive (>= 1.2 at its samples; the interpolant stays above 1), so that nothing
cancels inside a term and the energy bound 1e-11 sum|E_t| has room for the rounding of the arguments.  The bounds of the tables that
take hand-placed arguments are f32 numbers."""
import math

import numpy as np

import tabulated2d_oracle as tab2
from openmmtools_amd.system import Continuous2DFunction, Discrete2DFunction, Discrete3DFunction

# name: (nx, ny, xmin, xmax, ymin, ymax, periodic)
TABLES = dict(t2x2=(2, 2, 0.0, 1.5, -1.0, 1.0, False), t2x3=(2, 3, 0.0, 1.5, -1.0, 1.0, False), t3x2=(3, 2, -1.5, 1.5, -1.25, 1.5, False),
              t5x7=(5, 7, 0.25, 2.75, -1.0, 2.0, False), b5x7=(5, 7, 0.25, 4.25, -1.0, 2.0, False), p4x6=(4, 6, -math.pi, math.pi, -1.0, 1.5, True),
              p3x4=(3, 4, -1.0, 1.0, 0.0, 3.0, True), cmap=(24, 24, -math.pi, math.pi, -math.pi, math.pi, True))
# Discrete2DFunction [2 x 3] (values[i + 2 j]) and Discrete3DFunction [2 x 3 x 2] (values[i + 2 j + 6 k])
LOOKUP2 = np.array([4.0, 1.5, 6.5, 7.25, 2.0, 3.0])
LOOKUP3 = np.array([4.0, 1.5, 6.5, 7.25, 2.0, 3.0, 9.0, 8.5, 1.25, 5.0, 2.75, 3.5])


def samples(name):
    """flat values[i + nx*j]"""
    nx, ny, xmin, xmax, ymin, ymax, periodic = TABLES[name]
    s = 2.0 * math.pi * np.arange(nx)[None, :] / (nx - 1)
    t = 2.0 * math.pi * np.arange(ny)[:, None] / (ny - 1)
    if periodic:
        f = 3.0 + np.sin(s + 0.3) * np.cos(t + 0.1 * nx) + 0.5 * np.cos(2.0 * s - t + 0.7) + 0.3 * np.sin(t)
        f[:, -1], f[-1, :] = f[:, 0], f[0, :]
        f[-1, -1] = f[0, 0]
    else:
        f = 3.0 + np.sin(0.9 * s + 0.1 * nx) * np.cos(0.7 * t + 0.2) + 0.5 * np.cos(0.6 * s - 0.8 * t + 0.7) + 0.2 * np.sin(0.5 * t * s)
    assert f.shape == (ny, nx) and f.min() >= 1.2
    return f.reshape(-1)


def function(name):
    nx, ny, xmin, xmax, ymin, ymax, periodic = TABLES[name]
    return Continuous2DFunction(nx, ny, samples(name), xmin, xmax, ymin, ymax, periodic)


_TABLES = {}


def table(name):
    """the reference's function (fitted once per session: the fit is a dense solve per row and column)"""
    if name not in _TABLES:
        nx, ny, xmin, xmax, ymin, ymax, periodic = TABLES[name]
        _TABLES[name] = tab2.Table2D(nx, ny, samples(name), xmin, xmax, ymin, ymax, periodic)
    return _TABLES[name]


def lookup2_function():
    return Discrete2DFunction(2, 3, LOOKUP2)


def lookup3_function():
    return Discrete3DFunction(2, 3, 2, LOOKUP3)


def lookup2():
    return tab2.Lookup2D(2, 3, LOOKUP2)


def lookup3():
    return tab2.Lookup3D(2, 3, 2, LOOKUP3)
