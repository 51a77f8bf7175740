"""Shared by tests/test_custom_tabulated_cpu.py and tests/test_custom_tabulated_gpu.py: the tables the GPU cases use, as the package's
functions and as the helper's (tests/tabulated_oracle.py).  Every table is positive (>= 1.1 at its samples), so that nothing cancels in
a term and the energy bound 1e-11 sum|E_t| has room for the rounding of the argument (the CPU file checks exactly that).  The bounds
of the tables that take hand-placed arguments are f32 numbers, and so are their nodes (h a power of two times 1.5)."""
import math

import numpy as np

import tabulated_oracle as tab
from openmmtools_amd.system import Continuous1DFunction, Discrete1DFunction

# name: (n, min, max, periodic)
TABLES = dict(r65=(65, 0.0, 5.5, False), a65=(65, 0.0, 3.25, False), per65=(65, -math.pi, math.pi, True), xy65=(65, -1.5, 1.5, False),
              xy33=(33, -1.5, 1.5, False), e2=(2, 0.5, 2.0, False), e3=(3, 0.5, 2.0, False), e65=(65, 0.5, 2.0, False),
              p3=(3, -1.0, 1.0, True), p4=(4, -1.0, 1.0, True), p65=(65, -1.0, 1.0, True))
LOOKUP = np.array([4.0, 1.5, 6.5, 7.25, 2.0, 3.0, 9.0])


def samples(name):
    n, lo, hi, periodic = TABLES[name]
    s = 2.0 * math.pi * np.arange(n) / (n - 1)
    y = 2.5 + np.sin(s + 0.1 * len(name)) + 0.4 * np.cos(3.0 * s + 0.7) if periodic else \
        2.5 + np.sin(1.7 * s + 0.1 * n) + 0.4 * np.cos(4.1 * s + 0.7)
    if periodic:
        y[-1] = y[0]
    return y


def function(name):
    n, lo, hi, periodic = TABLES[name]
    return Continuous1DFunction(samples(name), lo, hi, periodic)


def spline(name):
    n, lo, hi, periodic = TABLES[name]
    return tab.Spline(samples(name), lo, hi, periodic)


def splines():
    return {name: spline(name) for name in TABLES}


def lookup_function():
    return Discrete1DFunction(LOOKUP)
