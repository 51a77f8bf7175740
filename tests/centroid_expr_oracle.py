"""f64 reference for OpenMM energy expressions of a CustomCentroidBondForce, independent of openmmtools_amd/custom_expr.py and of the
device: the groups' centroids with numpy under the engine's stated convention,

    c = x_first + sum_i w_i img(x_i - x_first)          (w normalised to sum 1; img the minimum image where the force is periodic),

then tests/compound_expr_oracle.py's ``evaluate`` with the centroids as its "particles" (the group names g1 ... become the particle
names p1 ... of that helper: the same slots), and the forces it returns on the centroids spread over the groups' atoms with the
weights: dc/dx_i = w_i for every atom, the first one included (its coefficient is 1 - sum_i w_i + w_first = w_first).
"""
import re

import numpy as np

import compound_expr_oracle as compound
from custom_expr_oracle import minimum_image


def normalised(weights):
    w = np.asarray(weights, dtype=np.float64)
    return w / w.sum()


def centroids(groups, positions, box=None, periodic=False):
    """[G][3]: the centroid of every group ((atoms, weights) pairs, the weights summing to 1)"""
    x = np.asarray(positions, dtype=np.float64)
    out = np.zeros((len(groups), 3))
    for g, (atoms, w) in enumerate(groups):
        first = x[atoms[0]]
        acc = np.zeros(3)
        for a, wa in zip(atoms, w):
            d = x[a] - first
            acc += wa * (minimum_image(d, box) if periodic else d)
        out[g] = first + acc
    return out


def as_particles(energy):
    """the energy string with the group names g1, g2, ... written as the particle names p1, p2, ... of the compound helper, and a
    parameter called ``lambda`` (legal in OpenMM; the helper evaluates the string as Python, where it is a keyword) as ``lambda_``"""
    return _python_name_text(re.sub(r'\bg([1-9][0-9]*)\b', r'p\1', energy))


def _python_name_text(text):
    return re.sub(r'\blambda\b', 'lambda_', text)


def evaluate(n_groups_per_bond, energy, bonds, names, params, global_values, groups, positions, box=None, periodic=False, h=1e-4):
    """Per-bond energies [n] and forces [N][3] of one centroid-bond force at ``positions`` (f64).  bonds [n][P]: group numbers;
    groups: (atoms, weights) pairs, any weights (normalised here)."""
    x = np.asarray(positions, dtype=np.float64)
    groups = [(list(a), normalised(w)) for a, w in groups]
    c = centroids(groups, x, box, periodic)
    E, Fc = compound.evaluate(n_groups_per_bond, as_particles(energy), bonds, [_python_name_text(n) for n in names], params,
                              {_python_name_text(n): v for n, v in global_values.items()}, c, box, periodic, h)
    F = np.zeros_like(x)
    for g, (atoms, w) in enumerate(groups):
        for a, wa in zip(atoms, w):
            F[a] += wa * Fc[g]
    return E, F


def evaluate_force(force, masses, positions, box=None, global_values=None):
    """``evaluate`` for a system.CustomCentroidBondForce (or anything with its accessors): groups without weights take the masses"""
    masses = np.asarray(masses, dtype=np.float64)
    groups = []
    for g in range(force.getNumGroups()):
        atoms, w = force.getGroupParameters(g)
        groups.append((atoms, w if len(w) else masses[atoms]))
    bonds, params = [], []
    for b in range(force.getNumBonds()):
        gs, p = force.getBondParameters(b)
        bonds.append(gs); params.append(p)
    g = {force.getGlobalParameterName(i): force.getGlobalParameterDefaultValue(i) for i in range(force.getNumGlobalParameters())}
    g.update(global_values or {})
    names = [force.getPerBondParameterName(i) for i in range(force.getNumPerBondParameters())]
    return evaluate(force.getNumGroupsPerBond(), force.getEnergyFunction(), bonds, names, params, g, groups, positions, box,
                    force.usesPeriodicBoundaryConditions())
