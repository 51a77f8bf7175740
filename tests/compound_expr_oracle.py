"""f64 reference for OpenMM energy expressions of a CustomCompoundBondForce, independent of openmmtools_amd/custom_expr.py: the string
is evaluated by ``Expression`` of tests/custom_expr_oracle.py with the bond's coordinates x1 y1 z1 ... as values, the particle names
p1 ... as slot numbers and distance / angle / dihedral / pointdistance as Python functions over the bond's particle positions (minimum
images when the force is periodic); forces are five-point central differences of the f64 energy in Cartesian coordinates, with the step
checked by halving it.
"""
import math

import numpy as np

from custom_expr_oracle import Expression, minimum_image

# the orientational (Boresch) receptor-ligand restraint: one distance, two angles, three dihedrals of six particles
BORESCH = ('lambda_restraints*E; E = (K_r/2)*(distance(p3,p4)-r_aA0)^2 + (K_thetaA/2)*(angle(p2,p3,p4)-theta_A0)^2 '
           '+ (K_thetaB/2)*(angle(p3,p4,p5)-theta_B0)^2 + (K_phiA/2)*dphi_A^2 + (K_phiB/2)*dphi_B^2 + (K_phiC/2)*dphi_C^2; '
           'dphi_A = dA - floor(dA/(2*pi)+0.5)*(2*pi); dA = dihedral(p1,p2,p3,p4)-phi_A0; '
           'dphi_B = dB - floor(dB/(2*pi)+0.5)*(2*pi); dB = dihedral(p2,p3,p4,p5)-phi_B0; '
           'dphi_C = dC - floor(dC/(2*pi)+0.5)*(2*pi); dC = dihedral(p3,p4,p5,p6)-phi_C0; pi = 3.1415926535897932385')
BORESCH_PARAMETERS = ('K_r', 'r_aA0', 'K_thetaA', 'theta_A0', 'K_thetaB', 'theta_B0', 'K_phiA', 'phi_A0', 'K_phiB', 'phi_B0', 'K_phiC', 'phi_C0')


def geometry(x, box=None, periodic=False):
    """distance, angle, dihedral, pointdistance over the particle positions x [P][3] (slots zero-based)"""
    x = np.asarray(x, dtype=np.float64)

    def diff(a, b):
        d = a - b
        return minimum_image(d, box) if periodic else d

    def distance(i, j):
        return float(np.linalg.norm(diff(x[j], x[i])))

    def angle(i, j, k):
        v0, v1 = diff(x[i], x[j]), diff(x[k], x[j])
        c = float(np.dot(v0, v1) / math.sqrt(np.dot(v0, v0) * np.dot(v1, v1)))
        return math.acos(max(-1.0, min(1.0, c)))

    def dihedral(i, j, k, l):
        b1, b2, b3 = diff(x[j], x[i]), diff(x[k], x[j]), diff(x[l], x[k])
        m, n = np.cross(b1, b2), np.cross(b2, b3)
        return math.atan2(float(np.linalg.norm(b2) * np.dot(b1, n)), float(np.dot(m, n)))

    def pointdistance(x1, y1, z1, x2, y2, z2):
        return float(np.linalg.norm(diff(np.array([x2, y2, z2], dtype=np.float64), np.array([x1, y1, z1], dtype=np.float64))))

    return dict(distance=distance, angle=angle, dihedral=dihedral, pointdistance=pointdistance)


def bond_energy(expression, x, names, values, global_values, box=None, periodic=False):
    """the energy of one bond at its particle positions x [P][3]"""
    v = geometry(x, box, periodic)
    for i, p in enumerate(np.asarray(x, dtype=np.float64)):
        v['p%d' % (i + 1)] = i
        v.update({'x%d' % (i + 1): float(p[0]), 'y%d' % (i + 1): float(p[1]), 'z%d' % (i + 1): float(p[2])})
    v.update(zip(names, values))
    v.update(global_values)
    return expression(v)


def boresch_values(x, box=None, periodic=False):
    """(r, theta_A, theta_B, phi_A, phi_B, phi_C) of the six particles x"""
    g = geometry(x, box, periodic)
    return (g['distance'](2, 3), g['angle'](1, 2, 3), g['angle'](2, 3, 4), g['dihedral'](0, 1, 2, 3), g['dihedral'](1, 2, 3, 4),
            g['dihedral'](2, 3, 4, 5))


def wrap(d):
    """d - floor(d / 2 pi + 0.5) 2 pi: the dihedral difference of BORESCH, in [-pi, pi)"""
    return d - math.floor(d / (2.0 * math.pi) + 0.5) * (2.0 * math.pi)


def gradient(f, x, h):
    """Five-point central differences of f(x) in every coordinate of x [P][3]."""
    g = np.zeros_like(x)
    for a in range(x.shape[0]):
        for k in range(3):
            e = []
            for m in (-2, -1, 1, 2):
                y = x.copy()
                y[a, k] += m * h
                e.append(f(y))
            g[a, k] = (e[0] - 8.0 * e[1] + 8.0 * e[2] - e[3]) / (12.0 * h)
    return g


def evaluate(n_particles, energy, atoms, names, params, global_values, positions, box=None, periodic=False, h=1e-4):
    """Per-bond energies [n] and forces [N][3] of one compound-bond force at ``positions`` (f64).  The difference step is checked by
    halving it: the two force sets must agree within 1e-8 of max|F|."""
    expression = Expression(energy)
    positions = np.asarray(positions, dtype=np.float64)
    atoms = np.asarray(atoms, dtype=np.int64).reshape(-1, n_particles)
    params = np.asarray(params, dtype=np.float64).reshape(len(atoms), -1)
    E = np.zeros(len(atoms))
    F, F2 = np.zeros_like(positions), np.zeros_like(positions)
    for t, (idx, p) in enumerate(zip(atoms, params)):
        def f(x, p=p):
            return bond_energy(expression, x, names, p, global_values, box, periodic)
        x = positions[idx].copy()
        E[t] = f(x)
        g, g2 = gradient(f, x, h), gradient(f, x, 0.5 * h)
        for a, i in enumerate(idx):
            F[i] -= g2[a]
            F2[i] -= g[a]
    fmax = np.abs(F).max()
    assert np.abs(F - F2).max() <= 1e-8 * fmax, 'difference step %g: %g of max|F|' % (h, np.abs(F - F2).max() / fmax)
    return E, F
