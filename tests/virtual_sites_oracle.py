"""Numpy f64 oracle of the virtual sites (include/remd_hip_vsites.h): where a site sits and how the force on it goes to its
parents, written independently of openmmtools_amd/virtual_sites.py and of the device code.

Kinds: 0 two-particle average, 1 three-particle average (x = sum w_i x_i), 2 out of plane
(x = x1 + w12 r12 + w13 r13 + wcross r12 x r13 with plain differences)."""
import numpy as np

TWO, THREE, PLANE = 0, 1, 2
N_PARENTS = {TWO: 2, THREE: 3, PLANE: 3}


def place(kind, parents, weights):
    """parents [n_parents][3] -> the site [3]"""
    p = np.asarray(parents, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    if kind in (TWO, THREE):
        n = N_PARENTS[kind]
        return (w[:n, None] * p[:n]).sum(axis=0)
    r12, r13 = p[1] - p[0], p[2] - p[0]
    return p[0] + w[0] * r12 + w[1] * r13 + w[2] * np.cross(r12, r13)


def redistribute(kind, parents, weights, force):
    """The force [3] on the site as forces [n_parents][3] on its parents: F_i = (d x_site / d x_i)^T F."""
    p = np.asarray(parents, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    f = np.asarray(force, dtype=np.float64)
    if kind in (TWO, THREE):
        n = N_PARENTS[kind]
        return w[:n, None] * f[None, :]
    r12, r13 = p[1] - p[0], p[2] - p[0]
    f2 = w[0] * f + w[2] * np.cross(r13, f)           # d/d r12 of (r12 x r13) . f = r13 x f
    f3 = w[1] * f + w[2] * np.cross(f, r12)           # d/d r13 of (r12 x r13) . f = f x r12
    return np.array([f - f2 - f3, f2, f3])


def place_table(table, x):
    """A copy of x [..., N, 3] with every site of a system_to_desc 'virtual_sites' table placed, in f64."""
    x = np.array(x, dtype=np.float64)
    flat = x.reshape(-1, x.shape[-2], 3)
    for s, kind, par, w in zip(table['site'], table['kind'], table['parent'], table['weight']):
        n = N_PARENTS[int(kind)]
        for r in range(len(flat)):
            flat[r, s] = place(int(kind), flat[r, par[:n]], w)
    return flat.reshape(x.shape)


def redistribute_table(table, x, forces):
    """forces [N, 3] of a System in which the sites are ordinary particles -> (forces with the sites' shares on the parents and 0
    on the sites, per particle the largest |contribution| it received, per particle the number of sites it is a parent of)"""
    f = np.array(forces, dtype=np.float64)
    out = f.copy()
    big = np.abs(f).copy()
    count = np.zeros(len(f), dtype=np.int64)
    for s, kind, par, w in zip(table['site'], table['kind'], table['parent'], table['weight']):
        n = N_PARENTS[int(kind)]
        share = redistribute(int(kind), x[par[:n]], w, f[s])
        for k in range(n):
            out[par[k]] += share[k]
            big[par[k]] = np.maximum(big[par[k]], np.abs(share[k]))
            count[par[k]] += 1
        out[s] = 0.0
    return out, big, count
