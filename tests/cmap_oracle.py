"""f64 reference for system.CMAPTorsionForce, independent of openmmtools_amd (it imports nothing from the package).

A map of ``size * size`` energies, ``energy[i + size*j]`` at the first angle 2 pi i / size and the second 2 pi j / size and periodic in
both, is the periodic ``tabulated2d_oracle.Table2D`` over [0, 2 pi]^2 on the grid of size + 1 points per axis with the first row and
column repeated at the end: the bicubic patch whose node derivatives come from periodic cubic splines (dense solves there, held to an
independent derivation by tests/test_custom_tabulated2d_cpu.py).  The two dihedrals and their gradients are compositions of the dual
numbers of tests/custom_dual_oracle.py over the 24 coordinates of a term's eight particles, minimum images inside each difference when
the force is periodic; the table chains its two exact partials through them.  Positions are taken as given: the tests hand over the
f32-rounded ones the engine holds.
"""
import math

import numpy as np

import custom_dual_oracle as dual
import tabulated2d_oracle as tab2

TWO_PI = 2.0 * math.pi


def edge_repeated(size, energy):
    """values [(size + 1)^2] of the grid with the first row and column repeated at the end, values[i + (size + 1)*j]"""
    g = np.asarray(energy, dtype=np.float64).reshape(size, size)                  # [j][i]
    g = np.concatenate([g, g[:1]], axis=0)
    return np.concatenate([g, g[:, :1]], axis=1).reshape(-1)


def table(size, energy):
    return tab2.Table2D(size + 1, size + 1, edge_repeated(size, energy), 0.0, TWO_PI, 0.0, TWO_PI, periodic=True)


def angles(x, box=None):
    """(phi, psi) of the eight positions x [8][3] as floats"""
    p = dual.seeds(np.asarray(x, dtype=np.float64), gradients=False)
    return dual._val(dual.dihedral(p, 0, 1, 2, 3, box)), dual._val(dual.dihedral(p, 4, 5, 6, 7, box))


def term(tab, x, box=None):
    """(energy, -dE/dx [8][3], phi, psi) of one term at its eight particle positions x; a particle both dihedrals name appears twice in
    x and each appearance carries its own share"""
    p = dual.seeds(np.asarray(x, dtype=np.float64))
    phi, psi = dual.dihedral(p, 0, 1, 2, 3, box), dual.dihedral(p, 4, 5, 6, 7, box)
    e = tab(phi, psi)
    return e.v, -e.g.reshape(8, 3), phi.v, psi.v


def evaluate(maps, torsions, positions, box=None, periodic=False):
    """maps: [(size, energy)]; torsions: [(map, a1 ... a4, b1 ... b4)]; positions [N][3].  Returns dict(E [n], F [N][3], G [n][8][3] each
    term's own forces on its eight slots, phi [n], psi [n], partners [N] the contributions an atom receives (one per slot that names it),
    peak [N][3] the largest |contribution| per component)."""
    positions = np.asarray(positions, dtype=np.float64)
    tabs = [table(size, energy) for size, energy in maps]
    torsions = np.asarray(torsions, dtype=np.int64).reshape(-1, 9)
    n = len(torsions)
    E, G, phi, psi = np.zeros(n), np.zeros((n, 8, 3)), np.zeros(n), np.zeros(n)
    F, partners, peak = np.zeros_like(positions), np.zeros(len(positions)), np.zeros_like(positions)
    for t, row in enumerate(torsions):
        E[t], G[t], phi[t], psi[t] = term(tabs[row[0]], positions[row[1:]], box if periodic else None)
        for a, i in enumerate(row[1:]):
            F[i] += G[t, a]
            partners[i] += 1
            peak[i] = np.maximum(peak[i], np.abs(G[t, a]))
    return dict(E=E, F=F, G=G, phi=phi, psi=psi, partners=partners, peak=peak)


def convention_term(tab, x):
    """(energy, forces [8][3]) of one term by the documented formulas, for degenerate geometry where the dual numbers divide by zero:
    with b1 = p1 - p0, b2 = p2 - p1, b3 = p3 - p2, m = b1 x b2, n = b2 x b3, the angle is atan2(|b2| b1.n, m.n), its gradients
    g0 = -|b2| m / max(|m|^2, 1e-24), g3 = |b2| n / max(|n|^2, 1e-24), g1 = -(1 + b1.b2 / |b2|^2) g0 + (b3.b2 / |b2|^2) g3,
    g2 = -(1 + b3.b2 / |b2|^2) g3 + (b1.b2 / |b2|^2) g0 (include/remd_hip_custom.h: REMD_CX_DIHEDRAL, REMD_CUSTOM_CMAP)"""
    x = np.asarray(x, dtype=np.float64)
    ang, g = [], np.zeros((8, 3))
    for q in (0, 4):
        b1, b2, b3 = x[q + 1] - x[q], x[q + 2] - x[q + 1], x[q + 3] - x[q + 2]
        m, n = np.cross(b1, b2), np.cross(b2, b3)
        lb2 = math.sqrt(np.dot(b2, b2))
        ang.append(math.atan2(lb2 * np.dot(b1, n), np.dot(m, n)))
        g[q], g[q + 3] = -lb2 * m / max(np.dot(m, m), 1e-24), lb2 * n / max(np.dot(n, n), 1e-24)
        s12, s32 = np.dot(b1, b2) / lb2 ** 2, np.dot(b3, b2) / lb2 ** 2
        g[q + 1], g[q + 2] = -(1.0 + s12) * g[q] + s32 * g[q + 3], -(1.0 + s32) * g[q + 3] + s12 * g[q]
    v, k0, k1 = tab.value_and_gradient(ang[0], ang[1])
    g[:4] *= -k0
    g[4:] *= -k1
    return v, g, ang[0], ang[1]


def force_bound(result):
    """[N][3]: n (2^-23 max|contribution| + 2^-31), n the contributions the atom receives: the f32 rounding of every contribution handed
    to the fixed-point accumulator, and the accumulator's own step (the bound of custom_nonbonded_oracle.force_bound, per component)"""
    return result['partners'][:, None] * (2.0 ** -23 * result['peak'] + 2.0 ** -31)


def energy_bound(result):
    return 1e-11 * np.abs(result['E']).sum()


# ---- the cases the CPU and GPU tests share (numbers only) ------------------------------------------------------------------------------
def _sampled(size, seed):
    """a smooth positive map with some roughness: energy[i + size*j] at (2 pi i / size, 2 pi j / size), kJ/mol"""
    a = TWO_PI * np.arange(size) / size
    phi, psi = a[None, :], a[:, None]                                            # [j][i]
    rough = np.random.default_rng(seed).uniform(-0.5, 0.5, (size, size))
    return (8.0 + 3.0 * np.cos(phi) + 2.0 * np.sin(2.0 * psi) + 1.5 * np.cos(phi - psi) + rough).reshape(-1)


MAPS = [(4, _sampled(4, 41)), (7, _sampled(7, 42)), (24, _sampled(24, 43))]


def _f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


# hand-placed segments of five atoms (units of 0.125 nm, exact in f32), by the atom they start at
CIS = np.array([[0, 1, 0], [0, 0, 0], [1, 0, 0], [1, 1, 0], [0.25, 1, 0]], dtype=np.float64)          # phi = 0, psi = 0: all in the plane z = 0
TRANS = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [2, 1, 0], [2, 2, 0]], dtype=np.float64)           # phi = psi = +-pi
QUARTER = np.array([[1, 0, 0], [0, 0, 0], [0, 1, 0], [0, 1, 1], [1, 1, 1]], dtype=np.float64)         # phi = -pi/2, psi = +pi/2
SEGMENTS = {0: CIS, 20: TRANS, 40: QUARTER}
HAIR = 1e-8                                                                                          # nm: the last CIS atom off the plane (an angle of 1.07e-7)


def chain_positions(n, replicas=2, seed=7, special=True):
    """[replicas][n][3] f32-rounded positions of a chain: a random walk of 0.15 nm bonds whose consecutive bonds are never nearly
    parallel, each replica a perturbed copy; with ``special`` the SEGMENTS replace their atoms (the same in every replica) and the last
    CIS atom sits HAIR above the plane in replica 0 and below it in replica 1"""
    rng = np.random.default_rng(seed)
    x = np.zeros((n, 3))
    prev = np.array([1.0, 0.0, 0.0])
    for i in range(1, n):
        while True:
            d = rng.normal(size=3); d /= np.linalg.norm(d)
            if abs(np.dot(d, prev)) < 0.8:
                break
        x[i] = x[i - 1] + 0.15 * d
        prev = d
    xs = np.stack([x + (rng.normal(0.0, 0.01, x.shape) if r else 0.0) for r in range(replicas)])
    if special:
        for start, seg in SEGMENTS.items():
            xs[:, start:start + 5] = 0.125 * seg + np.array([0.5 * start, 3.0, 0.0])
        xs[0, 4, 2], xs[1, 4, 2] = HAIR, -HAIR
    return _f32(xs)


XS70 = chain_positions(74)
# 70 terms on 74 atoms, consecutive terms sharing four atoms; the maps in a scrambled order, the QUARTER term on the size-4 map
TORSIONS70 = np.array([((5 * t + 1) % 3, t, t + 1, t + 2, t + 3, t + 1, t + 2, t + 3, t + 4) for t in range(70)])
TORSIONS70[40, 0] = 0
TORSIONS70[20, 0] = 2


def check_special_angles(refs):
    """the hand-placed angles of XS70 are what their docstrings say, in the reference's own arithmetic"""
    for r, ref in enumerate(refs):
        assert abs(ref['phi'][20]) == math.pi and abs(ref['psi'][20]) == math.pi
        assert ref['phi'][40] == -0.5 * math.pi and ref['psi'][40] == 0.5 * math.pi
        assert ref['phi'][0] == 0.0 and 0.5e-7 < abs(ref['psi'][0]) < 2e-7
    assert refs[0]['psi'][0] * refs[1]['psi'][0] < 0.0                            # a hair either side of 0 / 2 pi


def straddling_positions():
    """(boxes [2][3], xs [2][8][3]): eight atoms of a compact chain around the corner of the box, wrapped into [0, L): consecutive atoms
    lie across the x, y and z faces"""
    boxes = _f32([[2.0, 2.25, 2.5], [2.0, 2.25, 2.5]])
    rng = np.random.default_rng(5)
    base = np.array([[-0.10, -0.05, 0.08], [0.04, -0.12, -0.03], [0.12, 0.03, 0.05], [-0.02, 0.10, -0.09], [-0.13, 0.02, 0.04],
                     [0.03, -0.06, 0.13], [0.10, 0.09, -0.05], [-0.06, 0.14, 0.07]])
    xs = np.stack([base, base + rng.normal(0.0, 0.01, base.shape)])
    xs = _f32(xs - boxes[:, None, :] * np.floor(xs / boxes[:, None, :]))
    for x, box in zip(xs, boxes):
        across = np.abs(np.diff(x, axis=0)) > 0.5 * box
        assert across.any(axis=0).all() and np.all(x >= 0.0) and np.all(x < box)
    return boxes, xs
