"""Reference for the collective variables of stored frames (multistate/analysis.py: frame_cvs_numpy; csrc/frame_cvs.hip), by a route that
shares no code with either: the centroid kinds frame by frame at 50 digits with mpmath, straight from the definitions

    c = x_first + sum_i w_i img(x_i - x_first) / sum_i w_i        img(d) = d - L nint(d / L) under the frame's own box when periodic
    distance |img(c2 - c1)|      angle acos(clamp(v0.v1 / (|v0| |v1|)))      dihedral atan2(|b2| b1.(b2 x b3), (b1 x b2).(b2 x b3))

and the RMSD through the SVD reference of tests/custom_cv_oracle.py (Kabsch with the determinant correction; the evaluators
diagonalise Horn's matrix).  A variable is plain data here, not a descriptor of the package:

    ('distance' | 'angle' | 'dihedral', [atoms of each group], [weights of each group or None: masses], periodic)
    ('rmsd', reference [n_atoms][3], particles)

Values come back as mpmath numbers (RMSD: floats), so that an error can be taken against the unrounded value."""
import mpmath as mp
import numpy as np

import custom_cv_oracle

DIGITS = 50


def _centroid(x, L, atoms, w):
    """x [n_atoms][3] of mpf, L [3] of mpf or None"""
    x0 = x[atoms[0]]
    W = mp.fsum(w)
    c = []
    for a in range(3):
        d = [x[i][a] - x0[a] for i in atoms]
        if L is not None:
            d = [v - L[a] * mp.nint(v / L[a]) for v in d]
        c.append(x0[a] + mp.fdot(w, d) / W)
    return c


def _diff(a, b, L):
    d = [p - q for p, q in zip(a, b)]
    if L is not None:
        d = [v - l * mp.nint(v / l) for v, l in zip(d, L)]
    return d


def _dot(a, b):
    return mp.fdot(a, b)


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def evaluate(variables, pos, box=None, masses=None):
    """[F][n_variables] (a list of lists; mpf, or float for an RMSD) at the frames pos [F][n_atoms][3] (f32 or f64, taken exactly)"""
    out = []
    with mp.workdps(DIGITS):
        for f in range(len(pos)):
            x = [[mp.mpf(float(v)) for v in row] for row in pos[f]]
            row = []
            for var in variables:
                if var[0] == 'rmsd':
                    _, reference, particles = var
                    row.append(float(custom_cv_oracle.rmsd(np.asarray(pos[f], dtype=np.float64)[list(particles)],
                                                           np.asarray(reference, dtype=np.float64)[list(particles)])))
                    continue
                kind, groups, weights, periodic = var
                L = [mp.mpf(float(v)) for v in box[f]] if periodic and box is not None else None
                c = []
                for atoms, w in zip(groups, weights):
                    atoms = list(atoms)
                    if len(atoms) == 1:
                        w = [1.0]
                    elif w is None:
                        w = [masses[i] for i in atoms]
                    c.append(_centroid(x, L, atoms, [mp.mpf(float(v)) for v in w]))
                if kind == 'distance':
                    d = _diff(c[1], c[0], L)
                    row.append(mp.sqrt(_dot(d, d)))
                elif kind == 'angle':
                    v0, v1 = _diff(c[0], c[1], L), _diff(c[2], c[1], L)
                    cosine = _dot(v0, v1) / mp.sqrt(_dot(v0, v0) * _dot(v1, v1))
                    row.append(mp.acos(max(mp.mpf(-1), min(mp.mpf(1), cosine))))
                elif kind == 'dihedral':
                    b1, b2, b3 = _diff(c[1], c[0], L), _diff(c[2], c[1], L), _diff(c[3], c[2], L)
                    m, n = _cross(b1, b2), _cross(b2, b3)
                    row.append(mp.atan2(mp.sqrt(_dot(b2, b2)) * _dot(b1, n), _dot(m, n)))
                else:
                    raise ValueError(kind)
            out.append(row)
    return out


def errors(values, reference, modulo_2pi=False):
    """|value - reference| [F][n] as floats, taken at 50 digits against the unrounded reference; modulo_2pi: the distance on the circle"""
    err = np.zeros((len(reference), len(reference[0])))
    with mp.workdps(DIGITS):
        for f, row in enumerate(reference):
            for v, ref in enumerate(row):
                got = float(values[f][v])
                if got != got:
                    err[f, v] = np.nan
                    continue
                d = abs(mp.mpf(got) - mp.mpf(ref))
                if modulo_2pi:
                    d = min(d, abs(2 * mp.pi - d))
                err[f, v] = float(d)
    return err
