"""f64 reference for CustomHbondForce (openmmtools_amd/custom_expr.py kind 10, csrc/custom_hbond.hip), independent of the package (it
imports nothing from it): the donor x acceptor pairs enumerated in plain Python, the exclusions and the cutoff on distance(d1, a1)
(minimum image under CutoffPeriodic) applied to the positions it is handed -- the f32-rounded ones the device holds, the caller rounds
them -- and every surviving pair evaluated through the dual numbers of tests/custom_dual_oracle.py: d1 d2 d3 a1 a2 a3 are the particle
slots 0 ... 5, distance / angle / dihedral compositions of dual arithmetic over the pair's coordinates, so the derivatives are exact.
"""
import keyword
import re

import numpy as np

import custom_dual_oracle as dual

NO_CUTOFF, CUTOFF_NON_PERIODIC, CUTOFF_PERIODIC = 0, 1, 2
SLOTS = dict(d1=0, d2=1, d3=2, a1=3, a2=4, a3=5)


def _rename(name):
    """(the dual oracle evaluates the string as Python: a name that is a Python keyword -- a global called lambda -- gets a trailing _)"""
    return name + '_' if keyword.iskeyword(name) else name


def named_slots(energy):
    """the particle slots the expression names (every occurrence of d1 ... a3 as a whole word)"""
    return sorted({SLOTS[w] for w in re.findall(r'[A-Za-z_][A-Za-z_0-9]*', energy) if w in SLOTS})


def d1a1(x, donors, acceptors, box=None, method=NO_CUTOFF):
    """[nD][nA]: the distance of d1 and a1 of every pair, the image where the method is CutoffPeriodic"""
    x = np.asarray(x, dtype=np.float64)
    d = x[np.asarray(acceptors)[:, 0]][None, :, :] - x[np.asarray(donors)[:, 0]][:, None, :]
    if method == CUTOFF_PERIODIC:
        L = np.asarray(box, dtype=np.float64)
        d = d - L * np.rint(d / L)
    return np.sqrt((d * d).sum(axis=2))


def pair_energy(expression, x6, box, periodic, values, functions, gradients=True):
    """(energy, dE/dx [6][3]) of one pair at its six particle positions (an unused slot holds anything finite)"""
    p = dual.seeds(np.asarray(x6, dtype=np.float64), gradients)
    pbox = box if periodic else None
    v = dict(distance=lambda i, j: dual.distance(p, i, j, pbox), angle=lambda i, j, k: dual.angle(p, i, j, k, pbox),
             dihedral=lambda i, j, k, l: dual.dihedral(p, i, j, k, l, pbox))
    v.update(SLOTS)
    v.update(values)
    e = expression(v, dict(dual.FUNCTIONS, **functions))
    if not isinstance(e, dual.Dual):
        return float(e), np.zeros((6, 3))
    return e.v, (e.g.reshape(6, 3) if gradients and e.g.size else np.zeros((6, 3)))


def evaluate(energy, donor_names, acceptor_names, donors, acceptors, donor_params, acceptor_params, global_values, x, box=None,
             method=NO_CUTOFF, cutoff=0.0, exclusions=(), functions=None):
    """dict(E [P] pair energies, F [N][3], i [P] donors, j [P] acceptors, r_all the d1-a1 distances of ALL non-excluded pairs,
    count [N] contributions per atom (one per pair and named particle slot that is this atom), peak [N] the largest |component| any one
    contribution has) of one force.  donors [nD][3] and acceptors [nA][3] with -1 for an unused particle."""
    x = np.asarray(x, dtype=np.float64)
    donors, acceptors = np.asarray(donors, dtype=np.int64).reshape(-1, 3), np.asarray(acceptors, dtype=np.int64).reshape(-1, 3)
    donor_params = np.asarray(donor_params, dtype=np.float64).reshape(len(donors), -1)
    acceptor_params = np.asarray(acceptor_params, dtype=np.float64).reshape(len(acceptors), -1)
    expression = dual.Expression(re.sub(r'[A-Za-z_][A-Za-z_0-9]*', lambda m: _rename(m.group(0)), energy))
    slots = named_slots(energy)
    g = {_rename(n): float(v) for n, v in global_values.items()}
    excluded = {(int(a), int(b)) for a, b in exclusions}
    r = d1a1(x, donors, acceptors, box, method)
    allowed = np.ones(r.shape, dtype=bool)
    for a, b in excluded:
        allowed[a, b] = False
    r_all = r[allowed]
    inside = allowed if method == NO_CUTOFF else allowed & (r < cutoff)
    I, J = np.nonzero(inside)
    E, F = np.zeros(len(I)), np.zeros_like(x)
    count, peak = np.zeros(len(x), dtype=np.int64), np.zeros(len(x))
    periodic = method == CUTOFF_PERIODIC
    for p, (i, j) in enumerate(zip(I.tolist(), J.tolist())):
        atoms = np.concatenate([donors[i], acceptors[j]])
        for s in slots:
            assert atoms[s] >= 0, 'the expression names a particle donor %d / acceptor %d does not have' % (i, j)
        x6 = x[np.where(atoms >= 0, atoms, atoms[0])]
        values = dict(g)
        values.update(zip((_rename(n) for n in donor_names), donor_params[i].tolist()))
        values.update(zip((_rename(n) for n in acceptor_names), acceptor_params[j].tolist()))
        E[p], grad = pair_energy(expression, x6, box, periodic, values, functions or {})
        for s in slots:
            F[atoms[s]] -= grad[s]
            count[atoms[s]] += 1
            peak[atoms[s]] = max(peak[atoms[s]], np.abs(grad[s]).max())
    return dict(E=E, F=F, i=I, j=J, r_all=r_all, count=count, peak=peak, inside=inside)


def force_bound(result):
    """[N][1]: n (2^-23 max|contribution| + 2^-31), n the atom's contributions (every contribution is rounded to f32 once, then added in
    fixed point)"""
    return (result['count'] * (2.0 ** -23 * result['peak'] + 2.0 ** -31))[:, None]


def energy_bound(result):
    return 1e-11 * np.abs(result['E']).sum()


def clear_of_cutoff(result, cutoff, margin=1e-6):
    """the membership condition of every test with a cutoff: no non-excluded pair's d1-a1 distance within ``margin`` nm of the cutoff"""
    return len(result['r_all']) == 0 or float(np.abs(result['r_all'] - cutoff).min()) > margin
