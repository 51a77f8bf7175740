"""GPU: every opcode of the custom-force stack machine (csrc/custom_machine.h: cst_eval<false> through custom_terms.hip, cst_eval<true>
through custom_compound.hip) against the exact-derivative f64 reference tests/custom_dual_oracle.py, over the case table of
tests/custom_opcode_cases.py.

Systems are bare: no other force, nothing differenced.  Two replicas (x and 0.9 x + 0.05, rounded to f32), 70 terms per force.
Bounds, from the formats: an energy is f64 end to end, |E_force - sum E_t| <= 1e-11 sum|E_t|; a force contribution is rounded to f32
once (2^-24 relative) and truncated into a 2^-32 fixed-point accumulator, so per atom and component
|dF| <= n (2^-23 max|contribution| + 2^-31), n the number of terms that touch the atom (1 for the external and one-particle rows; in
the three-particle rows 70 x 3 > 200 atoms, so twelve atoms carry two terms)."""
import numpy as np
import pytest

import custom_dual_oracle as dual
import custom_opcode_cases as cases
from openmmtools_amd.system import (System, system_to_desc, CustomBondForce, CustomAngleForce, CustomTorsionForce, CustomExternalForce,
                                    CustomCompoundBondForce)

pytestmark = pytest.mark.gpu

KB = 0.008314462618153242
BETA = 1.0 / (KB * 300.0)
KIND = {'ext': dual.KIND_EXTERNAL, 'bond': dual.KIND_BOND, 'angle': dual.KIND_ANGLE, 'torsion': dual.KIND_TORSION}


def _force_of(row):
    place = row['place']
    if row['P']:
        f = CustomCompoundBondForce(row['P'], row['energy'])
        add_name, add = f.addPerBondParameter, lambda a, p: f.addBond([int(i) for i in a], list(p))
    elif place == 'ext':
        f = CustomExternalForce(row['energy'])
        add_name, add = f.addPerParticleParameter, lambda a, p: f.addParticle(int(a[0]), list(p))
    elif place == 'bond':
        f = CustomBondForce(row['energy'])
        add_name, add = f.addPerBondParameter, lambda a, p: f.addBond(int(a[0]), int(a[1]), list(p))
    elif place == 'angle':
        f = CustomAngleForce(row['energy'])
        add_name, add = f.addPerAngleParameter, lambda a, p: f.addAngle(int(a[0]), int(a[1]), int(a[2]), list(p))
    else:
        f = CustomTorsionForce(row['energy'])
        add_name, add = f.addPerTorsionParameter, lambda a, p: f.addTorsion(int(a[0]), int(a[1]), int(a[2]), int(a[3]), list(p))
    for name, value in row['globals'].items():
        f.addGlobalParameter(name, value)
    for name in row['names']:
        add_name(name)
    for a, p in zip(row['atoms'], row['params']):
        add(a, p)
    f.setUsesPeriodicBoundaryConditions(bool(row['periodic']))
    return f


def _reference(row, x, box=None, global_values=None, gradients=True):
    """(E [n], F [N][3], G [n][W][3]) of a row at positions x"""
    g = dict(row['globals'], **(global_values or {}))
    if row['P']:
        return dual.evaluate_compound(row['P'], row['energy'], row['atoms'], row['names'], row['params'], g, x, box, row['periodic'],
                                      per_term=True, gradients=gradients)
    return dual.evaluate(KIND[row['place']], row['energy'], row['atoms'], row['names'], row['params'], g, x, box, row['periodic'],
                         per_term=True, gradients=gradients)


def _handle(factory, rows, xs, boxes=None, global_table=None, labels=None):
    s = System()
    for _ in range(xs.shape[1]):
        s.addParticle(12.0)
    for row in rows:
        s.addForce(_force_of(row))
    desc = system_to_desc(s, box=None if boxes is None else boxes[0])
    eng = factory()
    eng.set_system(desc)
    K = 1 if global_table is None else len(global_table)
    eng.set_states(np.full(K, BETA))
    eng.set_custom_globals(np.tile(desc['custom_terms']['000']['global_defaults'], (K, 1)) if global_table is None else global_table)
    R = len(xs)
    eng.set_replicas(R, 0, xs, None, np.zeros((R, 3)) if boxes is None else boxes, np.zeros(R, dtype=np.int64) if labels is None else labels)
    return eng, desc


def force_bound(rows, G, n_atoms):
    """[N][3]: n (2^-23 max|contribution| + 2^-31) over the terms of every row that touch the atom"""
    n, top = np.zeros(n_atoms), np.zeros((n_atoms, 3))
    for row, g in zip(rows, G):
        for t, idx in enumerate(row['atoms']):
            for a, i in enumerate(idx):
                n[i] += 1
                top[i] = np.maximum(top[i], np.abs(g[t, a]))
    return n[:, None] * (2.0 ** -23 * top + 2.0 ** -31)


def _check(factory, rows, xs=cases.XS):
    """one handle of ``rows`` against the reference: every energy, every component of every atom, at both replicas"""
    periodic = any(r['periodic'] for r in rows)
    boxes = cases.BOXES if periodic else None
    eng, _ = _handle(factory, rows, xs, boxes)
    F_dev, E_dev = eng.get_forces(), eng.custom_energies()
    assert E_dev.shape == (len(xs), len(rows)) and np.isfinite(F_dev).all()
    worst = {row['name']: [0.0, 0.0] for row in rows}
    for r, x in enumerate(xs):
        ref = [_reference(row, x, None if boxes is None else boxes[r]) for row in rows]
        bound = force_bound(rows, [p[2] for p in ref], xs.shape[1])
        dF = np.abs(F_dev[r] - sum(p[1] for p in ref))
        for j, (row, (E, _, _)) in enumerate(zip(rows, ref)):
            tol_E = 1e-11 * np.abs(E).sum()
            touched = np.unique(row['atoms'])
            w = worst[row['name']]
            w[0] = max(w[0], abs(E_dev[r, j] - E.sum()) / tol_E)
            w[1] = max(w[1], (dF[touched] / bound[touched]).max())
        for row in rows:
            print('%-32s replica %d: |dE| / bound = %.3g, worst |dF| / bound = %.3g' % (row['name'], r, *worst[row['name']]))
        for j, (row, (E, _, _)) in enumerate(zip(rows, ref)):
            assert abs(E_dev[r, j] - E.sum()) <= 1e-11 * np.abs(E).sum(), (row['name'], r)
        assert np.all(dF <= bound), (r, np.argwhere(dF > bound)[:5])


def _handles():
    """(id, rows): ext and c1 rows in pairs on atoms of their own, every other row a handle of its own"""
    out = []
    for place in ('ext', 'c1'):
        rows = cases.rows_of(place)
        pairs, rest = rows[:-1], rows[-1:]                      # (the last row, (x+1)^(y*z), picks its own atoms)
        out += [pairs[i:i + 2] for i in range(0, len(pairs), 2)] + [rest]
    out += [[row] for row in cases.rows_of('c3') + cases.particle_rows()]
    return [pytest.param(h, id=' + '.join(r['name'] for r in h)) for h in out]


@pytest.mark.parametrize('rows', _handles())
def test_rows_against_the_dual_reference(hip_engine_factory, rows):
    assert len(rows) <= 8 and all(len(r['atoms']) == cases.N_TERMS for r in rows)
    _check(hip_engine_factory, rows)


def test_eight_forces_in_one_handle(hip_engine_factory):
    """MAX_FORCES forces of both machines in one launch: the programs change at wavefront boundaries; atoms carry up to eight terms"""
    ext, c3 = cases.rows_of('ext'), cases.rows_of('c3')
    by = {r['name']: r for r in ext + c3}
    rows = [by[n] for n in ('ext/log', 'c3/tan', 'ext/erfc', 'c3/atan2', 'ext/u^-6', 'c3/min', 'ext/abs', 'c3/u^p, u < 0')]
    _check(hip_engine_factory, rows)


# ---- u_kl ---------------------------------------------------------------------------------------------------------------------------------
def test_ukl_with_globals_inside_the_new_opcodes(hip_engine_factory):
    table = np.array([[0.8, 2.0], [1.3, 1.0], [1.3, 1.0]])                         # (g1, g2); states 1 and 2 carry the same globals
    labels = np.array([2, 0])
    g = dict(g1=0.8, g2=2.0)
    k = (5.0 + 0.1 * np.arange(cases.N_TERMS))[:, None]

    def row(name, place, P, energy, atoms):
        return dict(name=name, place=place, P=P, energy=energy, names=['k'], atoms=atoms, params=k, globals=dict(g), periodic=False)
    rows = [row('erfc(g1*r)', 'bond', 0, 'k*erfc(g1*r)', cases._chain_atoms(2, 100)),
            row('min(g1, r)^g2', 'bond', 0, 'k*min(g1, r)^g2', cases._chain_atoms(2, 100))]
    for place in ('ext', 'c3'):
        u = cases._u_row('tanh(g1*u)', place, 'k*tanh(g1*u)', -2.0, 2.0, global_values=g)
        s = cases._u_row('select(g2-1)', place, 'k*select(g2-1, tanh(g1*u), erfc(g1*u))', -2.0, 2.0, global_values=g, block=1)
        rows += [u, s]
    xs = cases.XS
    eng, _ = _handle(hip_engine_factory, rows, xs, global_table=table, labels=labels)
    u = eng.compute_energies()
    e = np.array([[[_reference(rw, x, global_values=dict(g1=gl[0], g2=gl[1]), gradients=False)[0] for rw in rows] for gl in table] for x in xs])
    e = e.reshape(len(xs), len(table), -1)                                         # [r][l][every term of every force]
    for r in range(len(xs)):
        own = labels[r]
        for l in range(len(table)):
            got, want = u[r, l] - u[r, own], BETA * (e[r, l].sum() - e[r, own].sum())
            tol = 1e-11 * (np.abs(e[r, l]).sum() + np.abs(e[r, own]).sum())
            print('replica %d state %d: |got - want| / bound = %.3g' % (r, l, abs(got - want) / tol))
            assert abs(got - want) <= tol
    assert u[0, 1] - u[0, 2] == 0.0                                                # a state with the own state's globals: exactly 0
    assert u[1, 1] != u[1, 0]


# ---- guards and exact ties ------------------------------------------------------------------------------------------------------------------
def test_guards_and_exact_ties(hip_engine_factory):
    """degenerate geometries (coincident atoms, collinear angle and torsion, directly and through distance / angle / dihedral) and
    exact arguments in lane 0 .. 2 of forces whose other lanes are ordinary: the degenerate lanes' energies are the reference's, their
    forces finite and summing to zero per term, a tie's force one of its two branches', and every other lane as in the rows above"""
    xs = cases.XS.copy()
    N = xs.shape[1]
    # atoms 190 .. 199 are laid out by hand, at both replicas (f32 numbers; exact collinearity)
    xs[:, 190] = xs[:, 191] = [0.25, 0.5, -0.75]                                    # coincident
    xs[:, 192], xs[:, 193], xs[:, 194] = [0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [1.0, 0.0, 0.0]       # collinear along x
    xs[:, 195] = [1.0, 0.5, 0.25]
    k = (5.0 + 0.1 * np.arange(cases.N_TERMS))[:, None]

    def row(name, place, P, energy, atoms, names='k', params=k):
        return dict(name=name, place=place, P=P, energy=energy, names=list(names), atoms=atoms, params=params, globals={}, periodic=False)

    def with_lanes(width, stride, lanes):
        a = (np.arange(cases.N_TERMS)[:, None] + stride * np.arange(width)[None, :]) % 180        # (ordinary lanes stay off atoms 190 ..)
        for t, idx in enumerate(lanes):
            a[t] = idx
        return a
    bonds, angles = with_lanes(2, 90, [[190, 191]]), with_lanes(3, 60, [[192, 193, 194], [193, 192, 194]])       # pi; 0
    torsions = with_lanes(4, 45, [[192, 193, 194, 195]])
    geometry = [row('bond r = 0', 'bond', 0, 'k*(r-0.3)^2 + sqrt(r)', bonds), row('angle 0, pi', 'angle', 0, 'k*(theta-1)^2', angles),
                row('torsion collinear', 'torsion', 0, 'k*cos(theta) + theta', torsions),
                row('distance = 0', 'compound', 2, 'k*(distance(p1,p2)-0.3)^2', bonds), row('angle() 0, pi', 'compound', 3, 'k*(angle(p1,p2,p3)-1)^2', angles),
                row('dihedral() collinear', 'compound', 4, 'k*cos(dihedral(p1,p2,p3,p4)) + dihedral(p1,p2,p3,p4)', torsions)]
    degenerate = {0: [0], 1: [0, 1], 2: [0], 3: [0], 4: [0, 1], 5: [0]}
    # exact arguments: e = x - x0 is exactly 0 in lanes 0 .. 2 (x0 the lane's own x at that replica is not possible for both replicas,
    # so the three atoms get the same position at both); w = x*y exactly (a product of two f32 numbers is an f64 number)
    xs[1, :3] = xs[0, :3]
    x0 = xs[0, :cases.N_TERMS, 0].copy(); x0[3:] -= 0.2 + 0.01 * np.arange(cases.N_TERMS - 3)
    w = xs[0, :cases.N_TERMS, 0] * xs[0, :cases.N_TERMS, 1]; w[3:] += 0.1
    q = np.where(np.arange(cases.N_TERMS) % 3 == 0, 2.0, np.where(np.arange(cases.N_TERMS) % 3 == 1, -3.0, -0.5))
    tie = ('k*(sqrt(e) + y*abs(e) + z*step(e) + y*step(-1*e) + z*delta(e) + y*floor(q) + z*ceil(q) + z*min(x*y, w) + y*max(x*y, w) '
           '+ z*e^0 + y*e^2); e = x - x0')
    exact = row('exact arguments', 'ext', 0, tie, np.arange(cases.N_TERMS)[:, None], ('k', 'x0', 'w', 'q'), np.column_stack([k, x0, w, q]))
    rows = geometry + [exact]
    eng, _ = _handle(hip_engine_factory, rows, xs)
    F_dev, E_dev = eng.get_forces(), eng.custom_energies()
    assert np.isfinite(F_dev).all() and np.isfinite(E_dev).all()
    quantum = 2.0 ** -32
    for r, x in enumerate(xs):
        E = [_reference(rw, x, gradients=False)[0] for rw in rows]
        for j, rw in enumerate(rows):
            print('%-24s replica %d: |dE| / bound = %.3g' % (rw['name'], r, abs(E_dev[r, j] - E[j].sum()) / (1e-11 * np.abs(E[j]).sum())))
            assert abs(E_dev[r, j] - E[j].sum()) <= 1e-11 * np.abs(E[j]).sum(), (rw['name'], r)
        # the ordinary lanes: the reference with the degenerate lanes taken out (their atoms carry nothing else)
        ordinary, alternatives = [], []
        for j, rw in enumerate(geometry):
            keep = np.array([t not in degenerate[j] for t in range(cases.N_TERMS)])
            ordinary.append(dict(rw, atoms=rw['atoms'][keep], params=rw['params'][keep]))
        # the exact lanes of the external force: min / max tie -> either operand; abs(0) -> either sign
        for m in ('(x*y)', '(w)'):
            for n in ('(x*y)', '(w)'):
                for a in ('(e)', '(-e)'):
                    alternatives.append(dict(exact, energy=tie.replace('min(x*y, w)', m).replace('max(x*y, w)', n).replace('abs(e)', a)))
        ref = [_reference(rw, x) for rw in ordinary]
        ref_exact = [_reference(rw, x) for rw in alternatives]
        ref_own = _reference(exact, x)                                             # (the reference's own picks: right in every ordinary lane)
        bound = force_bound(ordinary + [exact], [p[2] for p in ref] + [ref_own[2]], N)
        F_ordinary = sum(p[1] for p in ref)
        dF = np.abs(F_dev[r] - F_ordinary - ref_own[1])
        far = np.ones(N, dtype=bool); far[:3] = False; far[190:196] = False
        print('replica %d: ordinary lanes, worst |dF| / bound = %.3g' % (r, (dF[far] / np.maximum(bound[far], 2.0 ** -31)).max()))
        assert np.all(dF[far] <= bound[far])                                       # a degenerate lane poisons no neighbour
        for i in range(3):                                                         # a tie: one of its branches' forces
            best = min(np.max(np.abs(F_dev[r, i] - F_ordinary[i] - alt[1][i]) / bound[i]) for alt in ref_exact)
            print('replica %d: tie lane %d, nearest branch |dF| / bound = %.3g' % (r, i, best))
            assert best <= 1.0
        # the degenerate terms act on atoms 190 .. 195 alone: each term's forces sum to zero, so does their total per component
        # (each of the 24 contributions rounded to f32 once and truncated to the quantum)
        total = np.abs(F_dev[r, 190:196].sum(axis=0))
        assert np.all(total <= 24 * (2.0 ** -23 * np.abs(F_dev[r, 190:196]).max() + 2.0 * quantum)), total
        assert not F_dev[r, 190:192].any()                                         # r = 0: the unit vector is taken as zero
