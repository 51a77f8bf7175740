"""GPU: tabulated functions in custom-force expressions (REMD_CX_TABLE1D / REMD_CX_LOOKUP1D of csrc/custom_machine.h, reached through
every kernel that runs cst_eval) against the exact-derivative f64 reference: tests/custom_dual_oracle.py with the functions of
tests/tabulated_oracle.py among its names.

Shapes and bounds are those of tests/test_custom_opcodes_gpu.py: bare systems, two replicas (x and 0.9 x + 0.05 in f32), 70 terms per
force, at most 200 atoms; |E_force - sum E_t| <= 1e-11 sum|E_t|, and per atom and component |dF| <= n (2^-23 max|contribution| +
2^-31), n the number of terms that touch the atom.  The tables (tests/tabulated_cases.py) are positive, so that no term cancels and
the rounding of a table's argument (one f64 ulp moves a term by less than 1e-13 of itself: tests/test_custom_tabulated_cpu.py) stays
inside the energy bound; no bound here is wider than those."""
import math

import numpy as np
import pytest

import centroid_expr_oracle as centroid
import custom_dual_oracle as dual
import custom_nonbonded_oracle as nb_oracle
import custom_opcode_cases as oc
import tabulated_cases as cases
import tabulated_oracle as tab
from openmmtools_amd import custom_expr as cx
from openmmtools_amd.system import (System, system_to_desc, CustomBondForce, CustomAngleForce, CustomTorsionForce, CustomExternalForce,
                                    CustomCompoundBondForce, CustomCentroidBondForce, CustomNonbondedForce)

pytestmark = pytest.mark.gpu

KB = 0.008314462618153242
BETA = 1.0 / (KB * 300.0)
KIND = {'ext': dual.KIND_EXTERNAL, 'bond': dual.KIND_BOND, 'angle': dual.KIND_ANGLE, 'torsion': dual.KIND_TORSION}
K70 = (5.0 + 0.1 * np.arange(oc.N_TERMS))[:, None]


def _f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def _row(name, place, energy, atoms, functions, P=0, names=('k',), params=K70, global_values=None):
    """functions: {name in the expression: table of tabulated_cases.TABLES, or 'lookup'}"""
    return dict(name=name, place=place, P=P, energy=energy, names=list(names), atoms=np.asarray(atoms), params=np.asarray(params),
                globals=dict(global_values or {}), functions=dict(functions))


def _device_function(table):
    return cases.lookup_function() if table == 'lookup' else cases.function(table)


def _oracle_functions(row):
    return {n: tab.Lookup(cases.LOOKUP) if t == 'lookup' else cases.spline(t) for n, t in row['functions'].items()}


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
    for name, table in row['functions'].items():
        f.addTabulatedFunction(name, _device_function(table))
    for a, p in zip(row['atoms'], row['params']):
        add(a, p)
    return f


def _reference(row, x, global_values=None, gradients=True):
    """(E [n], F [N][3], G [n][W][3]) of a row at positions x"""
    g = dict(row['globals'], **(global_values or {}))
    with tab.registered(**_oracle_functions(row)):
        if row['P']:
            return dual.evaluate_compound(row['P'], row['energy'], row['atoms'], row['names'], row['params'], g, x, None, False,
                                          per_term=True, gradients=gradients)
        return dual.evaluate(KIND[row['place']], row['energy'], row['atoms'], row['names'], row['params'], g, x, None, False,
                             per_term=True, gradients=gradients)


def _engine(factory, forces, xs, boxes=None, global_table=None, labels=None, masses=None):
    s = System()
    for i in range(xs.shape[1]):
        s.addParticle(12.0 if masses is None else masses[i])
    if boxes is not None:
        s.setDefaultPeriodicBoxVectors([boxes[0][0], 0, 0], [0, boxes[0][1], 0], [0, 0, boxes[0][2]])
    for f in forces:
        s.addForce(f)
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


def _check(factory, rows, xs=oc.XS):
    """one handle of ``rows`` against the reference: every energy, every component of every atom, at both replicas"""
    eng, desc = _engine(factory, [_force_of(r) for r in rows], xs)
    F_dev, E_dev = eng.get_forces(), eng.custom_energies()
    assert E_dev.shape == (len(xs), len(rows)) and np.isfinite(F_dev).all()
    for r, x in enumerate(xs):
        ref = [_reference(row, x) for row in rows]
        bound = force_bound(rows, [p[2] for p in ref], xs.shape[1])
        dF = np.abs(F_dev[r] - sum(p[1] for p in ref))
        for j, (row, (E, _, _)) in enumerate(zip(rows, ref)):
            touched = np.unique(row['atoms'])
            print('%-28s replica %d: |dE| / bound = %.3g, worst |dF| / bound = %.3g' % (
                row['name'], r, abs(E_dev[r, j] - E.sum()) / (1e-11 * np.abs(E).sum()), (dF[touched] / bound[touched]).max()))
        for j, (row, (E, _, _)) in enumerate(zip(rows, ref)):
            assert np.abs(E).sum() > 0.0
            assert abs(E_dev[r, j] - E.sum()) <= 1e-11 * np.abs(E).sum(), (row['name'], r)
        assert np.all(dF <= bound), (r, np.argwhere(dF > bound)[:5])
    return eng, desc


# ---- every kind -------------------------------------------------------------------------------------------------------------------------
def test_the_five_bonded_kinds_in_one_handle(hip_engine_factory):
    """bond and angle (natural tables), torsion (a periodic table over [-pi, pi] whose argument 2 theta + 1 leaves it on both sides),
    external (two tables, three partials), compound (one table called twice, of distance and of angle, through all three seed passes):
    five forces with blocks of their own in one handle"""
    rows = [_row('bond', 'bond', 'k*tab(r)', oc._chain_atoms(2, 100), dict(tab='r65')),
            _row('angle', 'angle', 'k*tab(theta)', oc._chain_atoms(3, 67), dict(tab='a65')),
            _row('torsion', 'torsion', 'k*per(2*theta + 1)', oc._chain_atoms(4, 50), dict(per='per65')),
            _row('external', 'ext', 'tab(x) * tab2(y) + z', oc.place_atoms('ext'), dict(tab='xy65', tab2='xy33')),
            _row('compound', 'compound', 'k*tab(distance(p1,p2)) * tab(angle(p1,p2,p3))', oc.place_atoms('c3'), dict(tab='r65'), P=3)]
    _, desc = _check(hip_engine_factory, rows)
    terms = desc['custom_terms']
    assert [len(terms[k]['consts']) for k in sorted(terms)] == [4 + 130, 4 + 130, 2 + 4 + 130, 4 + 130 + 4 + 66, 4 + 130]


def test_centroid_bonds(hip_engine_factory):
    """70 bonds between the centroids of 40 groups of three atoms (weights of their own in every other group)"""
    xs = oc.XS
    N = xs.shape[1]
    masses = 1.0 + (np.arange(N) % 5)
    f = CustomCentroidBondForce(2, 'k*tab(distance(g1,g2))')
    f.addPerBondParameter('k')
    f.addTabulatedFunction('tab', cases.function('r65'))
    groups = []
    for g in range(40):
        atoms = [3 * g, 3 * g + 1, 3 * g + 2]
        w = [1.0, 2.0, 0.5] if g % 2 else None
        f.addGroup(atoms, w)
        groups.append((atoms, centroid.normalised(w if w else masses[atoms])))
    bonds = np.array([[t % 40, (t * 7 + 3) % 40] for t in range(oc.N_TERMS)])
    assert np.all(bonds[:, 0] != bonds[:, 1])
    for t, b in enumerate(bonds):
        f.addBond([int(b[0]), int(b[1])], [float(K70[t, 0])])
    eng, _ = _engine(hip_engine_factory, [f], xs, masses=masses)
    F_dev, E_dev = eng.get_forces(), eng.custom_energies()
    for r, x in enumerate(xs):
        c = centroid.centroids(groups, x)
        with tab.registered(tab=cases.spline('r65')):
            E, Fc, G = dual.evaluate_compound(2, 'k*tab(distance(p1,p2))', bonds, ['k'], K70, {}, c, per_term=True)
        F, n, top = np.zeros_like(x), np.zeros(N), np.zeros((N, 3))
        for t, b in enumerate(bonds):
            for slot, g in enumerate(b):
                for a, w in zip(*groups[g]):
                    F[a] += w * G[t, slot]
                    n[a] += 1
                    top[a] = np.maximum(top[a], np.abs(w * G[t, slot]))
        bound = n[:, None] * (2.0 ** -23 * top + 2.0 ** -31)
        dF = np.abs(F_dev[r] - F)
        print('replica %d: |dE| / bound = %.3g, worst |dF| / bound = %.3g' % (
            r, abs(E_dev[r, 0] - E.sum()) / (1e-11 * np.abs(E).sum()), (dF[:120] / bound[:120]).max()))
        assert abs(E_dev[r, 0] - E.sum()) <= 1e-11 * np.abs(E).sum()
        assert np.all(dF[:120] <= bound[:120]) and not F_dev[r, 120:].any()


@pytest.mark.parametrize('method', [CustomNonbondedForce.NoCutoff, CustomNonbondedForce.CutoffPeriodic])
def test_nonbonded_pairs_of_65_particles(hip_engine_factory, method):
    """65 particles: three tiles, one of them diagonal with 63 padding lanes; a per-particle parameter scales the argument, exclusions;
    without a cutoff pairs beyond the table's max (2.2 nm) are exactly 0, with one every pair inside it is inside the table"""
    n = 65
    boxes = _f32([[3.0, 3.2, 3.4], [3.3, 3.1, 3.5]])
    rng = np.random.default_rng(65)
    xs = _f32([rng.uniform(0.0, 1.0, (n, 3)) * L for L in boxes])
    f = CustomNonbondedForce('q1*q2*tab(r*0.5*(s1+s2))')
    f.addPerParticleParameter('q'); f.addPerParticleParameter('s')
    f.addTabulatedFunction('tab', cases.function('e65'))                      # over [0.5, 2.0]: pairs below 0.5 nm are 0 as well
    params = [[1.0 + 0.1 * (i % 4), 0.9 + 0.05 * (i % 3)] for i in range(n)]
    for p in params:
        f.addParticle(p)
    for i in range(0, n - 1, 3):
        f.addExclusion(i, i + 1)
    f.addExclusion(0, 64)
    f.setNonbondedMethod(method)
    f.setCutoffDistance(1.45)
    eng, _ = _engine(hip_engine_factory, [f], xs, boxes if method else None)
    F_dev, E_dev = eng.get_forces(), eng.custom_energies()
    for r in range(2):
        with tab.registered(tab=cases.spline('e65')):
            ref = nb_oracle.evaluate(f.getEnergyFunction(), ['q', 's'], params, {}, xs[r], boxes[r] if method else None, method, 1.45, -1.0,
                                     [f.getExclusionParticles(k) for k in range(f.getNumExclusions())])
        if method:
            assert np.abs(ref['r_all'] - 1.45).min() > 1e-9
        assert np.sum(ref['E'] == 0.0) > 10 and np.sum(ref['E'] != 0.0) > 100            # pairs outside the table, and inside
        print('method %d replica %d: %d pairs, |dE| / bound = %.3g, worst |dF| / bound = %.3g' % (
            method, r, len(ref['E']), abs(E_dev[r, 0] - ref['E'].sum()) / nb_oracle.energy_bound(ref),
            (np.abs(F_dev[r] - ref['F']) / nb_oracle.force_bound(ref).clip(min=1e-300)).max()))
        assert abs(E_dev[r, 0] - ref['E'].sum()) <= nb_oracle.energy_bound(ref)
        assert np.all(np.abs(F_dev[r] - ref['F']) <= nb_oracle.force_bound(ref))


# ---- table sizes and edges ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [2, 3, 65])
def test_table_sizes_and_edges(hip_engine_factory, n):
    """x of hand-placed atoms (f32 numbers, the same at both replicas): exactly min, exactly max, an interior node, the middle of an
    interval; in a force of their own the atoms one f32 step outside each end, at +-1e30 and far outside: energy and forces exactly 0;
    a periodic table (3, 4, 65 points over [-1, 1]) under a*x with a per lane: below min and up to seven periods above max"""
    name, pname = {2: ('e2', 'p3'), 3: ('e3', 'p4'), 65: ('e65', 'p65')}[n]
    _, lo, hi, _ = cases.TABLES[name]
    xs = oc.XS.copy()
    T = oc.N_TERMS
    h = (hi - lo) / (n - 1)
    inside = lo + (hi - lo) * ((0.6180339887 * np.arange(T)) % 1.0)
    inside[:4] = [lo, hi, lo + h * ((n - 1) // 2), lo + 0.5 * h]
    outside = np.where(np.arange(T) % 2, hi + 0.01 * np.arange(T) + 0.3, lo - 0.01 * np.arange(T) - 0.2)
    outside[:6] = [np.nextafter(np.float32(lo), np.float32(-np.inf)), np.nextafter(np.float32(hi), np.float32(np.inf)), 1e30, -1e30, 0.0, 77.0]
    xs[:, :T, 0] = _f32(inside)
    xs[:, T:2 * T, 0] = _f32(outside)
    assert xs[0, 0, 0] == lo and xs[0, 1, 0] == hi and xs[0, T, 0] < lo < xs[0, T, 0] + 1e-6 and xs[0, T + 1, 0] > hi
    a = np.where(np.arange(T) % 2, -1.0, 1.0) * (0.7 + 0.2 * np.arange(T))             # |a x| up to 14.5 * 1.4: seven periods of 2 and more
    rows = [_row('inside', 'ext', 'k*tab(x) + y', np.arange(T)[:, None], {'tab': name}),
            _row('outside', 'ext', 'k*tab(x)', T + np.arange(T)[:, None], {'tab': name}),
            _row('periodic', 'ext', 'k*per(a*y)', 2 * T + np.arange(60)[:, None], {'per': pname}, names=('k', 'a'),
                 params=np.column_stack([K70, a])[:60])]
    eng, desc = _engine(hip_engine_factory, [_force_of(r) for r in rows], xs)
    F_dev, E_dev = eng.get_forces(), eng.custom_energies()
    args = np.abs(rows[2]['params'][:, 1] * xs[0, 2 * T:2 * T + 60, 1])
    assert args.max() > 8.0 and args.min() < 1.0
    for r, x in enumerate(xs):
        ref = [_reference(row, x) for row in rows]
        assert not ref[1][0].any() and not ref[1][1].any()
        assert E_dev[r, 1] == 0.0 and not F_dev[r, T:2 * T].any()                      # exactly zero outside, 1e30 included
        bound = force_bound(rows, [p[2] for p in ref], xs.shape[1])
        dF = np.abs(F_dev[r] - sum(p[1] for p in ref))
        for j in (0, 2):
            E = ref[j][0]
            print('n = %d %-8s replica %d: |dE| / bound = %.3g' % (n, rows[j]['name'], r, abs(E_dev[r, j] - E.sum()) / (1e-11 * np.abs(E).sum())))
            assert abs(E_dev[r, j] - E.sum()) <= 1e-11 * np.abs(E).sum()
        print('n = %d replica %d: worst |dF| / bound = %.3g' % (n, r, (dF / bound.clip(min=2.0 ** -31)).max()))
        assert np.all(dF <= bound.clip(min=0.0))
        assert np.isfinite(F_dev[r]).all()


# ---- offsets, select, parameters and globals ----------------------------------------------------------------------------------------------
def test_two_forces_with_tables_select_parameters_and_a_global(hip_engine_factory):
    """two forces whose blocks lie behind different numbers of scalars (const0 and the operand both matter); one function called
    twice; a table in the taken and one in the untaken branch of select (the untaken one out of its range: it must not leak a zero
    or a NaN); a per-term parameter and a global multiplying the argument"""
    c = (0.8 + 0.004 * np.arange(oc.N_TERMS))[:, None]
    rows = [_row('twice', 'bond', 'k*tab(g*r) + 3*tab(c*r/2) + 7', oc._chain_atoms(2, 100), dict(tab='r65'), names=('k', 'c'),
                 params=np.column_stack([K70, c]), global_values=dict(g=1.1)),
            _row('select', 'ext', 'k*select(step(x), tab(x), 2*tab2(100*x - 500)) + k*select(step(-x), tab2(y), tab(y))',
                 oc.place_atoms('ext'), dict(tab='xy65', tab2='xy33'))]
    eng, desc = _check(hip_engine_factory, rows)
    ops = desc['custom_terms']['000']['program']
    assert [int(a) for o, a in ops if o == cx.TABLE1D] == [3, 3]
    signs = np.sign(oc.XS[0, :oc.N_TERMS, 0])
    assert (signs > 0).sum() > 10 and (signs < 0).sum() > 10                          # both branches are taken somewhere


# ---- u_kl ---------------------------------------------------------------------------------------------------------------------------------
def test_ukl_rows_with_a_global_inside_the_argument_and_one_scaling_the_value(hip_engine_factory):
    table = np.array([[0.8, 2.0], [1.3, 1.0], [1.3, 1.0]])                         # (g1, g2); states 1 and 2 carry the same globals
    labels = np.array([2, 0])
    g = dict(g1=0.8, g2=2.0)
    rows = [_row('bond', 'bond', 'g2*k*tab(g1*r)', oc._chain_atoms(2, 100), dict(tab='r65'), global_values=g),
            _row('compound', 'compound', 'k*per(g1*dihedral(p1,p2,p3,p4)) + g2', oc._chain_atoms(4, 50), dict(per='per65'), P=4, global_values=g)]
    xs = oc.XS
    eng, _ = _engine(hip_engine_factory, [_force_of(r) for r in rows], xs, global_table=table, labels=labels)
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
    assert u[0, 1] - u[0, 2] == 0.0 and u[1, 1] != u[1, 0]
    # the per-force energies and the forces of the custom forces' group hold the tabulated forces
    E = eng.custom_energies()
    for r in range(2):
        own = dict(g1=table[labels[r], 0], g2=table[labels[r], 1])
        for j, rw in enumerate(rows):
            want = _reference(rw, xs[r], global_values=own, gradients=False)[0]
            assert abs(E[r, j] - want.sum()) <= 1e-11 * np.abs(want).sum()
    assert np.array_equal(eng.get_forces(groups=1), eng.get_forces()) and not eng.get_forces(groups=2).any()
    assert np.abs(eng.get_forces()).max() > 1.0


# ---- the lookup ---------------------------------------------------------------------------------------------------------------------------
def test_lookup_of_every_index_and_out_of_range(hip_engine_factory):
    """look(c + d*x*0): the argument is the per-term parameter c, at every index, at index +- 0.49 and at the halves (away from zero);
    a second force holds a term out of range: its energy is NaN, the first force's energy and every other atom's force are finite"""
    T = oc.N_TERMS
    n = len(cases.LOOKUP)
    c = np.array([(t % n) + (0.0, 0.49, -0.49)[(t // n) % 3] for t in range(T)])
    c[63:] = [0.5, 1.5, 2.5, 5.5, -0.49999, 6.4999, 3.0]
    rows = [_row('lookup', 'ext', 'look(c)*x + 0.5*look(c + 0*y)', np.arange(T)[:, None], dict(look='lookup'), names=('c',), params=c[:, None]),
            _row('out of range', 'ext', 'look(c)*x', T + np.arange(T)[:, None], dict(look='lookup'), names=('c',),
                 params=np.where(np.arange(T) == 5, 6.5, np.where(np.arange(T) == 6, -0.5, c))[:, None])]
    xs = oc.XS
    eng, _ = _engine(hip_engine_factory, [_force_of(r) for r in rows], xs)
    F_dev, E_dev = eng.get_forces(), eng.custom_energies()
    for r, x in enumerate(xs):
        E, F, G = _reference(rows[0], x)
        assert np.isfinite(E).all()
        assert abs(E_dev[r, 0] - E.sum()) <= 1e-11 * np.abs(E).sum()
        bound = force_bound(rows[:1], [G], xs.shape[1])
        assert np.all(np.abs(F_dev[r, :T] - F[:T]) <= bound[:T])
        E1, F1, G1 = _reference(rows[1], x)
        assert np.isnan(E1[[5, 6]]).all() and np.isfinite(np.delete(E1, [5, 6])).all()
        assert np.isnan(E_dev[r, 1]) and np.isfinite(E_dev[r, 0])
        others = np.delete(np.arange(T, 2 * T), [5, 6])
        keep = dict(rows[1], atoms=rows[1]['atoms'][np.delete(np.arange(T), [5, 6])], params=rows[1]['params'][np.delete(np.arange(T), [5, 6])])
        _, Fk, Gk = _reference(keep, x)
        assert np.isfinite(F_dev[r, others]).all()
        assert np.all(np.abs(F_dev[r, others] - Fk[others]) <= force_bound([keep], [Gk], xs.shape[1])[others])


# ---- the descriptor check -----------------------------------------------------------------------------------------------------------------
def test_corrupted_descriptors_are_refused_before_any_kernel(hip_engine_factory):
    s = System()
    for _ in range(4):
        s.addParticle(12.0)
    f = CustomBondForce('tab(r) + look(r)')
    f.addTabulatedFunction('tab', cases.function('e3'))
    f.addTabulatedFunction('look', cases.lookup_function())
    f.addBond(0, 1, [])
    s.addForce(f)
    desc = system_to_desc(s)
    term = desc['custom_terms']['000']
    assert term['program'].tolist() == [[cx.VAR, 0], [cx.TABLE1D, 0], [cx.VAR, 0], [cx.LOOKUP1D, 10], [cx.ADD, 0]] and len(term['consts']) == 18
    eng = hip_engine_factory()
    eng.set_system(desc)                                                           # as compiled: accepted

    def refused(sentence, consts=None, program=None):
        bad = dict(desc, custom_terms={'000': dict(term, consts=term['consts'].copy() if consts is None else consts,
                                                   program=term['program'].copy() if program is None else program)})
        with pytest.raises(Exception, match=sentence):
            hip_engine_factory().set_system(bad)

    def consts_with(i, v):
        c = term['consts'].copy(); c[i] = v
        return c

    def program_with(pc, arg):
        p = term['program'].copy(); p[pc, 1] = arg
        return p
    refused('a table offset out of range', program=program_with(1, 18))
    refused('a table offset out of range', program=program_with(3, -1))
    refused('a table whose point count is not an integer 2 ... REMD_CUSTOM_MAX_TABLE_POINTS', consts=consts_with(0, 1.0))
    refused('a table whose point count is not an integer 2 ... REMD_CUSTOM_MAX_TABLE_POINTS', consts=consts_with(0, 2.5))
    refused('a table whose point count is not an integer 2 ... REMD_CUSTOM_MAX_TABLE_POINTS', consts=consts_with(0, 8193.0))
    refused('a table whose point count is not an integer 2 ... REMD_CUSTOM_MAX_TABLE_POINTS', consts=consts_with(0, math.nan))
    refused('a lookup table whose value count is not an integer 1 ... REMD_CUSTOM_MAX_TABLE_POINTS', consts=consts_with(10, 0.0))
    refused('a table whose bounds are not finite with min < max', consts=consts_with(1, 2.0))
    refused('a table whose bounds are not finite with min < max', consts=consts_with(2, math.inf))
    refused('a table whose periodic flag is neither 0 nor 1', consts=consts_with(3, 0.5))
    refused('a table that runs past n_consts', consts=consts_with(0, 8.0))
    refused('a table that runs past n_consts', consts=consts_with(10, 8.0))
    refused('a table that runs past n_consts', program=program_with(1, 10))        # (an offset inside, a block that is not: the lookup's n = 7 read as a spline's)
