"""GPU: tabulated functions of two and three arguments in custom-force expressions (REMD_CX_TABLE2D / LOOKUP2D / LOOKUP3D of
csrc/custom_machine.h, reached through every kernel that runs cst_eval) against the exact-derivative f64 reference:
tests/custom_dual_oracle.py with the functions of tests/tabulated2d_oracle.py among its names.

Bounds: those tests/test_custom_tabulated_gpu.py holds the functions of one argument to (its helpers are imported):
|E_force - sum E_t| <= 1e-11 sum|E_t|; per atom and component |dF| <= n (2^-23 max|contribution| + 2^-31), n the number of terms that
touch the atom; u_kl rows at rtol 1e-5, atol 1e-5 max|want|.  The tables (tests/tabulated2d_cases.py) are positive, so that no term
cancels.  Bare systems of the custom forces alone unless a test says otherwise, two replicas."""
import copy
import math

import numpy as np
import pytest

import custom_dual_oracle as dual
import custom_nonbonded_oracle as nb_oracle
import custom_opcode_cases as oc
import tabulated2d_cases as cases
import tabulated2d_oracle as tab2
import tabulated_oracle as tab
from test_custom_tabulated_gpu import BETA, K70, _engine, _f32, force_bound
from openmmtools_amd import custom_expr as cx, states, testsystems
from openmmtools_amd.system import (System, system_to_desc, CustomBondForce, CustomTorsionForce, CustomExternalForce, CustomCompoundBondForce,
                                    CustomCentroidBondForce, CustomNonbondedForce, Discrete2DFunction, Discrete3DFunction)

pytestmark = pytest.mark.gpu

KIND = {'ext': dual.KIND_EXTERNAL, 'bond': dual.KIND_BOND, 'torsion': dual.KIND_TORSION}
PHI_PSI = [4, 6, 8, 14, 16]             # C - N - CA - C - N of alanine dipeptide: phi = dihedral(p1 ... p4), psi = dihedral(p2 ... p5)
CMAP = 'lam*cmap(dihedral(p1,p2,p3,p4), dihedral(p2,p3,p4,p5))'


def _row(name, place, energy, atoms, functions, names=('k',), params=K70, P=0, global_values=None):
    """functions: {name in the expression: (the package's function, the reference's)}"""
    return dict(name=name, place=place, P=P, energy=energy, names=list(names), atoms=np.asarray(atoms), params=np.asarray(params, dtype=np.float64),
                globals=dict(global_values or {}), functions=dict(functions))


def _table(name):
    return cases.function(name), cases.table(name)


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
    else:
        f = CustomTorsionForce(row['energy'])
        add_name, add = f.addPerTorsionParameter, lambda a, p: f.addTorsion(int(a[0]), int(a[1]), int(a[2]), int(a[3]), list(p))
    for name, value in row['globals'].items():
        f.addGlobalParameter(name, value)
    for name in row['names']:
        add_name(name)
    for name, (function, _) in row['functions'].items():
        f.addTabulatedFunction(name, function)
    for a, p in zip(row['atoms'], row['params']):
        add(a, p)
    return f


def _reference(row, x, global_values=None, gradients=True):
    """(E [n], F [N][3], G [n][W][3]) of a row at positions x"""
    g = dict(row['globals'], **(global_values or {}))
    params = row['params'] if row['params'].shape[1] else np.zeros((len(row['atoms']), 1))       # (no parameter: a column nothing names)
    with tab.registered(**{n: ref for n, (_, ref) in row['functions'].items()}):
        if row['P']:
            return dual.evaluate_compound(row['P'], row['energy'], row['atoms'], row['names'], params, g, x, None, False,
                                          per_term=True, gradients=gradients)
        return dual.evaluate(KIND[row['place']], row['energy'], row['atoms'], row['names'], params, g, x, None, False,
                             per_term=True, gradients=gradients)


def _compare(rows, xs, F_dev, E_dev, columns=None):
    """every energy, every component of every atom, at every replica, against the reference"""
    out = []
    for r, x in enumerate(xs):
        ref = [_reference(row, x) for row in rows]
        out.append(ref)
        bound = force_bound(rows, [p[2] for p in ref], xs.shape[1])
        dF = np.abs(F_dev[r] - sum(p[1] for p in ref))
        for j, (row, (E, _, _)) in enumerate(zip(rows, ref)):
            col = j if columns is None else columns[j]
            touched = np.unique(row['atoms'])
            print('%-12s replica %d: |dE| / bound = %.3g, worst |dF| / bound = %.3g, %d of %d terms zero' % (
                row['name'], r, abs(E_dev[r, col] - E.sum()) / (1e-11 * np.abs(E).sum()), (dF[touched] / bound[touched].clip(min=2.0 ** -31)).max(),
                (E == 0.0).sum(), len(E)))
        for j, (row, (E, _, _)) in enumerate(zip(rows, ref)):
            col = j if columns is None else columns[j]
            assert np.abs(E).sum() > 0.0 and np.isfinite(E).all()
            assert abs(E_dev[r, col] - E.sum()) <= 1e-11 * np.abs(E).sum(), (row['name'], r)
        assert np.all(dF <= bound), (r, np.argwhere(dF > bound)[:5])
    return out


def _check(factory, rows, xs=oc.XS):
    eng, desc = _engine(factory, [_force_of(r) for r in rows], xs)
    F_dev, E_dev = eng.get_forces(), eng.custom_energies()
    assert E_dev.shape == (len(xs), len(rows)) and np.isfinite(F_dev).all()
    _compare(rows, xs, F_dev, E_dev)
    return eng, desc


# ---- 1. the instantiation of the one-variable kinds (GEOM = false) ------------------------------------------------------------------------
def test_bond_external_and_torsion_in_one_handle(hip_engine_factory):
    """70 terms per force (a second wavefront with padding lanes).  bond: tab(r, k), the per-bond k spread over and beyond [ymin, ymax]
    of the 5 x 7 table (a term outside either range is exactly 0 on both sides); external: the 3 x 2 table of the two varying arguments x
    and y (three partials live); torsion: the periodic 4 x 6 table over [-pi, pi] x [-1, 1.5] of theta and a per-torsion phase that
    leaves its range on both sides (both arguments wrap)"""
    T = oc.N_TERMS
    k = -1.5 + 4.0 * ((0.6180339887 * np.arange(T)) % 1.0)                     # [-1.5, 2.5] around [ymin, ymax] = [-1, 2]
    k[:2] = [-1.0, 2.0]
    phase = -4.0 + 9.0 * ((0.6180339887 * np.arange(T)) % 1.0)
    rows = [_row('bond', 'bond', 'c*tab(r, k)', oc._chain_atoms(2, 100), dict(tab=_table('b5x7')), names=('c', 'k'), params=np.column_stack([K70, k])),
            _row('external', 'ext', 'tab(x, y) + z^2', oc.place_atoms('ext'), dict(tab=_table('t3x2')), names=(), params=np.zeros((T, 0))),
            _row('torsion', 'torsion', 'k*tab(theta, phase)', oc._chain_atoms(4, 50), dict(tab=_table('p4x6')), names=('k', 'phase'),
                 params=np.column_stack([K70, phase]))]
    _, desc = _check(hip_engine_factory, rows)
    terms = desc['custom_terms']
    assert [len(terms[key]['consts']) for key in sorted(terms)] == [8 + 4 * 35, 8 + 4 * 6, 8 + 4 * 24]
    E = _reference(rows[0], oc.XS[0], gradients=False)[0]
    assert 5 < (E == 0.0).sum() < 60                                            # bonds outside the table, and inside


# ---- 2. the instantiation of the particle kinds (GEOM = true): a CMAP-style map of phi and psi --------------------------------------------
class LamState(states.GlobalParameterState):
    lam = states.GlobalParameterState.GlobalParameter('lam', standard_value=1.0)


def _cmap_force(lam=1.0):
    f = CustomCompoundBondForce(5, CMAP)
    f.addGlobalParameter('lam', lam)
    f.addTabulatedFunction('cmap', cases.function('cmap'))
    f.addBond(PHI_PSI, [])
    return f


def _cmap_row(lam=1.0):
    return _row('cmap', 'compound', CMAP, [PHI_PSI], dict(cmap=_table('cmap')), names=(), params=np.zeros((1, 0)), P=5, global_values=dict(lam=lam))


def _alanine_positions():
    """the test system's positions and two perturbed copies, as the f32 numbers the engine holds"""
    al = testsystems.AlanineDipeptideVacuum()
    x = np.asarray(al.positions, dtype=np.float64)
    rng = np.random.default_rng(24)
    return al, _f32([x, x + rng.normal(0.0, 0.01, x.shape), x + rng.normal(0.0, 0.02, x.shape)])


def test_cmap_of_phi_and_psi_against_the_reference(hip_engine_factory):
    """one five-particle compound bond on the phi / psi atoms of alanine dipeptide with the periodic 24 x 24 map over [-pi, pi]^2 (all
    five seed passes); the same map through a centroid-bond force of single-atom groups"""
    al, xs = _alanine_positions()
    row = _cmap_row(lam=0.75)
    eng, _ = _engine(hip_engine_factory, [_force_of(row)], xs)
    F, E = eng.get_forces(), eng.custom_energies()
    ref = _compare([row], xs, F, E)
    assert all(np.abs(F[:, a]).max() > 0.1 for a in PHI_PSI) and not np.delete(F, PHI_PSI, axis=1).any()
    c = CustomCentroidBondForce(5, 'lam*cmap(dihedral(g1,g2,g3,g4), dihedral(g2,g3,g4,g5))')
    c.addGlobalParameter('lam', 0.75)
    c.addTabulatedFunction('cmap', cases.function('cmap'))
    for a in PHI_PSI:
        c.addGroup([a])
    c.addBond([0, 1, 2, 3, 4], [])
    eng2, _ = _engine(hip_engine_factory, [c], xs)
    E2, F2 = eng2.custom_energies(), eng2.get_forces()
    for r in range(len(xs)):
        want = ref[r][0][0]
        assert abs(E2[r, 0] - want.sum()) <= 1e-11 * np.abs(want).sum()
    _compare([row], xs, F2, E2)                                                 # (a group of one atom with weight 1: the same forces)


def test_cmap_ukl_rows_over_a_global_parameter_state(hip_engine_factory):
    """three states of a GlobalParameterState over lam; rows relative to the own state against beta (lam_l - lam_own) cmap(phi, psi); the
    column of a state that repeats the replica's own lam is the own column to the bit"""
    al, xs = _alanine_positions()
    system = copy.deepcopy(al.system)
    system.addForce(_cmap_force())
    ts = states.ThermodynamicState(system, 300.0)
    sts = states.create_thermodynamic_state_protocol(ts, {'lam': [1.0, 0.5, 0.0]}, composable_states=[LamState(lam=1.0)])
    table = cx.custom_globals(system, ['lam'], sts)
    assert table.tolist() == [[1.0], [0.5], [0.0]]
    labels = np.array([2, 0, 1])
    eng, _ = _engine(hip_engine_factory, [_cmap_force()], xs, global_table=table, labels=labels)
    u = eng.compute_energies()
    row = _cmap_row()
    E = np.array([_reference(row, x, gradients=False)[0].sum() for x in xs])
    want = BETA * table[None, :, 0] * E[:, None]
    own = np.arange(3), labels
    got, want = u - u[own][:, None], want - want[own][:, None]
    print('u_kl rows: max |got - want| / max|want| = %.3g' % (np.abs(got - want).max() / np.abs(want).max()))
    assert np.allclose(got, want, rtol=1e-5, atol=1e-5 * np.abs(want).max()) and np.abs(want).max() > 0.1
    eng.set_custom_globals(np.array([[1.0], [0.5], [0.5]]))
    eng.set_labels(np.array([1, 2, 0]))
    u2 = eng.compute_energies()
    assert u2[0, 2] == u2[0, 1] and u2[1, 1] == u2[1, 2] and u2[0, 0] != u2[0, 1]


# ---- 3. type tables in a pair force ---------------------------------------------------------------------------------------------------------
LJ_TABLE = '4*eps(t1,t2)*((sig(t1,t2)/r)^12-(sig(t1,t2)/r)^6)'
LJ_CLOSED = '4*e1*e2*((s1*s2/r)^12-(s1*s2/r)^6)'
E_TYPE, S_TYPE = np.array([0.8, 1.5]), np.array([0.55, 0.62])


def _seven_particles():
    box = _f32([[3.0, 3.2, 3.4], [3.1, 3.0, 3.3]])
    base = np.array([[0.2, 0.3, 0.4], [0.7, 0.35, 0.5], [0.3, 0.9, 0.45], [0.85, 0.95, 0.6], [0.5, 0.6, 1.0], [2.9, 0.4, 0.5], [0.4, 2.8, 0.9]])
    xs = _f32([base, base * 1.03 + 0.02])
    types = [0, 1, 0, 1, 1, 0, 1]
    return box, xs, types


def _pair_force(energy, types, functions=(), closed=False):
    f = CustomNonbondedForce(energy)
    if closed:
        f.addPerParticleParameter('e'); f.addPerParticleParameter('s')
    else:
        f.addPerParticleParameter('t')
    for name, fn in functions:
        f.addTabulatedFunction(name, fn)
    for t in types:
        f.addParticle([E_TYPE[t], S_TYPE[t]] if closed else [float(t)])
    f.addExclusion(0, 1)
    f.setNonbondedMethod(CustomNonbondedForce.CutoffPeriodic)
    f.setCutoffDistance(1.2)
    f.setUseLongRangeCorrection(False)
    return f


def test_nonbonded_type_tables(hip_engine_factory):
    """seven particles of two types (one tile, 57 padding lanes), CutoffPeriodic without the long-range correction: eps(t1, t2) and
    sig(t1, t2) from 2 x 2 Discrete2DFunctions against the reference, and against the same products as per-particle parameters in closed
    form; w(t1, t2, step(r - 0.5)) of a 2 x 2 x 2 Discrete3DFunction pops three arguments"""
    boxes, xs, types = _seven_particles()
    eps, sig = np.outer(E_TYPE, E_TYPE).reshape(-1), np.outer(S_TYPE, S_TYPE).reshape(-1)
    f = _pair_force(LJ_TABLE, types, [('eps', Discrete2DFunction(2, 2, eps)), ('sig', Discrete2DFunction(2, 2, sig))])
    eng, desc = _engine(hip_engine_factory, [f], xs, boxes)
    assert np.isin(desc['custom_terms']['000']['program'][:, 0], [cx.LOOKUP2D]).sum() == 3
    F, E = eng.get_forces(), eng.custom_energies()
    closed, _ = _engine(hip_engine_factory, [_pair_force(LJ_CLOSED, types, closed=True)], xs, boxes)
    Fc, Ec = closed.get_forces(), closed.custom_energies()
    w = np.array([1.0, 2.0, 2.0, 3.5, 0.5, 0.25, 0.25, 0.75])
    three, _ = _engine(hip_engine_factory, [_pair_force('w(t1, t2, step(r - 0.5))*r^2', types, [('w', Discrete3DFunction(2, 2, 2, w))])], xs, boxes)
    F3, E3 = three.get_forces(), three.custom_energies()
    exclusions = [(0, 1)]
    for r in range(2):
        with tab.registered(eps=tab2.Lookup2D(2, 2, eps), sig=tab2.Lookup2D(2, 2, sig), w=tab2.Lookup3D(2, 2, 2, w)):
            ref = nb_oracle.evaluate(LJ_TABLE, ['t'], [[float(t)] for t in types], {}, xs[r], boxes[r], 2, 1.2, -1.0, exclusions)
            ref3 = nb_oracle.evaluate('w(t1, t2, step(r - 0.5))*r^2', ['t'], [[float(t)] for t in types], {}, xs[r], boxes[r], 2, 1.2, -1.0, exclusions)
        assert len(ref['E']) >= 8 and np.abs(ref['r_all'] - 1.2).min() > 1e-6 and np.abs(ref3['r'] - 0.5).min() > 1e-6
        assert (ref3['r'] < 0.5).any() and (ref3['r'] > 0.5).any()
        print('replica %d: %d pairs, |dE| / bound = %.3g, worst |dF| / bound = %.3g; three arguments: %.3g, %.3g' % (
            r, len(ref['E']), abs(E[r, 0] - ref['E'].sum()) / nb_oracle.energy_bound(ref),
            (np.abs(F[r] - ref['F']) / nb_oracle.force_bound(ref).clip(min=1e-300)).max(),
            abs(E3[r, 0] - ref3['E'].sum()) / nb_oracle.energy_bound(ref3), (np.abs(F3[r] - ref3['F']) / nb_oracle.force_bound(ref3).clip(min=1e-300)).max()))
        assert abs(E[r, 0] - ref['E'].sum()) <= nb_oracle.energy_bound(ref)
        assert np.all(np.abs(F[r] - ref['F']) <= nb_oracle.force_bound(ref))
        assert abs(Ec[r, 0] - ref['E'].sum()) <= nb_oracle.energy_bound(ref)
        assert np.all(np.abs(Fc[r] - F[r]) <= nb_oracle.force_bound(ref))         # the table and the closed form: the same forces
        assert abs(E3[r, 0] - ref3['E'].sum()) <= nb_oracle.energy_bound(ref3)
        assert np.all(np.abs(F3[r] - ref3['F']) <= nb_oracle.force_bound(ref3))
    assert np.abs(F).max() > 1.0 and np.abs(F3).max() > 1.0


# ---- 4. the guards on the device ------------------------------------------------------------------------------------------------------------
def test_arguments_at_the_edges_outside_huge_and_nan(hip_engine_factory):
    """one handle of four forces.  edges: tab(s*x, k) of hand-placed x (f32 numbers) and per-term k: exactly min and max of either
    argument, one step outside, 1e300 (through the factor s, and as k) -- against the reference, which is exactly 0 outside.  bonds: 65
    bonds, so that the second wavefront holds one term and 63 padding lanes that repeat it, its k = 1e300.  nan: one term whose k is a
    NaN: that force's energy is NaN, the others' stay finite.  lookup: an index out of range gives a NaN energy."""
    xs = oc.XS.copy()
    T = 65
    name = 't3x2'
    nx, ny, xmin, xmax, ymin, ymax, _ = cases.TABLES[name]
    assert all(float(np.float32(v)) == v for v in (xmin, xmax, ymin, ymax))
    up, down = lambda v: float(np.nextafter(v, np.inf)), lambda v: float(np.nextafter(v, -np.inf))
    x = xmin + (xmax - xmin) * ((0.6180339887 * np.arange(T)) % 1.0)
    k = ymin + (ymax - ymin) * ((0.7548776662 * np.arange(T)) % 1.0)
    s = np.ones(T)
    x[:8] = [xmin, xmax, float(np.nextafter(np.float32(xmin), np.float32(-np.inf))), float(np.nextafter(np.float32(xmax), np.float32(np.inf))), 0.5, 0.5, 1e30, -1e30]
    k[8:14] = [ymin, ymax, down(ymin), up(ymax), 1e300, -1e300]
    s[14:16] = [1e300, -1e300]                                                  # s*x = +-1e300 or so; with x = 1e30 below: an infinity
    s[6] = 1e300
    xs[:, :T, 0] = _f32(x)
    edges = _row('edges', 'ext', 'c*tab(s*x, k) + y^2', np.arange(T)[:, None], dict(tab=_table(name)), names=('c', 's', 'k'),
                 params=np.column_stack([K70[:T, 0], s, k]))
    kb = -1.0 + 3.0 * ((0.6180339887 * np.arange(T)) % 1.0)
    kb[-1] = 1e300
    bonds = _row('bonds', 'bond', 'c*tab(r, k) + r', oc._chain_atoms(2, 100)[:T], dict(tab=_table('b5x7')), names=('c', 'k'),
                 params=np.column_stack([K70[:T, 0], kb]))
    kn = np.full(20, 0.5)                                                       # (atoms 65 ... 84 and 165 ... 184: none of the forces above)
    kn[3] = math.nan
    nan = _row('nan', 'ext', 'tab(x, k) + 1', 65 + np.arange(20)[:, None], dict(tab=_table(name)), names=('k',), params=kn[:, None])
    index = (np.arange(20) % 2).astype(np.float64)
    index[5] = 2.0
    look = _row('lookup', 'ext', 'two(i, 2) + three(i, 1, 1) + x', 165 + np.arange(20)[:, None], dict(two=(cases.lookup2_function(), cases.lookup2()),
                three=(cases.lookup3_function(), cases.lookup3())), names=('i',), params=index[:, None])
    rows = [edges, bonds, nan, look]
    eng, _ = _engine(hip_engine_factory, [_force_of(r) for r in rows], xs)
    F, E = eng.get_forces(), eng.custom_energies()
    assert np.isfinite(E[:, :2]).all() and np.isnan(E[:, 2:]).all()
    for r in range(2):
        Ee = _reference(edges, xs[r])[0]
        assert np.isfinite(Ee).all() and np.all(Ee[[0, 1, 8, 9]] > 1.0)            # exactly min and max: inside
        quiet = _reference(dict(edges, energy='c*tab(s*x, k)'), xs[r], gradients=False)[0]
        assert np.all(quiet[[2, 3, 6, 7, 10, 11, 12, 13, 14, 15]] == 0.0)           # a step outside, 1e30, 1e300, an infinity: exactly 0
        En, El = _reference(nan, xs[r])[0], _reference(look, xs[r])[0]
        assert np.isnan(En[3]) and np.isfinite(np.delete(En, 3)).all() and np.isnan(El[5]) and np.isfinite(np.delete(El, 5)).all()
    _compare(rows[:2], xs, _forces_without(F, rows), E)
    assert np.isfinite(np.delete(F, [65 + 3], axis=1)).all()                     # at most the atom of the NaN term carries a NaN force


def _forces_without(F, rows):
    """the device forces with the atoms of the forces that hold a NaN term (rows 2 and 3: atoms of their own) zeroed: what _compare
    sums from the reference for rows 0 and 1 does not reach them either"""
    out = F.copy()
    for row in rows[2:]:
        out[:, np.unique(row['atoms'])] = 0.0
    touched = np.unique(np.concatenate([np.unique(r['atoms']) for r in rows[:2]]))
    assert not set(touched.tolist()) & set(np.concatenate([np.unique(r['atoms']) for r in rows[2:]]).tolist())
    return out


# ---- 5. integration -------------------------------------------------------------------------------------------------------------------------
def test_minimize_group_forces_and_repeatability_on_alanine_dipeptide(hip_engine_factory):
    """the full AlanineDipeptideVacuum with the map of test 2 scaled to 30 kJ/mol: minimize() lowers the energy; custom_energies() and
    get_forces(groups=...) report the map's share; two evaluations are bit-identical"""
    al, xs = _alanine_positions()
    xs = xs[1:]                                                                 # (the perturbed copies: there is energy to lose)
    f = _cmap_force(lam=30.0)
    f.setForceGroup(3)
    system = copy.deepcopy(al.system)
    system.addForce(f)
    desc = system_to_desc(system)
    eng = hip_engine_factory()
    eng.set_system(desc)
    eng.set_states(np.full(1, BETA))
    eng.set_custom_globals(np.array([[30.0]]))
    eng.set_replicas(2, 0, xs, None, np.zeros((2, 3)), np.zeros(2, dtype=np.int64))
    row = _cmap_row(lam=30.0)
    F, share, E = eng.get_forces(), eng.get_forces(groups=1 << 3), eng.custom_energies()
    for r in range(2):
        Er, Fr, G = _reference(row, xs[r])
        assert abs(E[r, 0] - Er.sum()) <= 1e-11 * np.abs(Er).sum()
        assert np.all(np.abs(share[r] - Fr) <= force_bound([row], [G], xs.shape[1]))
    assert np.allclose(eng.get_forces(groups=1 << 0) + share, F, rtol=1e-9, atol=1e-6)      # (fixed-point sums: the groups add up)
    assert np.array_equal(eng.get_forces(), F) and np.array_equal(eng.custom_energies(), E) and np.array_equal(eng.get_forces(groups=1 << 3), share)
    u0 = eng.get_replicas(positions=False, velocities=False, potential=True)[2]
    eng.minimize(tolerance=1.0, max_iterations=200)
    u1 = eng.get_replicas(positions=False, velocities=False, potential=True)[2]
    print('potential before', u0, 'after', u1, 'map', E[:, 0], '->', eng.custom_energies()[:, 0])
    assert np.all(u1 < u0 - 1.0) and np.isfinite(eng.custom_energies()).all()


# ---- 6. the descriptor check ----------------------------------------------------------------------------------------------------------------
def test_corrupted_descriptors_are_refused_before_any_kernel(hip_engine_factory):
    s = System()
    for _ in range(4):
        s.addParticle(12.0)
    f = CustomBondForce('tab(r, 1) + two(r, 1) + three(r, 1, 0)')
    f.addTabulatedFunction('tab', cases.function('t3x2'))
    f.addTabulatedFunction('two', cases.lookup2_function())
    f.addTabulatedFunction('three', cases.lookup3_function())
    f.addBond(0, 1, [])
    s.addForce(f)
    desc = system_to_desc(s)
    term = desc['custom_terms']['000']
    assert term['program'].tolist() == [[cx.VAR, 0], [cx.CONST, 0], [cx.TABLE2D, 2], [cx.VAR, 0], [cx.CONST, 0], [cx.LOOKUP2D, 34], [cx.ADD, 0],
                                        [cx.VAR, 0], [cx.CONST, 0], [cx.CONST, 1], [cx.LOOKUP3D, 42], [cx.ADD, 0]] and len(term['consts']) == 58
    hip_engine_factory().set_system(desc)                                          # as compiled: accepted

    def refused(sentence, consts=None, program=None, **other):
        bad = dict(desc, custom_terms={'000': dict(term, consts=term['consts'].copy() if consts is None else consts,
                                                   program=term['program'].copy() if program is None else program, **other)})
        with pytest.raises(Exception, match=sentence):
            hip_engine_factory().set_system(bad)

    def consts_with(i, v):
        c = term['consts'].copy(); c[i] = v
        return c

    def program_with(pc, arg=None, op=None):
        p = term['program'].copy()
        if arg is not None:
            p[pc, 1] = arg
        if op is not None:
            p[pc, 0] = op
        return p
    refused('a table offset out of range', program=program_with(2, 58))
    refused('a table offset out of range', program=program_with(5, -1))
    refused('a table that runs past n_consts', program=program_with(10, 56))       # (not even the header fits)
    refused('a 2D table whose size is not an integer 2 ... REMD_CUSTOM_MAX_TABLE_CELLS', consts=consts_with(2, 1.0))
    refused('a 2D table whose size is not an integer 2 ... REMD_CUSTOM_MAX_TABLE_CELLS', consts=consts_with(3, 2.5))
    refused('a 2D table whose size is not an integer 2 ... REMD_CUSTOM_MAX_TABLE_CELLS', consts=consts_with(2, math.nan))
    refused('a 2D table whose size is not an integer 2 ... REMD_CUSTOM_MAX_TABLE_CELLS', consts=consts_with(2, 65537.0))
    refused('a lookup table whose size is not an integer 1 ... REMD_CUSTOM_MAX_TABLE_CELLS', consts=consts_with(34, 0.0))
    refused('a lookup table whose size is not an integer 1 ... REMD_CUSTOM_MAX_TABLE_CELLS', consts=consts_with(44, -1.0))
    refused('a table of more than REMD_CUSTOM_MAX_TABLE_CELLS cells', consts=consts_with(2, 40000.0))
    big = consts_with(42, 4096.0); big[44] = 4096.0                                # (each size in range, the product not)
    refused('a table of more than REMD_CUSTOM_MAX_TABLE_CELLS cells', consts=big)
    refused('a table whose bounds are not finite with min < max', consts=consts_with(4, 2.0))
    refused('a table whose bounds are not finite with min < max', consts=consts_with(7, math.inf))
    refused('a table whose periodic flag is neither 0 nor 1', consts=consts_with(8, 0.5))
    refused('a table that runs past n_consts', consts=consts_with(2, 8.0))
    refused('a table that runs past n_consts', consts=consts_with(35, 30.0))
    refused('a table that runs past n_consts', consts=consts_with(44, 3.0))
    refused('a program that pops an empty stack', program=program_with(1, op=cx.VAR)[[0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]], stack_depth=3)
    refused('a program that does not leave exactly one value', program=program_with(10, arg=34, op=cx.LOOKUP2D))       # (three arguments, two popped)
