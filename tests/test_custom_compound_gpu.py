"""GPU: CustomCompoundBondForce (openmmtools_amd/custom_expr.py, csrc/custom_compound.hip, include/remd_hip_custom.h) against the
independent f64 helper tests/compound_expr_oracle.py.

Every check is a difference "with the force minus without it" at the same positions.  Bounds (the project's HIP-leg standard, those of
tests/test_custom_terms_gpu.py): forces within 1e-5 max|F_custom|, energies within 1e-5 sum|E_term|, u_kl differences within rtol
1e-5, atol 1e-5 max|want|.  Positions are rounded to f32 before they go to either side: that is what the engine stores."""
import copy
import math

import numpy as np
import pytest

import compound_expr_oracle as oracle
import custom_expr_oracle as term_oracle
from openmmtools_amd import custom_expr as cx, mcmc, states, testsystems, unit
from openmmtools_amd.system import (system_to_desc, CustomBondForce, CustomAngleForce, CustomTorsionForce, CustomCompoundBondForce,
                                    HarmonicBondForce, HarmonicAngleForce, PeriodicTorsionForce)

pytestmark = pytest.mark.gpu

KB = 0.008314462618153242
BETA = 1.0 / (KB * 300.0)
HEAVY = [1, 4, 6, 8, 14, 16]            # CH3 - C - N - CA - C - N of alanine dipeptide: the six particles of the Boresch bond


def _f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def _setup(engine, system, xs, boxes=None, global_table=None, labels=None):
    desc = system_to_desc(system, box=None if boxes is None else boxes[0])
    engine.set_system(desc)
    custom = desc.get('custom_terms')
    K = 1 if global_table is None else len(global_table)
    engine.set_states(np.full(K, BETA))
    if custom:
        engine.set_custom_globals(np.tile(custom['000']['global_defaults'], (K, 1)) if global_table is None else global_table)
    R = len(xs)
    engine.set_replicas(R, 0, xs, None, np.zeros((R, 3)) if boxes is None else boxes, np.zeros(R, dtype=np.int64) if labels is None else labels)
    return desc


def _device(engine, system, xs, boxes=None, global_table=None, labels=None):
    """forces [R][N][3], potentials [R], per-force energies [R][n] (None without custom forces)"""
    desc = _setup(engine, system, xs, boxes, global_table, labels)
    f = engine.get_forces()
    u = engine.get_replicas(positions=False, velocities=False, potential=True)[2]
    return f, u, engine.custom_energies() if desc.get('custom_terms') else None


def _helper(force, x, box=None, global_values=None):
    """per-term energies and forces of one custom force from the helpers"""
    atoms, params = force._term_arrays()
    g = {force.getGlobalParameterName(i): force.getGlobalParameterDefaultValue(i) for i in range(force.getNumGlobalParameters())}
    g.update(global_values or {})
    if isinstance(force, CustomCompoundBondForce):
        return oracle.evaluate(force.getNumParticlesPerBond(), force.getEnergyFunction(), atoms, list(force._per_bond), params, g, x, box,
                               force.usesPeriodicBoundaryConditions())
    kind = cx.KIND_OF_CLASS[[c.__name__ for c in type(force).__mro__ if c.__name__ in cx.KIND_OF_CLASS][0]]
    return term_oracle.evaluate(kind, force.getEnergyFunction(), atoms, list(force._per_bond), params, g, x, box, force.usesPeriodicBoundaryConditions())


def _check(factory, base, customs, xs, boxes=None):
    """the custom forces added to ``base`` against the helpers, at R positions (and boxes): forces, potential and per-force energies (in
    the forces' order); -> the force differences [R][N][3]"""
    xs = _f32(xs)
    system = copy.deepcopy(base)
    for f in customs:
        system.addForce(f)
    f0, u0, _ = _device(factory(), base, xs, boxes)
    f1, u1, e1 = _device(factory(), system, xs, boxes)
    assert e1.shape == (len(xs), len(customs))
    for r, x in enumerate(xs):
        per = [_helper(f, x, None if boxes is None else boxes[r]) for f in customs]
        F = sum(p[1] for p in per)
        E = np.array([p[0].sum() for p in per])
        tol_E = 1e-5 * sum(np.abs(p[0]).sum() for p in per)
        print('replica %d: |dF| / max|F| = %.3g, |dE| / sum|E| = %.3g' % (r, np.abs(f1[r] - f0[r] - F).max() / np.abs(F).max(),
                                                                         np.abs(e1[r] - E).max() / (tol_E / 1e-5)))
        assert np.abs(f1[r] - f0[r] - F).max() <= 1e-5 * np.abs(F).max()
        assert np.abs(e1[r] - E).max() <= tol_E
        assert abs((u1[r] - u0[r]) - E.sum()) <= tol_E + 2e-7 * abs(u0[r])          # (the base potential is summed in f32 partials)
    return f1 - f0


def _alanine(R=3, seed=1):
    al = testsystems.AlanineDipeptideVacuum()
    rng = np.random.default_rng(seed)
    xs = np.array([np.asarray(al.positions, dtype=np.float64) + rng.normal(0.0, 0.004, (len(al.positions), 3)) for _ in range(R)])
    return al, xs


def _builtin(system, cls):
    return [f for f in system.getForces() if isinstance(f, cls)][0]


# reference values this far off the geometry (nm, rad): every term of the restraint pulls
OFFSETS = (0.05, 0.4, -0.35, 0.45, -0.3, 0.5)
SPRINGS = (4000.0, 80.0, 90.0, 70.0, 60.0, 50.0)


def _boresch(x, atoms=HEAVY, lam=1.0, box=None, periodic=False, group=0):
    """the Boresch restraint on ``atoms`` with the reference values OFFSETS off the geometry at positions x"""
    f = CustomCompoundBondForce(6, oracle.BORESCH)
    f.addGlobalParameter('lambda_restraints', lam)
    for name in oracle.BORESCH_PARAMETERS:
        f.addPerBondParameter(name)
    v = oracle.boresch_values(np.asarray(x, dtype=np.float64)[atoms], box, periodic)
    f.addBond(atoms, [p for k, a, o in zip(SPRINGS, v, OFFSETS) for p in (k, a - o)])
    f.setUsesPeriodicBoundaryConditions(periodic)
    f.setForceGroup(group)
    return f


def _assert_no_dihedral_near_its_wrap(f, xs, box=None):
    """no dphi of the restraint within 0.1 rad of its wrap at any of the positions: the helper's differences never straddle the floor"""
    atoms, p = f.getBondParameters(0)
    for x in xs:
        v = oracle.boresch_values(_f32(x)[atoms], box, f.usesPeriodicBoundaryConditions())
        for phi, ref in zip(v[3:], (p[7], p[9], p[11])):
            assert abs(abs(oracle.wrap(phi - ref)) - math.pi) > 0.1


# ---- 1. the Boresch restraint against the helper ---------------------------------------------------------------------------------------
def test_boresch_restraint_against_the_helper(hip_engine_factory):
    al, xs = _alanine()
    f = _boresch(al.positions, lam=0.7)
    _assert_no_dihedral_near_its_wrap(f, xs)
    dF = _check(hip_engine_factory, al.system, [f], xs)
    assert all(np.abs(dF[:, a]).max() > 0.0 for a in HEAVY)                        # (every particle of the bond is pulled)


# ---- 2. launch-shape edges ---------------------------------------------------------------------------------------------------------------
def test_launch_shape_edges_in_one_handle(hip_engine_factory):
    """a plain CustomBondForce between compound forces of 2, 4 and 8 particles with one bond each (63 padding lanes), a 64-bond and a
    65-bond force (a full wavefront; one bond in a second one), a bond that ignores one of its particles, bonds sharing atoms, and the
    per-force energies in the forces' order although the compound forces' wavefronts lie behind the plain one's"""
    al, xs = _alanine(seed=2)
    lone = 19                                                                      # an atom that only the ignoring bond names
    bonds = _builtin(al.system, HarmonicBondForce).bonds
    torsions = [t for t in _builtin(al.system, PeriodicTorsionForce).torsions if lone not in t[:4]]
    assert all(lone not in b[:2] for b in bonds)
    plain = CustomBondForce('0.5*K*(r-r0)^2'); plain.addPerBondParameter('K'); plain.addPerBondParameter('r0')
    for (i, j, r0, k) in bonds:
        plain.addBond(i, j, [k, r0 * 1.03])
    p2 = CustomCompoundBondForce(2, 'k*(distance(p1,p2)-0.2)^2 + k*(z2-z1)^2'); p2.addPerBondParameter('k'); p2.addBond([1, 8], [300.0])
    p4 = CustomCompoundBondForce(4, 'k*(distance(p1,p2)-0.1)^2 + 7*angle(p1,p2,p4)^2 + 0*k'); p4.addPerBondParameter('k')
    p4.addBond([8, 14, lone, 16], [500.0])                                         # (p3 is not in the expression)
    p8 = CustomCompoundBondForce(8, 'k*cos(dihedral(p1,p2,p3,p4))*sin(dihedral(p5,p6,p7,p8)) + k*pointdistance(x1,y1,z1,x8,y8,z8)^2 + cos(angle(p8,p1,p4)) + x5*y6')
    p8.addGlobalParameter('k', 20.0); p8.addBond([1, 4, 6, 8, 10, 14, 16, 18])
    c64 = CustomCompoundBondForce(2, '0.5*K*(distance(p2,p1)-r0)^2'); c64.addPerBondParameter('K'); c64.addPerBondParameter('r0')
    for n in range(64):
        i, j, r0, k = bonds[n % len(bonds)]
        c64.addBond([i, j], [k * (1.0 + 0.01 * n), r0 * 0.98])
    c65 = CustomCompoundBondForce(4, 'k*(1+cos(n*dihedral(p1,p2,p3,p4)-phase))')
    for name in ('n', 'phase', 'k'):
        c65.addPerBondParameter(name)
    for n in range(65):
        a, b, c, d, per, phase, k = torsions[n % len(torsions)]
        c65.addBond([a, b, c, d], [per, phase + 0.01 * n, k + 1.0])
    customs = [p2, plain, p4, c64, p8, c65]
    system = copy.deepcopy(al.system)
    for f in customs:
        system.addForce(f)
    terms = system_to_desc(system)['custom_terms']
    assert [len(terms[k]['atoms']) for k in sorted(terms)] == [1, len(bonds), 1, 64, 1, 65]
    assert [terms[k].get('n_particles', 0) for k in sorted(terms)] == [2, 0, 4, 2, 8, 4]
    dF = _check(hip_engine_factory, al.system, customs, xs)
    assert not dF[:, lone].any()                                                   # exactly zero: no pass gives the ignored particle a force


# ---- 3. equivalence with the one-variable path ---------------------------------------------------------------------------------------------
def test_compound_forces_with_one_variable_agree_with_the_one_variable_kinds(hip_engine_factory):
    al, xs = _alanine(seed=3)
    xs = _f32(xs)
    b = CustomBondForce('0.5*k*(r-r0)^2'); cb = CustomCompoundBondForce(2, '0.5*k*(distance(p1,p2)-r0)^2')
    a = CustomAngleForce('0.5*k*(theta-theta0)^2'); ca = CustomCompoundBondForce(3, '0.5*k*(angle(p1,p2,p3)-theta0)^2')
    t = CustomTorsionForce('k*(1+cos(n*theta-phase))'); ct = CustomCompoundBondForce(4, 'k*(1+cos(n*dihedral(p1,p2,p3,p4)-phase))')
    for f in (b, cb):
        f.addPerBondParameter('r0'); f.addPerBondParameter('k')
    for f, g in ((a, a.addPerAngleParameter), (ca, ca.addPerBondParameter)):
        g('theta0'); g('k')
    for f, g in ((t, t.addPerTorsionParameter), (ct, ct.addPerBondParameter)):
        g('n'); g('phase'); g('k')
    for term in _builtin(al.system, HarmonicBondForce).bonds:
        b.addBond(term[0], term[1], [term[2] * 1.02, term[3]]); cb.addBond(term[:2], [term[2] * 1.02, term[3]])
    for term in _builtin(al.system, HarmonicAngleForce).angles:
        a.addAngle(term[0], term[1], term[2], [term[3] + 0.05, term[4]]); ca.addBond(term[:3], [term[3] + 0.05, term[4]])
    tor = _builtin(al.system, PeriodicTorsionForce).torsions
    for term in tor:
        t.addTorsion(term[0], term[1], term[2], term[3], [term[4], term[5], term[6] + 1.0]); ct.addBond(term[:4], [term[4], term[5], term[6] + 1.0])
    thetas = [term_oracle.variables(cx.KIND_TORSION, xs[0][list(term[:4])])['theta'] for term in tor]
    assert min(thetas) < -0.5 and max(thetas) > 0.5                                # both signs of the dihedral
    one, compound = copy.deepcopy(al.system), copy.deepcopy(al.system)
    for f in (b, a, t):
        one.addForce(f)
    for f in (cb, ca, ct):
        compound.addForce(f)
    f0 = _device(hip_engine_factory(), al.system, xs)[0]
    f1, _, e1 = _device(hip_engine_factory(), one, xs)
    f2, _, e2 = _device(hip_engine_factory(), compound, xs)
    scale = np.abs(f1 - f0).max()
    print('|F_compound - F_one_variable| / max|F| =', np.abs(f2 - f1).max() / scale)
    assert np.abs(f2 - f1).max() <= 1e-5 * scale
    for r, x in enumerate(xs):
        tol = [1e-5 * np.abs(_helper(f, x)[0]).sum() for f in (b, a, t)]
        print('replica %d: |E_compound - E_one_variable| / sum|E_term| =' % r, np.abs(e2[r] - e1[r]) / (np.array(tol) / 1e-5))
        assert np.all(np.abs(e2[r] - e1[r]) <= tol)


# ---- 4. periodic ---------------------------------------------------------------------------------------------------------------------------
def test_periodic_compound_force_under_each_replicas_own_box(hip_engine_factory):
    """a bond between two water molecules on opposite faces of AlanineDipeptideExplicit's box, three replicas with three boxes: the periodic
    force sees the minimum images under each replica's own box, the copy that is not periodic the raw differences"""
    al = testsystems.AlanineDipeptideExplicit()
    box = np.diag(al.system.getDefaultPeriodicBoxVectors())
    boxes = np.array([box, box * 1.01, box * 1.02])
    x = _f32(al.positions)
    xs = np.array([x, x + 0.001, x - 0.001])
    oxygens = np.arange(22, len(x), 3)
    lo, hi = oxygens[np.argmin(x[oxygens, 0])], oxygens[np.argmax(x[oxygens, 0])]
    atoms = [int(lo), int(lo) + 1, int(hi), int(hi) + 1]                           # O, H of one water; O, H of the other
    for b in boxes:                                                                # (the minimum image is not the raw difference)
        d = x[hi] - x[lo]
        assert abs(d[0]) > 0.5 * b[0] + 0.01 and not np.array_equal(term_oracle.minimum_image(d, b), d)
    energy = ('k*(distance(p1,p3)-0.3)^2 + ka*(angle(p2,p1,p3)-1.5)^2 + kd*cos(dihedral(p2,p1,p3,p4)-0.4) '
              '+ kp*pointdistance(x2,y2,z2,x4,y4,z4)^2')
    made = []
    for periodic in (True, False):
        f = CustomCompoundBondForce(4, energy)
        for name, v in (('k', 900.0), ('ka', 60.0), ('kd', 25.0), ('kp', 40.0)):
            f.addGlobalParameter(name, v)
        f.addBond(atoms)
        f.setUsesPeriodicBoundaryConditions(periodic)
        made.append(f)
    e_periodic, e_raw = (_helper(f, xs[0], boxes[0])[0][0] for f in made)
    assert abs(e_raw - e_periodic) > 0.5 * abs(e_raw)                               # (two different results to tell apart)
    for f in made:
        _check(hip_engine_factory, al.system, [f], xs, boxes)


# ---- 5. u_kl and replica exchange ------------------------------------------------------------------------------------------------------------
LAMBDAS = np.array([1.0, 0.5, 0.0])


class RestraintState(states.GlobalParameterState):
    lambda_restraints = states.GlobalParameterState.GlobalParameter('lambda_restraints', standard_value=1.0)


def test_ukl_carries_the_restraint_at_every_states_lambda(hip_engine_factory):
    al, xs = _alanine(seed=5)
    xs = _f32(xs)
    f = _boresch(al.positions)
    _assert_no_dihedral_near_its_wrap(f, xs)
    system = copy.deepcopy(al.system); system.addForce(f)
    labels = np.array([2, 0, 1])
    table = LAMBDAS[:, None].copy()
    e0 = hip_engine_factory(); _setup(e0, al.system, xs, global_table=table, labels=labels)        # (three states, no custom force)
    u0 = e0.compute_energies()
    e1 = hip_engine_factory(); _setup(e1, system, xs, global_table=table, labels=labels)
    u1 = e1.compute_energies()
    E = np.array([_helper(f, x, global_values=dict(lambda_restraints=1.0))[0].sum() for x in xs])
    want = BETA * LAMBDAS[None, :] * E[:, None]                                    # beta_l lambda_l E_r
    got = u1 - u0
    print('u_kl rows: max |got - want| / max|want| =', np.abs(got - want).max() / np.abs(want).max())
    own = np.arange(3), labels
    share = (u1 - u1[own][:, None]) - (u0 - u0[own][:, None])                      # (relative to the own state: the base cancels)
    print('u_kl share: max |got - want| / max|want| =', np.abs(share - (want - want[own][:, None])).max() / np.abs(want).max())
    assert np.allclose(got, want, rtol=1e-5, atol=1e-5 * np.abs(want).max())
    # a state with the replica's own globals: its column is the own column, to the bit (the kernel skips it; other states differ, so the
    # launch itself is not skipped)
    e1.set_custom_globals(np.array([[1.0], [0.5], [0.5]]))
    e1.set_labels(np.array([1, 2, 0]))
    u2 = e1.compute_energies()
    assert u2[0, 2] == u2[0, 1] and u2[1, 1] == u2[1, 2] and u2[0, 0] != u2[0, 1]


def test_replica_exchange_over_lambda_restraints(hip_engine_factory):
    from openmmtools_amd.multistate import ReplicaExchangeSampler
    al = testsystems.AlanineDipeptideVacuum()
    f = _boresch(al.positions)
    al.system.addForce(f)
    ts = states.ThermodynamicState(al.system, 300.0)
    sts = states.create_thermodynamic_state_protocol(ts, {'lambda_restraints': list(LAMBDAS)},
                                                     composable_states=[RestraintState(lambda_restraints=1.0)])
    assert all(isinstance(s, states.CompoundThermodynamicState) for s in sts)
    move = mcmc.LangevinSplittingDynamicsMove(timestep=1.0 * unit.femtosecond, collision_rate=1.0 / unit.picosecond, n_steps=20,
                                              reassign_velocities=True, splitting='V R O R V')
    engine = hip_engine_factory()
    s = ReplicaExchangeSampler(mcmc_moves=move, number_of_iterations=10 ** 9, engine=engine, seed=0xBEEF)
    s.create(sts, [states.SamplerState(al.positions)], storage=None)
    s.run(3)
    u, x = np.array(s.energy_thermodynamic_states), engine.get_replicas()[0]
    _assert_no_dihedral_near_its_wrap(f, x)
    E = np.array([_helper(f, _f32(xr), global_values=dict(lambda_restraints=1.0))[0].sum() for xr in x])
    want = sts[0].beta * (LAMBDAS[None, :] - LAMBDAS[0]) * E[:, None]
    got = u - u[:, :1]
    print('sampler u_kl: max |got - want| / max|want| =', np.abs(got - want).max() / np.abs(want).max())
    assert np.allclose(got, want, rtol=1e-5, atol=1e-5 * np.abs(want).max())


# ---- 6. force groups -----------------------------------------------------------------------------------------------------------------------
def test_multiple_time_step_splitting_and_group_forces(hip_engine_factory):
    al = testsystems.AlanineDipeptideVacuum()
    f = CustomCompoundBondForce(2, '0.5*K*distance(p1,p2)^2'); f.addPerBondParameter('K'); f.addBond([0, 21], [1000.0])
    f.setForceGroup(2)
    al.system.addForce(f)
    x = np.array(al.positions, dtype=np.float64)
    r_start = np.linalg.norm(x[21] - x[0])
    eng = hip_engine_factory()
    _setup(eng, al.system, np.tile(x, (2, 1, 1)))
    only = eng.get_forces(groups=1 << 2)
    E, F = _helper(f, _f32(x))
    assert np.abs(only - F[None]).max() <= 1e-5 * np.abs(F).max()
    assert np.allclose(eng.get_forces(groups=1 << 0) + only, eng.get_forces(), rtol=1e-9, atol=1e-6)     # (fixed-point sums: the groups add up)
    eng.set_integrator('V0 V1 R V1 V0', 0.001, 5.0, 10, True, 1e-8)
    with pytest.raises(RuntimeError, match='custom forces sit in a force group'):
        eng.propagate(0)
    eng.set_integrator('V2 V0 R O R V0 V2', 0.001, 5.0, 500, True, 1e-8)
    eng.propagate(1)
    y = eng.get_replicas()[0]
    assert np.all(np.linalg.norm(y[:, 21] - y[:, 0], axis=1) < r_start - 0.15)


# ---- 7. phases -----------------------------------------------------------------------------------------------------------------------------
def test_two_blocks_of_replicas_do_not_change_a_bit(hip_engine_factory):
    """six replicas of AlanineDipeptideExplicit with a periodic Boresch restraint at three lambdas, as one block and as two (the second
    block's handle holds a clone of the tables): the same positions and the same energy matrix after 10 steps"""
    al = testsystems.AlanineDipeptideExplicit()
    box = np.diag(al.system.getDefaultPeriodicBoxVectors())
    f = _boresch(al.positions, box=box, periodic=True)
    al.system.addForce(f)
    x = _f32(al.positions)
    xs = np.array([x + 0.0005 * r for r in range(6)])
    out = []
    for phases in (1, 2):
        eng = hip_engine_factory()
        eng.set_phases(phases)
        _setup(eng, al.system, xs, np.tile(box, (6, 1)), global_table=LAMBDAS[:, None].copy(), labels=np.array([0, 1, 2, 2, 1, 0]))
        eng.set_integrator('V R O R V', 0.001, 1.0, 10, True, 1e-8)
        eng.seed(11)
        eng.propagate(0)
        assert eng.phases_active() == phases
        out.append((eng.get_replicas()[0], eng.compute_energies(), eng.custom_energies()))
    for q, name in enumerate(('positions', 'u_kl', 'custom energies')):
        assert np.array_equal(out[0][q], out[1][q]), name
    assert np.abs(out[0][0] - xs).max() > 1e-4 and out[0][2][0, 0] > 0.0 and out[0][2][2, 0] == 0.0       # (moved; lambda 1 and lambda 0)
