"""GPU: custom bond / angle / torsion / external forces (openmmtools_amd/custom_expr.py, csrc/custom_terms.hip,
include/remd_hip_custom.h) against the independent f64 helper tests/custom_expr_oracle.py.

Every check is a difference "with the force minus without it" at the same positions.  Bounds (the project's HIP-leg standard): forces
within 1e-5 max|F_custom|, energies within 1e-5 sum|E_term|, u_kl differences within rtol 1e-5, atol 1e-5 max|want|.  Positions are
rounded to f32 before they go to either side: that is what the engine stores."""
import copy

import numpy as np
import pytest

import custom_expr_oracle as oracle
from openmmtools_amd import custom_expr as cx, mcmc, states, testsystems, unit
from openmmtools_amd.system import (System, system_to_desc, CustomBondForce, CustomAngleForce, CustomTorsionForce, CustomExternalForce,
                                    HarmonicBondForce, HarmonicAngleForce, PeriodicTorsionForce)

pytestmark = pytest.mark.gpu

KB = 0.008314462618153242
BETA = 1.0 / (KB * 300.0)


def _f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def _customs(system):
    return [f for f in system.getForces() if cx.is_custom_term_force(f)]


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
    """per-term energies and forces of one custom force from the helper"""
    kind = cx.KIND_OF_CLASS[[c.__name__ for c in type(force).__mro__ if c.__name__ in cx.KIND_OF_CLASS][0]]
    atoms, params = force._term_arrays()
    g = {force.getGlobalParameterName(i): force.getGlobalParameterDefaultValue(i) for i in range(force.getNumGlobalParameters())}
    g.update(global_values or {})
    return oracle.evaluate(kind, force.getEnergyFunction(), atoms, list(force._per_bond), params, g, x, box, force.usesPeriodicBoundaryConditions())


def _check(factory, base, customs, xs, boxes=None):
    """the custom forces added to ``base`` against the helper, at R positions (and boxes): forces, potential and per-force energies"""
    xs = _f32(xs)
    system = copy.deepcopy(base)
    for f in customs:
        system.addForce(f)
    if base.getNumForces():
        f0, u0, _ = _device(factory(), base, xs, boxes)
    else:
        f0, u0 = np.zeros_like(xs), np.zeros(len(xs))
    f1, u1, e1 = _device(factory(), system, xs, boxes)
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


def _alanine(R=3, seed=1):
    al = testsystems.AlanineDipeptideVacuum()
    rng = np.random.default_rng(seed)
    xs = np.array([np.asarray(al.positions, dtype=np.float64) + rng.normal(0.0, 0.004, (len(al.positions), 3)) for _ in range(R)])
    return al, xs


def _builtin(system, cls):
    return [f for f in system.getForces() if isinstance(f, cls)][0]


def _bond_force(system, energy='lambda_bonds^gamma * 0.5*K*(r-r0)^2', lam=0.7, gamma=1.5):
    f = CustomBondForce(energy)
    f.addGlobalParameter('lambda_bonds', lam); f.addGlobalParameter('gamma', gamma)
    f.addPerBondParameter('K'); f.addPerBondParameter('r0')
    for (i, j, r0, k) in _builtin(system, HarmonicBondForce).bonds:
        f.addBond(i, j, [k, r0])
    return f


# ---- a. each kind against the helper ---------------------------------------------------------------------------------------------
def test_bond_forces_against_the_helper(hip_engine_factory):
    al, xs = _alanine()
    morse = CustomBondForce('D*(1-exp(-a*(r-r0)))^2; a = sqrt(K/(2*D))')
    morse.addGlobalParameter('D', 400.0); morse.addPerBondParameter('K'); morse.addPerBondParameter('r0')
    for (i, j, r0, k) in _builtin(al.system, HarmonicBondForce).bonds[::2]:
        morse.addBond(i, j, [k, r0 * 1.02])
    _check(hip_engine_factory, al.system, [_bond_force(al.system), morse], xs)


def test_angle_force_against_the_helper(hip_engine_factory):
    al, xs = _alanine(seed=2)
    f = CustomAngleForce('0.5*k*(cos(theta)-cos(t0))^2/sin(t0)^2')
    f.addPerAngleParameter('k'); f.addPerAngleParameter('t0')
    for (a, b, c, t0, k) in _builtin(al.system, HarmonicAngleForce).angles:
        f.addAngle(a, b, c, [k, t0])
    _check(hip_engine_factory, al.system, [f], xs)


def test_torsion_forces_against_the_helper(hip_engine_factory):
    al, xs = _alanine(seed=3)
    tor = _builtin(al.system, PeriodicTorsionForce).torsions
    f = CustomTorsionForce('k*(1+cos(n*theta-phase))')
    for name in ('n', 'phase', 'k'):
        f.addPerTorsionParameter(name)
    # (the branch is picked by a per-torsion flag: smooth in theta, so the helper's differences never straddle a kink)
    g = CustomTorsionForce('select(flag-1, k*sin(theta)^2, k2*(1-cos(3*theta+0.3))) + scale*cos(theta)')
    g.addGlobalParameter('scale', 0.25); g.addPerTorsionParameter('k'); g.addPerTorsionParameter('k2'); g.addPerTorsionParameter('flag')
    for n, (a, b, c, d, per, phase, k) in enumerate(tor):
        f.addTorsion(a, b, c, d, [per, phase, k + 1.0])
        g.addTorsion(a, b, c, d, [2.0 + 0.1 * n, 5.0 - 0.05 * n, float(n % 2)])
    _check(hip_engine_factory, al.system, [f, g], xs)
    thetas = [oracle.variables(cx.KIND_TORSION, xs[0][list(t[:4])])['theta'] for t in tor]
    assert min(thetas) < -0.5 and max(thetas) > 0.5                                # both signs of theta


def test_external_quartic_well_against_the_helper(hip_engine_factory):
    al, xs = _alanine(seed=4)
    f = CustomExternalForce('k*((x-x0)^2+(y-y0)^2+(z-z0)^2)^2 + kz*z')
    f.addGlobalParameter('kz', 30.0)
    for name in ('k', 'x0', 'y0', 'z0'):
        f.addPerParticleParameter(name)
    x0 = np.asarray(al.positions, dtype=np.float64)
    for i in range(0, len(x0), 2):
        f.addParticle(i, [4.0e4 + 100.0 * i, x0[i, 0] + 0.03, x0[i, 1] - 0.02, x0[i, 2] + 0.025])       # (x0 not representable in f32)
    _check(hip_engine_factory, al.system, [f], xs)


def _particles(n, seed, spread=2.0):
    s = System()
    for _ in range(n):
        s.addParticle(12.0)
    return s, np.random.default_rng(seed).uniform(0.0, spread, (n, 3))


def test_periodic_forces_under_each_replicas_own_box(hip_engine_factory):
    """a position restraint with periodicdistance and a periodic bond force: particles near the faces of a DIFFERENT box per replica"""
    boxes = np.array([[2.6, 2.8, 3.0], [3.3, 3.1, 2.9], [2.7, 3.4, 3.2]])
    s, x = _particles(40, 5)
    xs = np.array([x * (b / 2.0) for b in boxes])                                  # spread over the whole of each box
    e = CustomExternalForce('k*periodicdistance(x,y,z,x0,y0,z0)^2')
    e.setUsesPeriodicBoundaryConditions(True)
    for name in ('k', 'x0', 'y0', 'z0'):
        e.addPerParticleParameter(name)
    for i in range(40):
        ref = (x[i] + np.array([1.9, -1.7, 2.1])) % 2.5                            # reference points across the faces from the particles
        e.addParticle(i, [300.0 + i, ref[0], ref[1], ref[2]])
    b = CustomBondForce('0.5*K*(r-0.4)^2')
    b.setUsesPeriodicBoundaryConditions(True); b.addPerBondParameter('K')
    for i in range(39):
        b.addBond(i, (i * 7 + 3) % 40 if (i * 7 + 3) % 40 != i else (i + 1) % 40, [500.0 + 3 * i])
    _check(hip_engine_factory, s, [e, b], xs, boxes)
    d = xs[0][[t[1] for t in b._bonds]] - xs[0][[t[0] for t in b._bonds]]
    assert (np.abs(d) > 0.5 * boxes[0]).any()                                      # (imaging is exercised)


def test_alanine_explicit_pme_with_a_periodic_bond_force(hip_engine_factory):
    al = testsystems.AlanineDipeptideExplicit()
    box = np.diag(al.system.getDefaultPeriodicBoxVectors())
    f = _bond_force(al.system, lam=0.6, gamma=2.0)
    f.setUsesPeriodicBoundaryConditions(True)
    x = np.asarray(al.positions, dtype=np.float64)
    _check(hip_engine_factory, al.system, [f], np.array([x, x + 0.001]), np.tile(box, (2, 1)))


# ---- b. launch-shape edges -----------------------------------------------------------------------------------------------------------
def test_launch_shape_edges_in_one_handle(hip_engine_factory):
    """three forces of 1, 63 and 130 terms (programs change at wavefront boundaries, padding lanes in each), zero and the most per-term
    parameters, a program at the deepest stack the engine has, one atom shared by 130 terms"""
    s, x = _particles(140, 6)
    one = CustomAngleForce('theta^2')                                              # no parameters, one term
    one.addAngle(5, 6, 7)
    most = CustomTorsionForce('+'.join('p%d*cos(%d*theta+%d/7)' % (k, k % 4 + 1, k) for k in range(cx.MAX_PARAMS)))
    for k in range(cx.MAX_PARAMS):
        most.addPerTorsionParameter('p%d' % k)
    for t in range(63):
        most.addTorsion(t, t + 20, t + 41, t + 63, [0.5 + 0.01 * (t + k) for k in range(cx.MAX_PARAMS)])
    deep = 'k*(r-1)^2'
    for _ in range(cx.MAX_STACK - 3):
        deep = 'r+(%s)' % deep
    hub = CustomBondForce(deep)
    hub.addPerBondParameter('k')
    for j in range(1, 131):
        hub.addBond(0, j, [10.0 + j])
    s2 = copy.deepcopy(s)
    for f in (one, most, hub):
        s2.addForce(f)
    terms = system_to_desc(s2)['custom_terms']
    assert [len(terms[k]['atoms']) for k in sorted(terms)] == [1, 63, 130]
    assert terms['002']['stack_depth'] == cx.MAX_STACK and terms['001']['params'].shape[1] == cx.MAX_PARAMS and terms['000']['params'].shape[1] == 0
    _check(hip_engine_factory, s, [one, most, hub], np.array([x, x * 0.9 + 0.05]))


# ---- c. agreement with the built-ins ---------------------------------------------------------------------------------------------------
def _alanine_with_custom_bonded():
    al = testsystems.AlanineDipeptideVacuum()              # (constraints on the bonds to hydrogen only: HarmonicBondForce holds the others)
    base, custom = copy.deepcopy(al.system), copy.deepcopy(al.system)
    drop = (HarmonicBondForce, HarmonicAngleForce, PeriodicTorsionForce)
    base.forces = [f for f in base.forces if not isinstance(f, drop)]
    custom.forces = list(base.forces)
    b = CustomBondForce('0.5*k*(r-r0)^2'); b.addPerBondParameter('r0'); b.addPerBondParameter('k')
    for t in _builtin(al.system, HarmonicBondForce).bonds:
        b.addBond(t[0], t[1], t[2:])
    a = CustomAngleForce('0.5*k*(theta-theta0)^2'); a.addPerAngleParameter('theta0'); a.addPerAngleParameter('k')
    for t in _builtin(al.system, HarmonicAngleForce).angles:
        a.addAngle(t[0], t[1], t[2], t[3:])
    p = CustomTorsionForce('k*(1+cos(n*theta-phase))')
    for name in ('n', 'phase', 'k'):
        p.addPerTorsionParameter(name)
    for t in _builtin(al.system, PeriodicTorsionForce).torsions:
        p.addTorsion(t[0], t[1], t[2], t[3], t[4:])
    for f in (b, a, p):
        custom.addForce(f)
    return al, base, custom


def test_custom_forces_with_the_built_in_formulas_agree_with_the_built_ins(hip_engine_factory):
    al, base, custom = _alanine_with_custom_bonded()
    xs = _f32(_alanine(seed=7)[1])
    f_builtin, u_builtin, _ = _device(hip_engine_factory(), al.system, xs)
    f_base = _device(hip_engine_factory(), base, xs)[0]
    f_custom, u_custom, _ = _device(hip_engine_factory(), custom, xs)
    scale = np.abs(f_custom - f_base).max()
    print('|F_custom - F_builtin| / max|F_custom| =', np.abs(f_custom - f_builtin).max() / scale)
    assert np.abs(f_custom - f_builtin).max() <= 1e-5 * scale


def test_custom_bonded_trajectory_follows_the_built_in_one(hip_engine_factory):
    """10 V R O R V steps, same seed: within the tolerances of test_forcefield_parity.test_alanine_short_trajectory"""
    al, _, custom = _alanine_with_custom_bonded()
    x = _f32(al.positions)[None]
    out = []
    for system in (al.system, custom):
        eng = hip_engine_factory()
        _setup(eng, system, x)
        eng.set_integrator('V R O R V', 0.001, 1.0, 10, True, 1e-8)
        eng.seed(5)
        assert not eng.propagate(3).any()
        out.append(eng.get_replicas()[:2])
    (xa, va), (xb, vb) = out
    print('max|dx| =', np.abs(xa - xb).max(), ' rms dv / rms v =', np.sqrt(((va - vb) ** 2).mean() / (va ** 2).mean()))
    assert np.abs(xa - xb).max() < 5e-5
    assert np.sqrt(((va - vb) ** 2).mean()) < 2e-3 * np.sqrt((va ** 2).mean())


# ---- d. u_kl ----------------------------------------------------------------------------------------------------------------------------
GLOBALS = np.array([[1.0, 1.0], [0.5, 2.0], [0.2, 1.5]])                           # (lambda_bonds, gamma) of the three states


def test_ukl_carries_the_energy_at_every_states_globals(hip_engine_factory):
    al, xs = _alanine(seed=8)
    xs = _f32(xs)
    f = _bond_force(al.system, lam=1.0, gamma=1.0)
    system = copy.deepcopy(al.system); system.addForce(f)
    labels = np.array([2, 0, 1])
    e0 = hip_engine_factory(); _setup(e0, al.system, xs, global_table=GLOBALS, labels=labels)       # (three states, no custom force)
    u0 = e0.compute_energies()
    e1 = hip_engine_factory(); _setup(e1, system, xs, global_table=GLOBALS, labels=labels)
    u1 = e1.compute_energies()
    E = np.array([[_helper(f, x, global_values=dict(lambda_bonds=g[0], gamma=g[1]))[0].sum() for g in GLOBALS] for x in xs])      # [r][l]
    # without the force every column holds beta U_r; with it beta (U_r + E_r(g_l)): the u_kl share is relative to the own state
    want = BETA * (E - E[np.arange(3), labels][:, None])
    own0, own1 = u0[np.arange(3), labels], u1[np.arange(3), labels]
    got = (u1 - own1[:, None]) - (u0 - own0[:, None])
    print('u_kl share: max |got - want| / max|want| =', np.abs(got - want).max() / np.abs(want).max())
    assert np.allclose(got, want, rtol=1e-5, atol=1e-5 * np.abs(want).max())
    assert np.allclose(own1 - own0, BETA * E[np.arange(3), labels], rtol=1e-5, atol=2e-7 * np.abs(own0).max())
    # equal globals at every state: the share is exactly zero
    e1.set_custom_globals(np.tile(GLOBALS[1], (3, 1)))
    u2 = e1.compute_energies()
    assert np.array_equal(u2 - u2[:, :1], np.zeros((3, 3)))
    # a new set of states: the terms refuse to act on the old globals
    e1.set_states(np.full(3, 1.0 / (KB * 310.0)))
    with pytest.raises(RuntimeError, match='states changed since remd_set_custom_globals'):
        e1.get_forces()
    e1.set_custom_globals(GLOBALS)
    e1.get_forces()


# ---- e. through the public interface ----------------------------------------------------------------------------------------------------
class BondState(states.GlobalParameterState):
    lambda_bonds = states.GlobalParameterState.GlobalParameter('lambda_bonds', standard_value=1.0)
    gamma = states.GlobalParameterState.GlobalParameter('gamma', standard_value=1.0)


def _sampler_run(engine, phases, n_iter=3):
    from openmmtools_amd.multistate import ReplicaExchangeSampler
    al = testsystems.AlanineDipeptideExplicit()
    f = _bond_force(al.system, lam=1.0, gamma=1.0)
    al.system.addForce(f)
    engine.set_phases(phases)
    ts = states.ThermodynamicState(al.system, 300.0)
    sts = states.create_thermodynamic_state_protocol(ts, {'lambda_bonds': list(GLOBALS[:, 0]), 'gamma': list(GLOBALS[:, 1])},
                                                     composable_states=[BondState(lambda_bonds=1.0, gamma=1.0)])
    ss = states.SamplerState(al.positions, box_vectors=al.system.getDefaultPeriodicBoxVectors())
    move = mcmc.LangevinSplittingDynamicsMove(timestep=1.0 * unit.femtosecond, collision_rate=1.0 / unit.picosecond, n_steps=20,
                                              reassign_velocities=True, splitting='V R O R V')
    s = ReplicaExchangeSampler(mcmc_moves=move, number_of_iterations=10 ** 9, engine=engine, seed=0xBEEF)
    s.create(sts, [ss], storage=None)
    out = []
    for _ in range(n_iter):
        s.run(1)
        out.append((np.array(s._replica_thermodynamic_states), np.array(s.energy_thermodynamic_states), engine.get_replicas()[0]))
    return out, engine.phases_active(), f, sts


def test_replica_exchange_over_global_parameter_states(hip_engine_factory):
    one, p1, f, sts = _sampler_run(hip_engine_factory(), 1)
    labels, u, x = one[-1]
    E = np.array([[_helper(f, xr, global_values=dict(lambda_bonds=g[0], gamma=g[1]))[0].sum() for g in GLOBALS] for xr in x])
    want = sts[0].beta * (E - E[:, :1])
    got = u - u[:, :1]
    print('sampler u_kl: max |got - want| / max|want| =', np.abs(got - want).max() / np.abs(want).max())
    assert np.allclose(got, want, rtol=1e-5, atol=1e-5 * np.abs(want).max())
    two, p2, _, _ = _sampler_run(hip_engine_factory(), 2)
    assert (p1, p2) == (1, 2)
    for it, (a, b) in enumerate(zip(one, two)):
        for q, name in enumerate(('labels', 'u_kl', 'positions')):
            assert np.array_equal(a[q], b[q]), (it, name)


# ---- f. neighbours ------------------------------------------------------------------------------------------------------------------------
def _pulled_alanine(group=0):
    al = testsystems.AlanineDipeptideVacuum()
    f = CustomBondForce('0.5*K*r^2'); f.addPerBondParameter('K'); f.addBond(0, 21, [1000.0])
    f.setForceGroup(group)
    al.system.addForce(f)
    x = np.array(al.positions, dtype=np.float64)
    return al, f, x, np.linalg.norm(x[21] - x[0])


def test_multiple_time_step_splitting_and_group_forces(hip_engine_factory):
    al, f, x, r_start = _pulled_alanine(group=2)
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


class LambdaBondsState(states.GlobalParameterState):
    lambda_bonds = states.GlobalParameterState.GlobalParameter('lambda_bonds', standard_value=1.0)


def test_sampler_minimize_lowers_a_custom_bond_energy(hip_engine_factory):
    """sampler.minimize() over two lambda_bonds states: the engine minimises every replica at its own state's globals and the sampler
    states take the minimised positions"""
    from openmmtools_amd.multistate import MultiStateSampler
    al = testsystems.AlanineDipeptideVacuum()
    f = CustomBondForce('lambda_bonds*0.5*K*r^2'); f.addGlobalParameter('lambda_bonds', 1.0); f.addPerBondParameter('K'); f.addBond(0, 21, [1000.0])
    al.system.addForce(f)
    sts = states.create_thermodynamic_state_protocol(states.ThermodynamicState(al.system, 300.0), {'lambda_bonds': [1.0, 0.5]},
                                                     composable_states=[LambdaBondsState(lambda_bonds=1.0)])
    s = MultiStateSampler(mcmc_moves=mcmc.LangevinDynamicsMove(n_steps=1), number_of_iterations=0, engine=hip_engine_factory(),
                          online_analysis_interval=None)
    s.create(sts, [states.SamplerState(al.positions), states.SamplerState(al.positions)], storage=None)       # one replica per state
    assert list(s._replica_thermodynamic_states) == [0, 1]
    x0 = np.array(al.positions, dtype=np.float64)
    before = s._engine.custom_energies()[:, 0]
    want = np.array([1.0, 0.5]) * _helper(f, _f32(x0), global_values=dict(lambda_bonds=1.0))[0].sum()
    assert np.allclose(before, want, rtol=1e-5)                                    # each replica at its own state's lambda_bonds
    s.minimize(max_iterations=200)
    after = s._engine.custom_energies()[:, 0]
    assert np.all(after < 0.5 * before), (before, after)
    for r, st in enumerate(s.sampler_states):
        y = np.asarray(st.positions, dtype=np.float64)
        assert np.linalg.norm(y[21] - y[0]) < np.linalg.norm(x0[21] - x0[0]) - 0.05
        assert 0.5 * 1000.0 * (1.0, 0.5)[r] * np.sum((y[21] - y[0]) ** 2) == pytest.approx(after[r], rel=1e-5)


def test_resident_small_system_path_steps_aside(hip_engine_factory):
    """AlanineDipeptideVacuum (22 atoms, NoCutoff) runs on the resident small-system kernel; with a custom force it takes the general
    step, which the force acts in: the bond between two distant atoms pulls them together within 500 steps"""
    al, f, x, r_start = _pulled_alanine()
    eng = hip_engine_factory()
    _setup(eng, al.system, np.tile(x, (2, 1, 1)))
    eng.set_integrator('V R O R V', 0.001, 5.0, 500, True, 1e-8)
    eng.propagate(0)
    y = eng.get_replicas()[0]
    assert np.all(np.linalg.norm(y[:, 21] - y[:, 0], axis=1) < r_start - 0.15)


def test_resident_lennard_jones_path_steps_aside(hip_engine_factory):
    """216 Lennard-Jones particles (no listed terms, under 1024 atoms) run on the resident Lennard-Jones kernel; with a custom external
    force they take the general step, which the force acts in: a periodic harmonic well 0.5 nm from particle 0 captures it.  Its
    thermal spread in the well is sqrt(3 kT / K) = 0.04 nm; a particle the force did not act on would stay a free flight away."""
    lj = testsystems.LennardJonesFluid(nparticles=216)
    box = np.diag(lj.system.getDefaultPeriodicBoxVectors())
    x = np.array(lj.positions, dtype=np.float64)
    target = x[0] + np.array([0.3, -0.3, 0.27])
    e = CustomExternalForce('0.5*K*periodicdistance(x,y,z,x0,y0,z0)^2')
    e.setUsesPeriodicBoundaryConditions(True); e.addGlobalParameter('K', 5000.0)
    for name in ('x0', 'y0', 'z0'):
        e.addPerParticleParameter(name)
    e.addParticle(0, list(target))
    lj.system.addForce(e)
    eng = hip_engine_factory()
    _setup(eng, lj.system, np.tile(x, (2, 1, 1)), np.tile(box, (2, 1)))
    eng.set_integrator('V R O R V', 0.002, 5.0, 1500, True, 1e-8)
    eng.seed(3)
    eng.propagate(0)
    y = eng.get_replicas()[0]
    d = y[:, 0] - target
    d -= box * np.rint(d / box)
    assert np.all(np.linalg.norm(d, axis=1) < 0.15), np.linalg.norm(d, axis=1)


# ---- every kind in one handle, against the order of the parts ----------------------------------------------------------------------------
def _every_kind(x):
    """one force of each kind over a chain of 65 atoms, in the reverse of the order their parts have in the padded term space: a CMAP
    force, a collective-variable force, a centroid force, a nonbonded force (65 particles: 3 tiles), a compound-bond force, a torsion,
    an angle and a bond force of 65 terms (two wavefronts).  With the external force that is nine, one more than REMD_CUSTOM_MAX_FORCES:
    the engine refuses nine in a handle, so the external force comes back alone, for a second handle"""
    from openmmtools_amd.system import (CMAPTorsionForce, CustomCVForce, RMSDForce, CustomCentroidBondForce, CustomNonbondedForce,
                                        CustomCompoundBondForce)
    n = len(x)
    a = 2.0 * np.pi * np.arange(6) / 6
    cmap = CMAPTorsionForce()
    cmap.addMap(6, (3.0 * np.cos(a[None, :]) + 2.0 * np.sin(a[:, None]) + np.cos(a[None, :] - a[:, None])).reshape(-1))
    cmap.addMap(6, (2.0 * np.sin(2.0 * a[None, :]) - np.cos(a[:, None])).reshape(-1))
    for t in range(0, 30, 3):
        cmap.addTorsion(t % 2, t, t + 1, t + 2, t + 3, t + 1, t + 2, t + 3, t + 4)
    cv = CustomCVForce('40*v^2')
    cv.addCollectiveVariable('v', RMSDForce(x + 0.01 * np.cos(7.0 * x), list(range(40, 52))))
    cen = CustomCentroidBondForce(2, '0.5*k*(distance(g1,g2)-d0)^2')
    cen.addPerBondParameter('k'); cen.addPerBondParameter('d0')
    for atoms in ([52, 53, 54], [55, 56], [57, 58, 59, 60]):
        cen.addGroup(atoms)
    cen.addBond([0, 1], [300.0, 0.3]); cen.addBond([1, 2], [200.0, 0.4])
    nb = CustomNonbondedForce('a1*a2*exp(-r/0.08)')
    nb.addPerParticleParameter('a')
    for i in range(n):
        nb.addParticle([1.0 + 0.01 * i])
    for i in range(n - 1):
        nb.addExclusion(i, i + 1)
    comp = CustomCompoundBondForce(3, '0.5*k*(distance(p1,p3)-0.25)^2+angle(p1,p2,p3)')
    comp.addPerBondParameter('k')
    for t in range(0, 60, 4):
        comp.addBond([t, t + 1, t + 2], [50.0 + t])
    tor = CustomTorsionForce('k*(1+cos(2*theta-0.3))'); tor.addPerTorsionParameter('k')
    for t in range(0, 61, 5):
        tor.addTorsion(t, t + 1, t + 2, t + 3, [2.0 + 0.1 * t])
    ang = CustomAngleForce('0.5*k*(theta-1.9)^2'); ang.addPerAngleParameter('k')
    for t in range(0, 63, 2):
        ang.addAngle(t, t + 1, t + 2, [80.0])
    bond = CustomBondForce('0.5*k*(r-r0)^2'); bond.addPerBondParameter('k'); bond.addPerBondParameter('r0')
    for t in range(n - 1):
        bond.addBond(t, t + 1, [20000.0, 0.15])
    bond.addBond(0, 2, [500.0, 0.25])
    ext = CustomExternalForce('2*(x^2+y^2+z^2)')
    for i in range(n):
        ext.addParticle(i, [])
    return [cmap, cv, cen, nb, comp, tor, ang, bond], ext


def _chain_handle(factory, x, customs, phases=0, R=6):
    """a NoCutoff system of 65 atoms (a NonbondedForce beside the custom forces: the general NoCutoff step) at 6 replicas"""
    from openmmtools_amd.system import NonbondedForce
    s = System()
    for _ in range(len(x)):
        s.addParticle(12.0)
    nbf = NonbondedForce(); nbf.setNonbondedMethod(NonbondedForce.NoCutoff)
    for i in range(len(x)):
        nbf.addParticle(0.05 * (-1) ** i, 0.1, 0.2)
    for i in range(len(x) - 1):
        nbf.addException(i, i + 1, 0.0, 0.1, 0.0)
    s.addForce(nbf)
    for f in customs:
        s.addForce(copy.deepcopy(f))
    desc = system_to_desc(s)
    eng = factory()
    if phases:
        eng.set_phases(phases)
    eng.set_system(desc)
    eng.set_states(1.0 / (KB * np.linspace(300.0, 330.0, R)))
    eng.set_custom_globals(np.zeros((R, 0)))
    eng.set_integrator('V R R O R R V', 0.001, 1.0, 20, True, 1e-8)
    eng.seed(11)
    xs = _f32(np.stack([x + 0.002 * r * np.sin(5.0 * x + r) for r in range(R)]))
    eng.set_replicas(R, 0, xs, None, np.zeros((R, 3)), np.arange(R))
    return eng, desc


def test_every_kind_in_one_handle_against_the_part_order(hip_engine_factory):
    """Eight kinds in one handle, the descriptors in the reverse of the order of their parts in the padded term space, the bond force
    crossing a wavefront boundary (65 terms); the external force sits in a second handle (a handle takes REMD_CUSTOM_MAX_FORCES = 8).
    Each column of custom_energies() equals, bit for bit, the energy of the same force alone in a handle of its own: the reduction adds
    a force's wavefront partials in an order that does not depend on where its slots lie.  And with remd_set_phases(1) and (2) the
    columns and the positions after a short propagation are bit-identical (the check of tests/test_phases_gpu.py): the second block's
    tables are a clone of the first's"""
    import cmap_oracle
    x = cmap_oracle.chain_positions(65, replicas=1, seed=3, special=False)[0].astype(np.float64)
    customs, ext = _every_kind(x)
    eng, desc = _chain_handle(hip_engine_factory, x, customs)
    kinds = [t['kind'] for _, t in sorted(desc['custom_terms'].items())]
    assert kinds == [cx.KIND_CMAP, cx.KIND_CV, cx.KIND_CENTROID, cx.KIND_NONBONDED, cx.KIND_COMPOUND, cx.KIND_TORSION, cx.KIND_ANGLE, cx.KIND_BOND]
    assert len(desc['custom_terms']['007']['atoms']) == 65
    E = eng.custom_energies()
    assert E.shape == (6, 8) and np.all(np.isfinite(E)) and np.all(np.abs(E).min(axis=0) > 0.0)
    for k, f in enumerate(customs):
        alone = _chain_handle(hip_engine_factory, x, [f])[0].custom_energies()
        assert alone.shape == (6, 1) and np.array_equal(alone[:, 0], E[:, k]), (k, alone[:, 0], E[:, k])
    both = _chain_handle(hip_engine_factory, x, [ext, customs[7]])[0].custom_energies()       # the second handle: the external force, beside the bonds
    assert np.array_equal(both[:, 1], E[:, 7]) and np.array_equal(both[:, 0], _chain_handle(hip_engine_factory, x, [ext])[0].custom_energies()[:, 0])
    out = []
    for phases in (1, 2):
        e = _chain_handle(hip_engine_factory, x, customs, phases)[0]
        for it in range(2):
            assert not e.propagate(it).any()
            u = e.compute_energies()
        xs, vs = e.get_replicas()[:2]
        out.append((xs.copy(), vs.copy(), u.copy(), e.custom_energies(), e.phases_active()))
    assert out[0][4] == 1 and out[1][4] == 2
    for p, q in zip(out[0][:4], out[1][:4]):
        assert np.array_equal(p, q)
    assert np.all(np.isfinite(out[0][0])) and not np.array_equal(out[0][3], E)
