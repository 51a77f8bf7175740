"""GPU: energy parameter derivatives of the custom forces (addEnergyParameterDerivative, HipEngine.custom_energy_parameter_derivatives;
csrc/custom_machine.h's derivative mode and the *_dpar launches) against the dual-number oracle tests/custom_param_derivative_oracle.py.

Bound: the device evaluates in f64 from the same f32 positions the oracle gets, so a derivative lies within 1e-11 sum_t |dE_t/dglobal|
of the oracle's (the project's bound for the machine's energies, here over the per-term derivatives); an exact zero is asserted as
equality.  No test sits where a term's own derivative cancels to within 1e-5 of its parts, so the per-term form is the bound everywhere.
Every test prints error / bound before it asserts."""
import copy

import numpy as np
import pytest

import custom_dual_oracle as dual
import custom_hbond_oracle
import custom_manyparticle_oracle
import custom_param_derivative_oracle as oracle
from openmmtools_amd.system import (System, system_to_desc, CustomBondForce, CustomAngleForce, CustomTorsionForce, CustomExternalForce,
                                    CustomCompoundBondForce, CustomCentroidBondForce, CustomHbondForce, CustomManyParticleForce,
                                    NonbondedForce, Continuous1DFunction, Continuous2DFunction, Discrete1DFunction)

pytestmark = pytest.mark.gpu

KB = 0.008314462618153242
BETA = 1.0 / (KB * 300.0)


def _f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def _system(n, forces, box=None):
    s = System()
    for _ in range(n):
        s.addParticle(12.0)
    if box is not None:
        s.setDefaultPeriodicBoxVectors([box[0], 0, 0], [0, box[1], 0], [0, 0, box[2]])
    for f in forces:
        s.addForce(f)
    return s


def _handle(factory, system, xs, boxes=None, states=None, labels=None):
    """an engine holding ``system`` at the positions xs [R][N][3]; states: a list of dicts global name -> value (default: one state of
    the defaults).  Returns (engine, names of the global columns, [K] dicts of every state's globals)."""
    desc = system_to_desc(system, box=None if boxes is None else boxes[0])
    engine = factory()
    engine.set_system(desc)
    names = list(desc['custom_globals']['names'])
    defaults = dict(zip(names, desc['custom_globals']['defaults']))
    table = [dict(defaults, **s) for s in (states or [{}])]
    engine.set_states(np.full(len(table), BETA))
    engine.set_custom_globals(np.array([[t[n] for n in names] for t in table]).reshape(len(table), len(names)))
    R = len(xs)
    labels = np.zeros(R, dtype=np.int64) if labels is None else np.asarray(labels, dtype=np.int64)
    engine.set_replicas(R, 0, xs, None, np.zeros((R, 3)) if boxes is None else boxes, labels)
    return engine, names, [table[int(l)] for l in labels]


def _own(force, g):
    return {force.getGlobalParameterName(i): g[force.getGlobalParameterName(i)] for i in range(force.getNumGlobalParameters())}


def _simple(force, kind, g, wrt, x, box=None, functions=None):
    atoms, params = force._term_arrays()
    return oracle.evaluate(kind, force.getEnergyFunction(), atoms, list(force._per_bond), params, _own(force, g), wrt, x, box,
                           force.usesPeriodicBoundaryConditions(), functions)


def _compound(force, g, wrt, x, box=None):
    atoms, params = force._term_arrays()
    return oracle.evaluate(None, force.getEnergyFunction(), atoms, list(force._per_bond), params, _own(force, g), wrt, x, box,
                           force.usesPeriodicBoundaryConditions(), n_particles=force.getNumParticlesPerBond())


def _close(tag, got, refs):
    """got against the sum of the oracle results ``refs`` (the forces that declared the parameter)"""
    want, bound = sum(r['total'] for r in refs), sum(r['bound'] for r in refs)
    print('%s: device %.17g oracle %.17g, |error| / bound = %.3g' % (tag, got, want, abs(got - want) / max(bound, 1e-300)))
    assert np.isfinite(got) and abs(got - want) <= bound
    return abs(got - want) / max(bound, 1e-300)


# ---- 1. the four one-variable kinds: 65 terms each, 3 replicas in 3 different states of a 4-state ladder -----------------------------------
def _one_variable_forces():
    rng = np.random.default_rng(4101)
    N = 68
    x = np.cumsum(rng.normal(0.0, 0.08, (N, 3)) + np.array([0.1, 0.0, 0.0]), axis=0)
    b = CustomBondForce('lam_b*0.5*k*(r-r0)^2'); b.addGlobalParameter('lam_b', 1.0); b.addPerBondParameter('k'); b.addPerBondParameter('r0')
    a = CustomAngleForce('lam_a^2*k*(theta-t0)^2'); a.addGlobalParameter('lam_a', 1.0); a.addPerAngleParameter('k'); a.addPerAngleParameter('t0')
    t = CustomTorsionForce('k*(1+cos(lam_t*theta-ph))'); t.addGlobalParameter('lam_t', 1.0); t.addPerTorsionParameter('k'); t.addPerTorsionParameter('ph')
    e = CustomExternalForce('lam_e*k*((x-x0)^2+y^2)+exp(-lam_e*z*z)'); e.addGlobalParameter('lam_e', 1.0); e.addPerParticleParameter('k'); e.addPerParticleParameter('x0')
    for i in range(65):
        b.addBond(i, i + 1, [rng.uniform(1e3, 3e3), rng.uniform(0.1, 0.2)])
        a.addAngle(i, i + 1, i + 2, [rng.uniform(50.0, 90.0), rng.uniform(1.5, 2.2)])
        t.addTorsion(i, i + 1, i + 2, i + 3, [rng.uniform(2.0, 9.0), rng.uniform(-3.0, 3.0)])
        e.addParticle(i, [rng.uniform(5.0, 9.0), rng.uniform(0.0, 5.0)])
    xs = _f32([x + rng.normal(0.0, 0.005, x.shape) for _ in range(3)])
    return [b, a, t, e], xs


LADDER = [dict(lam_b=v, lam_a=1.5 - v, lam_t=0.5 + v, lam_e=0.3 * v + 0.1) for v in (0.2, 0.5, 0.8, 1.0)]
KINDS = [dual.KIND_BOND, dual.KIND_ANGLE, dual.KIND_TORSION, dual.KIND_EXTERNAL]


def test_one_variable_kinds_at_each_replicas_own_state(hip_engine_factory):
    forces, xs = _one_variable_forces()
    for f in forces:
        f.addEnergyParameterDerivative(f.getGlobalParameterName(0))
    eng, names, own = _handle(hip_engine_factory, _system(68, forces), xs, states=LADDER, labels=[0, 2, 3])
    assert eng.custom_derivative_names == ['lam_b', 'lam_a', 'lam_t', 'lam_e']
    D = eng.custom_energy_parameter_derivatives()
    assert D.shape == (3, 4)
    for r in range(3):
        for c, (f, kind) in enumerate(zip(forces, KINDS)):
            ref = _simple(f, kind, own[r], eng.custom_derivative_names[c], xs[r])
            assert len(ref['dE']) == 65 and ref['scale'] > 0.0
            _close('replica %d %s' % (r, eng.custom_derivative_names[c]), D[r, c], [ref])
    # reproducibility: a second call gives the same bits; a derivative's bits do not depend on which others share the call
    assert np.array_equal(D, eng.custom_energy_parameter_derivatives())
    alone, _ = _one_variable_forces()
    alone[0].addEnergyParameterDerivative('lam_b')
    e2, _, _ = _handle(hip_engine_factory, _system(68, alone), xs, states=LADDER, labels=[0, 2, 3])
    D2 = e2.custom_energy_parameter_derivatives()
    assert D2.shape == (3, 1) and np.array_equal(D2[:, 0], D[:, 0])


def test_identical_globals_in_every_state_still_give_the_derivative(hip_engine_factory):
    """every state carries the same globals (the u_kl share is skipped as exactly zero): the derivative is not zero and is computed"""
    forces, xs = _one_variable_forces()
    forces[0].addEnergyParameterDerivative('lam_b')
    eng, names, own = _handle(hip_engine_factory, _system(68, forces), xs, states=[LADDER[1]] * 4, labels=[0, 2, 3])
    D = eng.custom_energy_parameter_derivatives()
    for r in range(3):
        ref = _simple(forces[0], dual.KIND_BOND, own[r], 'lam_b', xs[r])
        assert abs(ref['total']) > 1.0
        _close('replica %d' % r, D[r, 0], [ref])


# ---- 2. every way a global can enter a program -------------------------------------------------------------------------------------------
T1 = [np.sin(0.7 * k) + 0.1 * k for k in range(9)]
GX, HY = [1.0 + 0.3 * np.cos(1.1 * k) for k in range(6)], [0.5 + 0.2 * k * k for k in range(5)]
OPCODE_CASES = [                                       # (energy, globals)
    ('c*r + (r-off)^2', dict(c=2.5, off=0.27)),
    ('r^ex', dict(ex=2.3)),
    ('exp(-a*r) + cos(a2*r)', dict(a=1.7, a2=4.0)),
    ('min(m*r, 1) + max(m2*r, 1) + min(tie*r, r) + 3*max(tie*r, r)', dict(m=3.0, m2=3.5, tie=1.0)),
    ('select(step(r-0.3), s*r, 2*s*r^2)', dict(s=1.3)),
    ('t1(q*r) + t2(q2*r, 0.5+r) + lk(idx)*r', dict(q=2.0, q2=1.5, idx=2.0)),
    ('u*u2; u = g*r; u2 = g + r', dict(g=0.8)),
]
LENGTHS = [0.12, 0.22, 0.29, 0.31, 0.38, 0.47]


def _opcode_forces():
    forces = []
    for energy, g in OPCODE_CASES:
        f = CustomBondForce(energy)
        for n, v in g.items():
            f.addGlobalParameter(n, v)
            f.addEnergyParameterDerivative(n)
        if 't1(' in energy:
            f.addTabulatedFunction('t1', Continuous1DFunction(T1, 0.0, 1.2))
            f.addTabulatedFunction('t2', Continuous2DFunction(6, 5, [gx * hy for hy in HY for gx in GX], 0.0, 1.0, 0.5, 1.0))
            f.addTabulatedFunction('lk', Discrete1DFunction([4.0, 5.0, 7.0, 1.0]))
        for k in range(len(LENGTHS)):
            f.addBond(2 * k, 2 * k + 1)
        forces.append(f)
    return forces


def test_a_global_through_every_kind_of_opcode(hip_engine_factory):
    forces = _opcode_forces()
    x = np.zeros((2 * len(LENGTHS), 3))
    for k, L in enumerate(LENGTHS):
        x[2 * k] = [k, 0.0, 0.0]
        x[2 * k + 1] = [k + L * 0.6, L * 0.8, 0.0]
    xs = _f32([x])
    functions = dict(t1=oracle.continuous1d(T1, 0.0, 1.2), t2=oracle.separable2d(GX, 0.0, 1.0, HY, 0.5, 1.0), lk=oracle.discrete1d([4.0, 5.0, 7.0, 1.0]))
    eng, names, own = _handle(hip_engine_factory, _system(len(x), forces), xs)
    D = eng.custom_energy_parameter_derivatives()[0]
    r = np.linalg.norm(xs[0][1::2] - xs[0][0::2], axis=1)
    assert (3.0 * r < 1).any() and (3.0 * r > 1).any() and (3.5 * r < 1).any() and (3.5 * r > 1).any()      # both arms of min and max
    assert (r < 0.3).any() and (r > 0.3).any()                                                                # both arms of select
    assert (2.0 * r).max() < 1.2 and (1.5 * r).max() < 1.0 and (0.5 + r).max() < 1.0                             # inside the tables
    got = dict(zip(eng.custom_derivative_names, D))
    for f, (energy, g) in zip(forces, OPCODE_CASES):
        for n in g:
            ref = _simple(f, dual.KIND_BOND, own[0], n, xs[0], functions=functions)
            if n in ('tie', 'idx'):
                # the tie: tie*r == r exactly at tie = 1, min and max take the second operand (x < y, x > y both false): derivative 0;
                # the index of a lookup has derivative 0
                assert ref['total'] == 0.0 and got[n] == 0.0, (n, got[n], ref['total'])
                print('%s: exactly 0 on both sides' % n)
            else:
                assert ref['scale'] > 0.0
                _close(n, got[n], [ref])


# ---- 3. who contributes: only a force that declared the parameter ----------------------------------------------------------------------------
def _two_bond_forces(declare_second):
    rng = np.random.default_rng(4103)
    f1, f2 = CustomBondForce('lam*k*r^2'), CustomBondForce('0.5*lam^2*(r-0.1)^2')
    f1.addGlobalParameter('lam', 0.6); f1.addGlobalParameter('unused', 3.0); f1.addPerBondParameter('k')
    f2.addGlobalParameter('lam', 0.6)
    for i in range(5):
        f1.addBond(i, i + 1, [rng.uniform(10.0, 20.0)])
        f2.addBond(i, i + 2)
    f1.addEnergyParameterDerivative('unused'); f1.addEnergyParameterDerivative('lam')
    if declare_second:
        f2.addEnergyParameterDerivative('lam')
    return [f1, f2], _f32([rng.uniform(0.0, 0.6, (7, 3))])


@pytest.mark.parametrize('declare_second', [False, True])
def test_only_the_forces_that_declared_a_parameter_contribute(hip_engine_factory, declare_second):
    forces, xs = _two_bond_forces(declare_second)
    eng, names, own = _handle(hip_engine_factory, _system(7, forces), xs)
    assert eng.custom_derivative_names == ['unused', 'lam']
    D = eng.custom_energy_parameter_derivatives()[0]
    assert D[0] == 0.0                                   # a declared global that the expression does not name: exactly 0
    refs = [_simple(f, dual.KIND_BOND, own[0], 'lam', xs[0]) for f in forces]
    assert abs(refs[1]['total']) > 1e-3 * abs(refs[0]['total'])
    _close('lam', D[1], refs if declare_second else refs[:1])


# ---- 4. compound bonds: a Boresch restraint, also across the box ----------------------------------------------------------------------------
BORESCH = ('lambda_restraints*0.5*(K_r*(distance(p3,p4)-r_aA0)^2 + K_thetaA*(angle(p2,p3,p4)-theta_A0)^2 + K_thetaB*(angle(p3,p4,p5)-theta_B0)^2'
           ' + K_phi*(2-cos(dihedral(p1,p2,p3,p4)-phi_A0)-cos(dihedral(p3,p4,p5,p6)-phi_C0)))')
BORESCH_GLOBALS = dict(lambda_restraints=0.7, K_r=4184.0, r_aA0=0.45, K_thetaA=41.84, theta_A0=1.9, K_thetaB=41.84, theta_B0=1.4, K_phi=30.0,
                       phi_A0=0.3, phi_C0=-1.1)


@pytest.mark.parametrize('periodic', [False, True])
def test_boresch_compound_bond(hip_engine_factory, periodic):
    f = CustomCompoundBondForce(6, BORESCH)
    for n, v in BORESCH_GLOBALS.items():
        f.addGlobalParameter(n, v)
    f.addBond([0, 1, 2, 3, 4, 5])
    f.setUsesPeriodicBoundaryConditions(periodic)
    for n in ('lambda_restraints', 'K_r', 'theta_A0'):
        f.addEnergyParameterDerivative(n)
    x = np.array([[0.0, 0.0, 0.0], [0.15, 0.02, 0.0], [0.22, 0.14, 0.03], [0.6, 0.3, 0.1], [0.72, 0.25, 0.2], [0.8, 0.36, 0.27]]) + 0.4
    box = np.array([2.0, 2.1, 2.2])
    if periodic:
        x[3:] -= box                                     # the ligand's three atoms in the neighbouring cell: the bond crosses the boundary
    xs, boxes = _f32([x]), _f32([box])
    eng, names, own = _handle(hip_engine_factory, _system(6, [f], box if periodic else None), xs, boxes if periodic else None)
    D = eng.custom_energy_parameter_derivatives()[0]
    for c, n in enumerate(eng.custom_derivative_names):
        ref = _compound(f, own[0], n, xs[0], boxes[0])
        assert ref['scale'] > 0.0
        _close(n, D[c], [ref])
    if periodic:                                         # the images matter: without them the oracle gives something else
        far = oracle.evaluate(None, BORESCH, [[0, 1, 2, 3, 4, 5]], [], np.zeros((1, 0)), own[0], 'K_r', xs[0], None, False, n_particles=6)
        assert abs(far['total'] - D[1]) > 1e-3 * abs(D[1])


# ---- 5. centroid bonds: groups of 3 and 5 atoms, one wrapped across the box --------------------------------------------------------------------
def test_centroid_bond_with_a_wrapped_group(hip_engine_factory):
    f = CustomCentroidBondForce(2, '0.5*kc*(distance(g1,g2)-d0)^2')
    f.addGlobalParameter('kc', 800.0); f.addGlobalParameter('d0', 0.35)
    f.addGroup([0, 1, 2]); f.addGroup([3, 4, 5, 6, 7])
    f.addBond([0, 1])
    f.setUsesPeriodicBoundaryConditions(True)
    f.addEnergyParameterDerivative('kc'); f.addEnergyParameterDerivative('d0')
    rng = np.random.default_rng(4105)
    box = np.array([2.0, 2.2, 2.4])
    x = np.concatenate([rng.uniform(0.05, 0.25, (3, 3)), rng.uniform(0.5, 0.8, (5, 3))])
    x[4] += [box[0], 0.0, 0.0]; x[6] -= [0.0, box[1], 0.0]      # two atoms of the second group sit in other cells
    xs, boxes = _f32([x]), _f32([box])
    eng, names, own = _handle(hip_engine_factory, _system(8, [f], box), xs, boxes)
    D = eng.custom_energy_parameter_derivatives()[0]
    groups = [([0, 1, 2], [1.0 / 3] * 3), ([3, 4, 5, 6, 7], [0.2] * 5)]
    for c, n in enumerate(('kc', 'd0')):
        ref = oracle.evaluate_centroid(2, f.getEnergyFunction(), groups, [[0, 1]], [], np.zeros((1, 0)), own[0], n, xs[0], boxes[0], True)
        assert ref['scale'] > 0.0
        _close(n, D[c], [ref])
    unwrapped = oracle.evaluate_centroid(2, f.getEnergyFunction(), groups, [[0, 1]], [], np.zeros((1, 0)), own[0], 'kc', xs[0], None, False)
    assert abs(unwrapped['total'] - D[0]) > 1e-3 * abs(D[0])


# ---- 6. donor-acceptor pairs: 5 x 7, an exclusion, a cutoff that removes some ------------------------------------------------------------------
def test_donor_acceptor_force(hip_engine_factory):
    rng = np.random.default_rng(4106)
    f = CustomHbondForce('scale*kd*ka*(distance(d1,a1)-0.3)^2*(1+cos(angle(d2,d1,a1)))^w')
    f.addGlobalParameter('scale', 1.2); f.addGlobalParameter('w', 1.5)
    f.addPerDonorParameter('kd'); f.addPerAcceptorParameter('ka')
    for k in range(5):
        f.addDonor(2 * k, 2 * k + 1, -1, [rng.uniform(50.0, 90.0)])
    for k in range(7):
        f.addAcceptor(10 + k, -1, -1, [rng.uniform(0.5, 1.5)])
    f.addExclusion(1, 2)
    f.setNonbondedMethod(CustomHbondForce.CutoffNonPeriodic)
    f.setCutoffDistance(0.6)
    f.addEnergyParameterDerivative('scale'); f.addEnergyParameterDerivative('w')
    xs = _f32([rng.uniform(0.0, 0.9, (17, 3))])
    donors = [f.getDonorParameters(k) for k in range(5)]
    acceptors = [f.getAcceptorParameters(k) for k in range(7)]
    args = ([d[:3] for d in donors], [a[:3] for a in acceptors], [d[3] for d in donors], [a[3] for a in acceptors])
    eng, names, own = _handle(hip_engine_factory, _system(17, [f]), xs)
    member = custom_hbond_oracle.evaluate(f.getEnergyFunction(), ['kd'], ['ka'], *args, own[0], xs[0], None, 1, 0.6, [(1, 2)])
    assert custom_hbond_oracle.clear_of_cutoff(member, 0.6, 1e-6)                 # no pair within 1e-6 nm of the cutoff: checked on the CPU
    assert 0 < len(member['i']) < 34 and member['r_all'].max() > 0.6
    D = eng.custom_energy_parameter_derivatives()[0]
    for c, n in enumerate(('scale', 'w')):
        ref = oracle.evaluate_hbond(f.getEnergyFunction(), ['kd'], ['ka'], *args, own[0], n, list(zip(member['i'], member['j'])), xs[0])
        assert ref['scale'] > 0.0
        _close(n, D[c], [ref])


# ---- 7. sets of three: 27 particles, both permutation modes, a type filter ---------------------------------------------------------------------
MW = 'lam3*eps1*exp(-3*(distance(p1,p2)+distance(p1,p3)))*(cos(angle(p2,p1,p3))+1/3)^2'


@pytest.mark.parametrize('mode', [CustomManyParticleForce.SinglePermutation, CustomManyParticleForce.UniqueCentralParticle])
def test_many_particle_force(hip_engine_factory, mode):
    rng = np.random.default_rng(4107)
    grid = np.array([[i, j, k] for i in range(3) for j in range(3) for k in range(3)], dtype=np.float64) * 0.3
    xs = _f32([grid + rng.uniform(-0.04, 0.04, grid.shape)])
    f = CustomManyParticleForce(3, MW)
    f.addGlobalParameter('lam3', 0.9); f.addPerParticleParameter('eps')
    eps, types = rng.uniform(20.0, 30.0, 27), [k % 2 for k in range(27)]
    for k in range(27):
        f.addParticle([eps[k]], types[k])
    f.setPermutationMode(mode)
    f.setNonbondedMethod(CustomManyParticleForce.CutoffNonPeriodic)
    f.setCutoffDistance(0.45)
    f.setTypeFilter(0, [0])
    f.addEnergyParameterDerivative('lam3')
    eng, names, own = _handle(hip_engine_factory, _system(27, [f]), xs)
    member = custom_manyparticle_oracle.evaluate(MW, ['eps'], eps[:, None], types, [[0], [], []], own[0], xs[0], None, 1, 0.45, (), mode)
    assert custom_manyparticle_oracle.clear_of_cutoff(member, 0.45, 1e-6) and len(member['sets']) > 64
    D = eng.custom_energy_parameter_derivatives()[0]
    ref = oracle.evaluate_manyparticle(MW, ['eps'], eps[:, None], own[0], 'lam3', member['sets'], xs[0])
    assert ref['scale'] > 0.0
    _close('lam3 mode %d (%d sets)' % (mode, len(member['sets'])), D[0], [ref])


# ---- 8. a declaration changes nothing else ---------------------------------------------------------------------------------------------------
def test_a_declaration_leaves_energies_forces_and_u_kl_rows_as_they_are(hip_engine_factory):
    out = []
    for declare in (False, True):
        forces, xs = _one_variable_forces()
        if declare:
            forces[0].addEnergyParameterDerivative('lam_b'); forces[3].addEnergyParameterDerivative('lam_e')
        eng, _, _ = _handle(hip_engine_factory, _system(68, forces), xs, states=LADDER, labels=[0, 2, 3])
        if declare:
            eng.custom_energy_parameter_derivatives()
        out.append((eng.custom_energies(), eng.get_forces(), eng.compute_energies()))
        if not declare:
            with pytest.raises(ValueError, match='no custom force of the system declares an energy parameter derivative'):
                eng.custom_energy_parameter_derivatives()
    for p, q in zip(*out):
        assert np.array_equal(p, q)


# ---- 9. a propagation in two blocks ------------------------------------------------------------------------------------------------------------
def _chain_engine(factory, forces, x, phases):
    s = System()
    for _ in range(len(x)):
        s.addParticle(12.0)
    nbf = NonbondedForce(); nbf.setNonbondedMethod(NonbondedForce.NoCutoff)
    for i in range(len(x)):
        nbf.addParticle(0.05 * (-1) ** i, 0.1, 0.2)
    for i in range(len(x) - 1):
        nbf.addException(i, i + 1, 0.0, 0.1, 0.0)
    s.addForce(nbf)
    for f in forces:
        s.addForce(copy.deepcopy(f))
    eng = factory()
    eng.set_phases(phases)
    eng.set_system(system_to_desc(s))
    R = 6
    eng.set_states(1.0 / (KB * np.linspace(300.0, 330.0, R)))
    eng.set_custom_globals(np.tile([0.2, 0.5, 0.8, 1.0, 0.4, 0.6], (1, 1)).T)
    eng.set_integrator('V R R O R R V', 0.001, 1.0, 20, True, 1e-8)
    eng.seed(11)
    xs = _f32(np.stack([x + 0.002 * r * np.sin(5.0 * x + r) for r in range(R)]))
    eng.set_replicas(R, 0, xs, None, np.zeros((R, 3)), np.arange(R))
    return eng


def test_after_a_propagation_in_two_blocks(hip_engine_factory):
    forces, xs = _one_variable_forces()
    bond = forces[0]
    bond.addEnergyParameterDerivative('lam_b')
    out = []
    for phases in (1, 2):
        eng = _chain_engine(hip_engine_factory, [bond], xs[0], phases)
        assert not eng.propagate(0).any()
        out.append((eng.get_replicas()[0].copy(), eng.custom_energy_parameter_derivatives(), eng.phases_active()))
    assert out[0][2] == 1 and out[1][2] == 2
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    lam = [0.2, 0.5, 0.8, 1.0, 0.4, 0.6]
    for r in range(6):
        ref = _simple(bond, dual.KIND_BOND, dict(lam_b=lam[r]), 'lam_b', _f32(out[1][0][r]))
        _close('replica %d' % r, out[1][1][r, 0], [ref])
