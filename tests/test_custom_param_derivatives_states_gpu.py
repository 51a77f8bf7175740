"""GPU: energy parameter derivatives of the custom forces under EVERY state's globals
(HipEngine.custom_energy_parameter_derivatives_at_states; the STATES instantiations of the *_dpar kernels) against the dual-number
oracle tests/custom_param_derivative_oracle.py evaluated at state l's globals, and thermodynamic integration end to end.

Bound: that of tests/test_custom_param_derivatives_gpu.py -- |device - oracle| <= 1e-11 sum_t |dE_t/dglobal| -- and an exact zero is
asserted as equality.  Every test prints error / bound before it asserts."""
import numpy as np
import pytest

import custom_dual_oracle as dual
import custom_hbond_oracle
import custom_manyparticle_oracle
import custom_param_derivative_oracle as oracle
from test_custom_param_derivatives_gpu import (_f32, _system, _handle, _simple, _compound, _close, _one_variable_forces, _two_bond_forces,
                                               LADDER, KINDS, BORESCH, BORESCH_GLOBALS, MW, BETA)
from openmmtools_amd import states, mcmc, unit
from openmmtools_amd.system import (System, CustomBondForce, CustomExternalForce, CustomCompoundBondForce, CustomCentroidBondForce,
                                    CustomHbondForce, CustomManyParticleForce)

pytestmark = pytest.mark.gpu


def _tables(own, ladder):
    """every state's globals: the defaults (as the first replica's own table carries them) under the state's own values"""
    return [dict(own[0], **s) for s in ladder]


def _bit_equal(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


# ---- 1. the four one-variable kinds: 65 terms each, 3 replicas at labels [0, 2, 3] of the 4-state ladder ------------------------------------
def test_one_variable_kinds_at_every_state(hip_engine_factory):
    forces, xs = _one_variable_forces()
    for f in forces:
        f.addEnergyParameterDerivative(f.getGlobalParameterName(0))
    labels = [0, 2, 3]
    eng, names, own = _handle(hip_engine_factory, _system(68, forces), xs, states=LADDER, labels=labels)
    table = _tables(own, LADDER)
    D = eng.custom_energy_parameter_derivatives_at_states()
    assert D.shape == (3, 4, 4) and eng.custom_derivative_names == ['lam_b', 'lam_a', 'lam_t', 'lam_e']
    for r in range(3):
        for l in range(4):
            for c, (f, kind) in enumerate(zip(forces, KINDS)):
                ref = _simple(f, kind, table[l], eng.custom_derivative_names[c], xs[r])
                assert len(ref['dE']) == 65 and ref['scale'] > 0.0
                _close('replica %d state %d %s' % (r, l, eng.custom_derivative_names[c]), D[r, l, c], [ref])
    own_state = eng.custom_energy_parameter_derivatives()
    for r in range(3):
        assert _bit_equal(D[r, labels[r]], own_state[r])              # the replica's own state: the own-state call, to the bit
    assert _bit_equal(D, eng.custom_energy_parameter_derivatives_at_states())      # a second call: the same bits
    alone, _ = _one_variable_forces()
    alone[0].addEnergyParameterDerivative('lam_b')
    e2, _, _ = _handle(hip_engine_factory, _system(68, alone), xs, states=LADDER, labels=labels)
    D2 = e2.custom_energy_parameter_derivatives_at_states()
    assert D2.shape == (3, 4, 1) and _bit_equal(D2[:, :, 0], D[:, :, 0])         # declared alone: the bits it has among four


# ---- 2. the other families, all states against the oracle ---------------------------------------------------------------------------------------
def _check_own_state(eng, D, labels):
    own_state = eng.custom_energy_parameter_derivatives()
    for r, l in enumerate(labels):
        assert _bit_equal(D[r, l], own_state[r])


def test_compound_bonds_across_a_wavefront_and_a_boresch_bond(hip_engine_factory):
    rng = np.random.default_rng(5201)
    pair = CustomCompoundBondForce(2, 'lam2*0.5*k*(distance(p1,p2)-r0)^2')
    pair.addGlobalParameter('lam2', 1.0); pair.addPerBondParameter('k'); pair.addPerBondParameter('r0')
    for i in range(65):
        pair.addBond([6 + i, 7 + i], [rng.uniform(1e3, 3e3), rng.uniform(0.1, 0.2)])
    pair.addEnergyParameterDerivative('lam2')
    bor = CustomCompoundBondForce(6, BORESCH)
    for n, v in BORESCH_GLOBALS.items():
        bor.addGlobalParameter(n, v)
    bor.addBond([0, 1, 2, 3, 4, 5])
    bor.addEnergyParameterDerivative('lambda_restraints'); bor.addEnergyParameterDerivative('theta_A0')
    six = np.array([[0.0, 0.0, 0.0], [0.15, 0.02, 0.0], [0.22, 0.14, 0.03], [0.6, 0.3, 0.1], [0.72, 0.25, 0.2], [0.8, 0.36, 0.27]]) + 0.4
    chain = np.cumsum(rng.normal(0.0, 0.08, (66, 3)) + [0.1, 0.0, 0.0], axis=0) + 2.0
    x = np.concatenate([six, chain])
    xs = _f32([x + rng.normal(0.0, 0.004, x.shape) for _ in range(2)])
    ladder = [dict(lam2=v, lambda_restraints=1.0 - 0.3 * k, theta_A0=1.9 + 0.05 * k) for k, v in enumerate((0.2, 0.5, 0.8, 1.0))]
    labels = [1, 3]
    eng, names, own = _handle(hip_engine_factory, _system(72, [pair, bor]), xs, states=ladder, labels=labels)
    table = _tables(own, ladder)
    D = eng.custom_energy_parameter_derivatives_at_states()
    assert D.shape == (2, 4, 3) and eng.custom_derivative_names == ['lam2', 'lambda_restraints', 'theta_A0']
    for r in range(2):
        for l in range(4):
            for c, (f, n) in enumerate(((pair, 'lam2'), (bor, 'lambda_restraints'), (bor, 'theta_A0'))):
                ref = _compound(f, table[l], n, xs[r])
                assert ref['scale'] > 0.0
                _close('replica %d state %d %s' % (r, l, n), D[r, l, c], [ref])
    _check_own_state(eng, D, labels)


def test_centroid_bond_with_a_group_of_65_atoms(hip_engine_factory):
    rng = np.random.default_rng(5202)
    f = CustomCentroidBondForce(2, '0.5*kc*(distance(g1,g2)-d0)^2')
    f.addGlobalParameter('kc', 800.0); f.addGlobalParameter('d0', 0.35)
    f.addGroup(list(range(65))); f.addGroup([65, 66, 67])
    f.addBond([0, 1])
    f.addEnergyParameterDerivative('kc'); f.addEnergyParameterDerivative('d0')
    x = np.concatenate([rng.uniform(0.0, 0.6, (65, 3)), rng.uniform(0.9, 1.2, (3, 3))])
    xs = _f32([x, x + rng.normal(0.0, 0.01, x.shape)])
    ladder = [dict(kc=800.0 - 150.0 * k, d0=0.35 + 0.1 * k) for k in range(4)]
    labels = [3, 0]
    eng, names, own = _handle(hip_engine_factory, _system(68, [f]), xs, states=ladder, labels=labels)
    table = _tables(own, ladder)
    D = eng.custom_energy_parameter_derivatives_at_states()
    assert D.shape == (2, 4, 2)
    groups = [(list(range(65)), [1.0 / 65] * 65), ([65, 66, 67], [1.0 / 3] * 3)]
    for r in range(2):
        for l in range(4):
            for c, n in enumerate(('kc', 'd0')):
                ref = oracle.evaluate_centroid(2, f.getEnergyFunction(), groups, [[0, 1]], [], np.zeros((1, 0)), table[l], n, xs[r], None, False)
                assert ref['scale'] > 0.0
                _close('replica %d state %d %s' % (r, l, n), D[r, l, c], [ref])
    _check_own_state(eng, D, labels)


def test_donor_acceptor_force_of_two_tiles_under_a_periodic_cutoff(hip_engine_factory):
    rng = np.random.default_rng(5203)
    f = CustomHbondForce('scale*kd*ka*(distance(d1,a1)-0.3)^2*(1+cos(angle(d2,d1,a1)))^w')
    f.addGlobalParameter('scale', 1.2); f.addGlobalParameter('w', 1.5)
    f.addPerDonorParameter('kd'); f.addPerAcceptorParameter('ka')
    for k in range(65):                                                     # 65 donors x 3 acceptors: two tiles of 64 donors
        f.addDonor(2 * k, 2 * k + 1, -1, [rng.uniform(50.0, 90.0)])
    for k in range(3):
        f.addAcceptor(130 + k, -1, -1, [rng.uniform(0.5, 1.5)])
    f.addExclusion(1, 2)
    f.setNonbondedMethod(CustomHbondForce.CutoffPeriodic)
    f.setCutoffDistance(0.6)
    f.addEnergyParameterDerivative('scale'); f.addEnergyParameterDerivative('w')
    box = np.array([2.0, 2.1, 2.2])
    xs = [rng.uniform(0.0, 2.0, (133, 3)) for _ in range(2)]
    for x in xs:                                                            # the 65th donor, alone in the second tile, bonds to acceptor 0
        x[128] = x[130] + [0.35, 0.05, 0.0]
    xs, boxes = _f32(xs), _f32([box, box])
    donors = [f.getDonorParameters(k) for k in range(65)]
    acceptors = [f.getAcceptorParameters(k) for k in range(3)]
    args = ([d[:3] for d in donors], [a[:3] for a in acceptors], [d[3] for d in donors], [a[3] for a in acceptors])
    ladder = [dict(scale=1.2 - 0.2 * k, w=1.5 + 0.25 * k) for k in range(4)]
    labels = [2, 1]
    eng, names, own = _handle(hip_engine_factory, _system(133, [f], box), xs, boxes, states=ladder, labels=labels)
    table = _tables(own, ladder)
    D = eng.custom_energy_parameter_derivatives_at_states()
    assert D.shape == (2, 4, 2)
    for r in range(2):
        member = custom_hbond_oracle.evaluate(f.getEnergyFunction(), ['kd'], ['ka'], *args, table[0], xs[r], boxes[r], 2, 0.6, [(1, 2)])
        assert custom_hbond_oracle.clear_of_cutoff(member, 0.6, 1e-6)          # no pair within 1e-6 nm of the cutoff: checked on the CPU
        assert len(member['i']) > 8 and 64 in member['i'] and member['i'].min() < 64 and member['r_all'].max() > 0.6      # pairs in both tiles, some cut off
        pairs = list(zip(member['i'], member['j']))
        for l in range(4):
            for c, n in enumerate(('scale', 'w')):
                ref = oracle.evaluate_hbond(f.getEnergyFunction(), ['kd'], ['ka'], *args, table[l], n, pairs, xs[r], boxes[r], True)
                assert ref['scale'] > 0.0
                _close('replica %d state %d %s (%d pairs)' % (r, l, n, len(pairs)), D[r, l, c], [ref])
    _check_own_state(eng, D, labels)


def test_many_particle_force_of_70_particles(hip_engine_factory):
    rng = np.random.default_rng(5204)
    N = 70
    xs = _f32([rng.uniform(0.0, 1.6, (N, 3)) for _ in range(2)])
    f = CustomManyParticleForce(3, MW)
    f.addGlobalParameter('lam3', 0.9); f.addPerParticleParameter('eps')
    eps, types = rng.uniform(20.0, 30.0, N), [k % 2 for k in range(N)]
    for k in range(N):
        f.addParticle([eps[k]], types[k])
    mode = CustomManyParticleForce.SinglePermutation
    f.setPermutationMode(mode)
    f.setNonbondedMethod(CustomManyParticleForce.CutoffNonPeriodic)
    f.setCutoffDistance(0.45)
    f.setTypeFilter(0, [0])
    f.addEnergyParameterDerivative('lam3')
    ladder = [dict(lam3=0.9 - 0.25 * k) for k in range(4)]
    labels = [0, 3]
    eng, names, own = _handle(hip_engine_factory, _system(N, [f]), xs, states=ladder, labels=labels)
    table = _tables(own, ladder)
    D = eng.custom_energy_parameter_derivatives_at_states()
    assert D.shape == (2, 4, 1)
    for r in range(2):
        member = custom_manyparticle_oracle.evaluate(MW, ['eps'], eps[:, None], types, [[0], [], []], table[0], xs[r], None, 1, 0.45, (), mode)
        assert custom_manyparticle_oracle.clear_of_cutoff(member, 0.45, 1e-6) and len(member['sets']) > 64
        assert member['sets'][:, 0].max() >= 64                              # central particles in the second wavefront of the part
        for l in range(4):
            ref = oracle.evaluate_manyparticle(MW, ['eps'], eps[:, None], table[l], 'lam3', member['sets'], xs[r])
            assert ref['scale'] > 0.0
            _close('replica %d state %d lam3 (%d sets)' % (r, l, len(member['sets'])), D[r, l, 0], [ref])
    _check_own_state(eng, D, labels)


# ---- 3. the tie to the energy path ---------------------------------------------------------------------------------------------------------
def test_a_linear_global_ties_the_derivative_to_the_u_kl_rows(hip_engine_factory):
    """E = lam f(x): u_kl[r][l] - u_kl[r][own] = beta (lam_l - lam_own) dE/dlam, for compute_energies() and the new kernels.  Bounds: the
    u_kl share of a custom force is formed per term in f64, so the difference lies within beta 1e-11 sum_t (|E_t(g_l)| + |E_t(g_own)|) of
    the exact one, plus the f64 rounding of assembling the two row entries and subtracting them, 4 * 2^-52 (|u_l| + |u_own|); the
    derivative side within beta |lam_l - lam_own| 1e-11 sum_t |dE_t/dlam|."""
    forces, xs = _one_variable_forces()
    bond = forces[0]                                                        # lam_b * 0.5 k (r - r0)^2
    bond.addEnergyParameterDerivative('lam_b')
    lams = [0.2, 0.5, 0.8, 1.0]
    ladder = [dict(lam_b=v) for v in lams]
    labels = [0, 2, 3]
    eng, names, own = _handle(hip_engine_factory, _system(68, [bond]), xs, states=ladder, labels=labels)
    u = eng.compute_energies()
    D = eng.custom_energy_parameter_derivatives_at_states()
    for r in range(3):
        o = labels[r]
        ref_own = _simple(bond, dual.KIND_BOND, dict(lam_b=lams[o]), 'lam_b', xs[r])
        for l in range(4):
            ref_l = _simple(bond, dual.KIND_BOND, dict(lam_b=lams[l]), 'lam_b', xs[r])
            lhs, rhs = u[r, l] - u[r, o], BETA * (lams[l] - lams[o]) * D[r, o, 0]
            bound = (BETA * 1e-11 * (np.abs(ref_l['E']).sum() + np.abs(ref_own['E']).sum()) + 4.0 * 2.0 ** -52 * (abs(u[r, l]) + abs(u[r, o]))
                     + BETA * abs(lams[l] - lams[o]) * ref_own['bound'])
            print('replica %d state %d: u_kl difference %.17g, beta dlam dE/dlam %.17g, |difference| / bound = %.3g'
                  % (r, l, lhs, rhs, abs(lhs - rhs) / max(bound, 1e-300)))
            assert abs(lhs - rhs) <= bound
            assert l == o or abs(lhs) > 1.0                                 # (not a comparison of zeros)


# ---- 4. same and different globals -----------------------------------------------------------------------------------------------------------
def test_identical_rows_give_identical_bits_and_an_undeclared_global_still_counts(hip_engine_factory):
    rng = np.random.default_rng(5205)
    f = CustomBondForce('lam*k*(r-r0g)^2')
    f.addGlobalParameter('lam', 0.6); f.addGlobalParameter('r0g', 0.15); f.addPerBondParameter('k')
    for i in range(65):
        f.addBond(i, i + 1, [rng.uniform(1e3, 3e3)])
    f.addEnergyParameterDerivative('lam')
    x = np.cumsum(rng.normal(0.0, 0.08, (66, 3)) + [0.1, 0.0, 0.0], axis=0)
    xs = _f32([x, x + rng.normal(0.0, 0.005, x.shape)])
    ladder = [dict(lam=0.6, r0g=0.15), dict(lam=0.3, r0g=0.15), dict(lam=0.6, r0g=0.15), dict(lam=0.6, r0g=0.25)]
    eng, names, own = _handle(hip_engine_factory, _system(66, [f]), xs, states=ladder, labels=[1, 0])
    D = eng.custom_energy_parameter_derivatives_at_states()
    assert D.shape == (2, 4, 1)
    assert _bit_equal(D[:, 0], D[:, 2])                                     # states 0 and 2: the same row of globals
    for r in range(2):
        for l in range(4):
            ref = _simple(f, dual.KIND_BOND, ladder[l], 'lam', xs[r])
            _close('replica %d state %d' % (r, l), D[r, l, 0], [ref])
        # state 3 differs from state 0 in r0g alone, which no force declared: the derivative with respect to lam is another number
        other = _simple(f, dual.KIND_BOND, ladder[0], 'lam', xs[r])
        assert abs(D[r, 3, 0] - other['total']) > 1e3 * other['bound']
        assert D[r, 1, 0] == D[r, 0, 0]                                     # (E is linear in lam: its own value does not enter)


# ---- 5. the mask rule ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('declare_second', [False, True])
def test_only_the_forces_that_declared_a_parameter_contribute_at_every_state(hip_engine_factory, declare_second):
    forces, xs = _two_bond_forces(declare_second)
    ladder = [dict(lam=0.6, unused=3.0), dict(lam=0.9, unused=1.0), dict(lam=0.1, unused=2.0)]
    eng, names, own = _handle(hip_engine_factory, _system(7, forces), xs, states=ladder, labels=[1])
    assert eng.custom_derivative_names == ['unused', 'lam']
    D = eng.custom_energy_parameter_derivatives_at_states()
    assert D.shape == (1, 3, 2)
    for l in range(3):
        assert D[0, l, 0] == 0.0                                            # a declared global that the expression does not name: exactly 0
        refs = [_simple(f, dual.KIND_BOND, ladder[l], 'lam', xs[0]) for f in forces]
        assert abs(refs[1]['total']) > 1e-3 * abs(refs[0]['total'])       # the second force's share would show
        _close('state %d lam' % l, D[0, l, 1], refs if declare_second else refs[:1])


# ---- 6. a neighbour row over capacity ----------------------------------------------------------------------------------------------------------
def test_an_overflowing_row_gives_nan_at_every_state_in_that_forces_columns_only(hip_engine_factory):
    """the geometry of tests/test_custom_manyparticle_gpu.py: particle 70, the only admitted central particle, with 129 neighbours inside
    the cutoff in replica 0 and 128 in replica 1"""
    rng = np.random.default_rng(1104)
    N = 131
    f = CustomManyParticleForce(3, '0.01*lam3*distance(p1,p2)*distance(p1,p3)*(1+cos(angle(p2,p1,p3)))')
    f.addGlobalParameter('lam3', 0.9)
    for k in range(N):
        f.addParticle([], 1 if k == 70 else 0)
    f.setPermutationMode(CustomManyParticleForce.UniqueCentralParticle)
    f.setNonbondedMethod(CustomManyParticleForce.CutoffNonPeriodic)
    f.setCutoffDistance(0.5)
    f.setTypeFilter(0, [1])
    f.addEnergyParameterDerivative('lam3')
    b = CustomBondForce('lam_b*r^2'); b.addGlobalParameter('lam_b', 1.0); b.addBond(0, 1); b.addBond(2, 3)
    b.addEnergyParameterDerivative('lam_b')
    u = rng.normal(size=(N, 3))
    x = 0.45 * u / np.linalg.norm(u, axis=1, keepdims=True) + [2.0, 2.0, 2.0]
    x[70] = [2.0, 2.0, 2.0]
    x[130] = [9.0, 9.0, 9.0]
    full, over = x.copy(), x.copy()
    full[129] = [2.7, 2.0, 2.0]
    over[129] = [2.3, 2.0, 2.0]
    xs = _f32([over, full])
    assert ((custom_manyparticle_oracle.distances(xs[0])[70] < 0.5).sum() - 1) == 129
    assert ((custom_manyparticle_oracle.distances(xs[1])[70] < 0.5).sum() - 1) == 128
    ladder = [dict(lam3=0.9, lam_b=1.0), dict(lam3=0.5, lam_b=0.7), dict(lam3=0.1, lam_b=0.2)]
    eng, names, own = _handle(hip_engine_factory, _system(N, [f, b]), xs, states=ladder, labels=[0, 2])
    assert eng.custom_derivative_names == ['lam3', 'lam_b']
    D = eng.custom_energy_parameter_derivatives_at_states()
    assert D.shape == (2, 3, 2)
    assert np.isnan(D[0, :, 0]).all()                                       # the overflowing replica: NaN at every state, that force's column
    assert np.isfinite(D[0, :, 1]).all() and np.isfinite(D[1]).all() and np.all(D[1, :, 0] != 0.0)
    for r in range(2):
        for l in range(3):
            _close('replica %d state %d lam_b' % (r, l), D[r, l, 1], [_simple(b, dual.KIND_BOND, ladder[l], 'lam_b', xs[r])])
    own_state = eng.custom_energy_parameter_derivatives()
    assert np.isnan(own_state[0, 0]) and _bit_equal(own_state[:, 1], D[[0, 1], [0, 2], 1]) and own_state[1, 0] == D[1, 2, 0]


# ---- 7. no side effects ------------------------------------------------------------------------------------------------------------------------
def test_the_call_leaves_energies_forces_and_own_state_derivatives_as_they_are(hip_engine_factory):
    out = []
    for call in (True, False):
        forces, xs = _one_variable_forces()
        forces[0].addEnergyParameterDerivative('lam_b'); forces[3].addEnergyParameterDerivative('lam_e')
        eng, _, _ = _handle(hip_engine_factory, _system(68, forces), xs, states=LADDER, labels=[0, 2, 3])
        if call:
            eng.custom_energy_parameter_derivatives_at_states()
        first = eng.custom_energy_parameter_derivatives()
        if call:
            eng.custom_energy_parameter_derivatives_at_states()
        out.append((eng.compute_energies(), eng.get_forces(), first, eng.custom_energy_parameter_derivatives(), eng.custom_energies()))
    for p, q in zip(*out):
        assert np.array_equal(p, q)


def test_refusals(hip_engine_factory):
    forces, xs = _one_variable_forces()
    eng, _, _ = _handle(hip_engine_factory, _system(68, forces), xs, states=LADDER, labels=[0, 2, 3])
    with pytest.raises(ValueError, match='no custom force of the system declares an energy parameter derivative'):
        eng.custom_energy_parameter_derivatives_at_states()
    forces, xs = _one_variable_forces()
    forces[0].addEnergyParameterDerivative('lam_b')
    eng, _, _ = _handle(hip_engine_factory, _system(68, forces), xs, states=LADDER, labels=[0, 2, 3])
    eng.set_states(np.full(3, BETA))                                       # new states, no globals for them yet
    with pytest.raises(RuntimeError, match='remd_set_custom_globals'):
        eng.custom_energy_parameter_derivatives_at_states()


# ---- 8. end to end: thermodynamic integration of a sampled ladder ------------------------------------------------------------------------------
class LamState(states.GlobalParameterState):
    lam = states.GlobalParameterState.GlobalParameter('lam', standard_value=1.0)


K_WELL, LAMS, N_ITERATIONS = 4.0, [0.0, 0.5, 1.0, 1.5], 300


def test_thermodynamic_integration_of_a_shifted_harmonic_well(hip_engine_factory, tmp_path):
    """8 particles in 0.5 k r^2 + lam k x, lam = 0, 0.5, 1, 1.5 at 300 K: f(lam) = -8 beta k lam^2 / 2 exactly, <du/dlam> = -8 beta k lam
    is linear in lam (the trapezoid rule is exact) and BAOAB samples a harmonic well's positions without bias.
    N_ITERATIONS = 300 with this seed, measured on an MI355X: exact -14.433 kT; 'mbar' -14.466 +- 0.198, 'samples' -14.478 +- 0.248,
    get_free_energy() -14.488 +- 0.246 (13 iterations of equilibration, g = 2.1): sigma is 1.4 % and 1.7 % of |Delta_f|, under the 5 %
    the test asks for, and both estimates lie 0.2 sigma from the exact value."""
    from openmmtools_amd.multistate import ReplicaExchangeSampler, MultiStateReporter
    from openmmtools_amd.multistate import analysis as an
    system = System()
    for _ in range(8):
        system.addParticle(12.0)
    f = CustomExternalForce('0.5*k*(x^2+y^2+z^2)+lam*k*x')
    f.addGlobalParameter('k', K_WELL); f.addGlobalParameter('lam', 0.0)
    for i in range(8):
        f.addParticle(i)
    f.addEnergyParameterDerivative('lam')
    system.addForce(f)
    ts = states.ThermodynamicState(system, 300.0 * unit.kelvin)
    sts = states.create_thermodynamic_state_protocol(ts, {'lam': LAMS}, composable_states=[LamState(lam=0.0)])
    move = mcmc.LangevinSplittingDynamicsMove(timestep=20.0 * unit.femtosecond, collision_rate=1.0 / unit.picosecond, n_steps=100,
                                              reassign_velocities=True, splitting='V R O R V')
    sampler = ReplicaExchangeSampler(mcmc_moves=move, number_of_iterations=N_ITERATIONS, engine=hip_engine_factory(), seed=0x71C0,
                                     online_analysis_interval=None, store_parameter_derivatives=True)
    rep = MultiStateReporter(str(tmp_path / 'store'), checkpoint_interval=100)
    sampler.create(sts, [states.SamplerState(np.zeros((8, 3)))], storage=rep)
    sampler.run()
    assert rep.read_parameter_derivative_names() == ['lam'] and rep.read_parameter_derivatives().shape == (N_ITERATIONS + 1, 4, 4, 1)
    # the last record against the positions still on the device: dE/dlam = k sum x, the same under every state's globals
    x = sampler.engine.get_replicas()[0]
    assert np.allclose(rep.read_parameter_derivatives(-1)[:, 0, 0], K_WELL * np.asarray(x, dtype=np.float64)[:, :, 0].sum(axis=1), rtol=1e-6, atol=1e-9)
    a = an.MultiStateSamplerAnalyzer(rep)
    beta = sts[0].beta
    exact = -8.0 * beta * K_WELL * (LAMS[3] ** 2 - LAMS[0] ** 2) / 2.0
    f_mbar, df_mbar = a.get_free_energy()
    print('exact Delta_f(0->3) = %.5f kT; MBAR %.5f +- %.5f; n_equilibration %d, g %.3f'
          % (exact, f_mbar[0, 3], df_mbar[0, 3], a.n_equilibration_iterations, a.statistical_inefficiency))
    for estimator in ('mbar', 'samples'):
        ti = a.get_thermodynamic_integration(estimator=estimator)
        got, sig = ti['Delta_f'][0, 3], ti['dDelta_f'][0, 3]
        print('%s: Delta_f(0->3) = %.5f +- %.5f kT, (TI - exact) / sigma = %.3f, (TI - MBAR) / combined sigma = %.3f, sigma / |Delta_f| = %.4f'
              % (estimator, got, sig, (got - exact) / sig, (got - f_mbar[0, 3]) / np.hypot(sig, df_mbar[0, 3]), sig / abs(exact)))
        print('%s: mean %s, exact %s' % (estimator, np.round(ti['mean'][:, 0], 4), np.round(-8.0 * beta * K_WELL * np.array(LAMS), 4)))
        assert np.array_equal(ti['lambdas'][:, 0], LAMS) and ti['names'] == ['lam']
        assert 0.0 < sig < 0.05 * abs(exact)                                # against a vacuous pass
        assert abs(got - exact) <= 5.0 * sig
        assert abs(got - f_mbar[0, 3]) <= 5.0 * np.hypot(sig, df_mbar[0, 3])
