"""GPU: a CustomGBForce on the general path (openmmtools_amd/custom_gb.py compile_custom_gb, csrc/custom_gb.hip, REMD_CUSTOM_GB of
include/remd_hip_custom.h) against tests/custom_gb_expr_oracle.py, the force by its definition over dual numbers.

Bounds: the energy within 1e-11 sum|summand| (f64 sums of f64 energies); the force on an atom, per component, within
n (2^-23 max|contribution| + 2^-31): the contributions are the pair pieces of the force on the atom, two per partner inside the cutoff
(the pair terms' dE/dr and the values' chain dE/dV_0 df/dr, each along the pair's axis), n the nonzero ones and the maximum taken over
them (tests/custom_gb_expr_oracle.py pair_pieces).  The device sums them in f64 and hands the fixed-point accumulators one f32-rounded
partial sum per launch and column slice, at most 2 x 3 per atom here.  Positions
are rounded to f32 before either side sees them; with a cutoff no pair lies within 1e-6 nm of it, and r > 0.2 nm throughout
(asserted on the CPU).  Sizes: 3 (one lane), 64 (a full tile), 65 (one past it: two row blocks, two slices), 130 (three)."""
import copy

import numpy as np
import pytest

import custom_gb_expr_cases as cases
import custom_gb_expr_oracle as oracle
from openmmtools_amd import mcmc, states, testsystems as ts, unit
from openmmtools_amd.system import System, system_to_desc, CustomGBForce

pytestmark = pytest.mark.gpu

KB = 0.008314462618153242
BETA = 1.0 / (KB * 300.0)
_CACHE = {}


def _system(n, force, box=None):
    s = System()
    for _ in range(n):
        s.addParticle(12.0)
    if box is not None:
        s.setDefaultPeriodicBoxVectors([box[0], 0, 0], [0, box[1], 0], [0, 0, box[2]])
    s.addForce(force)
    return s


def _device(engine, system, xs, boxes=None, betas=(BETA,)):
    desc = system_to_desc(system, box=None if boxes is None else boxes[0])
    assert 'gbsa' not in desc and desc['custom_terms']['000']['kind'] == 12
    engine.set_system(desc)
    engine.set_states(np.asarray(betas, dtype=np.float64))
    engine.set_custom_globals(np.zeros((len(betas), 0)))
    R = len(xs)
    engine.set_replicas(R, 0, xs, None, np.zeros((R, 3)) if boxes is None else boxes, np.zeros(R, dtype=np.int64))
    f = engine.get_forces()
    u = engine.get_replicas(positions=False, velocities=False, potential=True)[2]
    return f, u, engine.custom_energies()


def _references(key, spec, xs, boxes=None):
    """the oracle's results, once per case (the tests share them and leave them unchanged)"""
    if key not in _CACHE:
        refs = [oracle.evaluate(spec, x, None if boxes is None else boxes[r]) for r, x in enumerate(xs)]
        for ref in refs:
            assert ref['r_all'][~np.eye(len(xs[0]), dtype=bool)].min() > 0.2
            if spec['method']:
                assert not oracle.borderline(ref, spec['cutoff'], 1e-6)
        _CACHE[key] = refs
    return _CACHE[key]


def _assert_matches(tag, f, e, ref):
    de, df = abs(e - ref['E']) / max(oracle.energy_bound(ref), 1e-300), (np.abs(f - ref['F']) / oracle.force_bound(ref).clip(min=1e-300)).max()
    print('%s: E = %.6g, |dE| / bound = %.3g, worst |dF| / bound = %.3g, max|F| = %.3g' % (tag, ref['E'], de, df, np.abs(ref['F']).max()))
    assert abs(e - ref['E']) <= oracle.energy_bound(ref)
    assert np.all(np.abs(f - ref['F']) <= oracle.force_bound(ref))


def _check(engine, key, spec, n, boxes=None, seed=5):
    xs = cases.positions(n, seed)
    refs = _references(key, spec, xs, boxes)
    fd, u, e = _device(engine, _system(n, cases.build(spec), None if boxes is None else boxes[0]), xs, boxes)
    for r, ref in enumerate(refs):
        _assert_matches('%s replica %d' % (key, r), fd[r], e[r, 0], ref)
        assert u[r] == e[r, 0]
    assert abs(refs[0]['E'] - refs[1]['E']) > 1e-6               # the replicas are at different positions
    return fd, u, e


@pytest.mark.parametrize('n', [3, 64, 65, 130])
def test_hct_without_a_cutoff(hip_engine_factory, n):
    _check(hip_engine_factory(), ('hct', n), cases.born(n, cases.HCT_B), n)


@pytest.mark.parametrize('method', [0, 1, 2])
def test_obc2_in_redundant_parentheses_under_every_method(hip_engine_factory, method):
    n = 65
    # (the device keeps the box edges in f32: rounded before the oracle sees them, like the positions)
    boxes = np.array([[2.0, 2.1, 2.2], [2.05, 2.0, 2.3]], dtype=np.float32).astype(np.float64) if method == 2 else None
    _check(hip_engine_factory(), ('obc2', method), cases.born(n, cases.OBC2_B, method, 0.9 if method else 0.0), n, boxes)


def test_gbn2_shaped_model_with_tables(hip_engine_factory):
    _check(hip_engine_factory(), 'gbn2', cases.gbn2_shaped(65), 65)


def test_exclusions_in_a_value_and_in_a_term(hip_engine_factory):
    _check(hip_engine_factory(), 'excluded', cases.excluded(65, [(0, 1), (63, 64), (3, 40), (1, 2)]), 65)       # (63, 64) spans two tiles


def test_three_values_and_a_pair_term_of_two_passes(hip_engine_factory):
    spec = cases.three_values(65)
    desc = system_to_desc(_system(65, cases.build(spec)))['custom_terms']['000']
    assert [int(s[3]) for s in desc['stages'] if s[0] == 3] == [0, 1]
    _check(hip_engine_factory(), 'three', spec, 65)


@pytest.mark.parametrize('n', [3, 65])
def test_single_particle_terms_only(hip_engine_factory, n):
    _check(hip_engine_factory(), ('single', n), cases.single_only(n), n)


# ---- agreement with the template path -----------------------------------------------------------------------------------------------------
def _general(system):
    """the System with its OBC2 force in strings the recognizer refuses (one pair of parentheses more): the same model"""
    s = copy.deepcopy(system)
    for k, f in enumerate(s.forces):
        if type(f).__name__ == 'GBSAOBCForce':
            spec = cases.born(f.getNumParticles(), cases.OBC2_B)
            spec['params'] = np.array(f.particles, dtype=np.float64)
            spec['globals'] = dict(solventDielectric=f.getSolventDielectric(), soluteDielectric=f.getSoluteDielectric())
            s.forces[k] = cases.build(spec)
        elif isinstance(f, CustomGBForce):
            name, text, kind = f.computed[1]
            f.computed[1] = (name, text.replace('tanh(1*psi-0.8*psi^2+4.85*psi^3)', 'tanh((1*psi-0.8*psi^2+4.85*psi^3))'), kind)
    return s


@pytest.mark.parametrize('name', ['AlanineDipeptideImplicit', 'CustomGBForceSystem'])
def test_obc2_agrees_with_the_template_path(hip_engine_factory, name):
    t = getattr(ts, name)()
    box = np.diag(t.system.getDefaultPeriodicBoxVectors()) if name == 'CustomGBForceSystem' else np.zeros(3)
    x = np.asarray(t.positions, dtype=np.float64)
    xs = np.stack([x, x + 0.01 * np.random.default_rng(3).normal(size=x.shape)])
    out = []
    for system in (t.system, _general(t.system)):
        desc = system_to_desc(system)
        assert ('gbsa' in desc) == (system is t.system) and ('custom_terms' in desc) == (system is not t.system)
        eng = hip_engine_factory()
        eng.set_system(desc)
        eng.set_states(np.array([BETA]))
        if 'custom_terms' in desc:
            eng.set_custom_globals(np.zeros((1, 0)))
        eng.set_replicas(2, 0, xs, None, np.tile(box, (2, 1)), np.zeros(2, dtype=np.int64))
        out.append((eng.get_forces(), eng.get_replicas(positions=False, velocities=False, potential=True)[2]))
    (f0, u0), (f1, u1) = out
    print('%s: U = %s against %s, max|dF| / max|F| = %.3g' % (name, u1, u0, np.abs(f1 - f0).max() / np.abs(f0).max()))
    # (the tolerance tests/test_custom_gb_gpu.py grants gbsa.hip against its oracle)
    assert np.allclose(u1, u0, rtol=1e-5, atol=1e-5 * np.abs(u0).max())
    assert np.abs(f1 - f0).max() < 2e-4 * np.abs(f0).max()


# ---- behaviour ------------------------------------------------------------------------------------------------------------------------------
def test_two_evaluations_are_bit_identical_and_the_force_group_selects(hip_engine_factory):
    n, spec = 130, cases.born(130, cases.HCT_B)
    xs = cases.positions(n, 5)
    force = cases.build(spec)
    force.setForceGroup(3)
    runs = [_device(hip_engine_factory(), _system(n, force), xs) for _ in range(2)]
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)
    eng = hip_engine_factory()
    f, u, e = _device(eng, _system(n, force), xs)
    assert np.array_equal(eng.get_forces(groups=1 << 3), f) and not np.any(eng.get_forces(groups=1 << 0))
    assert e.shape == (2, 1) and np.array_equal(e[:, 0], u)


def test_hct_dipeptide_runs_and_reads_back_its_energy(hip_engine_factory):
    t = ts.AlanineDipeptideImplicit(implicitSolvent='HCT')
    desc = system_to_desc(t.system)
    eng = hip_engine_factory()
    eng.set_system(desc)
    eng.set_states(np.array([BETA]))
    eng.set_custom_globals(np.zeros((1, 0)))
    eng.set_integrator('V R O R V', 0.002, 1.0, 20, True, 1e-8)
    eng.seed(11)
    x = np.asarray(t.positions, dtype=np.float64)[None]
    eng.set_replicas(1, 0, x, None, np.zeros((1, 3)), np.zeros(1, dtype=np.int64))
    assert not np.any(eng.propagate(0))
    xd, _, u = eng.get_replicas(potential=True)[:3]
    assert np.all(np.isfinite(u))
    fresh = hip_engine_factory()
    fresh.set_system(desc)
    fresh.set_states(np.array([BETA]))
    fresh.set_custom_globals(np.zeros((1, 0)))
    fresh.set_replicas(1, 0, xd, None, np.zeros((1, 3)), np.zeros(1, dtype=np.int64))
    assert np.array_equal(fresh.get_replicas(positions=False, velocities=False, potential=True)[2], u)
    assert np.abs(xd - x).max() > 1e-4


def test_parallel_tempering_rows_are_beta_times_the_potential(hip_engine_factory):
    from openmmtools_amd.multistate import ParallelTemperingSampler
    t = ts.AlanineDipeptideImplicit(implicitSolvent='HCT')
    eng = hip_engine_factory()
    move = mcmc.LangevinSplittingDynamicsMove(timestep=2.0 * unit.femtosecond, collision_rate=1.0 / unit.picosecond, n_steps=10,
                                              reassign_velocities=True, splitting='V R O R V')
    s = ParallelTemperingSampler(mcmc_moves=move, number_of_iterations=1, engine=eng, seed=7, online_analysis_interval=None)
    temperatures = [300.0, 350.0, 400.0, 450.0]
    s.create(states.ThermodynamicState(t.system, 300.0 * unit.kelvin), [states.SamplerState(t.positions)],
             temperatures=[T * unit.kelvin for T in temperatures])
    s.run(1)
    rows = np.array(s.energy_thermodynamic_states)
    x = eng.get_replicas()[0]
    e = eng.custom_energies()
    assert e.shape == (4, 1) and np.all(np.isfinite(e)) and np.all(e != 0.0)
    # the rest: the same System without the CustomGBForce at the same positions, on an engine of its own
    bare = copy.deepcopy(t.system)
    bare.forces = [f for f in bare.forces if not isinstance(f, CustomGBForce)]
    rest = hip_engine_factory()
    rest.set_system(system_to_desc(bare))
    rest.set_states(np.array([BETA]))
    rest.set_replicas(4, 0, x, None, np.zeros((4, 3)), np.zeros(4, dtype=np.int64))
    u = e[:, 0] + rest.get_replicas(positions=False, velocities=False, potential=True)[2]
    betas = 1.0 / (KB * np.array(temperatures))
    print('u_kl rows against beta_l (custom_energies + rest): max relative difference %.3g' % (np.abs(rows - u[:, None] * betas[None, :]) / np.abs(rows)).max())
    # (the rest is summed in f32 force kernels with f64 energies; the two engines add the same numbers in another order)
    assert np.allclose(rows, u[:, None] * betas[None, :], rtol=1e-9, atol=0.0)
