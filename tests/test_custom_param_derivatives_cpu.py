"""CPU: the oracle of the energy parameter derivatives (tests/custom_param_derivative_oracle.py) against closed forms in mpmath at 50 digits
and against central differences of its own energy; the compiler's derivative list and masks (custom_expr.custom_terms_desc); every
refusal with its sentence; copies and from_openmm; the kinds that keep refusing; a library without the entry points."""
import copy
import types

import mpmath
import numpy as np
import pytest

import custom_dual_oracle as dual
import custom_param_derivative_oracle as oracle
from openmmtools_amd import _engine, forces as restraint_forces
from openmmtools_amd.system import (System, system_to_desc, hbond_force_from_openmm, manyparticle_force_from_openmm, gb_force_from_openmm,
                                    CustomBondForce, CustomAngleForce, CustomTorsionForce, CustomExternalForce, CustomCompoundBondForce,
                                    CustomCentroidBondForce, CustomHbondForce, CustomManyParticleForce, CustomNonbondedForce, CustomCVForce,
                                    CustomGBForce, CMAPTorsionForce)

mpmath.mp.dps = 50
X = np.array([[0.0, 0.0, 0.0], [0.21, 0.13, 0.05]])
R = mpmath.sqrt(mpmath.mpf(0.21) ** 2 + mpmath.mpf(0.13) ** 2 + mpmath.mpf(0.05) ** 2)
T1 = [np.sin(0.7 * k) + 0.1 * k for k in range(9)]


def _bond(energy, g, wrt, functions=None):
    return oracle.evaluate(dual.KIND_BOND, energy, [[0, 1]], [], np.zeros((1, 0)), g, wrt, X, functions=functions)


def _mp(v):
    return mpmath.mpf(float(v))


@pytest.mark.parametrize('energy, g, wrt, closed', [
    ('k*(r-r0)^2', dict(k=900.0, r0=0.2), 'k', lambda g: (R - _mp(g['r0'])) ** 2),
    ('k*(r-r0)^2', dict(k=900.0, r0=0.2), 'r0', lambda g: -2 * _mp(g['k']) * (R - _mp(g['r0']))),
    ('r^lam', dict(lam=1.7), 'lam', lambda g: R ** _mp(g['lam']) * mpmath.log(R)),
    ('min(lam*r, 1)', dict(lam=2.0), 'lam', lambda g: R),                      # lam r = 0.5 < 1
    ('min(lam*r, 1)', dict(lam=6.0), 'lam', lambda g: mpmath.mpf(0)),          # lam r = 1.5 > 1
    ('select(lam-1, lam*r, lam^2*r)', dict(lam=1.0), 'lam', lambda g: 2 * _mp(g['lam']) * R),     # the condition is 0: the third argument
    ('select(lam-1, lam*r, lam^2*r)', dict(lam=1.5), 'lam', lambda g: R),
    ('step(lam-r)*lam*r', dict(lam=0.5), 'lam', lambda g: R),                  # step is flat: only the factor differentiates
    ('step(lam-r)*lam*r', dict(lam=0.1), 'lam', lambda g: mpmath.mpf(0)),
])
def test_oracle_against_closed_forms(energy, g, wrt, closed):
    got, want = _bond(energy, g, wrt)['total'], closed(g)
    assert abs(_mp(got) - want) <= mpmath.mpf(2) ** -48 * max(abs(want), mpmath.mpf(1))


def test_oracle_spline_of_a_scaled_distance_against_mpmath():
    """a Continuous1DFunction of lam*r: d/dlam = r s'(lam r), s the natural spline evaluated here in mpmath from the oracle's own M"""
    lo, hi, lam = 0.0, 1.2, 2.0
    h, y, M = oracle.natural_spline(T1, lo, hi)
    t = _mp(lam) * R
    i = int(t / _mp(h))
    b = t / _mp(h) - i
    a = 1 - b
    slope = (_mp(y[i + 1]) - _mp(y[i])) / _mp(h) + ((1 - 3 * a * a) * _mp(M[i]) + (3 * b * b - 1) * _mp(M[i + 1])) * _mp(h) / 6
    got = _bond('t1(lam*r)', dict(lam=lam), 'lam', dict(t1=oracle.continuous1d(T1, lo, hi)))['total']
    assert abs(_mp(got) - R * slope) <= mpmath.mpf(2) ** -44 * abs(R * slope)
    # and the spline's M solve the natural spline's equations
    for k in range(1, len(y) - 1):
        assert abs(M[k - 1] + 4 * M[k] + M[k + 1] - 6 * (y[k - 1] - 2 * y[k] + y[k + 1]) / h ** 2) <= 1e-9
    assert M[0] == 0.0 and M[-1] == 0.0


@pytest.mark.parametrize('energy, g', [
    ('c*r + (r-off)^2', dict(c=2.5, off=0.27)), ('exp(-a*r) + cos(a2*r)', dict(a=1.7, a2=4.0)), ('r^ex', dict(ex=2.3)),
    ('u*u2; u = g*r; u2 = g + r', dict(g=0.8)), ('t1(q*r)', dict(q=2.0)),
])
def test_oracle_against_central_differences_of_its_own_energy(energy, g):
    fn = dict(t1=oracle.continuous1d(T1, 0.0, 1.2))
    for n in g:
        h = 1e-6
        ep = _bond(energy, dict(g, **{n: g[n] + h}), n, fn)['E'].sum()
        em = _bond(energy, dict(g, **{n: g[n] - h}), n, fn)['E'].sum()
        d = _bond(energy, g, n, fn)['total']
        assert abs(d - (ep - em) / (2 * h)) <= 1e-8 * max(1.0, abs(d))


def test_oracle_compound_centroid_and_scale():
    x = np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [0.5, 0.1, 0.0], [0.6, 0.2, 0.1]])
    r = oracle.evaluate(None, 'k*(distance(p1,p2)-d0)^2', [[0, 2], [1, 3]], [], np.zeros((2, 0)), dict(k=3.0, d0=0.2), 'k', x, n_particles=2)
    want = [(np.linalg.norm(x[2] - x[0]) - 0.2) ** 2, (np.linalg.norm(x[3] - x[1]) - 0.2) ** 2]
    assert np.allclose(r['dE'], want, rtol=1e-14) and r['scale'] == np.abs(r['dE']).sum() and r['bound'] == 1e-11 * r['scale']
    c = oracle.evaluate_centroid(2, 'k*distance(g1,g2)', [([0, 1], [0.5, 0.5]), ([2, 3], [0.5, 0.5])], [[0, 1]], [], np.zeros((1, 0)), dict(k=2.0), 'k', x)
    assert np.isclose(c['total'], np.linalg.norm(x[2:].mean(axis=0) - x[:2].mean(axis=0)), rtol=1e-14)


# ---- the declarations and what the compiler makes of them -------------------------------------------------------------------------------------
def _bonds(energy, globals_, declare=()):
    f = CustomBondForce(energy)
    for n, v in globals_.items():
        f.addGlobalParameter(n, v)
    f.addBond(0, 1)
    for n in declare:
        f.addEnergyParameterDerivative(n)
    return f


def _system(fs, n=4):
    s = System()
    for _ in range(n):
        s.addParticle(12.0)
    for f in fs:
        s.addForce(f)
    return s


def test_the_interface_of_the_served_classes():
    made = [CustomBondForce('a*r'), CustomAngleForce('a*theta'), CustomTorsionForce('a*theta'), CustomExternalForce('a*x'),
            CustomCompoundBondForce(2, 'a*distance(p1,p2)'), CustomCentroidBondForce(2, 'a*distance(g1,g2)'), CustomHbondForce('a*distance(d1,a1)'),
            CustomManyParticleForce(3, 'a*distance(p1,p2)')]
    for f in made:
        f.addGlobalParameter('a', 1.0); f.addGlobalParameter('b', 2.0)
        assert f.getNumEnergyParameterDerivatives() == 0
        assert f.addEnergyParameterDerivative('b') == 0 and f.addEnergyParameterDerivative('a') == 1
        assert [f.getEnergyParameterDerivativeName(i) for i in range(f.getNumEnergyParameterDerivatives())] == ['b', 'a']
        cls = type(f).__name__
        with pytest.raises(ValueError, match=r"%s: addEnergyParameterDerivative\('c'\): the force has no global parameter of that name" % cls):
            f.addEnergyParameterDerivative('c')
        with pytest.raises(ValueError, match=r"%s: addEnergyParameterDerivative\('a'\): the derivative with respect to that parameter was already added" % cls):
            f.addEnergyParameterDerivative('a')
        g = copy.deepcopy(f)
        assert g._derivatives == ['b', 'a'] and g._derivatives is not f._derivatives


def test_the_list_and_the_masks():
    """distinct columns in the order of first declaration over the forces in System order; per force the mask of what it declared"""
    f1 = _bonds('a*b*r', dict(a=1.0, b=2.0), ['b'])
    f2 = _bonds('a*c*r', dict(c=3.0, a=1.0), ['a', 'c'])
    f3 = _bonds('b*r', dict(b=2.0))                       # names b, declares nothing
    f4 = _bonds('b*c*r', dict(b=2.0, c=3.0), ['c', 'b'])
    d = system_to_desc(_system([f1, f2, f3, f4]))
    terms = [t for _, t in sorted(d['custom_terms'].items())]
    assert terms[0]['global_names'] == ['a', 'b', 'c']
    for t in terms:
        assert t['derivative_names'] == ['b', 'a', 'c'] and list(t['derivative_columns']) == [1, 0, 2]
    assert [t['derivative_mask'] for t in terms] == [0b001, 0b110, 0, 0b101]
    none = system_to_desc(_system([_bonds('a*r', dict(a=1.0))]))['custom_terms']['000']
    assert none['derivative_names'] == [] and len(none['derivative_columns']) == 0 and none['derivative_mask'] == 0


def test_a_declaration_after_the_system_went_to_an_engine_is_refused_and_a_copy_starts_afresh():
    f = _bonds('a*b*r', dict(a=1.0, b=2.0), ['a'])
    s = _system([f])
    system_to_desc(s)
    with pytest.raises(NotImplementedError, match=r"CustomBondForce: adding an energy parameter derivative \('b'\) after set_system is not supported"):
        f.addEnergyParameterDerivative('b')
    g = copy.deepcopy(s).getForce(0)
    g.addEnergyParameterDerivative('b')
    assert g._derivatives == ['a', 'b'] and f._derivatives == ['a']


def test_the_kinds_that_refuse():
    nb = CustomNonbondedForce('a*r'); nb.addGlobalParameter('a', 1.0)
    with pytest.raises(NotImplementedError, match=r'CustomNonbondedForce: energy parameter derivatives \(addEnergyParameterDerivative\) are not supported'):
        nb.addEnergyParameterDerivative('a')
    cv = CustomCVForce('a*v'); cv.addGlobalParameter('a', 1.0)
    with pytest.raises(NotImplementedError, match=r"CustomCVForce: energy parameter derivatives \(addEnergyParameterDerivative 'a'\) are not supported"):
        cv.addEnergyParameterDerivative('a')
    gb = CustomGBForce(); gb.addGlobalParameter('a', 1.0)
    with pytest.raises(NotImplementedError, match=r"CustomGBForce: energy parameter derivatives \(addEnergyParameterDerivative 'a'\) are not supported"):
        gb.addEnergyParameterDerivative('a')
    assert nb.getNumEnergyParameterDerivatives() == cv.getNumEnergyParameterDerivatives() == gb.getNumEnergyParameterDerivatives() == 0
    assert not hasattr(CMAPTorsionForce(), 'addEnergyParameterDerivative')              # (it has no globals)
    r = restraint_forces.HarmonicRestraintBondForce(spring_constant=100.0, restrained_atom_index1=0, restrained_atom_index2=1)
    with pytest.raises(NotImplementedError, match=r"HarmonicRestraintBondForce: energy parameter derivatives \(addEnergyParameterDerivative 'lambda_restraints'\) of a restraint force"):
        r.addEnergyParameterDerivative('lambda_restraints')
    ho = CustomExternalForce(CustomExternalForce.HARMONIC_EXPRESSION)
    for n in ('testsystems_HarmonicOscillator_K', 'testsystems_HarmonicOscillator_x0', 'testsystems_HarmonicOscillator_U0'):
        ho.addGlobalParameter(n, 1.0)
    ho.addParticle(0)
    ho.addEnergyParameterDerivative('testsystems_HarmonicOscillator_K')
    with pytest.raises(NotImplementedError, match='CustomExternalForce: energy parameter derivatives .* of the built-in harmonic oscillator form'):
        system_to_desc(_system([ho]))


class _Foreign:
    """an object with OpenMM's getters and none of this package's attributes"""

    def __init__(self, force):
        self._f = force

    def __getattr__(self, name):
        if name.startswith('_'):
            raise AttributeError(name)
        return getattr(self._f, name)


def test_from_openmm_by_the_objects_getters():
    h = CustomHbondForce('a*distance(d1,a1)'); h.addGlobalParameter('a', 1.0); h.addGlobalParameter('b', 1.0)
    h.addDonor(0, -1, -1); h.addAcceptor(1, -1, -1); h.addEnergyParameterDerivative('b')
    assert hbond_force_from_openmm(_Foreign(h))._derivatives == ['b']
    m = CustomManyParticleForce(3, 'a*distance(p1,p2)'); m.addGlobalParameter('a', 1.0)
    for _ in range(3):
        m.addParticle([], 0)
    m.addEnergyParameterDerivative('a')
    assert manyparticle_force_from_openmm(_Foreign(m))._derivatives == ['a']
    gb = CustomGBForce(); gb.addGlobalParameter('a', 1.0)
    declared = _Foreign(gb)
    declared.getNumEnergyParameterDerivatives = lambda: 1
    declared.getEnergyParameterDerivativeName = lambda i: 'a'
    with pytest.raises(NotImplementedError, match='CustomGBForce: energy parameter derivatives'):
        gb_force_from_openmm(declared)


def test_a_library_without_the_entry_points():
    eng = _engine.HipEngine.__new__(_engine.HipEngine)
    eng.lib = types.SimpleNamespace()                     # (the CPU port: none of the GPU-only entry points)
    for call in (lambda: eng.custom_energy_parameter_derivatives(), lambda: eng.set_custom_parameter_derivatives([0], [1], ['a'])):
        with pytest.raises(NotImplementedError, match=r'remd_[gs]et_custom_parameter_derivatives: this build of the engine library has no energy parameter '
                                                      r'derivatives of custom forces .*include/remd_hip_custom.h'):
            call()
