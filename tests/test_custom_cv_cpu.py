"""CPU: system.RMSDForce and system.CustomCVForce on the host (openmmtools_amd/system.py, custom_expr.py, _engine.py) and the helper
the GPU tests compare against (tests/custom_cv_oracle.py): the helper is held to finite differences of its own RMSD and to mpmath at 50
digits; the compiler and the descriptor; every refusal by its message; the accessors; the stores' and pools' refusals."""
import copy

import numpy as np
import pytest

import custom_cv_oracle as oracle
from openmmtools_amd import alchemy, custom_expr as cx, states, testsystems, unit
from openmmtools_amd.system import (System, system_to_desc, RMSDForce, CustomCVForce, CustomBondForce, Continuous1DFunction, NonbondedForce)

RNG = np.random.default_rng(11)
N = 12
REF = RNG.uniform(-0.6, 0.6, (N, 3))


def _system(n=N):
    s = System()
    for _ in range(n):
        s.addParticle(12.0)
    return s


def _harmonic(particles=(7, 1, 2, 9, 4), k=500.0, v0=0.05):
    f = CustomCVForce('0.5*k*(v-v0)^2')
    f.addGlobalParameter('k', k); f.addGlobalParameter('v0', v0)
    f.addCollectiveVariable('v', RMSDForce(REF, particles))
    return f


def _desc(*forces, n=N):
    s = _system(n)
    for f in forces:
        s.addForce(f)
    return system_to_desc(s)


# ---- the helper itself -------------------------------------------------------------------------------------------------------------------
def _rotation(rng):
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    a, b, c, d = q
    return np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                     [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                     [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])


@pytest.mark.parametrize('n', [3, 4, 17])
def test_the_helpers_gradient_against_central_differences_of_its_own_rmsd(n):
    rng = np.random.default_rng(n)
    ref = rng.uniform(-0.5, 0.5, (n, 3))
    x = ref @ _rotation(rng).T + rng.normal(0.0, 0.05, (n, 3)) + [3.0, -2.0, 1.0]
    v, U, grad = oracle.kabsch(x, ref)
    assert abs(np.linalg.det(U) - 1.0) < 1e-12 and v > 0.01
    h = 1e-6
    fd = np.zeros_like(x)
    for i in range(n):
        for c in range(3):
            p, m = x.copy(), x.copy()
            p[i, c] += h; m[i, c] -= h
            fd[i, c] = (oracle.rmsd(p, ref) - oracle.rmsd(m, ref)) / (2 * h)
    # (central differences of a smooth function: h^2 f''' / 6 ~ 1e-12 / v^2 truncation and 1e-16 / h rounding)
    assert np.abs(fd - grad).max() < 1e-8
    assert np.abs(grad.sum(axis=0)).max() < 1e-14 and np.abs(np.cross(x - x.mean(axis=0), grad).sum(axis=0)).max() < 1e-14


def _mp_rmsd(x, ref):
    """the RMSD at 50 digits through the largest eigenvalue of Horn's matrix (another route than the helper's SVD)"""
    import mpmath                                                                  # (absent: a failure, these tests anchor the GPU bounds)
    mp = mpmath.mp
    mp.dps = 50
    n = len(x)
    X = [[mpmath.mpf(float(v)) for v in row] for row in x]
    Y = [[mpmath.mpf(float(v)) for v in row] for row in ref]
    cx_ = [sum(r[k] for r in X) / n for k in range(3)]
    cy = [sum(r[k] for r in Y) / n for k in range(3)]
    X = [[r[k] - cx_[k] for k in range(3)] for r in X]
    Y = [[r[k] - cy[k] for k in range(3)] for r in Y]
    S = [[sum(Y[i][a] * X[i][b] for i in range(n)) for b in range(3)] for a in range(3)]      # Horn's M = sum y x^T
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = S
    Nm = mpmath.matrix([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                        [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                        [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy],
                        [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]])
    lam = max(mpmath.eigsy(Nm, eigvals_only=True))
    G = sum(v * v for r in X for v in r) + sum(v * v for r in Y for v in r)
    msd = (G - 2 * lam) / n
    return mpmath.sqrt(msd) if msd > 0 else mpmath.mpf(0)


@pytest.mark.parametrize('case', ['generic', 'small', 'mirrored', 'planar', 'half_turn'])
def test_the_helpers_rmsd_against_mpmath_at_50_digits(case):
    rng = np.random.default_rng(5)
    n = 7
    ref = rng.uniform(-0.5, 0.5, (n, 3))
    if case == 'planar':
        ref[:, 2] = 0.1
    R = _rotation(rng)
    if case == 'half_turn':
        a = rng.normal(size=3); a /= np.linalg.norm(a)
        R = 2.0 * np.outer(a, a) - np.eye(3)
    x = ref @ R.T + rng.normal(0.0, 1e-4 if case == 'small' else 0.05, (n, 3))
    if case == 'mirrored':
        x[:, 0] *= -1.0
    want = float(_mp_rmsd(x, ref))
    got = oracle.rmsd(x, ref)
    print(case, got, want, abs(got - want) / want)
    assert want > 1e-5 and abs(got - want) <= 1e-12 * want
    if case == 'mirrored':
        assert got > 0.1                                                           # (an improper U would have brought it to ~0.05)


# ---- compiler and descriptor ----------------------------------------------------------------------------------------------------------
def test_variables_compile_to_var_operands_and_the_reference_is_centred():
    a, b, c = RMSDForce(REF, [0, 1, 2, 3]), RMSDForce(REF, [3, 4, 5, 6, 7]), RMSDForce(REF)
    f = CustomCVForce('k*first*second + third; k = 2*scale')
    f.addGlobalParameter('scale', 3.0)
    for name, v in (('first', a), ('second', b), ('third', c)):
        f.addCollectiveVariable(name, v)
    t = _desc(f)['custom_terms']['000']
    assert t['kind'] == cx.KIND_CV == 7 and t['cv_names'] == ['first', 'second', 'third']
    ops = [tuple(i) for i in t['program'].tolist()]
    assert [(cx.VAR, 0), (cx.VAR, 1), (cx.VAR, 2)] == [i for i in ops if i[0] == cx.VAR]
    assert (cx.GLOBAL, 0) in ops and not any(i[0] == cx.PARAM for i in ops)
    assert t['cv_offsets'].tolist() == [0, 4, 9, 9 + N] and t['cv_offsets'].dtype == np.int32
    assert t['cv_atoms'].tolist() == [0, 1, 2, 3, 3, 4, 5, 6, 7] + list(range(N))
    assert t['cv_reference'].dtype == np.float64 and t['cv_reference'].shape == (9 + N, 3)
    for k, rows in enumerate(([0, 1, 2, 3], [3, 4, 5, 6, 7], list(range(N)))):
        got = t['cv_reference'][t['cv_offsets'][k]:t['cv_offsets'][k + 1]]
        assert np.abs(got.sum(axis=0)).max() < 1e-15 * len(rows) and np.allclose(got, REF[rows] - REF[rows].mean(axis=0), rtol=0, atol=1e-16)
    assert t['periodic'] == 0 and t['atoms'].shape == (1, 0) and t['params'].shape == (1, 0)
    assert t['global_names'] == ['scale'] and t['energy'] == f.getEnergyFunction()


def test_a_bare_rmsd_force_acts_as_a_cv_force_of_v_and_shares_the_limits():
    r = RMSDForce(REF, [5, 6, 7]); r.setForceGroup(3)
    other = CustomBondForce('q*r^2'); other.addGlobalParameter('q', 2.0); other.addBond(0, 1, []); other.setForceGroup(3)
    terms = _desc(other, r)['custom_terms']
    assert [terms[k]['kind'] for k in sorted(terms)] == [cx.KIND_BOND, cx.KIND_CV]
    t = terms['001']
    assert t['program'].tolist() == [[cx.VAR, 0]] and t['cv_names'] == ['v'] and t['force_group'] == 3 and t['global_names'] == ['q']
    with pytest.raises(NotImplementedError, match=r'9 custom forces in one System \(the engine takes 8\)'):
        _desc(*[RMSDForce(REF, [0, 1, 2]) for _ in range(9)])
    r2 = RMSDForce(REF, [0, 1, 2]); r2.setForceGroup(1)
    with pytest.raises(NotImplementedError, match='custom forces in several force groups'):
        _desc(r, r2)
    many = CustomCVForce('v' + ''.join('+g%d' % i for i in range(17)))
    many.addCollectiveVariable('v', RMSDForce(REF))
    for i in range(17):
        many.addGlobalParameter('g%d' % i, 0.0)
    with pytest.raises(NotImplementedError, match='17 global parameters'):
        _desc(many)


def test_tables_and_definitions_compile():
    f = CustomCVForce('scale*t(a) + w; w = 0.5*a^2')
    f.addGlobalParameter('scale', 1.0)
    f.addCollectiveVariable('a', RMSDForce(REF, [0, 1, 2, 3]))
    f.addTabulatedFunction('t', Continuous1DFunction(np.linspace(0.0, 1.0, 9) ** 2, 0.0, 1.0))
    t = _desc(f)['custom_terms']['000']
    assert cx.TABLE1D in t['program'][:, 0]


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _cv(energy, *variables, globals_=()):
    f = CustomCVForce(energy)
    for name, v in variables:
        f.addCollectiveVariable(name, v)
    for name in globals_:
        f.addGlobalParameter(name, 1.0)
    return f


def test_refusals_name_the_force_and_the_item():
    ok = RMSDForce(REF, [0, 1, 2])
    with pytest.raises(NotImplementedError, match=r'CustomCVForce \(energy .*\): 4 collective variables \(the engine takes 1 ... 3\): a, b, c, d'):
        _desc(_cv('a+b+c+d', ('a', ok), ('b', ok), ('c', ok), ('d', ok)))
    with pytest.raises(ValueError, match='has no collective variable'):
        _desc(_cv('1'))
    with pytest.raises(NotImplementedError, match=r"CustomCVForce: collective variable 'd' is a CustomBondForce \(only RMSDForce"):
        _desc(_cv('d', ('d', CustomBondForce('r'))))
    with pytest.raises(ValueError, match=r"collective variable 'v': RMSDForce over 2 particles \(an RMSD after superposition needs at least 3\)"):
        _desc(_cv('v', ('v', RMSDForce(REF, [0, 1]))))
    with pytest.raises(ValueError, match=r"collective variable 'v': RMSDForce names particle 12 \(the System has 12\)"):
        _desc(_cv('v', ('v', RMSDForce(REF, [0, 1, 12]))))
    with pytest.raises(ValueError, match="collective variable 'v': RMSDForce names particle -1"):
        _desc(_cv('v', ('v', RMSDForce(REF, [0, 1, -1]))))
    with pytest.raises(ValueError, match="collective variable 'v': RMSDForce names particle 4 twice"):
        _desc(_cv('v', ('v', RMSDForce(REF, [4, 1, 4]))))
    with pytest.raises(ValueError, match=r"collective variable 'v': RMSDForce has 11 reference positions, the System has 12 particles"):
        _desc(_cv('v', ('v', RMSDForce(REF[:11], [0, 1, 2]))))
    with pytest.raises(ValueError, match=r"RMSDForce has 12 reference positions, the System has 13"):
        _desc(RMSDForce(REF), n=13)
    with pytest.raises(ValueError, match="collective variable 'k' is also a global parameter of the force"):
        _desc(_cv('k', ('k', ok), globals_=('k',)))
    with pytest.raises(ValueError, match="collective variable 'v' is named twice"):
        _desc(_cv('v', ('v', ok), ('v', ok)))
    with pytest.raises(NotImplementedError, match=r"CustomCVForce.*unknown variable 'w'"):
        _desc(_cv('v+w', ('v', ok)))
    with pytest.raises(NotImplementedError, match=r"CustomCVForce: energy parameter derivatives \(addEnergyParameterDerivative 'k'\)"):
        _cv('k*v', ('v', ok), globals_=('k',)).addEnergyParameterDerivative('k')
    with pytest.raises(NotImplementedError, match='RMSDForce: changing the reference positions or the particles after set_system'):
        ok.updateParametersInContext(None)
    with pytest.raises(ValueError, match=r'RMSDForce: reference positions of shape \(12,\)'):
        RMSDForce(np.zeros(12))


def test_a_variable_across_molecules_of_a_periodic_system_is_refused():
    """two three-site molecules (joined by exceptions) in a periodic box: a variable inside one passes, one across both is refused by
    name; without a box nothing wraps and both pass"""
    def build(method, particles):
        s = _system(6)
        nb = NonbondedForce(); nb.setNonbondedMethod(method); nb.setCutoffDistance(0.9)
        for _ in range(6):
            nb.addParticle(0.0, 0.3, 0.1)
        for a, b in ((0, 1), (1, 2), (0, 2), (3, 4), (4, 5), (3, 5)):
            nb.addException(a, b, 0.0, 0.3, 0.0)
        s.addForce(nb)
        s.setDefaultPeriodicBoxVectors([3.0, 0, 0], [0, 3.0, 0], [0, 0, 3.0])
        s.addForce(_cv('v', ('v', RMSDForce(REF[:6], particles))))
        return system_to_desc(s)
    assert build(NonbondedForce.CutoffPeriodic, [0, 1, 2])['custom_terms']['000']['kind'] == cx.KIND_CV
    with pytest.raises(NotImplementedError, match=r"collective variable 'v' spans 2 molecules of a periodic System.*imaging across molecules is not supported"):
        build(NonbondedForce.CutoffPeriodic, [1, 2, 3])
    assert build(NonbondedForce.NoCutoff, [1, 2, 3])['custom_terms']['000']['cv_atoms'].tolist() == [1, 2, 3]
    assert cx.barostat_molecules(build(NonbondedForce.CutoffPeriodic, [0, 1, 2])).tolist() == [0, 0, 0, 1, 1, 1]


# ---- API ----------------------------------------------------------------------------------------------------------------------------------
def test_accessors_round_trip():
    r = RMSDForce(REF * unit.nanometer, [3, 1, 2])
    assert np.array_equal(r.getReferencePositions(), REF) and r.getParticles() == [3, 1, 2] and r.usesPeriodicBoundaryConditions() is False
    r.getReferencePositions()[0, 0] = 99.0                                            # (a copy: the force keeps its own)
    assert r.getReferencePositions()[0, 0] == REF[0, 0]
    r.setParticles([4, 5, 6, 7]); r.setReferencePositions(2.0 * REF); r.setForceGroup(5)
    assert r.getParticles() == [4, 5, 6, 7] and np.array_equal(r.getReferencePositions(), 2.0 * REF) and r.getForceGroup() == 5
    assert RMSDForce(REF).getParticles() == []
    f = CustomCVForce('k*a*b')
    assert f.addGlobalParameter('k', 2.5) == 0 and f.addCollectiveVariable('a', r) == 0 and f.addCollectiveVariable('b', RMSDForce(REF)) == 1
    assert f.getNumCollectiveVariables() == 2 and f.getCollectiveVariableName(1) == 'b' and f.getCollectiveVariable(0) is r
    assert f.getEnergyFunction() == 'k*a*b' and f.getGlobalParameterDefaultValue(0) == 2.5 and f.usesPeriodicBoundaryConditions() is False
    assert f.getNumEnergyParameterDerivatives() == 0
    assert f.addTabulatedFunction('t', Continuous1DFunction([0.0, 1.0, 4.0], 0.0, 2.0)) == 0 and f.getNumTabulatedFunctions() == 1
    g = copy.deepcopy(f)
    assert g.getCollectiveVariable(0).getParticles() == [4, 5, 6, 7]


def test_stores_and_pools_refuse_by_name():
    from openmmtools_amd import system_xml
    from openmmtools_amd.multistate._reference_store import ReferenceStoreWriter
    from openmmtools_amd.multistate._engine_pool import EnginePool
    for force, name in ((_harmonic(), 'CustomCVForce'), (RMSDForce(REF, [0, 1, 2]), 'RMSDForce')):
        s = _system(); s.addForce(force)
        with pytest.raises(NotImplementedError, match='%s with the energy' % name):
            system_xml.to_xml(s)
        assert name in ReferenceStoreWriter.can_store([states.ThermodynamicState(s, 300.0)], [], [])      # (layout='auto' then keeps records)

    class Stub:
        def spawn(self): return Stub()
    d = system_to_desc(s)
    with pytest.raises(NotImplementedError, match='more than one compatibility group'):
        EnginePool(Stub(), [[0], [1]]).set_system([d, d])


def test_global_table_and_alchemical_factory_take_the_force():
    class KState(states.GlobalParameterState):
        k = states.GlobalParameterState.GlobalParameter('k', standard_value=1.0)
    f = _harmonic(k=40.0)
    s = _system(); s.addForce(f); s.addForce(RMSDForce(REF))
    assert KState.from_system(s).k == 40.0
    ts = states.ThermodynamicState(s, 300.0)
    compound_states = [states.CompoundThermodynamicState(copy.deepcopy(ts), [KState(k=v)]) for v in (100.0, 0.0)]
    assert np.array_equal(cx.custom_globals(s, ['k', 'v0'], compound_states + [ts]), [[100.0, 0.05], [0.0, 0.05], [40.0, 0.05]])
    al = testsystems.AlanineDipeptideVacuum()
    g = CustomCVForce('k*v'); g.addGlobalParameter('k', 3.0); g.addCollectiveVariable('v', RMSDForce(al.positions, [4, 6, 8, 14]))
    al.system.addForce(g)
    system = alchemy.AbsoluteAlchemicalFactory().create_alchemical_system(al.system, alchemy.AlchemicalRegion(alchemical_atoms=list(range(0, 6))))
    kept = [h for h in system.getForces() if isinstance(h, CustomCVForce)]
    assert len(kept) == 1 and kept[0].getEnergyFunction() == 'k*v' and kept[0].getCollectiveVariable(0).getParticles() == [4, 6, 8, 14]
    assert [t['kind'] for t in system_to_desc(system)['custom_terms'].values()] == [cx.KIND_CV]


def test_a_changed_reference_is_another_system():
    s1 = _system(); s1.addForce(RMSDForce(REF, [0, 1, 2, 3]))
    s2 = _system(); s2.addForce(RMSDForce(REF + [0.0, 0.0, 1.0], [0, 1, 2, 3]))      # a translated reference: the same centred rows
    s3 = _system(); s3.addForce(RMSDForce(1.01 * REF, [0, 1, 2, 3]))
    assert s1.fingerprint() != s3.fingerprint()
    a, b = (system_to_desc(s)['custom_terms']['000']['cv_reference'] for s in (s1, s2))
    assert np.abs(a - b).max() < 1e-15


# ---- engine binding ---------------------------------------------------------------------------------------------------------------------
def test_a_library_without_the_entry_points_names_the_header():
    from openmmtools_amd import _engine

    class Old:
        """a library built before the collective-variable forces: every custom entry point but remd_get_custom_cv_values"""
        def remd_set_custom_terms(self, *a): raise AssertionError('must not be reached')
    eng = _engine.HipEngine.__new__(_engine.HipEngine)
    eng.lib, eng.h = Old(), None
    terms = _desc(_harmonic())['custom_terms']
    with pytest.raises(NotImplementedError, match=r'remd_get_custom_cv_values.*CustomCVForce / RMSDForce.*include/remd_hip_custom.h'):
        eng.set_custom_terms([terms['000']])
    with pytest.raises(NotImplementedError, match=r'remd_get_custom_cv_values.*include/remd_hip_custom.h'):
        eng.custom_cv_values()
    assert _engine.RemdCustomForceDesc._fields_[-4:] == [('n_cvs', _engine.C.c_int32), ('cv_offsets', _engine.c_int32_p),
                                                         ('cv_atoms', _engine.c_int32_p), ('cv_reference', _engine.c_double_p)]


def test_the_cpu_port_refuses_the_force():
    import os
    from openmmtools_amd import _engine
    here = os.path.dirname(os.path.abspath(__file__))
    cpu_lib = os.path.join(os.path.dirname(here), 'oracle', '_build', 'libremd_cpu.so')
    if not os.path.exists(cpu_lib):
        import __graft_entry__
        __graft_entry__.build()
    eng = _engine.HipEngine(lib_path=cpu_lib)
    al = testsystems.AlanineDipeptideVacuum()
    al.system.addForce(RMSDForce(al.positions, [4, 6, 8, 14]))
    with pytest.raises(NotImplementedError, match='remd_set_custom_terms.*remd_hip_custom.h'):
        eng.set_system(system_to_desc(al.system))


def test_a_periodic_system_without_a_nonbonded_force_is_refused_in_its_own_words():
    """periodic through a CutoffPeriodic CustomNonbondedForce alone: the host has no molecule table to test the variable against"""
    fluid = testsystems.CustomLennardJonesFluidMixture(nparticles=64, dispersion_correction=False)
    fluid.system.forces[:] = [f for f in fluid.system.forces if not isinstance(f, NonbondedForce)]
    assert system_to_desc(fluid.system)['nb_method'] == 0
    fluid.system.addForce(RMSDForce(fluid.positions, [0, 1, 2, 3]))
    with pytest.raises(NotImplementedError, match=r"collective variable 'v' in a periodic System without a NonbondedForce.*known to the library only"):
        system_to_desc(fluid.system)


# ---- the device's superposition, compiled for the host ----------------------------------------------------------------------------------
HOST_WRAPPER = '''
#include "custom_cv_math.h"
extern "C" int superpose(const double* S, double* U)
{
    double s[3][3], u[3][3];
    for (int i = 0; i < 9; ++i) s[i / 3][i % 3] = S[i];
    const int sweeps = cv_superpose(s, u);
    for (int i = 0; i < 9; ++i) U[i] = u[i / 3][i % 3];
    return sweeps;
}
'''


def test_the_devices_superposition_on_the_host_against_the_helper(tmp_path):
    """csrc/custom_cv_math.h is plain C++: compiled here with the host compiler, cv_superpose is held to the SVD helper over random,
    planar, collinear, mirrored, exactly superposable and coincident sets (the degenerate spectra, without a GPU), and the Jacobi sweeps
    it takes are counted: the figure profiles/custom_cv_cost.txt quotes"""
    import ctypes
    import os
    import shutil
    import subprocess
    cxx = shutil.which('g++') or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'openmmtools_amd', 'csrc')
    (tmp_path / 'wrap.cpp').write_text(HOST_WRAPPER)
    lib_path = str(tmp_path / 'libcvhost.so')
    subprocess.check_call([cxx, '-O2', '-std=c++17', '-shared', '-fPIC', '-I', csrc, str(tmp_path / 'wrap.cpp'), '-o', lib_path])
    lib = ctypes.CDLL(lib_path)
    rng = np.random.default_rng(1)
    most, worst = 0, 0.0
    for case in range(1200):
        kind = case % 6
        n = int(rng.integers(3, 40))
        ref = rng.normal(size=(n, 3))
        if kind == 1:
            ref[:, 2] = 0.0
        if kind == 2:
            ref[:, 1:] = 0.0
        x = ref @ _rotation(rng).T
        if kind == 3:
            x[:, 0] *= -1.0
        x += rng.normal(size=x.shape) * (0.0 if kind == 4 else 0.1)
        if kind == 5:
            x[:] = x[0]
        xc, yc = x - x.mean(axis=0), ref - ref.mean(axis=0)
        S, U = np.ascontiguousarray(xc.T @ yc), np.zeros(9)
        most = max(most, lib.superpose(S.ctypes.data_as(ctypes.c_void_p), U.ctypes.data_as(ctypes.c_void_p)))
        U = U.reshape(3, 3)
        assert abs(np.linalg.det(U) - 1.0) < 1e-12 and np.abs(U @ U.T - np.eye(3)).max() < 1e-12
        got, want = np.sqrt(((xc - yc @ U.T) ** 2).sum() / n), oracle.rmsd(x, ref)
        worst = max(worst, abs(got - want) / want if want > 1e-9 else abs(got - want))
    print('cv_superpose on the host: at most %d Jacobi sweeps, RMSD within %.3g of the helper' % (most, worst))
    # (the direct sum is stationary in U: U's 1e-15 enters squared, what is left is the rounding of n terms of either sum)
    assert worst < 1e-12 and most <= 8
