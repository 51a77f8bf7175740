"""Forces of selected force groups (remd_get_group_forces, OpenMM's getState(getForces=True, groups=mask)) on both libraries.

A multiple-time-step splitting evaluates one force group at a time: remd_compute_forces with the class mask of that group.  Every
subset S of a system's force classes (1 bonds, 2 angles, 3 torsions, 4 direct-space nonbonded with exceptions, the Ewald exclusion
correction and GBSA, 5 reciprocal space) goes to group 0 and the rest to group 3, and then
  (a) the listed terms in atom order (the default) give the same bits as the term-per-thread launch (REMD_LISTED_ATOMS=0): an idle
      lane inside an atom's run of entries (a class switched off) must not make the segmented scan count a partial sum twice;
  (b) the groups add up to the whole, exactly: the forces are sums of 2^-32 kJ/mol/nm fixed-point integers;
  (c) each group follows the f64 oracle, class by class (oracle/forcefield.py; oracle/gbsa.py for the implicit solvent; the
      restraint in numpy);
  (d) a mask that selects nothing gives exact zeros, and groups 7 and 31 (which multiple-time-step programs refuse) work;
  (e) on PME systems the listed terms on the direct-space stream (REMD_LISTED_MAIN=0) or as a launch of their own
      (REMD_LISTED_RIDE=0) give the same bits.
(b), (c), (d) also hold for the C++ port of the ABI (libremd_cpu.so)."""
import copy
import itertools
import os

import numpy as np
import pytest

import oracle
from oracle.forcefield import ForceFieldOracle
from oracle.gbsa import gbsa_energy_forces
from oracle_engine import OracleEngine
from openmmtools_amd import testsystems as ts, forces
from openmmtools_amd.system import system_to_desc, System, HarmonicBondForce, HarmonicAngleForce, PeriodicTorsionForce

KB = 0.008314462618153242
CPU_LIB = os.path.join(os.path.dirname(os.path.abspath(oracle.__file__)), '_build', 'libremd_cpu.so')
NAMES = {1: 'bonds', 2: 'angles', 3: 'torsions', 4: 'nonbonded', 5: 'reciprocal'}


def _chain():
    """0-1-2-3: three bonds, two angles, one torsion (two periodicities), nothing else -- atom 0's entries are
    [bond, angle, torsion], so bonds + torsions leave an idle angle lane inside its run"""
    s = System()
    for _ in range(4):
        s.addParticle(12.0)
    b, a, t = HarmonicBondForce(), HarmonicAngleForce(), PeriodicTorsionForce()
    for i in range(3):
        b.addBond(i, i + 1, 0.15, 2.0e5)
    for i in range(2):
        a.addAngle(i, i + 1, i + 2, 1.9, 400.0)
    t.addTorsion(0, 1, 2, 3, 3, 0.0, 2.0)
    t.addTorsion(0, 1, 2, 3, 1, 0.5, 1.0)
    for f in (b, a, t):
        s.addForce(f)
    x = np.array([[0.0, 0.0, 0.0], [0.16, 0.01, 0.0], [0.21, 0.15, 0.02], [0.36, 0.17, 0.11]])
    return s, x, (1, 2, 3)


def _testsystem(name):
    """(System, positions, force classes present)"""
    if name == 'chain':
        return _chain()
    if name == 'hostguest':
        hg = ts.HostGuestExplicit()
        hg.system.addForce(forces.HarmonicRestraintForce(2000.0, list(range(0, 126)), list(range(126, 156))))
        return hg.system, np.array(hg.positions, dtype=np.float64), (1, 2, 3, 4, 5)
    t = {'vacuum': ts.AlanineDipeptideVacuum, 'implicit': ts.AlanineDipeptideImplicit, 'explicit': ts.AlanineDipeptideExplicit,
         'dhfr': ts.DHFRExplicit}[name]()
    return t.system, np.array(t.positions, dtype=np.float64), (1, 2, 3, 4) if name in ('vacuum', 'implicit') else (1, 2, 3, 4, 5)


def _subsets(classes):
    return [S for k in range(len(classes) + 1) for S in itertools.combinations(classes, k)]


def _groups(S, high=3):
    """force groups of (external, bonds, angles, torsions, direct space, reciprocal space): S in group 0, the rest in group `high`"""
    return [0] + [0 if c in S else high for c in range(1, 6)]


def _label(S):
    return '+'.join(NAMES[c] for c in S) or '(none)'


def _fix(f):
    """the device's fixed-point integers (REMD_FORCE_SCALE = 2^32; |f| 2^32 < 2^53, so exact)"""
    return np.rint(np.asarray(f) * 2.0 ** 32).astype(np.int64)


def _box(system, R):
    return np.tile(np.diag(np.asarray(system.getDefaultPeriodicBoxVectors(), dtype=np.float64)), (R, 1))


def _engine(eng, desc, x, box):
    R = len(x)
    eng.set_system(desc)
    eng.set_states(np.full(1, 1.0 / (KB * 300.0)))
    if desc.get('restraints'):
        eng.set_restraint_lambdas(np.ones((1, len(desc['restraints']))))
    eng.set_replicas(R, 0, x, None, box, np.zeros(R, dtype=np.int64))
    return eng


def _replicas(x, R=2):
    rng = np.random.default_rng(11)
    return np.stack([x + 0.002 * rng.normal(size=x.shape) * (r > 0) for r in range(R)])


def _set_restraint_group(eng, desc, g):
    rs = desc.get('restraints')
    if rs:
        eng.set_restraints([dict(rs[k], force_group=g) for k in sorted(rs)])
        eng.set_restraint_lambdas(np.ones((1, len(rs))))


def _numpy_restraint(desc, x, box):
    """f64 forces of the (harmonic, lambda 1) centroid restraints of a desc at positions x [N][3]"""
    F = np.zeros_like(x)
    for r in desc.get('restraints', {}).values():
        a1, a2 = np.asarray(r['atoms1']), np.asarray(r['atoms2'])
        w1, w2 = (np.asarray(r['weights%d' % g], dtype=np.float64) for g in (1, 2))
        w1, w2 = w1 / w1.sum(), w2 / w2.sum()
        d = (w2[:, None] * x[a2]).sum(0) - (w1[:, None] * x[a1]).sum(0)
        if r['periodic'] and box is not None:
            d -= box * np.rint(d / box)
        assert r['r0'] == 0.0
        np.add.at(F, a1, (r['K'] * d)[None, :] * w1[:, None])
        np.add.at(F, a2, -(r['K'] * d)[None, :] * w2[:, None])
    return F


def _oracle_classes(desc, x, box, classes):
    """f64 forces of every force class of `classes` (and of the restraints, key 'rst') at positions x [R][N][3]"""
    d0 = dict(desc)
    gb = d0.pop('gbsa', None)
    d0.pop('restraints', None)
    ff = ForceFieldOracle(d0)
    out = {}
    for c in classes:
        out[c] = np.stack([ff.energy_forces(x[r], box[r] if box[r].any() else None, classes={c})[1] for r in range(len(x))])
        if c == 4 and gb is not None:
            out[c] = out[c] + np.stack([gbsa_energy_forces(x[r], gb['charge'], gb['radius'], gb['scale'], gb['alchemical'], 1.0,
                                                           gb['solute_dielectric'], gb['solvent_dielectric'],
                                                           sasa=bool(gb['surface_area']))[1] for r in range(len(x))])
    if desc.get('restraints'):
        out['rst'] = np.stack([_numpy_restraint(desc, x[r], box[r] if box[r].any() else None) for r in range(len(x))])
    return out


def _follows(f, ref, what, max_rel=1e-3, rmse_max=2.5):
    """test_alanine_energy_and_forces's criteria for one group's forces: max error <= max_rel x the group's own max |f_ref|,
    RMS error per atom below rmse_max kJ/mol/nm"""
    scale = np.abs(ref).max()
    for r in range(len(f)):
        err = np.abs(f[r] - ref[r]).max()
        rmse = np.sqrt(((f[r] - ref[r]) ** 2).sum(axis=1).mean())
        assert err <= max_rel * scale and rmse < rmse_max, (what, r, err, scale, rmse)


# ---- GPU ----------------------------------------------------------------------------------------------------------------

GPU_SYSTEMS = ['chain', 'vacuum', 'implicit', 'explicit', 'hostguest', 'dhfr']


@pytest.fixture(scope='module')
def systems():
    cache = {}

    def get(name):
        if name not in cache:
            system, x, classes = _testsystem(name)
            desc = system_to_desc(system)
            cache[name] = (system, desc, _replicas(x), classes)
        return cache[name]
    return get


def _handle(make, monkeypatch, desc, x, box, **env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        eng = _engine(make(), desc, x, box)     # (the switches are read once, when the handle is created)
    finally:
        for k in env:
            monkeypatch.delenv(k)
    return eng


@pytest.mark.gpu
@pytest.mark.parametrize('name', GPU_SYSTEMS)
def test_group_forces_are_exact(hip_engine_factory, monkeypatch, systems, name):
    """(a), (b), (d), (e) for every subset of the force classes; the restraint in a group of its own (5) and in the bonds' group"""
    system, desc, x, classes = systems(name)
    box = _box(system, len(x))
    pme = desc['nb_method'] == 2
    eng = _handle(hip_engine_factory, monkeypatch, desc, x, box)
    variants = {'REMD_LISTED_ATOMS=0': _handle(hip_engine_factory, monkeypatch, desc, x, box, REMD_LISTED_ATOMS='0')}
    if pme:
        variants['REMD_LISTED_RIDE=0'] = _handle(hip_engine_factory, monkeypatch, desc, x, box, REMD_LISTED_RIDE='0')
        variants['REMD_LISTED_MAIN=0'] = _handle(hip_engine_factory, monkeypatch, desc, x, box, REMD_LISTED_MAIN='0')
    full = _fix(eng.get_forces())
    assert np.any(full != 0)
    rst_placements = ['own', 'bonds'] if desc.get('restraints') else [None]
    wrong, one = [], {}
    for S in _subsets(classes):
        for rst in rst_placements:
            fg = _groups(S)
            masks = [1, 8]
            for e in [eng] + list(variants.values()):
                e.set_force_groups(fg)
                if rst is not None:
                    _set_restraint_group(e, desc, 5 if rst == 'own' else fg[1])
            if rst == 'own':
                masks.append(32)
            got = {m: eng.get_forces(groups=m) for m in masks}
            # (b) the groups add up to the whole
            total = sum(_fix(got[m]) for m in masks)
            if not np.array_equal(total, full):
                wrong.append(('sum', _label(S), rst, np.abs(total - full).max() / 2.0 ** 32))
            # (a), (e) the other organisations of the listed terms give the same bits
            for what, e in variants.items():
                for m in masks:
                    fv = e.get_forces(groups=m)
                    if not np.array_equal(fv, got[m]):
                        wrong.append((what, _label(S), rst, m, np.abs(fv - got[m]).max()))
            if len(S) == 1 and rst in (None, 'own'):
                one[S[0]] = got[1]
    assert not wrong, 'groups whose forces differ (check, subset in group 0, restraint, mask, max |df| kJ/mol/nm): %s' % wrong
    # (d) an empty mask, and groups 7 and 31: bonds in 7, angles in 31, the rest in 0
    for e in [eng] + list(variants.values()):
        e.set_force_groups([0, 7, 31, 0, 0, 0])
        if desc.get('restraints'):
            _set_restraint_group(e, desc, 0)
        assert np.array_equal(e.get_forces(groups=0), np.zeros_like(x))
        g7, g31, g0 = (e.get_forces(groups=1 << g) for g in (7, 31, 0))
        assert np.array_equal(g7, one[1]) and np.array_equal(g31, one[2])
        assert np.array_equal(_fix(g7) + _fix(g31) + _fix(g0), full)
        assert np.array_equal(_fix(e.get_forces(groups=(1 << 7) | (1 << 31) | 1)), full)
        assert np.array_equal(_fix(e.get_forces()), full)


@pytest.mark.gpu
@pytest.mark.parametrize('name', [n for n in GPU_SYSTEMS if n != 'dhfr'])
def test_group_forces_follow_the_oracle(hip_engine_factory, systems, name):
    """(c): each group's forces against the f64 oracle, evaluated once per class and summed per subset"""
    system, desc, x, classes = systems(name)
    box = _box(system, len(x))
    eng = _engine(hip_engine_factory(), desc, x, box)
    xd = eng.get_replicas()[0]
    ref = _oracle_classes(desc, xd, box, classes)
    if 'rst' in ref:
        _set_restraint_group(eng, desc, 5)
        _follows(eng.get_forces(groups=32), ref['rst'], 'restraint')
    for S in _subsets(classes)[1:]:
        eng.set_force_groups(_groups(S))
        _follows(eng.get_forces(groups=1), sum(ref[c] for c in S), _label(S))


# ---- CPU: the same entry on the C++ port of the ABI -----------------------------------------------------------------------

@pytest.fixture(scope='module')
def cpu_lib():
    if not os.path.exists(CPU_LIB):
        oracle.build()
    return CPU_LIB


@pytest.mark.parametrize('name', ['chain', 'explicit'])
def test_cpu_library_group_forces(cpu_lib, name):
    """(b), (c), (d) on libremd_cpu.so; the OracleEngine's get_forces(groups=...) agrees with it"""
    from openmmtools_amd._engine import HipEngine
    system, x, classes = _testsystem(name)
    desc = system_to_desc(system)
    x = _replicas(x)
    box = _box(system, len(x))
    eng = _engine(HipEngine(lib_path=cpu_lib), desc, x, box)
    ora = OracleEngine(ForceFieldOracle)
    try:
        full = eng.get_forces()
        scale = np.abs(full).max()
        ref = _oracle_classes(desc, x, box, classes)
        one = {}
        for S in _subsets(classes):
            eng.set_force_groups(_groups(S))
            f0, f3 = eng.get_forces(groups=1), eng.get_forces(groups=8)
            # (b) two f64 sums of the same terms in another order
            assert np.abs(f0 + f3 - full).max() <= 1e-12 * scale, _label(S)
            # (c) two f64 implementations (the same PME mesh; different FFTs and summation orders)
            for T, f in ((S, f0), (tuple(c for c in classes if c not in S), f3)):
                if T:
                    _follows(f, sum(ref[c] for c in T), _label(T), max_rel=1e-10, rmse_max=1e-8)
                else:
                    assert np.array_equal(f, np.zeros_like(f))
            if len(S) == 1:
                one[S[0]] = f0
        # the test oracle's engine: the same selection through desc['force_groups']
        d3 = dict(desc, force_groups=np.array(_groups((1, 3)), dtype=np.int32))
        _engine(ora, d3, x, box)
        assert np.allclose(ora.get_forces(groups=1), ref[1] + ref[3], rtol=0, atol=1e-9 * scale)
        # (d)
        eng.set_force_groups([0, 7, 31, 0, 0, 0])
        assert np.array_equal(eng.get_forces(groups=0), np.zeros_like(x))
        assert np.array_equal(eng.get_forces(groups=1 << 7), one[1]) and np.array_equal(eng.get_forces(groups=1 << 31), one[2])
        assert np.abs(eng.get_forces(groups=(1 << 7) | (1 << 31) | 1) - full).max() <= 1e-12 * scale
    finally:
        eng.close()
