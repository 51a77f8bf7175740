"""GPU: collective variables of stored frames on the device (include/remd_hip_frame_cvs.h: remd_frame_cvs, csrc/frame_cvs.hip) through
_engine.frame_cvs, on the case table of tests/frame_cvs_cases.py against the independent reference of tests/frame_cvs_oracle.py.  The
bounds are those of the case table's docstring: 1e-10 (nm, rad) in general position, 4 x the device's own recorded error against the
oracle (profiles/frame_cv_errors.txt) for the degenerate families.  Bit-equality: of two calls, of chunked against unchunked calls, of a
variable alone against the same variable among nine.

Figures of the device against the oracle on an MI355X (max |error| over frames and variables; nm, rad): sizes 1.2e-15, sizes-unimaged
5.9e-16, far 1.6e-14, exact 9.7e-17, rmsd-shapes 1.1e-16 (bound 1e-10 each); angle-end 8.2e-10, dihedral-cut 2.3e-16, rmsd-floor 0 (these
three are the recorded values their bounds are 4 x of)."""
import ctypes as C

import numpy as np
import pytest

import frame_cvs_cases as fc
from openmmtools_amd import _engine
from openmmtools_amd._engine import frame_cvs
from openmmtools_amd.multistate import analysis as an

pytestmark = pytest.mark.gpu
CASES = [c.name for c in fc.all_cases()]


def _device(case, **kw):
    return frame_cvs(case.descriptors(an), case.pos, case.box, case.masses, **kw)


@pytest.mark.parametrize('name', CASES)
def test_device_against_the_oracle(name):
    case = fc.case(name)
    v = _device(case)
    assert v.shape == (len(case.pos), len(case.variables)) and v.dtype == np.float64
    err, bound = fc.errors(name, v), fc.bound(name)
    print(name, 'max error per variable', err.max(axis=0), 'bound', bound)
    assert np.all(np.isfinite(v)) and np.all(err <= bound), (name, err.max(), bound)
    assert np.array_equal(_device(case), v)                                     # twice the same call: the same bits


def test_the_degenerate_values_themselves():
    v = _device(fc.case('exact'))[0]
    assert v[0] == 0.0 and v[1] == 0.0 and v[2] == 0.0 and v[3] > 0.1
    a = _device(fc.case('angle-end'))[:, 0]
    assert a[0] == 0.0 and np.all(np.isfinite(a)) and np.all((a >= 0.0) & (a <= np.pi))
    d = _device(fc.case('dihedral-cut'))[:, 0]
    assert np.all(np.abs(d) <= np.pi) and np.all(np.pi - np.abs(d) < 1e-6)
    assert np.all(_device(fc.case('rmsd-floor')) == 0.0)


def test_values_do_not_depend_on_the_chunking_or_on_the_other_variables():
    case = fc.case('sizes')
    cvs = case.descriptors(an)
    timing = {}
    whole = _device(case, timing=timing)
    assert timing['kernel_ms'] > 0.0
    for F in (1, 7, 8, 9):
        for per_pass in (8, 1, 0):
            v = frame_cvs(cvs, case.pos[:F], case.box[:F], case.masses, frames_per_pass=per_pass)
            assert v.shape == (F, 9) and np.array_equal(v, whole[:F]), (F, per_pass)
    for i, cv in enumerate(cvs):
        alone = frame_cvs([cv], case.pos, case.box, case.masses, frames_per_pass=8)
        assert alone.shape == (9, 1) and np.array_equal(alone[:, 0], whole[:, i]), i
    # against the host evaluator: two orders of the same f64 sums
    host = an.frame_cvs_numpy(cvs, case.pos, case.box, case.masses)
    assert np.all(np.abs(host - whole) <= 2.0 * fc.GENERAL_BOUND)


def _raw(tables, pos, box, out, device=0):
    lib = _engine.load_library()
    t = _engine.RemdFrameCvTables(len(tables['kind']), _engine._ip(tables['kind']), _engine._ip(tables['periodic']), _engine._ip(tables['cv_groups']),
                                  _engine._ip(tables['group_off']), _engine._ip(tables['atoms']), _engine._dp(tables['weights']),
                                  _engine._dp(tables['reference']))
    rc = lib.remd_frame_cvs(device, pos.shape[0], pos.shape[1], _engine._fp(pos), _engine._fp(box), C.byref(t), 0, _engine._dp(out), None)
    return rc, lib.remd_last_error(None).decode()


def test_all_padding_lanes_and_untouched_neighbours():
    """Groups of one atom among 64: 63 lanes of every wavefront are padding.  The output is written where it belongs and nowhere else:
    the slots in front of and behind out[F][n_cv] keep their sentinel."""
    rng = np.random.default_rng(12)
    F, n_atoms, guard = 5, 64, 16
    pos = rng.uniform(-1.0, 1.0, (F, n_atoms, 3)).astype(np.float32)
    cvs = [an.DistanceCV(63, 0, periodic=False), an.AngleCV(1, 62, 31, periodic=False), an.DihedralCV(5, 40, 17, 63, periodic=False)]
    tables = an.frame_cv_tables(cvs, n_atoms)
    buf = np.full(F * 3 + 2 * guard, -7.0)
    out = buf[guard:guard + F * 3]
    rc, err = _raw(tables, pos, None, out)
    assert rc == 0, err
    assert np.all(buf[:guard] == -7.0) and np.all(buf[guard + F * 3:] == -7.0)
    host = an.frame_cvs_numpy(cvs, pos)
    assert np.all(np.abs(out.reshape(F, 3) - host) <= fc.GENERAL_BOUND)
    variables = [('distance', [[63], [0]], [None, None], False), ('angle', [[1], [62], [31]], [None] * 3, False),
                 ('dihedral', [[5], [40], [17], [63]], [None] * 4, False)]
    import frame_cvs_oracle
    err = frame_cvs_oracle.errors(out.reshape(F, 3), frame_cvs_oracle.evaluate(variables, pos))
    assert np.all(err <= fc.GENERAL_BOUND), err.max()


@pytest.mark.parametrize('change, message', [
    (dict(F=0), 'F must be at least 1'),
    (dict(kind=[7]), 'unknown kind 7 of variable 0'),
    (dict(cv_groups=[0, 3]), 'variable 0 of kind 0 must have 2 groups'),
    (dict(group_off=[0, 2, 2]), 'an empty group in variable 0'),
    (dict(atoms=[0, 4, 2]), 'atom index 4 of variable 0 is outside 0 ... n_atoms-1 = 3'),
    (dict(atoms=[0, -1, 2]), 'atom index -1 of variable 0 is outside'),
    (dict(weights=[0.5, 0.25, 1.0]), 'do not sum to 1'),
    (dict(weights=[1.5, -0.5, 1.0]), 'negative or non-finite weight'),
    (dict(box=[[3.0, 3.0, 3.0], [3.0, 0.0, 3.0]]), 'frame 1 has a non-finite or non-positive box edge'),
    (dict(kind=[3], cv_groups=[0, 1], group_off=[0, 2], atoms=[0, 1], weights=[0.5, 0.5]), 'needs at least 3 particles'),
])
def test_refusals_come_from_the_host_before_any_launch(change, message):
    """a device index no machine has: a refusal must come from the host-side checks, before the device is touched"""
    t = dict(kind=[0], periodic=[1], cv_groups=[0, 2], group_off=[0, 2, 3], atoms=[0, 1, 2], weights=[0.5, 0.5, 1.0],
             reference=np.zeros((3, 3)))
    F = change.pop('F', 2)
    box = change.pop('box', None)
    t.update(change)
    tables = {k: np.ascontiguousarray(v, dtype=np.float64 if k in ('weights', 'reference') else np.int32) for k, v in t.items()}
    pos = np.zeros((2, 4, 3), dtype=np.float32)
    pos[:, :, 0] = np.arange(4)
    out = np.full(4, -7.0)
    lib = _engine.load_library()
    ct = _engine.RemdFrameCvTables(1, *[_engine._ip(tables[k]) for k in ('kind', 'periodic', 'cv_groups', 'group_off', 'atoms')],
                                   _engine._dp(tables['weights']), _engine._dp(tables['reference']))
    b = None if box is None else np.ascontiguousarray(box, dtype=np.float32)
    rc = lib.remd_frame_cvs(10 ** 6, F, 4, _engine._fp(pos), _engine._fp(b), C.byref(ct), 0, _engine._dp(out), None)
    err = lib.remd_last_error(None).decode()
    assert rc != 0 and err.startswith('remd_frame_cvs: ') and message in err, err
    assert np.all(out == -7.0)


def test_a_valid_call_reaches_the_device_check():
    tables = an.frame_cv_tables([an.DistanceCV([0, 1], 2)], 4, np.ones(4))
    pos = np.zeros((2, 4, 3), dtype=np.float32)
    rc, err = _raw(tables, pos, np.full((2, 3), 3.0, dtype=np.float32), np.zeros(2), device=10 ** 6)
    assert rc != 0 and 'bad device index' in err, err


def test_the_analyzer_on_the_device_against_numpy(tmp_path):
    rep = fc.write_store(tmp_path / 'store')[0]
    cvs = fc.store_variables(an)
    kw = dict(n_equilibration_iterations=0, statistical_inefficiency=1.0, unbias_restraint=False)
    host = an.MultiStateSamplerAnalyzer(rep, **kw).get_collective_variables(cvs)
    a = an.MultiStateSamplerAnalyzer(rep, analysis_kwargs={'cv_solver': 'device'}, **kw)
    dev = a.get_collective_variables(cvs)
    assert dev.shape == host.shape == (25, 3, 4) and np.all(np.isfinite(dev))
    assert np.all(np.abs(dev - host) <= 2.0 * fc.GENERAL_BOUND), np.abs(dev - host).max()   # each within 1e-10 of the exact value
    assert np.array_equal(a.get_collective_variables(cvs, solver='numpy'), host)
    edges = np.linspace(-np.pi, np.pi, 7)
    f_d, _, n_d = a.get_pmf(dev[:, :, :2], (edges, np.linspace(0.0, 2.0, 4)), state=0)
    f_h, _, n_h = a.get_pmf(host[:, :, :2], (edges, np.linspace(0.0, 2.0, 4)), state=0)
    assert np.array_equal(n_d, n_h) and np.allclose(f_d, f_h, rtol=0.0, atol=1e-9, equal_nan=True)
