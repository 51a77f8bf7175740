"""CPU: collective variables of stored frames -- the descriptors, frame_cvs_numpy and MultiStateSamplerAnalyzer.get_collective_variables
(multistate/analysis.py) -- against the independent reference of tests/frame_cvs_oracle.py on the case table of tests/frame_cvs_cases.py
(whose docstring derives the bounds), the refusals by message, and the analyzer's round trip through a hand-written store into get_pmf.
No GPU: the device solver is only asked to refuse where the library lacks the entry point.

Figures of the host evaluator against the oracle (max |error| over frames and variables; nm, rad), taken on the committed inputs:
sizes 1.2e-15, sizes-unimaged 7.0e-16, far 1.6e-14, exact 9.7e-17, rmsd-shapes 1.1e-16 (bound 1e-10 each); angle-end 8.2e-10,
dihedral-cut 2.1e-16, rmsd-floor 0 (bounds: 4 x the device's recorded error, profiles/frame_cv_errors.txt)."""
import os

import numpy as np
import pytest

import frame_cvs_cases as fc
import oracle
from openmmtools_amd import _engine
from openmmtools_amd.multistate import analysis as an

CPU_LIB = os.path.join(os.path.dirname(os.path.abspath(oracle.__file__)), '_build', 'libremd_cpu.so')
CASES = [c.name for c in fc.all_cases()]


def _numpy(case, **kw):
    return an.frame_cvs_numpy(case.descriptors(an), case.pos, case.box, case.masses, **kw)


# ---- 1. against the oracle -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', CASES)
def test_numpy_against_the_oracle(name):
    case = fc.case(name)
    v = _numpy(case)
    assert v.shape == (len(case.pos), len(case.variables)) and v.dtype == np.float64
    err, bound = fc.errors(name, v), fc.bound(name)
    print(name, 'max error per variable', err.max(axis=0), 'bound', bound)
    assert np.all(np.isfinite(v)) and np.all(err <= bound), (name, err.max(), bound)


def test_the_degenerate_values_themselves():
    v = _numpy(fc.case('exact'))[0]
    assert v[0] == 0.0 and v[1] == 0.0 and v[2] == 0.0 and v[3] > 0.1           # cis dihedral, coincident atoms, identical groups
    a = _numpy(fc.case('angle-end'))[:, 0]
    assert a[0] == 0.0 and a[1] == np.pi and np.all(np.isfinite(a))
    assert np.all((a[2:10] > 0.0) & (a[2:10] < 1e-6)) and np.all((a[10:] < np.pi) & (a[10:] > np.pi - 1e-6))
    d = _numpy(fc.case('dihedral-cut'))[:, 0]
    assert d[0] == np.pi                                                        # the closed end of (-pi, pi]
    assert abs((d[1] + np.pi) - 1e-9) < 1e-12
    assert np.all(np.abs(d) <= np.pi) and np.all(np.pi - np.abs(d[2:]) < 1e-6) and np.any(d[2:] < 0.0) and np.any(d[2:] > 0.0)
    assert np.all(_numpy(fc.case('rmsd-floor')) == 0.0)                          # through the floor
    shapes = _numpy(fc.case('rmsd-shapes'))
    assert np.all(shapes > 0.005) and np.all(shapes[:, [0, 2, 3]] < 0.1)         # the noise; the mirrored set keeps a real deviation
    assert np.all(shapes[:, 1] > 0.1)


def test_periodic_false_gives_the_unimaged_value():
    imaged, plain = fc.case('sizes'), fc.case('sizes-unimaged')
    assert np.array_equal(imaged.pos[:2], plain.pos)
    a, b = _numpy(imaged)[:2], an.frame_cvs_numpy(plain.descriptors(an), plain.pos, imaged.box[:2], plain.masses)
    assert np.array_equal(b, _numpy(plain))                                     # a box that no variable asks for changes nothing
    centroid = [i for i, var in enumerate(imaged.variables) if var[0] != 'rmsd']
    assert np.count_nonzero(np.abs(a[:, centroid] - b[:, centroid]) > 1e-3) >= 8
    assert np.array_equal(a[:, 7:], b[:, 7:])                                   # an RMSD takes no images


# ---- 2. chunks and company -----------------------------------------------------------------------------------------------------------
def test_values_do_not_depend_on_the_chunking_or_on_the_other_variables():
    case = fc.case('sizes')
    cvs = case.descriptors(an)
    whole = _numpy(case)
    for F in (1, 7, 8, 9):                                                      # frames_per_pass - 1, frames_per_pass, frames_per_pass + 1
        for per_pass in (8, 1, 4096):
            v = an.frame_cvs_numpy(cvs, case.pos[:F], case.box[:F], case.masses, frames_per_pass=per_pass)
            assert v.shape == (F, 9) and np.array_equal(v, whole[:F]), (F, per_pass)
    for i, cv in enumerate(cvs):
        alone = an.frame_cvs_numpy([cv], case.pos, case.box, case.masses, frames_per_pass=8)
        assert alone.shape == (9, 1) and np.array_equal(alone[:, 0], whole[:, i]), i
    back = an.frame_cvs_numpy(cvs[::-1], case.pos, case.box, case.masses)
    assert np.array_equal(back[:, ::-1], whole)


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------
REF4 = np.zeros((4, 3))


@pytest.mark.parametrize('make, message', [
    (lambda: an.DistanceCV([], [1]), 'DistanceCV: group 1 is empty'),
    (lambda: an.AngleCV(0, 1, []), 'AngleCV: group 3 is empty'),
    (lambda: an.DihedralCV(0, [1, 2, 1], 3, 4), 'DihedralCV: group 2 names atom 1 twice'),
    (lambda: an.DistanceCV([0, 1], [2], weights1=[1.0]), 'DistanceCV: group 1 has 2 atoms but 1 weights'),
    (lambda: an.AngleCV([0, 1], 2, 3, weights=[[1.0, -1.0], None, None]), 'AngleCV: the weights of group 1 must be finite and not negative'),
    (lambda: an.DistanceCV([0, 1], [2, 3], weights2=[0.0, 0.0]), 'DistanceCV: the weights of group 2 sum to zero'),
    (lambda: an.AngleCV(0, 1, 2, weights=[None, None]), 'AngleCV: weights must hold one list'),
    (lambda: an.DihedralCV(0, 1, -2, 3), 'DihedralCV: group 3 holds the negative index -2'),
    (lambda: an.DistanceCV(0, [1.5]), 'DistanceCV: group 2 holds 1.5, which is not an atom index'),
    (lambda: an.RMSDCV(REF4, [0, 1]), 'RMSDCV: particles holds 2 atoms; an RMSD needs at least 3'),
    (lambda: an.RMSDCV(REF4, []), 'RMSDCV: particles is empty'),
    (lambda: an.RMSDCV(REF4, [0, 1, 1]), 'RMSDCV: particles names atom 1 twice'),
    (lambda: an.RMSDCV(REF4, [0, 1, -3]), 'RMSDCV: particles holds the negative index -3'),
    (lambda: an.RMSDCV([[0.0, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0] * 3], [0, 1, 2]), r'RMSDCV: reference_positions are not finite \(particle 1\)'),
    (lambda: an.RMSDCV(np.zeros((4, 2)), [0, 1, 2]), r'RMSDCV: reference_positions must be \[N\]\[3\]'),
])
def test_descriptor_refusals(make, message):
    with pytest.raises(ValueError, match=message):
        make()


def test_evaluator_refusals():
    pos, box, masses = np.zeros((2, 4, 3), dtype=np.float32), np.full((2, 3), 3.0, dtype=np.float32), np.ones(4)
    d = an.DistanceCV([0, 1], [2])
    for call, message in [
        (lambda: an.frame_cvs_numpy([d], pos, None, masses), r'variable 0 \(DistanceCV\) is periodic but the frames have no box'),
        (lambda: an.frame_cvs_numpy([an.AngleCV(0, 1, 2, periodic=False), d], pos, None, masses), r'variable 1 \(DistanceCV\) is periodic'),
        (lambda: an.frame_cvs_numpy([d], pos, box), r'variable 0 \(DistanceCV\): group 1 has no weights and no masses were given'),
        (lambda: an.frame_cvs_numpy([d], pos, box, np.zeros(4)), r'variable 0 \(DistanceCV\): the masses of group 1 sum to zero'),
        (lambda: an.frame_cvs_numpy([an.DistanceCV(0, 4)], pos, box, masses), r'variable 0 \(DistanceCV\): atom 4 is outside the 4 atoms'),
        (lambda: an.frame_cvs_numpy([an.RMSDCV(np.zeros((5, 3)), [0, 1, 2])], pos, box, masses),
         r'variable 0 \(RMSDCV\): reference_positions holds 5 particles but the frames have 4'),
        (lambda: an.frame_cvs_numpy([d], pos, np.zeros((2, 3, 3)), masses), r'box must be \[F\]\[3\] .*triclinic boxes are not supported'),
        (lambda: an.frame_cvs_numpy([d], pos, np.array([[3.0, 3.0, 3.0], [3.0, 0.0, 3.0]]), masses), 'non-finite or non-positive box edge'),
        (lambda: an.frame_cvs_numpy([d], pos[0], box, masses), r'pos must be \[F\]\[n_atoms\]\[3\]'),
        (lambda: an.frame_cvs_numpy([], pos, box, masses), 'no collective variable'),
        (lambda: an.frame_cvs_numpy(['phi'], pos, box, masses), "variable 0 is 'phi', not a DistanceCV"),
        (lambda: an.frame_cvs_numpy([d], pos, box, masses, frames_per_pass=0), 'frames_per_pass must be at least 1'),
        (lambda: an.frame_cvs_numpy([d], pos, box, np.ones(3)), 'masses must have one entry per atom of pos: 4, not 3'),
    ]:
        with pytest.raises(ValueError, match=message):
            call()
    # a single atom needs neither weights nor masses: its weight is 1
    assert an.frame_cvs_numpy([an.DistanceCV(0, 1, periodic=False)], pos).shape == (2, 1)


# ---- 4. the analyzer -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def store(tmp_path_factory):
    return fc.write_store(tmp_path_factory.mktemp('frame_cvs') / 'store')


KW = dict(n_equilibration_iterations=0, statistical_inefficiency=1.0, unbias_restraint=False)


def test_analyzer_round_trip_into_get_pmf(store):
    rep, system, positions, box = store
    assert tuple(rep.analysis_particle_indices) == tuple(sorted(fc.STORE_ANALYSIS_PARTICLES)) != fc.STORE_ANALYSIS_PARTICLES
    a = an.MultiStateSamplerAnalyzer(rep, **KW)
    cvs = fc.store_variables(an)
    v = a.get_collective_variables(cvs)
    n_it, R = a.n_iterations + 1, a.n_replicas
    assert v.shape == (n_it, R, 4) == (25, 3, 4) and v.dtype == np.float64
    # by hand: the stored frames, the descriptors moved to the columns of the store
    x, b = rep.read_analysis_positions(range(n_it))
    columns = list(rep.analysis_particle_indices)
    where = {atom: k for k, atom in enumerate(columns)}
    assert np.array_equal(x, positions[:, :, columns, :]) and np.array_equal(b, box)
    col = lambda group: [where[i] for i in group]
    ref = cvs[3].reference_positions[columns]
    mapped = [an.DihedralCV(*col([0, 4, 5, 9])), an.DistanceCV(col([7, 2]), col([9, 4, 0])),
              an.AngleCV(col([2, 5]), where[7], col([0, 9]), weights=[[1.0, 2.0], None, None]), an.RMSDCV(ref, col([5, 2, 7, 4]))]
    masses = np.asarray(system.masses, dtype=np.float64)[columns]
    want = an.frame_cvs_numpy(mapped, x.reshape(n_it * R, len(columns), 3), b.reshape(n_it * R, 3), masses).reshape(n_it, R, 4)
    assert np.array_equal(v, want)
    # ... which is the variable over all ten particles of the frames that were written
    full = an.frame_cvs_numpy(cvs, positions.reshape(n_it * R, 10, 3), box.reshape(n_it * R, 3), system.masses).reshape(n_it, R, 4)
    assert np.array_equal(v[..., :3], full[..., :3]) and np.allclose(v[..., 3], full[..., 3], rtol=0.0, atol=1e-13)
    # a bare descriptor: no last axis; the cache serves copies until clear()
    phi = a.get_collective_variables(cvs[0])
    assert phi.shape == (n_it, R) and np.array_equal(phi, v[:, :, 0])
    v[:] = 0.0
    assert np.array_equal(a.get_collective_variables(cvs), want) and len(a._collective_variables) == 2
    a.clear()
    assert a._collective_variables == {}
    # into get_pmf, one and two dimensions
    edges = np.linspace(-np.pi, np.pi, 7)
    f_i, df_i, n_i = a.get_pmf(phi, edges, state=0)
    assert f_i.shape == (6,) and n_i.sum() == n_it * R and np.isfinite(f_i).sum() >= 4
    f2, df2, n2 = a.get_pmf(want[:, :, :2], (edges, np.linspace(0.0, 2.0, 4)), state=1)
    assert f2.shape == (18,) and n2.sum() == np.count_nonzero((want[:, :, 1] >= 0.0) & (want[:, :, 1] <= 2.0))
    # max_n_iterations cuts the values as it cuts the energies
    short = an.MultiStateSamplerAnalyzer(rep, max_n_iterations=10, **KW)
    assert np.array_equal(short.get_collective_variables(cvs), want[:11])


def test_cv_solver_option(store):
    rep = store[0]
    with pytest.raises(ValueError, match=r"analysis_kwargs\['cv_solver'\] must be 'numpy' or 'device', not 'gpu'"):
        an.MultiStateSamplerAnalyzer(rep, analysis_kwargs={'cv_solver': 'gpu'})
    a = an.MultiStateSamplerAnalyzer(rep, **KW)
    assert a.cv_solver == 'numpy'
    cvs = fc.store_variables(an)
    a.get_collective_variables(cvs)
    assert len(a._collective_variables) == 1
    a.cv_solver = 'numpy'
    assert len(a._collective_variables) == 1
    a.cv_solver = 'device'
    assert a.cv_solver == 'device' and a._collective_variables == {}              # a change drops the cache
    with pytest.raises(ValueError, match="cv_solver"):
        a.cv_solver = 'cuda'
    with pytest.raises(ValueError, match="solver must be 'numpy' or 'device', not 'cpu'"):
        a.get_collective_variables(cvs, solver='cpu')
    assert a.get_collective_variables(cvs, solver='numpy').shape == (25, 3, 4)   # the argument overrides the key for one call
    assert a.cv_solver == 'device'


def test_analyzer_refusals(store, tmp_path):
    rep, system = store[0], store[1]
    a = an.MultiStateSamplerAnalyzer(rep, **KW)
    with pytest.raises(ValueError, match=r'variable 1 \(DistanceCV\): atom 3 is not one of the analysis particles of the store: create the '
                                         'reporter with analysis_particle_indices'):
        a.get_collective_variables([an.DistanceCV(0, 2), an.DistanceCV([0, 3], 2)])
    with pytest.raises(ValueError, match=r'variable 0 \(AngleCV\): atom 10 is outside the 10 particles of the System'):
        a.get_collective_variables(an.AngleCV(0, 10, 2))
    with pytest.raises(ValueError, match='RMSDCV: reference_positions holds 9 particles but the System has 10'):
        a.get_collective_variables(an.RMSDCV(np.zeros((9, 3)), [0, 2, 4]))
    with pytest.raises(ValueError, match='no collective variable'):
        a.get_collective_variables([])
    with pytest.raises(ValueError, match="variable 0 is 'phi'"):
        a.get_collective_variables(['phi'])
    # a store that is not periodic: a periodic variable takes no images there, and says nothing
    rep2, system2, positions2, _ = fc.write_store(tmp_path / 'vacuum', periodic=False, n_it=4)
    b = an.MultiStateSamplerAnalyzer(rep2, **KW)
    got = b.get_collective_variables(fc.store_variables(an, periodic=True))
    want = an.frame_cvs_numpy(fc.store_variables(an, periodic=False), positions2.reshape(12, 10, 3), None, system2.masses).reshape(4, 3, 4)
    assert np.array_equal(got[..., :3], want[..., :3])
    # an iteration without stored positions: the reporter's own sentence
    rep3 = fc.write_store(tmp_path / 'sparse', n_it=4, position_interval=2)[0]
    with pytest.raises(ValueError, match='iteration 1 has no stored positions of the analysis particles'):
        an.MultiStateSamplerAnalyzer(rep3, **KW).get_collective_variables(an.DistanceCV(0, 2))
    # a store without analysis particles at all
    rep4 = fc.write_store(tmp_path / 'none', n_it=2, analysis_particles=())[0]
    with pytest.raises(ValueError, match='atom 0 is not one of the analysis particles'):
        an.MultiStateSamplerAnalyzer(rep4, **KW).get_collective_variables(an.DistanceCV(0, 2))


def test_a_triclinic_store_is_refused(tmp_path, monkeypatch):
    rep = fc.write_store(tmp_path / 'skew', n_it=2)[0]
    f = rep._files['analysis_box_vectors']
    boxes = np.memmap(f.path, dtype=f.dtype, mode='r+', shape=(f.count(),) + f.shape)
    boxes[1, 0, 1, 0] = 0.25                                                    # a sheared cell in one frame
    boxes.flush()
    with pytest.raises(ValueError, match='triclinic boxes are not supported: the stored box vectors of the analysis particles are not rectangular'):
        an.MultiStateSamplerAnalyzer(rep, **KW).get_collective_variables(an.DistanceCV(0, 2))


# ---- 5. no device --------------------------------------------------------------------------------------------------------------------
def test_the_cpu_library_refuses_the_device_solver_by_name(store):
    assert os.path.exists(CPU_LIB), 'build() makes oracle/_build/libremd_cpu.so; without it this check would not run'
    case = fc.case('far')
    with pytest.raises(NotImplementedError, match='remd_frame_cvs.*include/remd_hip_frame_cvs.h'):
        _engine.frame_cvs(case.descriptors(an), case.pos, None, case.masses, lib_path=CPU_LIB)
    a = an.MultiStateSamplerAnalyzer(store[0], analysis_kwargs={'cv_solver': 'device', 'lib_path': CPU_LIB}, **KW)
    with pytest.raises(NotImplementedError, match='include/remd_hip_frame_cvs.h'):
        a.get_collective_variables(fc.store_variables(an))
    with pytest.raises(NotImplementedError, match='include/remd_hip_frame_cvs.h'):
        an.MultiStateSamplerAnalyzer(store[0], analysis_kwargs={'lib_path': CPU_LIB}, **KW).get_collective_variables(fc.store_variables(an), solver='device')


def test_the_tables_of_the_abi():
    """frame_cv_tables: what the device entry point is handed"""
    case = fc.case('sizes')
    t = an.frame_cv_tables(case.descriptors(an), case.pos.shape[1], case.masses)
    assert t['kind'].tolist() == [0, 0, 0, 1, 1, 2, 2, 3, 3] and t['periodic'].tolist() == [1] * 7 + [0, 0]
    assert t['cv_groups'].tolist() == [0, 2, 4, 6, 9, 12, 16, 20, 21, 22]
    sizes = np.diff(t['group_off'])
    assert sizes.tolist() == [1, 257, 2, 63, 64, 65, 1, 64, 65, 2, 63, 257, 1, 2, 63, 64, 65, 257, 64, 63, 257, 3]
    assert t['atoms'].dtype == np.int32 and t['weights'].dtype == np.float64 and t['reference'].shape == (t['atoms'].size, 3)
    for g in range(20):
        w = t['weights'][t['group_off'][g]:t['group_off'][g + 1]]
        assert abs(w.sum() - 1.0) < 1e-14 and np.all(w > 0.0)
    b = t['group_off'][20]
    assert np.allclose(t['reference'][b:b + 257].mean(axis=0), 0.0, atol=1e-15) and np.all(t['reference'][:b] == 0.0)
    assert np.array_equal(t['weights'][258:260], [0.25, 0.75])                  # the explicit weights [1, 3] of the group of two, normalised
