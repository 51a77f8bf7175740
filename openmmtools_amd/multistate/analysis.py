"""Free-energy analysis of a stored multistate simulation: what ``MultiStateSampler._offline_analysis`` needs.

The reference runs ``MultiStateSamplerAnalyzer`` (openmmtools/multistate/multistateanalyzer.py:1164) on the
reporter's energies and hands them to **pymbar** (a dependency that is not vendored in the reference tree and not
installed here; ``devtools/conda-envs/test_env.yaml:14`` lists it unpinned, i.e. pymbar 4).  This module restates the
published algorithms the analyzer relies on, in plain numpy:

* ``statistical_inefficiency`` / ``subsample_correlated_data`` — pymbar.timeseries (Chodera et al., JCTC 3, 26 (2007);
  integrated autocorrelation time summed until the normalised fluctuation autocorrelation function first crosses zero,
  ``mintime = 3``, optional ``fast`` increments); ``solver='device'`` runs the same lags and sums on the GPU for any number of time
  origins at once (include/remd_hip_timeseries.h, csrc/timeseries.hip; ``analysis_kwargs={'timeseries_solver': 'device'}``);
* ``get_equilibration_data_per_sample`` — openmmtools/multistate/utils.py:107-190 (automated equilibration detection of
  Chodera, JCTC 12, 1799 (2016) on at most ``max_subset`` time origins);
* ``MBAR`` — Shirts & Chodera, J. Chem. Phys. 129, 124105 (2008): self-consistent / Newton solution of eq. 11 for the
  dimensionless free energies and the asymptotic covariance of eq. 8 / D6 (SVD form) for their uncertainties;
* ``MultiStateSamplerAnalyzer`` — the analyzer's pipeline for global neighbourhoods: effective-energy timeseries
  (multistateanalyzer.py:1414-1478), equilibration data (:2026-2088), decorrelated u_ln / N_l assembly with the
  unsampled states at the end points (:1479-1545), free energy differences (:1919-2003); the unbiasing of a radially symmetric
  receptor-ligand restraint (:1355-1408, :1556-1913): the restraint is re-evaluated at every stored, decorrelated frame, frames
  outside a cutoff are dropped and two end states without the restraint join the MBAR problem.  The frames are evaluated in one
  call, by ``restraint_frames_numpy`` or on the device (``analysis_kwargs={'restraint_solver': 'device'}``, csrc/restraint_frames.hip),
  with the centroid convention the run was sampled with -- not the reference's, see DESIGN.md.  The walks over the stored energies
  (effective energies, u_ln / N_l assembly, transition counts and the state walk's statistical inefficiency) run as numpy loops or on
  the device (``analysis_kwargs={'assembly_solver': 'device'}``, include/remd_hip_energy_store.h, csrc/energy_store.hip).
* ``DistanceCV`` / ``AngleCV`` / ``DihedralCV`` / ``RMSDCV``, ``frame_cvs_numpy`` and ``get_collective_variables`` -- not in the
  reference: the coordinates ``get_pmf`` takes, computed from the stored frames of the analysis particles with the conventions of the
  force kernels, in numpy or on the device (``analysis_kwargs={'cv_solver': 'device'}``, include/remd_hip_frame_cvs.h, csrc/frame_cvs.hip).

Parity: unpinned against pymbar itself (absent); pinned against the analytical free energies of harmonic oscillators,
the reference's own acceptance test (tests/test_sampling.py:100-300), in tests/test_analysis_cpu.py.
"""
import collections

import numpy as np


# ---- timeseries ------------------------------------------------------------------------------------------------
_NO_VARIANCE = 'sample covariance is zero: cannot compute the statistical inefficiency'


def _check_timeseries_solver(solver):
    if solver not in ('numpy', 'device'):
        raise ValueError("solver must be 'numpy' or 'device', not %r" % (solver,))


def _device_inefficiencies(A_n, origins, fast, mintime, device, lib_path):
    """g of the suffixes ``A_n[t:]`` for t in ``origins``, in ONE call of the device (include/remd_hip_timeseries.h); the ValueError
    of the host loop where a suffix has no variance."""
    from .._engine import DeviceTimeseries
    ts = DeviceTimeseries(A_n, device=device, lib_path=lib_path)
    try:
        g, status, _ = ts.inefficiency(origins, fast=fast, mintime=mintime)
    finally:
        ts.close()
    if status.any():
        raise ValueError(_NO_VARIANCE)
    return g


def statistical_inefficiency(A_n, fast=False, mintime=3, solver='numpy', device=0, lib_path=None):
    """g = 1 + 2 tau of the stationary timeseries ``A_n`` (>= 1).  pymbar.timeseries.statistical_inefficiency.

    ``solver='numpy'`` (the default) runs the loop over the lags below; ``solver='device'`` runs the same lags, sums and stopping rule
    on the GPU (csrc/timeseries.hip).  ``device`` and ``lib_path`` choose the GPU and the engine library of the device solver."""
    _check_timeseries_solver(solver)
    if solver == 'device':
        return float(_device_inefficiencies(A_n, [0], fast, mintime, device, lib_path)[0])
    A = np.asarray(A_n, dtype=np.float64)
    N = A.size
    dA = A - A.mean()
    sigma2 = np.mean(dA * dA)
    if sigma2 == 0.0:
        raise ValueError(_NO_VARIANCE)
    g = 1.0
    t, increment = 1, 1
    while t < N - 1:
        C = np.dot(dA[:N - t], dA[t:]) / (float(N - t) * sigma2)
        if C <= 0.0 and t > mintime:
            break
        g += 2.0 * C * (1.0 - float(t) / float(N)) * float(increment)
        t += increment
        if fast:
            increment += 1
    return max(g, 1.0)


def statistical_inefficiency_multiple(A_kn, fast=False, mintime=3, solver='numpy', device=0, lib_path=None):
    """One statistical inefficiency from several timeseries of the same observable (pymbar.timeseries): the fluctuation
    autocorrelation function is averaged over the series before it is integrated.

    ``solver='device'`` runs the same lags, pooled sums and stopping rule on the GPU in one call (csrc/energy_store.hip); the series
    must then have one common length."""
    _check_timeseries_solver(solver)
    series = [np.asarray(a, dtype=np.float64) for a in A_kn]
    if solver == 'device':
        if len({a.size for a in series}) != 1 or any(a.ndim != 1 for a in series):
            raise ValueError("solver='device' needs series of one common length (ragged series run with solver='numpy')")
        from .._engine import series_inefficiency_multiple
        g, status = series_inefficiency_multiple(np.stack(series), fast=fast, mintime=mintime, device=device, lib_path=lib_path)[:2]
        if status:
            raise ValueError(_NO_VARIANCE)
        return g
    N_k = np.array([a.size for a in series])
    Nmax, N = int(N_k.max()), int(N_k.sum())
    mu = sum(a.sum() for a in series) / float(N)
    dA = [a - mu for a in series]
    sigma2 = sum((d * d).sum() for d in dA) / float(N)
    if sigma2 == 0.0:
        raise ValueError('sample covariance is zero: cannot compute the statistical inefficiency')
    g = 1.0
    t, increment = 1, 1
    while t < Nmax - 1:
        num, den = 0.0, 0
        for d in dA:
            if t >= d.size:
                continue
            x = d[:d.size - t] * d[t:]
            num += x.sum(); den += x.size
        C = (num / float(den)) / sigma2
        if C <= 0.0 and t > mintime:
            break
        g += 2.0 * C * (1.0 - float(t) / N_k.mean()) * float(increment)
        t += increment
        if fast:
            increment += 1
    return max(g, 1.0)


def subsample_correlated_data(A_t, g=None, fast=False, conservative=False, solver='numpy', device=0, lib_path=None):
    """Indices of an (approximately) uncorrelated subset: every ``g``-th sample, rounded (pymbar.timeseries).  ``solver``, ``device``
    and ``lib_path`` are statistical_inefficiency's, used when ``g`` is None."""
    _check_timeseries_solver(solver)
    T = len(A_t)
    if g is None:
        g = statistical_inefficiency(A_t, fast=fast, solver=solver, device=device, lib_path=lib_path)
    if conservative:
        stride = int(np.ceil(g))
        return list(range(0, T, stride))
    indices, n = [], 0
    while int(round(n * g)) < T:
        t = int(round(n * g))
        if n == 0 or t != indices[-1]:
            indices.append(t)
        n += 1
    return indices


def get_equilibration_data_per_sample(timeseries_to_analyze, fast=True, max_subset=100, solver='numpy', device=0, lib_path=None):
    """(i_t, g_i, n_effective_i) on at most ``max_subset`` evenly spaced time origins (multistate/utils.py:107-190).
    ``solver='device'``: the statistical inefficiencies of all origins in one call of the GPU (csrc/timeseries.hip)."""
    _check_timeseries_solver(solver)
    series = np.array(timeseries_to_analyze)
    time_size = series.size
    set_size = time_size - 1
    if max_subset is None or set_size < max_subset:
        max_subset = set_size
    if max_subset == 0:
        max_subset = 1
    if series.std() == 0.0 or max_subset == 1:
        return (np.arange(max_subset, dtype=int), np.array([1] * max_subset),
                np.arange(time_size, time_size - max_subset, -1))
    g_i = np.ones([max_subset], np.float32)
    n_effective_i = np.ones([max_subset], np.float32)
    counter = np.arange(max_subset)
    i_t = np.floor(counter * time_size / max_subset).astype(int)
    g_all = _device_inefficiencies(series, i_t, fast, 3, device, lib_path) if solver == 'device' else None
    for i, t in enumerate(i_t):
        if g_all is not None:
            g_i[i] = g_all[i]
        else:
            g_i[i] = statistical_inefficiency(series[t:], fast=fast)   # (:176-181: an error here is raised, not papered over)
        n_effective_i[i] = (time_size - t + 1) / g_i[i]
    return i_t[1:], g_i[1:], n_effective_i[1:]                          # :190: the origin t = 0 is not a candidate


def get_decorrelation_time(timeseries_to_analyze, solver='numpy', device=0, lib_path=None):
    """multistate/utils.py:98-104."""
    return statistical_inefficiency(timeseries_to_analyze, solver=solver, device=device, lib_path=lib_path)


def get_equilibration_data(timeseries_to_analyze, fast=True, max_subset=1000, solver='numpy', device=0, lib_path=None):
    """multistate/utils.py:195-235 (kept by the reference for old callers): (n_equilibration, g_t, n_effective_max)."""
    i_t, g_i, n_effective_i = get_equilibration_data_per_sample(timeseries_to_analyze, fast=fast, max_subset=max_subset, solver=solver,
                                                                device=device, lib_path=lib_path)
    i_max = n_effective_i.argmax()
    return i_t[i_max], g_i[i_max], n_effective_i.max()


def remove_unequilibrated_data(data, number_equilibrated, axis):
    """multistate/utils.py:238-266: drop the first ``number_equilibrated`` entries along ``axis``."""
    cast = np.asarray(data)
    slc = [slice(None)] * cast.ndim
    slc[axis] = slice(number_equilibrated, None)
    return cast[tuple(slc)]


def subsample_data_along_axis(data, subsample_rate, axis):
    """multistate/utils.py:269-300: every ``subsample_rate``-th entry (rounded as subsample_correlated_data does) along ``axis``."""
    cast = np.asarray(data)
    indices = subsample_correlated_data(np.zeros(cast.shape[axis]), g=subsample_rate)
    return np.take(cast, indices, axis=axis)


def generate_phase_name(current_name, name_list):
    """multistate/utils.py:60-95: a name not yet in ``name_list`` ('phase0', 'phase1', ... or the given name + counter)."""
    counter = 0
    if current_name is None:
        name = 'phase%d' % counter
        while name in name_list:
            counter += 1
            name = 'phase%d' % counter
        return name
    if current_name in name_list:
        name = current_name + str(counter)
        while name in name_list:
            counter += 1
            name = current_name + str(counter)
        return name
    return current_name


# ---- restraints at stored frames ---------------------------------------------------------------------------------
class InsufficientData(Exception):
    """multistateanalyzer.py:62-64: the stored data cannot answer the question (no frame of the bound state for an 'auto' cutoff)."""


def compute_centroid_distance(positions_group1, positions_group2, weights_group1, weights_group2):
    """multistateanalyzer.py:75-99: the distance between the weighted centres of two groups of positions (same units in, same out)."""
    assert len(positions_group1) == len(weights_group1)
    assert len(positions_group2) == len(weights_group2)
    com_group1 = np.average(positions_group1, axis=0, weights=weights_group1)
    com_group2 = np.average(positions_group2, axis=0, weights=weights_group2)
    return np.linalg.norm(com_group1 - com_group2)


def restraint_frames_numpy(desc, pos, box=None, masses=None, frames_per_pass=4096):
    """(energy [F] kJ/mol at lambda = 1, distance [F] nm) of one restraint at F stored frames, in f64: the host counterpart of
    remd_restraint_frames (include/remd_hip_restraints.h) with the engine's centroid convention, c = x_first + sum_i w_i img(x_i -
    x_first), img the minimum image under the frame's own box when the restraint is periodic; d = c2 - c1 imaged the same way.
    ``desc``: a dict of forces.restraint_terms whose atom indices address the atoms of ``pos`` [F][n_atoms][3]; weights None:
    ``masses``.  ``box`` [F][3] or None."""
    pos = np.asarray(pos)
    if pos.ndim != 3 or pos.shape[2] != 3 or pos.shape[0] < 1:
        raise ValueError('pos must be [F][n_atoms][3] with F >= 1')
    F, n_atoms = pos.shape[0], pos.shape[1]
    kind, K, r0 = int(desc['kind']), float(desc['K']), float(desc.get('r0', 0.0))
    if kind not in (0, 1):
        raise ValueError('unknown restraint kind %r' % (kind,))
    periodic = bool(desc.get('periodic', 0))
    if periodic:
        if box is None:
            raise ValueError('a periodic restraint needs the box of every frame')
        box = np.asarray(box, dtype=np.float64)
        if box.shape != (F, 3):
            raise ValueError('box must be [F][3] (the edges of a rectangular box; triclinic boxes are not supported)')
        if not (np.all(np.isfinite(box)) and np.all(box > 0.0)):
            raise ValueError('a non-finite or non-positive box edge')
    groups = []
    for g in (1, 2):
        atoms = np.asarray(desc['atoms%d' % g], dtype=np.int64).reshape(-1)
        if atoms.size == 0:
            raise ValueError('group %d is empty' % g)
        if atoms.min() < 0 or atoms.max() >= n_atoms:
            raise ValueError('an atom index of group %d is outside 0 ... %d' % (g, n_atoms - 1))
        w = desc.get('weights%d' % g)
        w = np.asarray(masses, dtype=np.float64)[atoms] if w is None else np.asarray(w, dtype=np.float64).reshape(-1)
        if w.shape != atoms.shape or np.any(w < 0.0) or not w.sum() > 0.0:
            raise ValueError('the weights of group %d are negative, sum to zero or do not match its atoms' % g)
        groups.append((atoms, w / w.sum()))
    energy, distance = np.empty(F), np.empty(F)
    for f0 in range(0, F, frames_per_pass):                     # (bounds the f64 copies of the positions)
        sl = slice(f0, min(F, f0 + frames_per_pass))
        L = box[sl, None, :] if periodic else None
        c = []
        for atoms, w in groups:
            x = pos[sl][:, atoms, :].astype(np.float64)
            d = x - x[:, :1, :]
            if periodic:
                d -= L * np.rint(d / L)
            c.append(x[:, 0, :] + np.einsum('k,fkc->fc', w, d))
        d = c[1] - c[0]
        if periodic:
            d -= L[:, 0, :] * np.rint(d / L[:, 0, :])
        r = np.sqrt((d * d).sum(axis=1))
        distance[sl] = r
        if kind == 0:
            energy[sl] = 0.5 * K * r * r
        else:
            x = r - r0
            energy[sl] = np.where(x >= 0.0, 1.0, 0.0) * 0.5 * K * x * x
    return energy, distance


# ---- MBAR --------------------------------------------------------------------------------------------------------
def _logsumexp(a, axis=None, b=None):
    a = np.asarray(a, dtype=np.float64)
    amax = np.max(a, axis=axis, keepdims=True)
    amax = np.where(np.isfinite(amax), amax, 0.0)
    e = np.exp(a - amax)
    if b is not None:
        e = e * b
    s = np.sum(e, axis=axis, keepdims=True)
    out = np.log(s) + amax
    return np.squeeze(out, axis=axis) if axis is not None else float(out.reshape(()))


class ParameterError(Exception):
    """Raised when the estimator cannot be computed from the data it was given (pymbar.utils.ParameterError)."""

def bin_samples(values, edges):
    """(bin_n [N], nbins): the flat bin index of every sample for ``MBAR.compute_pmf``.  ``values`` is [N], or [N][D] with D <= 3
    coordinates per sample; ``edges`` one ascending array of bin edges per dimension (for [N] values, the array itself will do).
    Intervals are half-open, [e_j, e_j+1), and the last is closed at its right edge, as numpy.histogram has them.  The first
    dimension varies fastest in the flat index; nbins is the product of the intervals per dimension.  A value outside the range of
    any dimension, or a NaN, gives -1: the sample lies in no bin."""
    v = np.asarray(values, dtype=np.float64)
    if v.ndim == 1:
        if len(edges) > 0 and np.ndim(edges[0]) == 0:
            edges = [edges]
        v = v[:, None]
    if v.ndim != 2 or not 1 <= v.shape[1] <= 3:
        raise ValueError('values must be [N] or [N][D] with D <= 3, not an array of shape %r' % (np.shape(values),))
    if len(edges) != v.shape[1]:
        raise ValueError('edges must hold one array per dimension: %d, not %d' % (v.shape[1], len(edges)))
    flat = np.zeros(v.shape[0], dtype=np.int64)
    inside = np.ones(v.shape[0], dtype=bool)
    stride = 1
    for d, e in enumerate(edges):
        e = np.asarray(e, dtype=np.float64)
        if e.ndim != 1 or e.size < 2 or not np.all(np.diff(e) > 0.0):
            raise ValueError('edges[%d] must be an ascending array of at least two bin edges' % d)
        x = v[:, d]
        ok = (x >= e[0]) & (x <= e[-1])                                   # (a NaN is outside)
        j = np.minimum(np.searchsorted(e, np.where(ok, x, e[0]), side='right') - 1, e.size - 2)
        flat += stride * j
        inside &= ok
        stride *= e.size - 1
    return np.where(inside, flat, -1), int(stride)


# ---- collective variables of stored frames ------------------------------------------------------------------------
# The coordinates a surface is taken over, with the conventions of the force kernels (include/remd_hip_frame_cvs.h): the centroid of
# a group is c = x_first + sum_i w_i img(x_i - x_first) / sum w, img the minimum image under the frame's own box when the variable is
# periodic (restraint_frames_numpy, csrc/custom_centroid.hip); differences between centroids are imaged the same way.
FRAME_CV_DISTANCE, FRAME_CV_ANGLE, FRAME_CV_DIHEDRAL, FRAME_CV_RMSD = 0, 1, 2, 3
_RMSD_MSD_FLOOR = 1e-20                 # nm^2 (csrc/custom_cv_superpose.h)


class _CentroidCV:
    """What DistanceCV, AngleCV and DihedralCV share: ``groups`` (tuples of atom indices in System numbering), ``weights`` (one tuple
    per group or None: the particles' masses; a group of one atom has weight 1) and ``periodic``."""
    kind = None

    def __init__(self, groups, weights, periodic):
        name = type(self).__name__
        self.groups = tuple(self._group(name, g + 1, group) for g, group in enumerate(groups))
        if weights is None:
            weights = [None] * len(self.groups)
        weights = list(weights)
        if len(weights) != len(self.groups):
            raise ValueError('%s: weights must hold one list (or None) per group: %d, not %d' % (name, len(self.groups), len(weights)))
        self.weights = tuple(self._weights(name, g + 1, w, self.groups[g]) for g, w in enumerate(weights))
        self.periodic = bool(periodic)

    @staticmethod
    def _group(name, g, group, what='group %d'):
        what = what % g if '%' in what else what
        atoms = [group] if np.ndim(group) == 0 else list(group)
        if not atoms:
            raise ValueError('%s: %s is empty' % (name, what))
        out = []
        for a in atoms:
            if isinstance(a, bool) or not isinstance(a, (int, np.integer)):
                raise ValueError('%s: %s holds %r, which is not an atom index' % (name, what, a))
            if a < 0:
                raise ValueError('%s: %s holds the negative index %d' % (name, what, a))
            if int(a) in out:
                raise ValueError('%s: %s names atom %d twice' % (name, what, a))
            out.append(int(a))
        return tuple(out)

    @staticmethod
    def _weights(name, g, w, atoms):
        if w is None:
            return None
        w = np.asarray(w, dtype=np.float64).reshape(-1)
        if w.size != len(atoms):
            raise ValueError('%s: group %d has %d atoms but %d weights' % (name, g, len(atoms), w.size))
        if not np.all(np.isfinite(w)) or np.any(w < 0.0):
            raise ValueError('%s: the weights of group %d must be finite and not negative' % (name, g))
        if not w.sum() > 0.0:
            raise ValueError('%s: the weights of group %d sum to zero' % (name, g))
        return tuple(float(x) for x in w)

    def _key(self):
        return (self.kind, self.groups, self.weights, self.periodic)

    def _atoms(self):
        return [a for group in self.groups for a in group]

    def _remapped(self, where, n_system):
        """the same variable over the columns ``where[atom]`` of the stored frames"""
        new = object.__new__(type(self))
        new.groups = tuple(tuple(where[a] for a in group) for group in self.groups)
        new.weights, new.periodic = self.weights, self.periodic
        return new

    def _not_periodic(self):
        new = object.__new__(type(self))
        new.groups, new.weights, new.periodic = self.groups, self.weights, False
        return new


class DistanceCV(_CentroidCV):
    """The distance |d| (nm) between the centroids of two groups, d the minimum image of c2 - c1 when periodic."""
    kind = FRAME_CV_DISTANCE

    def __init__(self, group1, group2, weights1=None, weights2=None, periodic=True):
        super().__init__((group1, group2), (weights1, weights2), periodic)


class AngleCV(_CentroidCV):
    """The angle (rad, [0, pi]) at the centroid of group2 between those of group1 and group3: acos of the cosine clamped to [-1, 1]."""
    kind = FRAME_CV_ANGLE

    def __init__(self, group1, group2, group3, weights=None, periodic=True):
        super().__init__((group1, group2, group3), weights, periodic)


class DihedralCV(_CentroidCV):
    """The dihedral (rad, (-pi, pi]) of the centroids of four groups, atan2(|b2| b1.(b2 x b3), (b1 x b2).(b2 x b3)) with b_k = c_k+1 -
    c_k: the sign and range of PeriodicTorsionForce and of dihedral(p1,p2,p3,p4) in a custom-force expression."""
    kind = FRAME_CV_DIHEDRAL

    def __init__(self, group1, group2, group3, group4, weights=None, periodic=True):
        super().__init__((group1, group2, group3, group4), weights, periodic)


class RMSDCV:
    """The RMSD (nm) of ``particles`` from ``reference_positions`` [N][3] (all particles of the System, as system.RMSDForce takes them)
    after the optimal superposition: system.RMSDForce's value.  A mean square deviation below 1e-20 nm^2 gives 0.  No minimum images
    are taken: the particles must belong to one molecule that the run kept whole."""
    kind = FRAME_CV_RMSD
    periodic = False

    def __init__(self, reference_positions, particles):
        ref = np.array(reference_positions, dtype=np.float64)
        if ref.ndim != 2 or ref.shape[1] != 3:
            raise ValueError('RMSDCV: reference_positions must be [N][3], not an array of shape %r' % (ref.shape,))
        if not np.all(np.isfinite(ref)):
            raise ValueError('RMSDCV: reference_positions are not finite (particle %d)' % int(np.flatnonzero(~np.isfinite(ref).all(axis=1))[0]))
        self.particles = _CentroidCV._group('RMSDCV', 0, particles, what='particles')
        if len(self.particles) < 3:
            raise ValueError('RMSDCV: particles holds %d atoms; an RMSD needs at least 3' % len(self.particles))
        self.reference_positions = ref

    def _key(self):
        return (self.kind, self.particles, self.reference_positions.tobytes())

    def _atoms(self):
        return list(self.particles)

    def _remapped(self, where, n_system):
        if len(self.reference_positions) != n_system:
            raise ValueError('RMSDCV: reference_positions holds %d particles but the System has %d' % (len(self.reference_positions), n_system))
        new = object.__new__(RMSDCV)
        columns = sorted(where.items(), key=lambda item: item[1])                   # (atom, column) in the order of the columns
        new.particles = tuple(where[a] for a in self.particles)
        new.reference_positions = self.reference_positions[[a for a, _ in columns]]
        return new

    def _not_periodic(self):
        return self


def _compile_frame_cvs(cvs, n_atoms, masses):
    """[(kind, periodic, [(atoms int64, normalised weights f64)], centred reference [n][3] or None)] of descriptors whose indices
    address the ``n_atoms`` atoms of a frame: what both evaluators work from."""
    if masses is not None:
        masses = np.asarray(masses, dtype=np.float64).reshape(-1)
        if masses.size != n_atoms:
            raise ValueError('masses must have one entry per atom of pos: %d, not %d' % (n_atoms, masses.size))
    out = []
    for v, cv in enumerate(cvs):
        who = 'variable %d (%s)' % (v, type(cv).__name__)
        if not isinstance(cv, (_CentroidCV, RMSDCV)):
            raise ValueError('variable %d is %r, not a DistanceCV, AngleCV, DihedralCV or RMSDCV' % (v, cv))
        for a in cv._atoms():
            if a >= n_atoms:
                raise ValueError('%s: atom %d is outside the %d atoms of the frames' % (who, a, n_atoms))
        if cv.kind == FRAME_CV_RMSD:
            if len(cv.reference_positions) != n_atoms:
                raise ValueError('%s: reference_positions holds %d particles but the frames have %d' % (who, len(cv.reference_positions), n_atoms))
            atoms = np.array(cv.particles, dtype=np.int64)
            ref = cv.reference_positions[atoms]
            out.append((cv.kind, False, [(atoms, np.full(atoms.size, 1.0 / atoms.size))], ref - ref.mean(axis=0)))
            continue
        groups = []
        for g, (group, w) in enumerate(zip(cv.groups, cv.weights)):
            atoms = np.array(group, dtype=np.int64)
            if atoms.size == 1:
                w = np.ones(1)
            elif w is None:
                if masses is None:
                    raise ValueError('%s: group %d has no weights and no masses were given' % (who, g + 1))
                w = masses[atoms]
                if not np.all(np.isfinite(w)) or np.any(w < 0.0) or not w.sum() > 0.0:
                    raise ValueError('%s: the masses of group %d sum to zero (or are negative): give weights' % (who, g + 1))
            else:
                w = np.array(w, dtype=np.float64)
            groups.append((atoms, w / w.sum()))
        out.append((cv.kind, bool(cv.periodic), groups, None))
    return out


def frame_cv_tables(cvs, n_atoms, masses=None):
    """The CSR tables of remd_frame_cv_tables (include/remd_hip_frame_cvs.h) for descriptors whose indices address the atoms of a frame:
    a dict of kind, periodic [n_cv] i4, cv_groups [n_cv + 1] i4, group_off i4, atoms i4, weights f8 (normalised) and reference
    [entries][3] f8 (the centred reference in the rows of an RMSD's particles, zeros elsewhere)."""
    compiled = _compile_frame_cvs(cvs, n_atoms, masses)
    kind, periodic, cv_groups, group_off, atoms, weights, reference = [], [], [0], [0], [], [], []
    for k, pbc, groups, ref in compiled:
        kind.append(k); periodic.append(int(pbc))
        for a, w in groups:
            atoms.append(a); weights.append(w)
            reference.append(np.zeros((a.size, 3)) if ref is None else ref)
            group_off.append(group_off[-1] + a.size)
        cv_groups.append(cv_groups[-1] + len(groups))
    i4 = lambda x: np.ascontiguousarray(x, dtype=np.int32)
    cat = lambda parts, shape: np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros(shape)
    return dict(kind=i4(kind), periodic=i4(periodic), cv_groups=i4(cv_groups), group_off=i4(group_off),
                atoms=i4(cat(atoms, (0,))), weights=cat(weights, (0,)), reference=cat(reference, (0, 3)))


def _check_frames(cvs, pos, box):
    """(cvs as a list, pos, box as f64 or None) of an evaluator call; the refusals both evaluators share"""
    cvs = list(cvs)
    if not cvs:
        raise ValueError('no collective variable was given')
    pos = np.asarray(pos)
    if pos.ndim != 3 or pos.shape[2] != 3 or pos.shape[0] < 1 or pos.shape[1] < 1:
        raise ValueError('pos must be [F][n_atoms][3] with F >= 1')
    F = pos.shape[0]
    if box is None:
        for v, cv in enumerate(cvs):
            if getattr(cv, 'periodic', False):
                raise ValueError('variable %d (%s) is periodic but the frames have no box: give box [F][3], or periodic=False'
                                 % (v, type(cv).__name__))
    else:
        box = np.asarray(box)
        if box.shape != (F, 3):
            raise ValueError('box must be [F][3] (the edges of a rectangular box; triclinic boxes are not supported)')
        if not (np.all(np.isfinite(box)) and np.all(box > 0.0)):
            raise ValueError('a non-finite or non-positive box edge')
    return cvs, pos, box


def _jacobi_superpose(S):
    """U [F][3][3] with x_i ~ U ref_i from S [F][3][3], S_ab = sum_i x_ia ref_ib (both centred): csrc/custom_cv_math.h over many frames
    at once -- Horn's 4 x 4 matrix, cyclic Jacobi rotations until the off-diagonal share falls below 1e-32 (a frame that has
    converged is rotated no further), the eigenvector of the largest eigenvalue (the first of equal ones) as a unit quaternion."""
    Sxx, Sxy, Sxz = S[:, 0, 0], S[:, 1, 0], S[:, 2, 0]
    Syx, Syy, Syz = S[:, 0, 1], S[:, 1, 1], S[:, 2, 1]
    Szx, Szy, Szz = S[:, 0, 2], S[:, 1, 2], S[:, 2, 2]
    A = np.empty((S.shape[0], 4, 4))
    A[:, 0, 0] = Sxx + Syy + Szz; A[:, 1, 1] = Sxx - Syy - Szz; A[:, 2, 2] = -Sxx + Syy - Szz; A[:, 3, 3] = -Sxx - Syy + Szz
    A[:, 0, 1] = A[:, 1, 0] = Syz - Szy; A[:, 0, 2] = A[:, 2, 0] = Szx - Sxz; A[:, 0, 3] = A[:, 3, 0] = Sxy - Syx
    A[:, 1, 2] = A[:, 2, 1] = Sxy + Syx; A[:, 1, 3] = A[:, 3, 1] = Szx + Sxz; A[:, 2, 3] = A[:, 3, 2] = Syz + Szy
    V = np.zeros_like(A)
    V[:, [0, 1, 2, 3], [0, 1, 2, 3]] = 1.0
    pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    with np.errstate(all='ignore'):
        for _ in range(30):
            off = sum(A[:, p, q] * A[:, p, q] for p, q in pairs)
            diag = sum(A[:, k, k] * A[:, k, k] for k in range(4))
            live = off > 1e-32 * (diag + 2.0 * off)
            if not live.any():
                break
            for p, q in pairs:
                apq = A[:, p, q].copy()
                turn = live & (apq != 0.0)
                theta = (A[:, q, q] - A[:, p, p]) / (2.0 * np.where(turn, apq, 1.0))
                t = np.where(np.abs(theta) > 1e150, 0.5 / theta, np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0)))
                t = np.where(turn, t, 0.0)                                     # (t = 0: c = 1, s = 0, the identity)
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                tau = s / (1.0 + c)
                A[:, p, p] -= t * apq; A[:, q, q] += t * apq
                A[:, p, q] = np.where(turn, 0.0, apq); A[:, q, p] = A[:, p, q]
                for k in range(4):
                    if k != p and k != q:
                        akp, akq = A[:, k, p].copy(), A[:, k, q].copy()
                        A[:, k, p] = A[:, p, k] = akp - s * (akq + tau * akp)
                        A[:, k, q] = A[:, q, k] = akq + s * (akp - tau * akq)
                for k in range(4):
                    vkp, vkq = V[:, k, p].copy(), V[:, k, q].copy()
                    V[:, k, p] = vkp - s * (vkq + tau * vkp)
                    V[:, k, q] = vkq + s * (vkp - tau * vkq)
        lam, quat = A[:, 0, 0].copy(), V[:, :, 0].copy()
        for j in range(1, 4):
            up = A[:, j, j] > lam
            lam = np.where(up, A[:, j, j], lam)
            quat = np.where(up[:, None], V[:, :, j], quat)
        nq = (quat * quat).sum(axis=1)
        quat = quat * np.where(nq > 0.0, 1.0 / np.sqrt(nq), 0.0)[:, None]
    q0, q1, q2, q3 = quat[:, 0], quat[:, 1], quat[:, 2], quat[:, 3]
    U = np.empty((S.shape[0], 3, 3))
    U[:, 0, 0] = q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3; U[:, 0, 1] = 2.0 * (q1 * q2 - q0 * q3); U[:, 0, 2] = 2.0 * (q1 * q3 + q0 * q2)
    U[:, 1, 0] = 2.0 * (q1 * q2 + q0 * q3); U[:, 1, 1] = q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3; U[:, 1, 2] = 2.0 * (q2 * q3 - q0 * q1)
    U[:, 2, 0] = 2.0 * (q1 * q3 - q0 * q2); U[:, 2, 1] = 2.0 * (q2 * q3 + q0 * q1); U[:, 2, 2] = q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3
    return U


def _frames_rmsd(x, ref):
    """RMSD [F] of x [F][n][3] (f64) against the centred reference [n][3]: the two passes of csrc/custom_cv_superpose.h"""
    d = x - x[:, :1, :]
    n = d.shape[1]
    c, S = np.zeros((d.shape[0], 3)), np.zeros((d.shape[0], 3, 3))
    for k in range(n):                                                         # (ascending order within the group)
        c += d[:, k, :]
        S += d[:, k, :, None] * ref[k][None, None, :]
    c /= n
    U = _jacobi_superpose(S)
    m = np.zeros(d.shape[0])
    for k in range(n):
        e = d[:, k, :] - c - U @ ref[k]
        m += (e * e).sum(axis=1)
    msd = m / n
    with np.errstate(invalid='ignore'):
        return np.where(msd >= _RMSD_MSD_FLOOR, np.sqrt(np.where(msd >= _RMSD_MSD_FLOOR, msd, 1.0)), np.where(np.isnan(msd), msd, 0.0))


def frame_cvs_numpy(cvs, pos, box=None, masses=None, frames_per_pass=4096):
    """values [F][n_cv] f64 (nm, rad) of the collective variables ``cvs`` (DistanceCV, AngleCV, DihedralCV, RMSDCV) at F frames, in
    f64 and vectorised over the frames: the host counterpart of remd_frame_cvs (include/remd_hip_frame_cvs.h) with the engine's
    conventions.  ``pos`` [F][n_atoms][3]; the descriptors' indices address its atoms.  ``box`` [F][3] or None (then no variable
    may be periodic); ``masses`` [n_atoms] weigh the groups that carry no weights of their own.  Within a group the sum runs over the
    atoms in ascending order of their place in the group, so a value depends neither on ``frames_per_pass`` nor on the other variables."""
    cvs, pos, box = _check_frames(cvs, pos, box)
    if int(frames_per_pass) < 1:
        raise ValueError('frames_per_pass must be at least 1')
    F, n_atoms = pos.shape[0], pos.shape[1]
    compiled = _compile_frame_cvs(cvs, n_atoms, masses)
    out = np.empty((F, len(compiled)))
    for f0 in range(0, F, int(frames_per_pass)):                 # (bounds the f64 copies of the positions)
        sl = slice(f0, min(F, f0 + int(frames_per_pass)))
        for v, (kind, periodic, groups, ref) in enumerate(compiled):
            if kind == FRAME_CV_RMSD:
                out[sl, v] = _frames_rmsd(pos[sl][:, groups[0][0], :].astype(np.float64), ref)
                continue
            L = box[sl].astype(np.float64) if periodic else None

            def img(d):
                return d - L * np.rint(d / L) if periodic else d
            c = []
            for atoms, w in groups:
                x = pos[sl][:, atoms, :].astype(np.float64)
                acc = np.zeros((x.shape[0], 3))
                for k in range(atoms.size):
                    acc += w[k] * img(x[:, k, :] - x[:, 0, :])
                c.append(x[:, 0, :] + acc)
            with np.errstate(invalid='ignore', divide='ignore'):
                if kind == FRAME_CV_DISTANCE:
                    d = img(c[1] - c[0])
                    out[sl, v] = np.sqrt((d * d).sum(axis=1))
                elif kind == FRAME_CV_ANGLE:
                    v0, v1 = img(c[0] - c[1]), img(c[2] - c[1])
                    cosine = (v0 * v1).sum(axis=1) / np.sqrt((v0 * v0).sum(axis=1) * (v1 * v1).sum(axis=1))
                    out[sl, v] = np.arccos(np.fmin(np.fmax(cosine, -1.0), 1.0))
                else:
                    b1, b2, b3 = img(c[1] - c[0]), img(c[2] - c[1]), img(c[3] - c[2])
                    m, nn = np.cross(b1, b2), np.cross(b2, b3)
                    out[sl, v] = np.arctan2(np.sqrt((b2 * b2).sum(axis=1)) * (b1 * nn).sum(axis=1), (m * nn).sum(axis=1))
    return out


class MBAR:
    """Multistate Bennett acceptance ratio estimator.

    ``u_kn[k, n]`` is the reduced potential of sample ``n`` evaluated in state ``k``; ``N_k[k]`` the number of samples
    drawn from state ``k`` (0 for unsampled states).  Solves  f_i = -ln sum_n exp(-u_in) / sum_k N_k exp(f_k - u_kn)
    (eq. 11) with f_0 = 0.

    ``solver='numpy'`` (the default) does every pass over ``u_kn`` on the host; ``solver='device'`` does them on the GPU
    (include/remd_hip_mbar.h: the same sweeps, Newton iteration, backtracking rule and convergence test, with the K x K algebra
    still on the host).  ``device`` and ``lib_path`` choose the GPU and the engine library of the device solver.

    ``compute_perturbed_free_energies``, ``compute_expectations``, ``compute_multiple_expectations``, ``compute_overlap`` and
    ``compute_effective_sample_number`` take pymbar 4's argument order and defaults and return dicts with pymbar 4's keys.  Their
    uncertainties use the same eq. 8 SVD form (``_theta_of_gram``) as ``compute_free_energy_differences`` and
    ``compute_entropy_and_enthalpy``, on the Gram matrix of the weights augmented by one column per perturbed state and per
    observable (N_k = 0 for those).  With ``solver='device'`` that matrix comes from one call of remd_mbar_augmented_gram and the
    ``[N][K]`` weights never leave the GPU.

    ``n_bootstraps=B`` > 0 also solves B bootstrap replicates (pymbar 4's ``n_bootstraps``), each from the full-sample ``f_k``, and
    keeps their free energies in ``f_k_boots`` [B][K] (each row shifted to f_0 = 0).  A replicate resamples every sampled state's
    samples with replacement, N_k draws from its own N_k samples, and is a vector of multiplicities c_n over the stored samples
    that weights every sum of the estimator (include/remd_hip_mbar.h states the equations and the Philox draws, which
    ``bootstrap_seed`` keys; both solvers draw the same replicates).  ``sample_states`` [N] names the row of ``u_kn`` each sample was
    drawn from; without it the samples lie in pymbar's blocks, the first N_0 from state 0 and so on.
    ``compute_free_energy_differences``, ``compute_perturbed_free_energies`` and ``compute_expectations`` then take
    ``uncertainty_method='bootstrap'``: the population standard deviation (ddof = 0) over the replicates in place of eq. 8.
    With ``solver='device'`` the multiplicities are drawn on the GPU and the replicates are solved there in batches, every pass
    one call for the whole batch; the K x K algebra stays on the host, batched.

    ``compute_pmf`` is the histogram estimator of a free energy surface (pymbar 3's computePMF): a bin index per sample, never a
    row per bin.  Its bin-bin block of the Gram matrix is diagonal and its state-bin block one pass of cost N x K; with
    ``solver='device'`` both come from remd_mbar_pmf, the bootstrap's weighted bin sums from remd_mbar_bootstrap_pmf.
    """

    UNCERTAINTY_METHODS = (None, 'svd', 'bootstrap')
    PMF_UNCERTAINTIES = ('from-lowest', 'from-specified', 'from-normalization', 'all-differences')
    PMF_MAX_BINS = 65536                         # REMD_MBAR_PMF_MAX_BINS of include/remd_hip_mbar.h, for both solvers
    PMF_MAX_COLUMNS = 4096                       # K + non-empty bins + 1 at most where Theta is wanted: it is a host SVD

    def __init__(self, u_kn, N_k, initial_f_k=None, relative_tolerance=1.0e-12, maximum_iterations=10000, solver='numpy',
                 device=0, lib_path=None, n_bootstraps=0, bootstrap_seed=0, sample_states=None):
        if solver not in ('numpy', 'device'):
            raise ValueError("solver must be 'numpy' or 'device', not %r" % (solver,))
        if isinstance(n_bootstraps, bool) or int(n_bootstraps) != n_bootstraps or n_bootstraps < 0:
            raise ValueError('n_bootstraps must be a non-negative integer, not %r' % (n_bootstraps,))
        if isinstance(bootstrap_seed, bool) or int(bootstrap_seed) != bootstrap_seed or not 0 <= bootstrap_seed < 2 ** 64:
            raise ValueError('bootstrap_seed must be an integer in 0 ... 2^64 - 1, not %r' % (bootstrap_seed,))
        self.n_bootstraps, self.bootstrap_seed = int(n_bootstraps), int(bootstrap_seed)
        self.f_k_boots = None
        self.solver = solver
        self._dev = None
        self.u_kn = np.array(u_kn, dtype=np.float64)
        self.N_k = np.array(N_k, dtype=np.int64)
        K, N = self.u_kn.shape
        if self.N_k.shape != (K,) or int(self.N_k.sum()) != N:
            raise ParameterError('N_k must have one entry per state and sum to the number of samples')
        if not np.all(np.isfinite(self.u_kn[self.N_k > 0])):
            raise ParameterError('non-finite reduced potentials in a sampled state')
        self.K, self.N = K, N
        self.sample_states = None
        if sample_states is not None:
            labels = np.array(sample_states)
            if labels.shape != (N,) or labels.dtype.kind not in 'iu' or np.any(labels < 0) or np.any(labels >= K) \
                    or not np.array_equal(np.bincount(labels, minlength=K), self.N_k):
                raise ParameterError('sample_states must name the state each of the %d samples was drawn from: its histogram must be N_k' % N)
            self.sample_states = labels.astype(np.int64)
        f = np.zeros(K) if initial_f_k is None else np.array(initial_f_k, dtype=np.float64) - float(np.asarray(initial_f_k)[0])
        if solver == 'device':
            from .._engine import DeviceMBAR
            self._dev = DeviceMBAR(self.u_kn, self.N_k, device=device, lib_path=lib_path)
            if self.n_bootstraps:
                self._dev._require_bootstrap()
            self.f_k = self._solve_device(f, relative_tolerance, maximum_iterations)
        else:
            self.f_k = self._solve(f, relative_tolerance, maximum_iterations)
        self._log_W = None
        if self.n_bootstraps:
            self._rtol, self._maxiter = relative_tolerance, maximum_iterations
            replicates = np.arange(self.n_bootstraps)
            if self._dev is not None:
                self.f_k_boots = np.concatenate([self._solve_bootstrap_device(r) for r in self._device_batches(replicates)], axis=0)
            else:
                self.f_k_boots = np.stack([self._solve_weighted(self._bootstrap_counts(b), b) for b in replicates])

    # log of the mixture denominator per sample: ln sum_k N_k exp(f_k - u_kn)
    def _log_denominator(self, f_k):
        s = self.N_k > 0
        return _logsumexp(f_k[s, None] - self.u_kn[s, :], axis=0, b=self.N_k[s, None].astype(np.float64))

    def _solve(self, f_k, rtol, maxiter):
        s = np.flatnonzero(self.N_k > 0)
        if s.size == 0:
            raise ParameterError('no sampled state')
        u = self.u_kn[s]
        Nk = self.N_k[s].astype(np.float64)
        f = f_k[s] - f_k[s][0]

        def objective_parts(f):
            log_den = _logsumexp(f[:, None] - u, axis=0, b=Nk[:, None])
            log_W = f[:, None] - u - log_den[None, :]                     # [Ks, N]
            return log_den, log_W

        # a few self-consistent sweeps bring any starting point into Newton's basin
        for _ in range(5):
            log_den, _ = objective_parts(f)
            f_new = -_logsumexp(-u - log_den[None, :], axis=1)
            f = f_new - f_new[0]
        for _ in range(maxiter):
            log_den, log_W = objective_parts(f)
            W = np.exp(log_W)
            g = Nk * (W.sum(axis=1) - 1.0)                                # gradient of the convex objective
            H = np.diag(Nk * W.sum(axis=1)) - (Nk[:, None] * Nk[None, :]) * (W @ W.T)
            if s.size > 1:
                try:
                    step = np.zeros_like(f)
                    step[1:] = np.linalg.solve(H[1:, 1:], g[1:])
                except np.linalg.LinAlgError:
                    step = np.zeros_like(f)
                    step[1:] = np.linalg.lstsq(H[1:, 1:], g[1:], rcond=None)[0]
            else:
                step = np.zeros_like(f)
            phi0 = log_den.sum() - np.dot(Nk, f)
            scale = 1.0
            while True:                                                   # backtrack: the objective must not increase
                f_try = f - scale * step
                phi = objective_parts(f_try)[0].sum() - np.dot(Nk, f_try)
                if phi <= phi0 + 1e-12 * abs(phi0) or scale < 1e-6:
                    break
                scale *= 0.5
            delta = np.max(np.abs(f_try - f))
            f = f_try
            if delta <= rtol * max(1.0, np.max(np.abs(f))):
                break
        else:
            raise ParameterError('MBAR did not converge')
        if not np.all(np.isfinite(f)):
            raise ParameterError('MBAR produced non-finite free energies')
        out = np.zeros(self.K)
        out[s] = f
        # unsampled states: one application of eq. 11 with the converged denominator
        log_den = _logsumexp(f[:, None] - u, axis=0, b=Nk[:, None])
        uns = np.flatnonzero(self.N_k == 0)
        if uns.size:
            out[uns] = -_logsumexp(-self.u_kn[uns] - log_den[None, :], axis=1)
        return out - out[0]

    def _solve_device(self, f_k, rtol, maxiter):
        """_solve with the passes over u_kn on the device: the same algorithm, line by line."""
        dev = self._dev
        s = np.flatnonzero(self.N_k > 0)
        if s.size == 0:
            raise ParameterError('no sampled state')
        Nk = self.N_k[s].astype(np.float64)
        f = f_k[s] - f_k[s][0]

        def full(f):                                                      # the device takes one f per state; the unsampled do not enter
            out = np.zeros(self.K)
            out[s] = f
            return out

        for _ in range(5):
            f_new = dev.self_consistent(full(f))[s]
            f = f_new - f_new[0]
        for _ in range(maxiter):
            W_sum, gram, phi0 = dev.newton_parts(full(f))
            W_sum, WWt = W_sum[s], gram[np.ix_(s, s)]
            g = Nk * (W_sum - 1.0)
            H = np.diag(Nk * W_sum) - (Nk[:, None] * Nk[None, :]) * WWt
            if s.size > 1:
                try:
                    step = np.zeros_like(f)
                    step[1:] = np.linalg.solve(H[1:, 1:], g[1:])
                except np.linalg.LinAlgError:
                    step = np.zeros_like(f)
                    step[1:] = np.linalg.lstsq(H[1:, 1:], g[1:], rcond=None)[0]
            else:
                step = np.zeros_like(f)
            scale = 1.0
            while True:                                                   # backtrack: the objective must not increase
                f_try = f - scale * step
                phi = dev.log_denominator(full(f_try), want_log_den=False)[1]
                if phi <= phi0 + 1e-12 * abs(phi0) or scale < 1e-6:
                    break
                scale *= 0.5
            delta = np.max(np.abs(f_try - f))
            f = f_try
            if delta <= rtol * max(1.0, np.max(np.abs(f))):
                break
        else:
            raise ParameterError('MBAR did not converge')
        if not np.all(np.isfinite(f)):
            raise ParameterError('MBAR produced non-finite free energies')
        out = full(f)
        uns = np.flatnonzero(self.N_k == 0)
        if uns.size:
            out[uns] = dev.self_consistent(out)[uns]
        return out - out[0]

    # ---- bootstrap replicates: the same equations with the multiplicity c_n as the weight of sample n -------------------------------
    def _bootstrap_counts(self, replicate):
        """c_n [N] of one replicate, as the device draws it"""
        from ._philox import bootstrap_counts
        return bootstrap_counts(self.bootstrap_seed, int(replicate), self.N_k, self.sample_states)

    def _solve_weighted(self, c_n, replicate):
        """_solve on the weighted equations, line by line, from the full-sample f_k.  Samples with c_n = 0 do not enter."""
        rtol, maxiter = self._rtol, self._maxiter
        s = np.flatnonzero(self.N_k > 0)
        n = np.flatnonzero(c_n)
        c = np.asarray(c_n, dtype=np.float64)[n]
        u = self.u_kn[np.ix_(s, n)]
        Nk = self.N_k[s].astype(np.float64)
        f = self.f_k[s] - self.f_k[s][0]

        def objective_parts(f):
            log_den = _logsumexp(f[:, None] - u, axis=0, b=Nk[:, None])
            log_W = f[:, None] - u - log_den[None, :]                     # [Ks, Nc]
            return log_den, log_W

        for _ in range(5):
            log_den, _ = objective_parts(f)
            f_new = -_logsumexp(-u - log_den[None, :], axis=1, b=c[None, :])
            f = f_new - f_new[0]
        for _ in range(maxiter):
            log_den, log_W = objective_parts(f)
            W = np.exp(log_W)
            cW = W * c[None, :]
            g = Nk * (cW.sum(axis=1) - 1.0)
            H = np.diag(Nk * cW.sum(axis=1)) - (Nk[:, None] * Nk[None, :]) * (cW @ W.T)
            if s.size > 1:
                try:
                    step = np.zeros_like(f)
                    step[1:] = np.linalg.solve(H[1:, 1:], g[1:])
                except np.linalg.LinAlgError:
                    step = np.zeros_like(f)
                    step[1:] = np.linalg.lstsq(H[1:, 1:], g[1:], rcond=None)[0]
            else:
                step = np.zeros_like(f)
            phi0 = np.dot(c, log_den) - np.dot(Nk, f)
            scale = 1.0
            while True:                                                   # backtrack: the objective must not increase
                f_try = f - scale * step
                phi = np.dot(c, objective_parts(f_try)[0]) - np.dot(Nk, f_try)
                if phi <= phi0 + 1e-12 * abs(phi0) or scale < 1e-6:
                    break
                scale *= 0.5
            delta = np.max(np.abs(f_try - f))
            f = f_try
            if delta <= rtol * max(1.0, np.max(np.abs(f))):
                break
        else:
            raise ParameterError('MBAR did not converge for bootstrap replicate %d' % replicate)
        if not np.all(np.isfinite(f)):
            raise ParameterError('MBAR produced non-finite free energies for bootstrap replicate %d' % replicate)
        out = np.zeros(self.K)
        out[s] = f
        log_den = _logsumexp(f[:, None] - u, axis=0, b=Nk[:, None])
        uns = np.flatnonzero(self.N_k == 0)
        if uns.size:
            out[uns] = -_logsumexp(-self.u_kn[np.ix_(uns, n)] - log_den[None, :], axis=1, b=c[None, :])
        return out - out[0]

    def _device_batches(self, replicates):
        """``replicates`` in runs of at most the device's resident batch; each run is drawn on the device before it is handed out"""
        most = self._dev.bootstrap_max_batch()
        for i in range(0, len(replicates), most):
            r = np.asarray(replicates[i:i + most], dtype=np.int64)
            self._dev.bootstrap_draw(self.bootstrap_seed, int(r.min()), int(r.max() - r.min()) + 1, self.sample_states)
            yield r

    def _solve_bootstrap_device(self, reps):
        """_solve_weighted for the drawn replicates ``reps`` at once: every pass is one call of the device for the replicates still
        iterating, the K x K algebra is batched on the host.  Returns f [len(reps)][K], each row shifted to f_0 = 0."""
        dev, rtol, maxiter = self._dev, self._rtol, self._maxiter
        reps = np.asarray(reps, dtype=np.int64)
        s = np.flatnonzero(self.N_k > 0)
        Ks, nb = s.size, reps.size
        Nk = self.N_k[s].astype(np.float64)
        F = np.tile(self.f_k[s] - self.f_k[s][0], (nb, 1))               # [nb][Ks]

        def full(F):
            out = np.zeros((F.shape[0], self.K))
            out[:, s] = F
            return out

        for _ in range(5):
            f_new = dev.bootstrap_self_consistent(reps, full(F))[:, s]
            F = f_new - f_new[:, :1]
        active = np.arange(nb)
        for _ in range(maxiter):
            f = F[active]
            W_sum, gram, phi0 = dev.bootstrap_newton_parts(reps[active], full(f))
            W_sum, WWt = W_sum[:, s], gram[:, s][:, :, s]
            g = Nk[None, :] * (W_sum - 1.0)
            H = -(Nk[:, None] * Nk[None, :])[None, :, :] * WWt
            H[:, np.arange(Ks), np.arange(Ks)] += Nk[None, :] * W_sum
            step = np.zeros_like(f)
            if Ks > 1:
                try:
                    step[:, 1:] = np.linalg.solve(H[:, 1:, 1:], g[:, 1:, None])[:, :, 0]
                except np.linalg.LinAlgError:                             # a singular replicate: each on its own, as _solve does
                    for i in range(len(active)):
                        try:
                            step[i, 1:] = np.linalg.solve(H[i, 1:, 1:], g[i, 1:])
                        except np.linalg.LinAlgError:
                            step[i, 1:] = np.linalg.lstsq(H[i, 1:, 1:], g[i, 1:], rcond=None)[0]
            scale = np.ones(len(active))
            f_try = f - scale[:, None] * step
            pending = np.arange(len(active))
            while pending.size:                                           # backtrack: the objective must not increase
                f_try[pending] = f[pending] - scale[pending, None] * step[pending]
                phi = dev.bootstrap_log_denominator(reps[active[pending]], full(f_try[pending]), want_log_den=False)[1]
                done = (phi <= phi0[pending] + 1e-12 * np.abs(phi0[pending])) | (scale[pending] < 1e-6)
                pending = pending[~done]
                scale[pending] *= 0.5
            delta = np.max(np.abs(f_try - f), axis=1)
            F[active] = f_try
            active = active[~(delta <= rtol * np.maximum(1.0, np.max(np.abs(f_try), axis=1)))]
            if not active.size:
                break
        else:
            raise ParameterError('MBAR did not converge for bootstrap replicate %d' % reps[active[0]])
        bad = np.flatnonzero(~np.all(np.isfinite(F), axis=1))
        if bad.size:
            raise ParameterError('MBAR produced non-finite free energies for bootstrap replicate %d' % reps[bad[0]])
        out = full(F)
        uns = np.flatnonzero(self.N_k == 0)
        if uns.size:
            out[:, uns] = dev.bootstrap_self_consistent(reps, out)[:, uns]
        return out - out[:, :1]

    def _check_uncertainty_method(self, uncertainty_method):
        """True for 'bootstrap'.  ValueError for a method that is not one of UNCERTAINTY_METHODS, ParameterError (pymbar's sentence) for
        'bootstrap' on an estimator built without replicates."""
        if uncertainty_method not in self.UNCERTAINTY_METHODS:
            raise ValueError("uncertainty_method must be None, 'svd' or 'bootstrap', not %r" % (uncertainty_method,))
        if uncertainty_method == 'bootstrap' and self.n_bootstraps == 0:
            raise ParameterError('Cannot request bootstrap sampling of free energy differences without any bootstraps.')
        return uncertainty_method == 'bootstrap'

    def _bootstrap_rows(self, u_ln=None, A_in=None, obs_state=None):
        """(f_l [B][L], log_cA [B][I]) replicate by replicate: one weighted row pass at each replicate's f_k, as _augmented_gram takes
        them for the full sample.  On the device: remd_mbar_bootstrap_rows, batch by batch."""
        if self._dev is not None:
            parts = [self._dev.bootstrap_rows(r, self.f_k_boots[r], u_ln, A_in, obs_state) for r in self._device_batches(np.arange(self.n_bootstraps))]
            return np.concatenate([p[0] for p in parts], axis=0), np.concatenate([p[1] for p in parts], axis=0)
        L = 0 if u_ln is None else len(u_ln)
        I = 0 if A_in is None else len(A_in)
        f_l, log_cA = np.zeros((self.n_bootstraps, L)), np.zeros((self.n_bootstraps, I))
        sampled = self.N_k > 0
        Nk = self.N_k[sampled, None].astype(np.float64)
        for b in range(self.n_bootstraps):
            c_n = self._bootstrap_counts(b)
            n = np.flatnonzero(c_n)
            c = c_n[n].astype(np.float64)
            f = self.f_k_boots[b]
            log_den = _logsumexp(f[sampled, None] - self.u_kn[np.ix_(sampled, n)], axis=0, b=Nk)
            log_W = f[:, None] - self.u_kn[:, n] - log_den[None, :]      # [K][Nc]
            if L:
                f_l[b] = -_logsumexp(-u_ln[:, n] - log_den[None, :], axis=1, b=c[None, :])
                log_W = np.concatenate([log_W, (f_l[b][:, None] - u_ln[:, n]) - log_den[None, :]], axis=0)
            if I:
                log_cA[b] = _logsumexp(log_W[np.asarray(obs_state, dtype=np.int64)] + np.log(A_in[:, n]), axis=1, b=c[None, :])
        return f_l, log_cA

    @staticmethod
    def _bootstrap_error_of_differences(x_b):
        """the population standard deviation over the replicates of x_j - x_i, [S][S], for x_b [B][S]"""
        return np.std(x_b[:, None, :] - x_b[:, :, None], axis=0)

    @property
    def log_W_nk(self):
        if self._log_W is None and self._dev is not None:
            self._log_W = self._dev.log_weights(self.f_k)
        if self._log_W is None:
            log_den = self._log_denominator(self.f_k)
            self._log_W = (self.f_k[:, None] - self.u_kn - log_den[None, :]).T          # [N, K]
        return self._log_W

    @staticmethod
    def _theta_of(W, N_k):
        """Asymptotic covariance (eq. 8), SVD form:  Theta = V S (I - S V^T N V S)^+ S V^T  with W = U S V^T — only
        the Gram matrix W^T W is needed.  ``W`` may carry extra columns with N_k = 0 (unsampled or observable-weighted
        states)."""
        return MBAR._theta_of_gram(W.T @ W, N_k)

    @staticmethod
    def _theta_of_gram(G, N_k):
        """_theta_of from the Gram matrix G = W^T W."""
        evals, V = np.linalg.eigh(G)
        evals = np.clip(evals, 0.0, None)
        S = np.sqrt(evals)
        M = np.eye(G.shape[0]) - (S[:, None] * (V.T @ (np.asarray(N_k, dtype=np.float64)[:, None] * V))) * S[None, :]
        return (V * S[None, :]) @ np.linalg.pinv(M, rcond=1e-10) @ (V * S[None, :]).T

    def _theta(self):
        if self._dev is not None:
            return self._theta_of_gram(self._dev.gram(self.f_k), self.N_k)
        return self._theta_of(np.exp(self.log_W_nk), self.N_k)

    def _refuse_bootstrap(self, method, uncertainty_method):
        if uncertainty_method not in self.UNCERTAINTY_METHODS:
            raise ValueError("uncertainty_method must be None, 'svd' or 'bootstrap', not %r" % (uncertainty_method,))
        if uncertainty_method == 'bootstrap':
            raise ValueError("%s does not support uncertainty_method='bootstrap'" % method)

    def compute_entropy_and_enthalpy(self, uncertainty_method=None):
        """Reduced enthalpy <u_i>_i and entropy s_i = <u_i>_i - f_i differences with their uncertainties
        (pymbar's compute_entropy_and_enthalpy; section IV of the MBAR paper: each <u_i>_i is the ratio of the
        normalisation constants of an extra, u-weighted state and of state i, so its error follows from the covariance
        of the augmented set of free energies).  Returns a dict with Delta_f, dDelta_f, Delta_u, dDelta_u, Delta_s,
        dDelta_s; Delta_x[i, j] = x_j - x_i.  Asymptotic uncertainties only: 'bootstrap' is a ValueError."""
        self._refuse_bootstrap('compute_entropy_and_enthalpy', uncertainty_method)
        K = self.K
        if self._dev is not None:
            shift = self.u_kn.min() - 1.0
            G, log_cA = self._dev.gram(self.f_k, with_observable=True)
            Theta = self._theta_of_gram(G, np.concatenate([self.N_k, np.zeros(K, dtype=np.int64)]))
        else:
            log_W = self.log_W_nk                                         # [N, K]
            u = self.u_kn.T                                               # [N, K]
            shift = u.min() - 1.0                                         # observable made positive for the logarithm
            A = u - shift
            log_WA_raw = log_W + np.log(A)
            log_cA = _logsumexp(log_WA_raw, axis=0)                       # ln <A>_i (shifted)
            W_aug = np.concatenate([np.exp(log_W), np.exp(log_WA_raw - log_cA[None, :])], axis=1)
            Theta = self._theta_of(W_aug, np.concatenate([self.N_k, np.zeros(K, dtype=np.int64)]))
        A_i = np.exp(log_cA)
        u_i = A_i + shift
        # x = (f_0..f_{K-1}, u_0..u_{K-1}) is linear in the augmented free energies: du_i = <A>_i (df_i - df_{K+i})
        J = np.zeros((2 * K, 2 * K))
        J[:K, :K] = np.eye(K)
        J[K:, :K] = np.diag(A_i)
        J[K:, K:] = -np.diag(A_i)
        C = J @ Theta @ J.T

        def diff_and_err(value, L):                                   # value_j - value_i and its error; L maps x -> value
            cov = L @ C @ L.T
            d2 = np.diag(cov)[:, None] + np.diag(cov)[None, :] - 2.0 * cov
            d2 = np.where(np.abs(d2) < 1e-14, 0.0, d2)
            with np.errstate(invalid='ignore'):
                err = np.sqrt(d2)
            np.fill_diagonal(err, 0.0)
            return value[None, :] - value[:, None], err
        Lf = np.concatenate([np.eye(K), np.zeros((K, K))], axis=1)
        Lu = np.concatenate([np.zeros((K, K)), np.eye(K)], axis=1)
        Df, dDf = diff_and_err(self.f_k, Lf)
        Du, dDu = diff_and_err(u_i, Lu)
        Ds, dDs = diff_and_err(u_i - self.f_k, Lu - Lf)
        return dict(Delta_f=Df, dDelta_f=dDf, Delta_u=Du, dDelta_u=dDu, Delta_s=Ds, dDelta_s=dDs)

    def compute_free_energy_differences(self, uncertainty_method=None):
        """(Delta_f_ij, dDelta_f_ij) with Delta_f_ij[i, j] = f_j - f_i (pymbar's convention).  ``uncertainty_method``: None or 'svd',
        the asymptotic covariance; 'bootstrap', the standard deviation of f_j - f_i over the replicates."""
        bootstrap = self._check_uncertainty_method(uncertainty_method)
        f = self.f_k
        Delta = f[None, :] - f[:, None]
        if bootstrap:
            return Delta, self._bootstrap_error_of_differences(self.f_k_boots)
        Theta = self._theta()
        d2 = np.diag(Theta)[:, None] + np.diag(Theta)[None, :] - 2.0 * Theta
        d2 = np.where(np.abs(d2) < 1e-14, 0.0, d2)
        with np.errstate(invalid='ignore'):
            dDelta = np.sqrt(d2)                     # NaN where the estimate of the variance is negative (under-sampling)
        np.fill_diagonal(dDelta, 0.0)
        return Delta, dDelta

    # ---- perturbed states, observables, overlap: one augmented Gram matrix each ------------------------------------
    @staticmethod
    def _sqrt_of_variance(v):
        """sqrt with the rule of compute_free_energy_differences: |v| < 1e-14 is 0, a negative variance gives NaN"""
        v = np.where(np.abs(v) < 1e-14, 0.0, v)
        with np.errstate(invalid='ignore'):
            return np.sqrt(v)

    @classmethod
    def _error_of_differences(cls, cov):
        err = cls._sqrt_of_variance(np.diag(cov)[:, None] + np.diag(cov)[None, :] - 2.0 * cov)
        np.fill_diagonal(err, 0.0)
        return err

    def _check_u_ln(self, u_ln, what='u_ln'):
        """[L][N] reduced potentials of perturbed states: +inf is a sample of weight 0, -inf and NaN are refused, and so is a state
        whose weights all vanish."""
        u = np.array(u_ln, dtype=np.float64)
        if u.ndim != 2 or u.shape[0] < 1 or u.shape[1] != self.N:
            raise ParameterError('%s must be [L][N] with L >= 1 and N = %d samples' % (what, self.N))
        if np.any(np.isnan(u)) or np.any(np.isneginf(u)):
            raise ParameterError('%s holds a NaN or -inf: only +inf (a sample of weight 0) is allowed' % what)
        empty = np.flatnonzero(np.all(np.isposinf(u), axis=1))
        if empty.size:
            raise ParameterError('state %d of %s has no sample with a non-zero weight' % (empty[0], what))
        return u

    def _check_observables(self, A, rows, what):
        A = np.array(A, dtype=np.float64)
        if A.shape != (rows, self.N):
            raise ParameterError('%s must be [%d][N] with N = %d samples' % (what, rows, self.N))
        if not np.all(np.isfinite(A)):
            raise ParameterError('%s holds a non-finite value' % what)
        return A

    def _augmented_gram(self, u_ln=None, A_in=None, obs_state=None):
        """(f_l [L], log_cA [I], G [C][C]): the Gram matrix of the weights of the K states, then of the L perturbed states ``u_ln``,
        then of the I observables ``A_in`` (> 0), observable i weighted into column ``obs_state[i]`` < K + L:
        exp(ln W_n,s + ln A_in - log_cA_i) with log_cA_i = ln sum_n W_ns A_in.  On the device: remd_mbar_augmented_gram."""
        if self._dev is not None:
            return self._dev.augmented_gram(self.f_k, u_ln, A_in, obs_state)
        log_den = self._log_denominator(self.f_k)
        log_W = self.log_W_nk.T                                               # [K][N]
        f_l = np.zeros(0)
        if u_ln is not None:
            f_l = -_logsumexp(-u_ln - log_den[None, :], axis=1)
            log_W = np.concatenate([log_W, (f_l[:, None] - u_ln) - log_den[None, :]], axis=0)
        W, log_cA = np.exp(log_W), np.zeros(0)
        if A_in is not None:
            raw = log_W[np.asarray(obs_state, dtype=np.int64)] + np.log(A_in)
            log_cA = _logsumexp(raw, axis=1)
            W = np.concatenate([W, np.exp(raw - log_cA[:, None])], axis=0)
        return f_l, log_cA, W @ W.T

    def _observable_covariance(self, G, obs_state, cA, constant):
        """Covariance of <A_i> = cA_i (+ shift): ln cA_i = f_s(i) - f_(column of observable i), so d cA_i = cA_i (df_s(i) - df_col(i));
        an observable that is constant over the samples has no variance and no covariance, exactly."""
        C, n_obs = G.shape[0], len(cA)
        Theta = self._theta_of_gram(G, np.concatenate([self.N_k, np.zeros(C - self.K, dtype=np.int64)]))
        J = np.zeros((n_obs, C))
        rows = np.arange(n_obs)
        J[rows, obs_state] = cA
        J[rows, C - n_obs + rows] = -cA
        J[constant] = 0.0
        return J @ Theta @ J.T

    def compute_perturbed_free_energies(self, u_ln, uncertainty_method=None):
        """Free energy differences between L states that were not simulated, from the stored samples: ``u_ln[l, n]`` is the reduced
        potential of sample n in new state l (+inf: the sample has weight 0 there).  f_l = -ln sum_n exp(-u_ln - log_den_n); the
        uncertainties come from Theta over the K + L columns, the new ones with N_k = 0, or with ``uncertainty_method='bootstrap'``
        from the f_l of every replicate (one weighted row pass at the replicate's f_k).  Returns a dict with Delta_f [L][L] and
        dDelta_f [L][L]; Delta_f[i, j] = f_j - f_i.  ParameterError for a -inf or NaN entry and for a state whose weights all vanish."""
        bootstrap = self._check_uncertainty_method(uncertainty_method)
        u_ln = self._check_u_ln(u_ln)
        f_l, _, G = self._augmented_gram(u_ln=u_ln)
        if bootstrap:
            return dict(Delta_f=f_l[None, :] - f_l[:, None], dDelta_f=self._bootstrap_error_of_differences(self._bootstrap_rows(u_ln=u_ln)[0]))
        K = self.K
        Theta = self._theta_of_gram(G, np.concatenate([self.N_k, np.zeros(len(f_l), dtype=np.int64)]))
        return dict(Delta_f=f_l[None, :] - f_l[:, None], dDelta_f=self._error_of_differences(Theta[K:, K:]))

    # ---- free energy surfaces over binned samples ---------------------------------------------------------------------------------
    @staticmethod
    def _bin_lists(bin_n, nbins):
        """(order, present, first): the binned samples by bin, ascending in each bin; the bins that hold a sample; where the list of
        each of those starts in ``order``"""
        order = np.flatnonzero(bin_n >= 0)
        order = order[np.argsort(bin_n[order], kind='stable')]
        present, first = np.unique(bin_n[order], return_index=True)
        return order, present, first

    @staticmethod
    def _bin_free_energies(term, weight, lists, nbins):
        """f_i [nbins] = -ln sum_{n in i} weight_n exp(term_n), every bin shifted by its own maximum over weight_n > 0; +inf for a bin
        without a sample of non-zero weight.  ``term`` and ``weight`` are [N]."""
        order, present, first = lists
        f_i = np.full(nbins, np.inf)
        if order.size == 0:
            return f_i
        w = weight[order]
        t = np.where(w > 0.0, term[order], -np.inf)
        m = np.maximum.reduceat(t, first)
        m = np.where(np.isfinite(m), m, 0.0)
        size = np.diff(np.append(first, order.size))
        with np.errstate(divide='ignore'):
            f_i[present] = -(np.log(np.add.reduceat(w * np.exp(t - np.repeat(m, size)), first)) + m)
        return f_i

    def _pmf_parts(self, u_n, bin_n, nbins, want_all):
        """(f_i [nbins], cross [K][nbins], diag [nbins], parts of the column z or None) at the solved f_k: what remd_mbar_pmf returns,
        and on the device its call."""
        if self._dev is not None:
            return self._dev.pmf(self.f_k, u_n, bin_n, nbins, want_all=want_all)
        K = self.K
        lists = order, present, first = self._bin_lists(bin_n, nbins)
        log_w = -u_n - self._log_denominator(self.f_k)
        f_i = self._bin_free_energies(log_w, np.ones(self.N), lists, nbins)
        cross, diag = np.zeros((K, nbins)), np.zeros(nbins)
        if order.size:
            f_of = f_i[bin_n[order]]
            finite = np.isfinite(f_of)
            W_i = np.zeros(order.size)
            W_i[finite] = np.exp(f_of[finite] + log_w[order][finite])     # W_n,i on the samples of the bins, 0 for an empty bin
            diag[present] = np.add.reduceat(W_i * W_i, first)
            cross[:, present] = np.add.reduceat(np.exp(self.log_W_nk[order]) * W_i[:, None], first, axis=0).T
        parts = None
        if want_all:                             # W_n,z = exp(f_z - f_i) W_n,i on the samples of bin i: the same per-bin sums
            parts = np.zeros(2 + K + nbins)
            full = np.isfinite(f_i)
            parts[0] = np.inf
            if full.any():
                f_z = parts[0] = -_logsumexp(-f_i[full])
                e = np.exp(f_z - f_i[full])
                parts[1] = np.sum(e * e * diag[full])
                parts[2:2 + K] = cross[:, full] @ e
                parts[2 + K:][full] = e * diag[full]
        return f_i, cross, diag, parts

    def _bootstrap_pmf(self, u_n, bin_n, nbins):
        """f_i [B][nbins] replicate by replicate: the weighted bin sums with the replicate's multiplicities and its log_den at
        f_k_boots[b].  On the device: remd_mbar_bootstrap_pmf, batch by batch."""
        if self._dev is not None:
            return np.concatenate([self._dev.bootstrap_pmf(r, self.f_k_boots[r], u_n, bin_n, nbins)
                                   for r in self._device_batches(np.arange(self.n_bootstraps))], axis=0)
        lists = self._bin_lists(bin_n, nbins)
        out = np.empty((self.n_bootstraps, nbins))
        for b in range(self.n_bootstraps):
            c_n = self._bootstrap_counts(b).astype(np.float64)
            out[b] = self._bin_free_energies(-u_n - self._log_denominator(self.f_k_boots[b]), c_n, lists, nbins)
        return out

    def compute_pmf(self, u_n, bin_n, nbins, uncertainties='from-lowest', pmf_reference=None, uncertainty_method=None):
        """The free energy surface over binned samples (pymbar 3's computePMF, histogram form): ``u_n[n]`` is the reduced potential
        of sample n at the state the surface is wanted at (+inf: the sample has weight 0), ``bin_n[n]`` its bin in 0 ... nbins - 1,
        or -1 for a sample in no bin (``bin_samples`` makes them from coordinates and edges).  f_i = -ln sum_{n in i}
        exp(-u_n - log_den_n); a bin without a sample of non-zero weight is empty: f_i = +inf, df_i = NaN, no part in the covariance.

        ``uncertainties``: 'from-lowest' shifts f_i by its lowest entry f_j and gives the error of f_i - f_j; 'from-specified' the same
        with j = ``pmf_reference`` in the errors; 'from-normalization' shifts to sum_i exp(-f_i) = 1 and gives the error against the
        normalised weight over all binned samples; 'all-differences' shifts as 'from-lowest' and gives the [nbins][nbins] matrix of the
        errors of f_i - f_j (NaN in the rows and columns of empty bins).  The errors come from Theta (eq. 8) over the K states and one
        column per non-empty bin (N = 0 for those), or with ``uncertainty_method='bootstrap'`` as the population standard deviation
        over the replicates in which both bins are non-empty (NaN with fewer than two such replicates).

        Returns a dict with f_i [nbins], df_i [nbins] (or [nbins][nbins]) and n_i [nbins], the samples per bin.  ParameterError: a NaN
        or -inf in u_n, every bin empty.  ValueError: bin_n, nbins, uncertainties, pmf_reference; K + non-empty bins + 1 above
        PMF_MAX_COLUMNS for the asymptotic errors."""
        bootstrap = self._check_uncertainty_method(uncertainty_method)
        if uncertainties not in self.PMF_UNCERTAINTIES:
            raise ValueError('uncertainties must be one of %s, not %r' % (', '.join(repr(x) for x in self.PMF_UNCERTAINTIES), uncertainties))
        if isinstance(nbins, bool) or not isinstance(nbins, (int, np.integer)) or not 1 <= nbins <= self.PMF_MAX_BINS:
            raise ValueError('nbins must be an integer in 1 ... %d, not %r' % (self.PMF_MAX_BINS, nbins))
        nbins = int(nbins)
        bins = np.asarray(bin_n)
        if bins.shape != (self.N,) or bins.dtype.kind not in 'iu' or np.any(bins < -1) or np.any(bins >= nbins):
            raise ValueError('bin_n must hold one integer in -1 ... nbins - 1 = %d for each of the %d samples' % (nbins - 1, self.N))
        bins = bins.astype(np.int64)
        u = np.array(u_n, dtype=np.float64)
        if u.shape != (self.N,):
            raise ParameterError('u_n must be [N] with N = %d samples' % self.N)
        if np.any(np.isnan(u)) or np.any(np.isneginf(u)):
            raise ParameterError('u_n holds a NaN or -inf: only +inf (a sample of weight 0) is allowed')
        f_i, cross, diag, parts = self._pmf_parts(u, bins, nbins, uncertainties == 'from-normalization')
        full = np.flatnonzero(np.isfinite(f_i))
        if full.size == 0:
            raise ParameterError('every bin is empty: no binned sample has a non-zero weight')
        lowest = int(np.argmin(f_i))
        reference = lowest
        if uncertainties == 'from-specified':
            if isinstance(pmf_reference, bool) or not isinstance(pmf_reference, (int, np.integer)) or not 0 <= pmf_reference < nbins \
                    or not np.isfinite(f_i[pmf_reference]):
                raise ValueError('pmf_reference must be a non-empty bin in 0 ... %d, not %r' % (nbins - 1, pmf_reference))
            reference = int(pmf_reference)
        n_i = np.bincount(bins[bins >= 0], minlength=nbins)
        normalised = uncertainties == 'from-normalization'
        f_z = -_logsumexp(-f_i[full])
        out_f = f_i - (f_z if normalised else f_i[lowest])
        if bootstrap:
            f_b = self._bootstrap_pmf(u, bins, nbins)                         # [B][nbins], +inf where a replicate leaves a bin empty
            with np.errstate(invalid='ignore'):
                if normalised:
                    ref_b = np.array([-_logsumexp(-row[np.isfinite(row)]) if np.isfinite(row).any() else np.inf for row in f_b])
                    d = f_b - ref_b[:, None]
                elif uncertainties == 'all-differences':
                    d = f_b[:, :, None] - f_b[:, None, :]
                else:
                    d = f_b - f_b[:, reference:reference + 1]
            return dict(f_i=out_f, df_i=self._std_of_finite(d), n_i=n_i)
        K, ne = self.K, full.size
        C = K + ne + (1 if normalised else 0)
        if K + ne + 1 > self.PMF_MAX_COLUMNS:
            raise ValueError("compute_pmf: K + non-empty bins + 1 = %d exceeds %d columns of the asymptotic covariance (a host SVD); "
                             "use uncertainty_method='bootstrap'" % (K + ne + 1, self.PMF_MAX_COLUMNS))
        G = np.zeros((C, C))
        G[:K, :K] = self._gram()
        G[:K, K:K + ne] = cross[:, full]
        G[K:K + ne, :K] = cross[:, full].T
        G[np.arange(K, K + ne), np.arange(K, K + ne)] = diag[full]
        if normalised:
            G[-1, -1] = parts[1]
            G[-1, :K] = G[:K, -1] = parts[2:2 + K]
            G[-1, K:K + ne] = G[K:K + ne, -1] = parts[2 + K:][full]
        Theta = self._theta_of_gram(G, np.concatenate([self.N_k, np.zeros(C - K, dtype=np.int64)]))
        err = self._error_of_differences(Theta[K:, K:])                       # [ne (+ 1)][ne (+ 1)]
        if uncertainties == 'all-differences':
            df = np.full((nbins, nbins), np.nan)
            df[np.ix_(full, full)] = err
        else:
            df = np.full(nbins, np.nan)
            df[full] = err[:ne, -1] if normalised else err[:ne, int(np.searchsorted(full, reference))]
        return dict(f_i=out_f, df_i=df, n_i=n_i)

    @staticmethod
    def _std_of_finite(d):
        """the population standard deviation over axis 0 of the finite entries of d; NaN where fewer than two are finite"""
        ok = np.isfinite(d)
        n = ok.sum(axis=0)
        x = np.where(ok, d, 0.0)
        with np.errstate(invalid='ignore', divide='ignore'):
            mean = x.sum(axis=0) / n
            var = np.where(ok, (d - mean) ** 2, 0.0).sum(axis=0) / n
        return np.where(n >= 2, np.sqrt(var), np.nan)

    def compute_expectations(self, A_n, u_kn=None, output='averages', state_dependent=False, uncertainty_method=None):
        """<A> at every state with its uncertainty.  ``A_n`` is [N], or [S][N] with ``state_dependent=True`` (row s is the observable
        of state s).  ``u_kn=None``: the S = K states of the estimator; otherwise the S = L perturbed states ``u_kn`` [L][N].
        ``output='averages'`` returns a dict with mu [S] and sigma [S]; ``'differences'`` one with mu [S][S] (mu_j - mu_i) and the
        sigma [S][S] of those differences.  The observable is shifted by min(A) - 1 to be positive for the logarithm, as in
        compute_entropy_and_enthalpy; a constant observable has sigma = 0.  ``uncertainty_method='bootstrap'``: sigma is the standard
        deviation over the replicates of mu (or of mu_j - mu_i), each replicate's mu from one weighted row pass at its own f_k."""
        if output not in ('averages', 'differences'):
            raise ParameterError("output must be 'averages' or 'differences', not %r" % (output,))
        bootstrap = self._check_uncertainty_method(uncertainty_method)
        u_ln = None if u_kn is None else self._check_u_ln(u_kn, 'u_kn')
        K = self.K
        S = K if u_ln is None else u_ln.shape[0]
        if state_dependent:
            A = self._check_observables(A_n, S, 'A_n (state_dependent)')
        else:
            A = np.broadcast_to(self._check_observables(np.reshape(np.asarray(A_n, dtype=np.float64), (1, -1)), 1, 'A_n'), (S, self.N))
        shift = A.min() - 1.0
        obs_state = np.arange(S) + (0 if u_ln is None else K)
        _, log_cA, G = self._augmented_gram(u_ln, np.ascontiguousarray(A - shift), obs_state)
        cA = np.exp(log_cA)
        constant = A.max(axis=1) == A.min(axis=1)
        mu = np.where(constant, A[:, 0], cA + shift)                          # <c> = c, not c (1 + the rounding of sum_n W)
        if bootstrap:
            log_cA_b = self._bootstrap_rows(u_ln, np.ascontiguousarray(A - shift), obs_state)[1]
            mu_b = np.where(constant[None, :], A[None, :, 0], np.exp(log_cA_b) + shift)             # [B][S]
            if output == 'averages':
                return dict(mu=mu, sigma=np.std(mu_b, axis=0))
            return dict(mu=mu[None, :] - mu[:, None], sigma=self._bootstrap_error_of_differences(mu_b))
        cov = self._observable_covariance(G, obs_state, cA, constant)
        if output == 'averages':
            return dict(mu=mu, sigma=self._sqrt_of_variance(np.diag(cov)))
        return dict(mu=mu[None, :] - mu[:, None], sigma=self._error_of_differences(cov))

    def compute_multiple_expectations(self, A_in, u_n, compute_covariance=False, uncertainty_method=None):
        """<A_i> of I observables ``A_in`` [I][N] at the one state whose reduced potentials of the stored samples are ``u_n`` [N].
        Returns a dict with mu [I] and sigma [I], and with ``compute_covariance`` also covariances [I][I].  Each observable is
        shifted by its own minimum - 1.  Asymptotic uncertainties only: 'bootstrap' is a ValueError."""
        self._refuse_bootstrap('compute_multiple_expectations', uncertainty_method)
        u_ln = self._check_u_ln(np.reshape(np.asarray(u_n, dtype=np.float64), (1, -1)), 'u_n')
        A = np.asarray(A_in, dtype=np.float64)
        if A.ndim != 2 or A.shape[0] < 1:
            raise ParameterError('A_in must be [I][N] with I >= 1')
        A = self._check_observables(A, A.shape[0], 'A_in')
        shift = A.min(axis=1) - 1.0
        obs_state = np.full(A.shape[0], self.K)
        _, log_cA, G = self._augmented_gram(u_ln, A - shift[:, None], obs_state)
        cA = np.exp(log_cA)
        constant = A.max(axis=1) == A.min(axis=1)
        cov = self._observable_covariance(G, obs_state, cA, constant)
        out = dict(mu=np.where(constant, A[:, 0], cA + shift), sigma=self._sqrt_of_variance(np.diag(cov)))
        if compute_covariance:
            out['covariances'] = cov
        return out

    def _gram(self):
        """W^T W [K][K] of the weights of the K states"""
        if self._dev is not None:
            return self._dev.gram(self.f_k)
        W = np.exp(self.log_W_nk)
        return W.T @ W

    def compute_overlap(self):
        """The overlap of the states: matrix = W^T W diag(N_k) [K][K] (row i: the probability that a sample weighted into state i
        was drawn from state j; rows sum to 1), its eigenvalues sorted from greatest to least (the first is 1) and
        scalar = 1 - the second eigenvalue (1 with a single state, where there is no second).  Returns a dict with scalar,
        eigenvalues, matrix.  The eigenvalues are those of the symmetric sqrt(N) W^T W sqrt(N), which has the same spectrum."""
        G = self._gram()
        root = np.sqrt(self.N_k.astype(np.float64))
        eigenvalues = np.linalg.eigvalsh(root[:, None] * G * root[None, :])[::-1]
        second = eigenvalues[1] if eigenvalues.size > 1 else 0.0
        return dict(scalar=1.0 - second, eigenvalues=eigenvalues, matrix=G * self.N_k[None, :].astype(np.float64))

    def compute_effective_sample_number(self):
        """Kish's effective number of samples of every state, 1 / sum_n W_nk^2 (pymbar returns the array itself; here, like the
        other methods, a dict: n_eff [K])."""
        with np.errstate(divide='ignore'):
            return dict(n_eff=1.0 / np.diag(self._gram()))


# ---- the analyzer pipeline (global neighbourhoods) --------------------------------------------------------------
class MultiStateSamplerAnalyzer:
    """Free energies from a ``MultiStateReporter`` (multistateanalyzer.py:1164; global neighbourhoods only)."""

    def __init__(self, reporter, n_equilibration_iterations=None, statistical_inefficiency=None, max_subset=100,
                 max_n_iterations=None, use_full_trajectory=False, analysis_kwargs=None, unbias_restraint=True,
                 restraint_energy_cutoff='auto', restraint_distance_cutoff='auto'):
        if statistical_inefficiency is not None and n_equilibration_iterations is None:
            raise Exception('Cannot specify statistical_inefficiency without n_equilibration_iterations, because '
                            'otherwise n_equilibration_iterations cannot be computed for the given '
                            'statistical_inefficiency.')                                     # :1209-1213
        self._reporter = reporter
        self._n_equilibration_iterations = n_equilibration_iterations
        self._statistical_inefficiency = statistical_inefficiency
        self._max_subset = max_subset
        self._max_n_iterations = max_n_iterations
        self.use_full_trajectory = use_full_trajectory
        self._kwargs = dict(analysis_kwargs or {})
        # who evaluates the restraint at the stored frames: 'numpy' (restraint_frames_numpy, no GPU) or 'device' (csrc/restraint_frames.hip)
        if self._kwargs.get('restraint_solver', 'numpy') not in ('numpy', 'device'):
            raise ValueError("analysis_kwargs['restraint_solver'] must be 'numpy' or 'device', not %r" % (self._kwargs['restraint_solver'],))
        # who scans the effective-energy timeseries for the equilibration time: 'numpy' (the loop over the lags) or 'device' (csrc/timeseries.hip)
        if self._kwargs.get('timeseries_solver', 'numpy') not in ('numpy', 'device'):
            raise ValueError("analysis_kwargs['timeseries_solver'] must be 'numpy' or 'device', not %r" % (self._kwargs['timeseries_solver'],))
        # who walks the stored energies (effective energies, u_ln / N_l assembly, transition counts and the state walk's statistical
        # inefficiency): 'numpy' (the loops below) or 'device' (csrc/energy_store.hip)
        if self._kwargs.get('assembly_solver', 'numpy') not in ('numpy', 'device'):
            raise ValueError("analysis_kwargs['assembly_solver'] must be 'numpy' or 'device', not %r" % (self._kwargs['assembly_solver'],))
        # who evaluates collective variables at the stored frames: 'numpy' (frame_cvs_numpy, no GPU) or 'device' (csrc/frame_cvs.hip)
        self._check_cv_solver(self._kwargs.get('cv_solver', 'numpy'))
        self._collective_variables = {}         # {descriptor keys: [n_iterations + 1][n_replicas][n_cv]}, kept until clear()
        self._parameter_derivatives = None      # (names, reduced [n_iterations + 1][n_replicas][n_states][n]), kept until clear()
        # bootstrap uncertainties of MBAR: the number of replicates (0: none), the key of their draws, and the uncertainty the free
        # energies are reported with (None or 'svd': asymptotic; 'bootstrap')
        self._check_bootstrap_option('n_bootstraps', self._kwargs.get('n_bootstraps', 0))
        self._check_bootstrap_option('bootstrap_seed', self._kwargs.get('bootstrap_seed', 0))
        self._check_bootstrap_option('uncertainty_method', self._kwargs.get('uncertainty_method'))
        self._sample_states = None              # [N]: the row of the matrix handed to MBAR each of its columns was drawn from
        self._sample_columns = None             # (iterations, kept columns or None): the frames behind the columns of that matrix
        self._energy_store = None               # the DeviceEnergyStore of assembly_solver = 'device', made on first use
        self._equilibration_data = None
        self._mbar = None
        self._unbiased = None                   # (u_ln, N_l, initial_f_k) handed to MBAR
        self._radially_symmetric_restraint_data = None
        self._restraint_energies, self._restraint_distances = {}, {}      # {iteration: [replica]} kJ/mol / nm, kept across cutoffs
        self._unbias_restraint = unbias_restraint
        self._restraint_energy_cutoff = restraint_energy_cutoff
        self._restraint_distance_cutoff = restraint_distance_cutoff
        self.name = None                       # :611-617: the phase name used when analyzers are combined
        self.reference_states = (0, -1)         # :633-643: the two states a phase's free energy is reported between
        self._sign = '+'

    # ---- the PhaseAnalyzer surface (multistateanalyzer.py:446-1134) ----------------------------------------------
    observables = ('free_energy', 'entropy', 'enthalpy')     # default registry (:304-340): two-state observables, errors in quadrature

    @property
    def reporter(self):
        return self._reporter

    def _restraint_option(name):                 # :1136-1169: a change forgets MBAR and the unbiased matrices, not the frame energies
        def fget(self):
            return getattr(self, '_' + name)

        def fset(self, value):
            old = getattr(self, '_' + name)
            same = type(old) is type(value) and old == value
            setattr(self, '_' + name, value)
            if not same:
                self._mbar = None
                self._unbiased = None
        return property(fget, fset)

    @staticmethod
    def _check_bootstrap_option(key, value):
        if key == 'uncertainty_method':
            ok = value in MBAR.UNCERTAINTY_METHODS
        else:
            ok = isinstance(value, (int, np.integer)) and not isinstance(value, bool) and 0 <= value < (2 ** 31 if key == 'n_bootstraps' else 2 ** 64)
        if not ok:
            raise ValueError("analysis_kwargs[%r] must be %s, not %r" % (key, {
                'n_bootstraps': 'a non-negative integer', 'bootstrap_seed': 'an integer in 0 ... 2^64 - 1',
                'uncertainty_method': "None, 'svd' or 'bootstrap'"}[key], value))

    def _bootstrap_option(key, default, forgets_mbar):      # a change of the replicates forgets MBAR alone; of the method, nothing
        def fget(self):
            return self._kwargs.get(key, default)

        def fset(self, value):
            self._check_bootstrap_option(key, value)
            if forgets_mbar and value != self._kwargs.get(key, default):
                self._mbar = None
            self._kwargs[key] = value
        return property(fget, fset)

    n_bootstraps = _bootstrap_option('n_bootstraps', 0, True)
    bootstrap_seed = _bootstrap_option('bootstrap_seed', 0, True)
    uncertainty_method = _bootstrap_option('uncertainty_method', None, False)
    del _bootstrap_option

    @staticmethod
    def _check_cv_solver(value, what="analysis_kwargs['cv_solver']"):
        if value not in ('numpy', 'device'):
            raise ValueError("%s must be 'numpy' or 'device', not %r" % (what, value))

    @property
    def cv_solver(self):
        """Who evaluates ``get_collective_variables``: 'numpy' or 'device'.  A change forgets the values computed so far."""
        return self._kwargs.get('cv_solver', 'numpy')

    @cv_solver.setter
    def cv_solver(self, value):
        self._check_cv_solver(value)
        if value != self.cv_solver:
            self._collective_variables = {}
        self._kwargs['cv_solver'] = value

    unbias_restraint = _restraint_option('unbias_restraint')
    restraint_energy_cutoff = _restraint_option('restraint_energy_cutoff')            # kT, 'auto' or None
    restraint_distance_cutoff = _restraint_option('restraint_distance_cutoff')        # nm, 'auto' or None
    del _restraint_option

    @property
    def n_iterations(self):
        """:646-652: the last completely written iteration (capped by ``max_n_iterations``)."""
        last = self._reporter.read_last_iteration(last_checkpoint=False)
        return last if self._max_n_iterations is None else min(last, self._max_n_iterations)

    @property
    def n_replicas(self):
        return int(self._read_energies()[0].shape[0])

    @property
    def n_states(self):
        return int(self._read_energies()[0].shape[1])

    @property
    def kT(self):
        """:684-693: kT of the first stored thermodynamic state, kJ/mol."""
        from .. import constants
        st = self._reporter.read_thermodynamic_states()[0][0]
        return constants.kB * float(st.temperature)

    def read_energies(self):
        """:831-896: (sampled [replica, state, iteration], unsampled, neighborhoods, replica state indices [replica, iteration])."""
        return self._read_energies()

    @staticmethod
    def reformat_energies_for_mbar(u_kln, n_k=None):
        """:993-1040: energies [sampled state k, evaluated state l, sample n] -> the [l, all samples] layout MBAR takes, the first
        ``n_k[k]`` samples of every k laid side by side in the order of k."""
        u_kln = np.asarray(u_kln)
        k, l, n = u_kln.shape
        n_k = np.full(k, n, dtype=np.int64) if n_k is None else np.asarray(n_k, dtype=np.int64)
        return np.concatenate([u_kln[i, :, :n_k[i]] for i in range(k)], axis=1).astype(np.float64) if k else np.zeros([l, 0])

    def clear(self):
        """:596-608 / :1230-1241: forget everything derived from the storage."""
        self._equilibration_data = None
        self._mbar = None
        self._unbiased = None
        self._radially_symmetric_restraint_data = None
        self._restraint_energies, self._restraint_distances = {}, {}
        self._collective_variables = {}
        self._parameter_derivatives = None
        self._release_energy_store()

    def _release_energy_store(self):
        store, self._energy_store = getattr(self, '_energy_store', None), None
        if store is not None:
            store.close()

    def __del__(self):
        try:
            self._release_energy_store()
        except Exception:
            pass

    @property
    def _assembles_on_device(self):
        return self._kwargs.get('assembly_solver', 'numpy') == 'device'

    def _device_energy_store(self):
        """The stored energies and state indices on the device (include/remd_hip_energy_store.h): uploaded on first use from the
        records ``_read_energies`` serves, in the reporter's own [iteration][replica][state] layout, and kept until ``clear()``."""
        if self._energy_store is None:
            from .._engine import DeviceEnergyStore
            e, eu, _, states = self._read_records()
            self._energy_store = DeviceEnergyStore(e, eu, states, device=self._kwargs.get('device', 0), lib_path=self._kwargs.get('lib_path'))
        return self._energy_store

    @property
    def effective_length(self):
        """:2207-2221: number of uncorrelated production samples."""
        e, _, _, states = self._read_energies()
        return self._get_equilibration_data(e, states)[2]

    def show_mixing_statistics(self, cutoff=0.05, number_equilibrated=None):
        """:1305-1351: log the state-to-state transition matrix (entries below ``cutoff`` blank) and what its second
        eigenvalue says about the equilibration of the state walk; returns the text."""
        import logging
        stats = self.generate_mixing_statistics(number_equilibrated=number_equilibrated)
        t_ij, mu = stats.transition_matrix, stats.eigenvalues
        n = t_ij.shape[0]
        lines = ['Cumulative symmetrized state mixing transition matrix:', '%6s' % '' + ''.join('%6d' % j for j in range(n))]
        for i in range(n):
            lines.append('%-6d' % i + ''.join(('%6.3f' % p) if p >= cutoff else '%6s' % '' for p in t_ij[i]))
        if mu[1] >= 1:
            lines.append('Perron eigenvalue is unity; Markov chain is decomposable.')
        elif mu[1] <= 0:
            lines.append('Perron eigenvalue is %9.5f; state equilibration timescale is less than one iteration.' % mu[1].real)
        else:
            lines.append('Perron eigenvalue is %9.5f; state equilibration timescale is ~ %.1f iterations' % (mu[1].real, 1.0 / (1.0 - mu[1].real)))
        text = '\n'.join(lines)
        logging.getLogger(__name__).info(text)
        return text

    def _combine(self, other, operator):
        mine = dict(phases=[self], names=[generate_phase_name(self.name, [])], signs=[self._sign])
        self._sign = '+'
        return MultiPhaseAnalyzer(mine)._combine_phases(other, operator)

    def __add__(self, other):
        return self._combine(other, '+')

    def __sub__(self, other):
        return self._combine(other, '-')

    def __neg__(self):
        self._sign = '-' if self._sign == '+' else '+'           # :1128-1134
        return self

    def _read_records(self):
        """(sampled [iteration, replica, state], unsampled, neighborhoods, replica state indices [iteration, replica]): the
        reporter's records up to the last good iteration and ``max_n_iterations``."""
        e, nb, eu = self._reporter.read_energies()
        states = self._reporter.read_replica_thermodynamic_states()
        # records beyond the last completely written iteration are stale (a resume from an earlier checkpoint leaves the
        # abandoned branch's records behind): the reference caps at the last good iteration (multistateanalyzer.py:1353-1412)
        last = self._reporter.read_last_iteration(last_checkpoint=False)
        n = e.shape[0] if last is None else min(e.shape[0], int(last) + 1)
        if self._max_n_iterations is not None:
            n = min(n, self._max_n_iterations + 1)
        return e[:n], eu[:n], nb[:n], states[:n]

    def _read_energies(self):
        """[replica, state, iteration] arrays like the reference's ``_read_energies`` (:1353-1412)."""
        return tuple(np.moveaxis(a, 0, -1) for a in self._read_records())

    @property
    def has_log_weights(self):
        """True when the storage holds per-iteration logZ / log_weights (SAMS), :898-909."""
        try:
            self._reporter.read_online_analysis_data(0, 'logZ', 'log_weights')
            return True
        except (ValueError, IndexError, KeyError):
            return False

    def get_effective_energy_timeseries(self, energies, replica_state_indices):
        """u_n[iteration] = sum over replicas of the reduced potential in the state the replica occupies (:1462-1472);
        with SAMS weights, the expanded-ensemble correction -sum log_w[state] + logsumexp(-f + log_w) per iteration
        (:1446-1470, f = the last online logZ estimate)."""
        n_replicas, _, n_iterations = energies.shape
        u_n = np.zeros([n_iterations], np.float64)
        rep = np.arange(n_replicas)
        log_weights = f_l = None
        if self.has_log_weights:
            lw = self._reporter._files['log_weights'].read()          # [iteration, state]
            if lw.shape[0] >= n_iterations:
                log_weights = lw[:n_iterations].T
                f_l = -self._reporter.read_online_analysis_data(None, 'logZ')['logZ']
        if self._assembles_on_device:
            store = self._device_energy_store()
            if energies.shape != (store.R, store.S, store.T) or replica_state_indices.shape != (store.R, store.T):
                raise ValueError("assembly_solver='device' answers from the stored energies: pass what _read_energies() returns")
            return store.effective_energy(None if log_weights is None else log_weights.T, f_l)
        for it in range(n_iterations):
            states = replica_state_indices[:, it]
            u_n[it] = np.sum(energies[rep, states, it])
            if log_weights is not None:
                u_n[it] += -np.sum(log_weights[states, it]) + _logsumexp(-f_l + log_weights[:, it])
        return u_n

    def _get_equilibration_data(self, energies=None, replica_state_indices=None):
        """(n_equilibration_iterations, statistical_inefficiency, n_effective_max), :2026-2088."""
        if energies is None:
            energies, _, _, replica_state_indices = self._read_energies()
        if self._n_equilibration_iterations is not None and self._statistical_inefficiency is not None:
            n_eq, g_t = self._n_equilibration_iterations, self._statistical_inefficiency
            n_eff = (energies.shape[-1] - 1 - n_eq + 1) / g_t
        else:
            u_n = self.get_effective_energy_timeseries(energies, replica_state_indices)
            t0 = self._n_equilibration_iterations if self._n_equilibration_iterations is not None else 1   # drop iteration 0
            t0_sams = self._sams_t0()                                     # :2068-2076: only the asymptotically optimal SAMS stage
            if t0_sams is not None:
                t0 = max(t0, t0_sams)
            i_t, g_i, n_effective_i = get_equilibration_data_per_sample(
                u_n[t0:], max_subset=self._max_subset, solver=self._kwargs.get('timeseries_solver', 'numpy'),
                device=self._kwargs.get('device', 0), lib_path=self._kwargs.get('lib_path'))
            n_eff = n_effective_i.max()
            i_max = n_effective_i.argmax()
            n_eq = int(i_t[i_max] + t0)
            g_t = self._statistical_inefficiency if self._statistical_inefficiency is not None else float(g_i[i_max])
        self._equilibration_data = (n_eq, g_t, n_eff)
        return self._equilibration_data

    def _sams_t0(self):
        """Start of SAMS' second stage when the storage records one (written with the online data at checkpoints)."""
        try:
            last = self._reporter.read_last_iteration(last_checkpoint=True)
            data = self._reporter.read_online_data_if_present(last) if last is not None else None
            st = (data or {}).get('sams_state')
            return int(st['t0']) if st and st.get('stage', 0) == 1 and st.get('t0', 0) > 0 else None
        except Exception:
            return None

    @property
    def n_equilibration_iterations(self):
        return (self._equilibration_data or self._get_equilibration_data())[0]

    @property
    def statistical_inefficiency(self):
        return (self._equilibration_data or self._get_equilibration_data())[1]

    def _decorrelated_selection(self):
        """(sampled energies, unsampled energies, replica state indices, iterations): the equilibrated, decorrelated iterations."""
        e, eu, nb, states = self._read_energies()
        n_eq, g_t, _ = self._get_equilibration_data(e, states)
        iterations = np.arange(e.shape[-1])
        if not self.use_full_trajectory:
            iterations = iterations[n_eq:]
            iterations = iterations[subsample_correlated_data(np.zeros(iterations.size), g=g_t)]
        return e[..., iterations], eu[..., iterations], states[..., iterations], iterations

    def _compute_mbar_decorrelated_energies(self, selection=None):
        """(u_ln, N_l) with the unsampled states at the two end points (:1479-1545)."""
        e, eu, states, iterations = selection or self._decorrelated_selection()
        if self._assembles_on_device:
            return self._device_energy_store().gather_u_ln(iterations)
        n_replicas, n_sampled, n_it = e.shape
        n_uns = eu.shape[1]
        n_total = n_sampled + n_uns
        first = int(n_uns / 2.0)
        last = n_total - first
        u_ln = np.zeros([n_total, n_it * n_replicas])
        N_l = np.zeros([n_total], dtype=int)
        u_ln[first:last, :] = np.concatenate([e[k] for k in range(n_replicas)], axis=1)      # kln' -> ln (:1027-1034)
        uniq, counts = np.unique(states, return_counts=True)
        N_l[first:last][uniq] = counts
        if n_uns > 0:
            u_ln[[0, -1], :] = np.concatenate([eu[k] for k in range(n_replicas)], axis=1)
        return u_ln, N_l

    # ---- unbiasing a radially symmetric restraint (:1355-1408, :1556-1913) ----------------------------------------
    def _get_radially_symmetric_restraint_data(self):
        """(restraint force of the first end state's System, masses of its group 1, masses of its group 2), :1355-1408.
        forces.NoForceFoundError without such a force (MultipleForcesError with several), TypeError when an end state has it off."""
        from .. import forces
        if self._radially_symmetric_restraint_data is not None:
            return self._radially_symmetric_restraint_data
        end_states = self._reporter.read_end_thermodynamic_states()
        system = end_states[0].system
        _, restraint_force = forces.find_forces(system, forces.RadiallySymmetricRestraintForce, only_one=True, include_subclasses=True)
        default = restraint_force.getGlobalParameterDefaultValue(1)         # (a state that does not control the parameter leaves it there)
        if getattr(end_states[0], 'lambda_restraints', default) != 1.0 or getattr(end_states[-1], 'lambda_restraints', default) != 1.0:
            raise TypeError('Cannot unbias a restraint that is turned off at one of the end states.')
        masses = np.asarray(system.masses, dtype=np.float64)
        self._radially_symmetric_restraint_data = (restraint_force, [float(masses[i]) for i in restraint_force.restrained_atom_indices1],
                                                   [float(masses[i]) for i in restraint_force.restrained_atom_indices2])
        return self._radially_symmetric_restraint_data

    def _evaluate_restraint_frames(self, desc, pos, box):
        """(energy [F], distance [F]) by the solver analysis_kwargs['restraint_solver'] names."""
        if self._kwargs.get('restraint_solver', 'numpy') == 'device':
            from .._engine import restraint_frames
            return restraint_frames(desc, pos, box, None, device=self._kwargs.get('device', 0), lib_path=self._kwargs.get('lib_path'))
        return restraint_frames_numpy(desc, pos, box)

    def _compute_restraint_energies(self, restraint_force, weights_group1, weights_group2, iterations=None):
        """(energies [n_replicas * n_iterations] kJ/mol, distances [...] nm) of the restraint at the decorrelated iterations, frame =
        replica * n_iterations + iteration index: the column order of _compute_mbar_decorrelated_energies (:1668-1825).  Iterations
        evaluated before are served from the cache; the others are read in bulk and evaluated in ONE call."""
        from .. import forces
        if iterations is None:
            iterations = self._decorrelated_selection()[3]
        iterations = [int(i) for i in iterations]
        todo = [i for i in iterations if i not in self._restraint_energies or i not in self._restraint_distances]
        if todo:
            analysis_indices = [int(i) for i in self._reporter.analysis_particle_indices]
            where = {a: k for k, a in enumerate(analysis_indices)}
            groups = (restraint_force.restrained_atom_indices1, restraint_force.restrained_atom_indices2)
            mass_of = dict(zip(list(groups[0]) + list(groups[1]), list(weights_group1) + list(weights_group2)))
            desc = forces.restraint_terms(restraint_force, mass_of)         # (a group without weights of its own: the masses)
            for g in (1, 2):
                atoms = [int(a) for a in groups[g - 1]]
                for a in atoms:
                    if a not in where:
                        raise ValueError('restrained atom %d is not one of the analysis particles of the store: create the reporter '
                                         'with analysis_particle_indices that include every restrained atom' % a)
                desc['atoms%d' % g] = np.array([where[a] for a in atoms], dtype=np.int32)
            x, box = self._reporter.read_analysis_positions(todo)            # [n_it][R][n_analysis][3], [n_it][R][3]
            n_it, R = x.shape[0], x.shape[1]
            pos = np.ascontiguousarray(x.transpose(1, 0, 2, 3)).reshape(R * n_it, x.shape[2], 3)
            if desc['periodic'] and box is None:
                raise ValueError('the restraint is periodic but the store holds no box vectors of the analysis particles')
            box = None if box is None else np.ascontiguousarray(box.transpose(1, 0, 2)).reshape(R * n_it, 3)
            energy, distance = self._evaluate_restraint_frames(desc, pos, box)
            energy, distance = np.asarray(energy).reshape(R, n_it), np.asarray(distance).reshape(R, n_it)
            for k, it in enumerate(todo):
                self._restraint_energies[it], self._restraint_distances[it] = energy[:, k].copy(), distance[:, k].copy()
        if not iterations:
            return np.zeros(0), np.zeros(0)
        return (np.stack([self._restraint_energies[i] for i in iterations], axis=1).reshape(-1),
                np.stack([self._restraint_distances[i] for i in iterations], axis=1).reshape(-1))

    def _get_use_restraint_cutoff(self):
        """(apply an energy cutoff, apply a distance cutoff), :1827-1836: a number applies; both 'auto': the distance cutoff alone."""
        is_number = lambda v: v is not None and not isinstance(v, str)
        apply_distance_cutoff = is_number(self.restraint_distance_cutoff)
        apply_energy_cutoff = is_number(self.restraint_energy_cutoff)
        if self.restraint_distance_cutoff == 'auto' and not apply_energy_cutoff:
            apply_distance_cutoff = True
        elif self.restraint_energy_cutoff == 'auto' and self.restraint_distance_cutoff is None:
            apply_energy_cutoff = True
        return apply_energy_cutoff, apply_distance_cutoff

    def _determine_automatic_restraint_cutoff(self, compute_energy_cutoff=True, compute_distance_cutoff=True):
        """:1838-1892: the 99.9th percentile of the restraint energies (kT) / distances (nm) over the evaluated frames whose replica was
        in state 0, the bound state."""
        replica_state_indices = self._reporter.read_replica_thermodynamic_states()
        out = []
        for wanted, cached, scale, what in ((compute_energy_cutoff, self._restraint_energies, 1.0 / self.kT, 'energy'),
                                            (compute_distance_cutoff, self._restraint_distances, 1.0, 'distance')):
            if not wanted:
                out.append(None)
                continue
            values = [cached[it][r] for it in cached for r in np.flatnonzero(replica_state_indices[it] == 0)]
            if len(values) == 0:
                raise InsufficientData('Thermodynamic state 0 has not been sampled enough to determine automatically the restraint '
                                       '%s cutoff.' % what)
            out.append(float(np.percentile(np.array(values) * scale, 99.9)))
        return tuple(out)

    def _get_restraint_cutoffs(self):
        """(energy cutoff in kT or None, distance cutoff in nm or None), :1894-1913."""
        from ..unit import to_md
        apply_energy_cutoff, apply_distance_cutoff = self._get_use_restraint_cutoff()
        if apply_distance_cutoff and self.restraint_distance_cutoff == 'auto':
            distance_cutoff = self._determine_automatic_restraint_cutoff(compute_energy_cutoff=False)[1]
        elif self.restraint_distance_cutoff == 'auto':
            distance_cutoff = None
        else:
            distance_cutoff = None if self.restraint_distance_cutoff is None else float(to_md(self.restraint_distance_cutoff))
        if apply_energy_cutoff and self.restraint_energy_cutoff == 'auto':
            energy_cutoff = self._determine_automatic_restraint_cutoff(compute_distance_cutoff=False)[0]
        elif self.restraint_energy_cutoff == 'auto':
            energy_cutoff = None
        else:
            energy_cutoff = None if self.restraint_energy_cutoff is None else float(self.restraint_energy_cutoff)
        return energy_cutoff, distance_cutoff

    def _compute_mbar_unbiased_energies(self):
        """(u_ln, N_l) with the restraint unbiased (:1556-1666): frames outside a cutoff dropped, two end states without the restraint
        added.  Without a restraint to unbias, exactly what _compute_mbar_decorrelated_energies returns."""
        from .. import forces
        self._unbiased = None
        selection = self._decorrelated_selection()
        u_ln, N_l = self._compute_mbar_decorrelated_energies(selection)
        # the column of frame [replica][iteration] was drawn from the sampled state the replica was in, past the unsampled rows in front
        self._sample_states = selection[2].reshape(-1) + int((len(N_l) - selection[0].shape[1]) / 2)
        self._sample_columns = (selection[3], None)         # the iterations of the columns, and which columns were kept (None: all)
        initial_f_k = self._kwargs.get('initial_f_k')
        restraint_data = None
        if self.unbias_restraint:
            try:
                restraint_data = self._get_radially_symmetric_restraint_data()
            except (TypeError, forces.NoForceFoundError):
                restraint_data = None                   # nothing to unbias
        if restraint_data is None:
            self._unbiased = (u_ln, N_l, initial_f_k)
            return u_ln, N_l
        e, _, states, iterations = selection
        energies_ln, distances_ln = self._compute_restraint_energies(*restraint_data, iterations=iterations)
        energies_kJ, energies_ln = energies_ln, energies_ln / self.kT           # (kT of the first state: what the energy cutoff is in)
        state_indices_ln = states.reshape(-1)                                 # [replica][iteration] -> frame
        assert len(energies_ln) == u_ln.shape[1] == len(state_indices_ln)
        energy_cutoff, distance_cutoff = self._get_restraint_cutoffs()
        n_states = e.shape[1]
        first_sampled_state_idx = int((len(u_ln) - n_states) / 2)
        drop = np.zeros(len(energies_ln), dtype=bool)
        if energy_cutoff is not None:
            drop |= energies_ln > energy_cutoff
        if distance_cutoff is not None:
            drop |= distances_ln > distance_cutoff
        N_l = N_l.copy()
        np.subtract.at(N_l, state_indices_ln[drop] + first_sampled_state_idx, 1)
        keep = np.flatnonzero(~drop)
        u_ln, energies_kJ = u_ln[:, keep], energies_kJ[keep]
        self._sample_states = self._sample_states[keep] + 1                  # (the kept columns, past the end row added in front)
        self._sample_columns = (iterations, keep)
        u_ln_new = np.zeros((u_ln.shape[0] + 2, u_ln.shape[1]), u_ln.dtype)
        N_l_new = np.zeros(len(N_l) + 2, N_l.dtype)
        # each end row loses the restraint in the kT of ITS OWN end state.  The reference divides both by the first state's kT
        # (:1603, 1647-1648), the same number whenever all states share one temperature -- the only case in which it is right
        from .. import constants
        end_states = self._reporter.read_end_thermodynamic_states()
        u_ln_new[0, :] = u_ln[0] - energies_kJ / (constants.kB * float(end_states[0].temperature))
        u_ln_new[-1, :] = u_ln[-1] - energies_kJ / (constants.kB * float(end_states[-1].temperature))
        u_ln_new[1:-1, :] = u_ln
        N_l_new[1:-1] = N_l
        if initial_f_k is not None and len(initial_f_k) == len(N_l):
            initial_f_k = np.concatenate([[0.0], np.asarray(initial_f_k, dtype=np.float64), [0.0]])
        self._unbiased = (u_ln_new, N_l_new, initial_f_k)
        return u_ln_new, N_l_new

    @property
    def mbar(self):
        if self._mbar is None:
            u_ln, N_l = self._compute_mbar_unbiased_energies()
            extra = {k: self._kwargs[k] for k in ('solver', 'device', 'lib_path') if k in self._kwargs}
            if self.n_bootstraps:
                extra.update(n_bootstraps=int(self.n_bootstraps), bootstrap_seed=int(self.bootstrap_seed), sample_states=self._sample_states)
            self._mbar = MBAR(u_ln, N_l, initial_f_k=self._unbiased[2], **extra)
        return self._mbar

    MixingStatistics = collections.namedtuple('MixingStatistics', ['transition_matrix', 'eigenvalues', 'statistical_inefficiency'])

    def generate_mixing_statistics(self, number_equilibrated=None):
        """(transition_matrix, eigenvalues sorted from greatest to least, statistical inefficiency of the replicas' state
        indices) from the stored state trajectory (:1243-1303; symmetrised empirical transition counts)."""
        if number_equilibrated is None:
            number_equilibrated = self.n_equilibration_iterations
        states = self._reporter.read_replica_thermodynamic_states()
        if self._max_n_iterations is not None:
            states = states[:self._max_n_iterations + 1]
        n_iter, n_replicas = states.shape
        n_states = int(self._reporter._meta['n_states'])
        if self._assembles_on_device:
            store = self._device_energy_store()
            if (n_iter, n_replicas, n_states) != (store.T, store.R, store.S):
                raise ValueError("assembly_solver='device': the stored state indices are [%d][%d] over %d states, the energies on the "
                                 'device [%d][%d] over %d' % (n_iter, n_replicas, n_states, store.T, store.R, store.S))
            n_ij = store.transition_counts(min(max(int(number_equilibrated), 0), n_iter), n_iter)
        else:
            n_ij = np.zeros([n_states, n_states], np.int64)
            for it in range(number_equilibrated, n_iter - 1):
                np.add.at(n_ij, (states[it], states[it + 1]), 1)
        t_ij = np.zeros([n_states, n_states], np.float64)
        for i in range(n_states):
            den = float(n_ij[i, :].sum() + n_ij[:, i].sum())
            if den > 0:
                t_ij[i, :] = (n_ij[i, :] + n_ij[:, i]) / den
            else:
                t_ij[i, i] = 1.0
        mu = -np.sort(-np.linalg.eigvals(t_ij))
        if self._assembles_on_device:
            g = statistical_inefficiency_multiple(np.transpose(states[number_equilibrated:]), solver='device',
                                                  device=self._kwargs.get('device', 0), lib_path=self._kwargs.get('lib_path'))
        else:
            g = statistical_inefficiency_multiple(np.transpose(states[number_equilibrated:]))
        return self.MixingStatistics(transition_matrix=t_ij, eigenvalues=mu, statistical_inefficiency=g)

    def get_enthalpy(self):
        """(Delta_u_ij, dDelta_u_ij) of the reduced enthalpy <u_i>_i, :1988-2005."""
        r = self.mbar.compute_entropy_and_enthalpy()
        return r['Delta_u'], r['dDelta_u']

    def get_entropy(self):
        """(Delta_s_ij, dDelta_s_ij) of the reduced entropy s_i = <u_i>_i - f_i, :2007-2024."""
        r = self.mbar.compute_entropy_and_enthalpy()
        return r['Delta_s'], r['dDelta_s']

    def get_free_energy(self):
        """(Delta_f_ij, dDelta_f_ij) in kT between all (unsampled + sampled) states (:1958-2003)."""
        if self.uncertainty_method is None:
            return self.mbar.compute_free_energy_differences()
        return self.mbar.compute_free_energy_differences(uncertainty_method=self.uncertainty_method)

    def get_collective_variables(self, cvs, solver=None):
        """values [n_iterations + 1][n_replicas][n_cv] f64 (nm, rad) of the collective variables ``cvs`` (DistanceCV, AngleCV,
        DihedralCV, RMSDCV; atom indices in System numbering) of every replica at every stored iteration: the ``values`` of ``get_pmf``.
        A single descriptor given bare returns [n_iterations + 1][n_replicas].  The frames are the analysis particles of the store,
        read in bulk and evaluated in ONE call by ``frame_cvs_numpy`` or on the device (``analysis_kwargs={'cv_solver': 'device'}``, or
        ``solver`` for this call: csrc/frame_cvs.hip); the masses are those of the first thermodynamic state's System.  A periodic
        variable takes minimum images under each frame's own stored box; in a store that is not periodic it takes none.  Values are
        kept per tuple of descriptors until ``clear()``."""
        bare = isinstance(cvs, (_CentroidCV, RMSDCV))
        cvs = [cvs] if bare else list(cvs)
        if solver is None:
            solver = self.cv_solver
        else:
            self._check_cv_solver(solver, what='solver')
        for v, cv in enumerate(cvs):
            if not isinstance(cv, (_CentroidCV, RMSDCV)):
                raise ValueError('variable %d is %r, not a DistanceCV, AngleCV, DihedralCV or RMSDCV' % (v, cv))
        if not cvs:
            raise ValueError('no collective variable was given')
        key = (solver,) + tuple(cv._key() for cv in cvs)
        if key not in self._collective_variables:
            n_it, n_replicas = self.n_iterations + 1, self.n_replicas      # (what get_pmf asks of its values)
            system = self._reporter.read_thermodynamic_states()[0][0].system
            masses = np.asarray(system.masses, dtype=np.float64)
            analysis_indices = [int(i) for i in self._reporter.analysis_particle_indices]
            where = {a: k for k, a in enumerate(analysis_indices)}
            for v, cv in enumerate(cvs):
                for a in cv._atoms():
                    if a >= len(masses):
                        raise ValueError('variable %d (%s): atom %d is outside the %d particles of the System' % (v, type(cv).__name__, a, len(masses)))
                    if a not in where:
                        raise ValueError('variable %d (%s): atom %d is not one of the analysis particles of the store: create the reporter '
                                         'with analysis_particle_indices that include every atom of the variable' % (v, type(cv).__name__, a))
            mapped = [cv._remapped(where, len(masses)) for cv in cvs]
            x, box = self._reporter.read_analysis_positions(range(n_it))     # [n_it][R][n_analysis][3], [n_it][R][3] or None
            if x.shape[1] != n_replicas:
                raise ValueError('the store holds the analysis particles of %d replicas but the energies of %d' % (x.shape[1], n_replicas))
            if box is None and any(cv.periodic for cv in mapped):
                try:
                    store_is_periodic = bool(self._reporter.is_periodic)
                except (TypeError, IndexError, KeyError):                     # (no checkpoint to ask: the analysis store holds no box)
                    store_is_periodic = False
                for v, cv in enumerate(mapped):
                    if cv.periodic and store_is_periodic:
                        raise ValueError('variable %d (%s) is periodic but the store holds no box vectors of the analysis particles: '
                                         'give periodic=False' % (v, type(cv).__name__))
                mapped = [cv._not_periodic() for cv in mapped]
            pos = x.reshape(n_it * n_replicas, x.shape[2], 3)
            box = None if box is None else box.reshape(n_it * n_replicas, 3)
            m = masses[analysis_indices]
            if solver == 'device':
                from .._engine import frame_cvs
                values = frame_cvs(mapped, pos, box, m, device=self._kwargs.get('device', 0), lib_path=self._kwargs.get('lib_path'))
            else:
                values = frame_cvs_numpy(mapped, pos, box, m)
            self._collective_variables[key] = np.asarray(values).reshape(n_it, n_replicas, len(cvs))
        values = self._collective_variables[key]
        return values[:, :, 0].copy() if bare else values.copy()

    def get_pmf(self, values, edges, state=0, uncertainties='from-lowest', pmf_reference=None):
        """(f_i, df_i, n_i) in kT: the free energy surface at sampled state ``state`` along the coordinate ``values``
        [n_iterations + 1][n_replicas] (or [...][D], D <= 3), the coordinate of every replica at every stored iteration, binned by
        ``edges`` (``bin_samples``).  The columns are those MBAR was given: the same equilibration cut and decorrelated selection, in
        the same order, less the frames a restraint cutoff dropped.  Errors by the analyzer's ``uncertainty_method``."""
        n_it, n_replicas, n_states = self.n_iterations + 1, self.n_replicas, self.n_states
        v = np.asarray(values, dtype=np.float64)
        if v.ndim not in (2, 3) or v.shape[:2] != (n_it, n_replicas):
            raise ValueError('values must be [n_iterations + 1][n_replicas] = [%d][%d], or that with a last axis of D <= 3 coordinates, '
                             'not an array of shape %r' % (n_it, n_replicas, v.shape))
        if isinstance(state, bool) or not isinstance(state, (int, np.integer)) or not 0 <= state < n_states:
            raise ValueError('state must be the index of a sampled state in 0 ... %d, not %r' % (n_states - 1, state))
        mbar = self.mbar
        iterations, keep = self._sample_columns
        v = np.swapaxes(v[iterations], 0, 1)                                  # [replica][iteration]: the order of the columns of u_ln
        v = v.reshape((-1,) + v.shape[2:])
        if keep is not None:
            v = v[keep]
        bin_n, nbins = bin_samples(v, edges)
        u_n = mbar.u_kn[int((mbar.K - n_states) / 2) + int(state)]
        r = mbar.compute_pmf(u_n, bin_n, nbins, uncertainties=uncertainties, pmf_reference=pmf_reference,
                             uncertainty_method=self.uncertainty_method)
        return r['f_i'], r['df_i'], r['n_i']

    # ---- thermodynamic integration over the stored energy parameter derivatives ----------------------------------------------
    def get_parameter_derivatives(self):
        """(names, dudl): the global parameters whose derivatives the store holds (a run with ``store_parameter_derivatives=True``)
        and dudl [n_iterations + 1][n_replicas][n_states][n], the REDUCED derivative beta_l dE/dparameter_d (no units, per unit of
        the parameter) of every replica's configuration under the globals of every sampled state l.  Kept until ``clear()``."""
        if self._parameter_derivatives is None:
            from .. import constants
            names = list(self._reporter.read_parameter_derivative_names())
            d = np.asarray(self._reporter.read_parameter_derivatives(), dtype=np.float64)[:self.n_iterations + 1]
            beta = np.array([1.0 / (constants.kB * float(s.temperature)) for s in self._reporter.read_thermodynamic_states()[0]])
            self._parameter_derivatives = (names, d * beta[None, None, :, None])
        names, dudl = self._parameter_derivatives
        return list(names), dudl.copy()

    @staticmethod
    def _state_parameters(state):
        """{name: value} of everything the composable states of ``state`` control (global parameters, alchemical lambdas)"""
        from ..states import AlchemicalState
        out = {}
        for g in getattr(state, '_globals', ()):
            for name in g._parameters:
                out[name] = g._get_global_parameter_value(name)
        for c in getattr(state, '_alchs', ()):
            sfx = c.parameters_name_suffix
            for p in AlchemicalState._PARAMETERS:
                out[p if sfx is None else p + '_' + sfx] = getattr(c, p)
        return out

    def get_thermodynamic_integration(self, estimator='mbar'):
        """Thermodynamic integration along the sampled states in index order: a dict with ``names`` [n] (the declared parameters),
        ``lambdas`` [K][n] (their values at every state), ``mean`` and ``sigma`` [K][n] (<du/dlambda_d> at state k, reduced, and its
        uncertainty), ``Delta_f`` and ``dDelta_f`` [K][K] in kT, the trapezoid rule over the path

            Delta_f[i][j] = sum_{k=i}^{j-1} 1/2 sum_d (mean[k][d] + mean[k+1][d]) (lambda[k+1][d] - lambda[k][d])       (antisymmetric)

        an estimate of ``get_free_energy()`` that does not share MBAR's route to it.  Both estimators work on the columns handed to
        MBAR (the same equilibration cut and decorrelated iterations): ``'samples'`` averages du/dlambda at state k over the samples
        drawn AT state k; ``'mbar'`` takes <du/dlambda>_k from all samples, reweighted (``mbar.compute_expectations(...,
        state_dependent=True)``, so with the analyzer's MBAR solver).

        Uncertainty: for a pair (i, j) every state k on the path carries ONE observable B_k = sum_d w_kd du/dlambda_d with its
        trapezoid weight w_kd (half the adjacent step at the ends, half the sum of both inside), and dDelta_f[i][j]^2 = sum_k
        sigma^2(B_k), sigma the standard error of the mean ('samples'; NaN for a state with fewer than two samples) or
        compute_expectations' sigma ('mbar').  The states are treated as independent (alchemlyb's convention for TI): for 'mbar'
        this NEGLECTS the correlation between the states' estimates, which all come from the same samples.

        ValueError: fewer than two states; states that differ in temperature, pressure or in any parameter that is not one of the
        stored derivative columns (a built-in alchemical lambda, a global no force declared) -- the integrand along that
        parameter is not in the store."""
        if estimator not in ('mbar', 'samples'):
            raise ValueError("estimator must be 'mbar' or 'samples', not %r" % (estimator,))
        names, dudl = self.get_parameter_derivatives()
        states = self._reporter.read_thermodynamic_states()[0]
        K, n = len(states), len(names)
        if K < 2:
            raise ValueError('thermodynamic integration needs at least 2 states, the store holds %d' % K)
        for what in ('temperature', 'pressure'):
            values = [getattr(s, what) for s in states]
            if any(v != values[0] for v in values):
                raise ValueError('thermodynamic integration over states that differ in %s (%s): the stored derivatives cover the '
                                 'declared parameters %s only' % (what, values, names))
        parameters = [self._state_parameters(s) for s in states]
        for p in sorted(set().union(*parameters)):
            values = [q.get(p) for q in parameters]
            if p not in names and any(v != values[0] for v in values):
                raise ValueError('thermodynamic integration: the states differ in %s (%s), which is not one of the stored energy parameter '
                                 'derivatives %s (addEnergyParameterDerivative on a custom force that carries it)' % (p, values, names))
        from ..custom_expr import custom_globals
        lambdas = custom_globals(states[0].system, names, states)                 # [K][n]
        step = np.diff(lambdas, axis=0)                                            # [K - 1][n]
        # the trapezoid weights of state k: what it takes from the step on its left, on its right, and from both
        left, right = np.zeros((K, n)), np.zeros((K, n))
        left[1:], right[:-1] = 0.5 * step, 0.5 * step
        mbar = self.mbar
        iterations, keep = self._sample_columns
        first = int((mbar.K - K) / 2)
        A = np.swapaxes(dudl[iterations], 0, 1).reshape(-1, K, n)                 # [replica][iteration] -> column, as in get_pmf
        if keep is not None:
            A = A[keep]
        A = np.ascontiguousarray(np.moveaxis(A, 0, -1))                           # [K][n][N]
        B = [np.einsum('kd,kdn->kn', w, A) for w in (left, right, left + right)]   # [3][K][N]
        mean, sigma, sB = np.zeros((K, n)), np.zeros((K, n)), np.zeros((3, K))
        if estimator == 'mbar':
            def expectation(a_kn):
                rows = np.zeros((mbar.K, a_kn.shape[1]))
                rows[first:first + K] = a_kn
                r = mbar.compute_expectations(rows, state_dependent=True)
                return r['mu'][first:first + K], r['sigma'][first:first + K]
            for d in range(n):
                mean[:, d], sigma[:, d] = expectation(A[:, d, :])
            for c in range(3):
                sB[c] = expectation(B[c])[1]
        else:
            def sem(x):              # standard error of the mean over the last axis; a constant observable has exactly 0, as in MBAR
                m = x.shape[-1]
                if m < 2:
                    return np.full(x.shape[:-1], np.nan)
                return np.where(x.max(axis=-1) == x.min(axis=-1), 0.0, np.std(x, axis=-1, ddof=1) / np.sqrt(m))
            drawn = np.asarray(self._sample_states) - first
            for k in range(K):
                at = np.flatnonzero(drawn == k)
                if at.size == 0:
                    raise ValueError("estimator='samples': no sample was drawn at state %d" % k)
                mean[k], sigma[k] = A[k][:, at].mean(axis=1), sem(A[k][:, at])
                sB[:, k] = [sem(B[c][k, at]) for c in range(3)]
        seg = 0.5 * np.sum((mean[:-1] + mean[1:]) * step, axis=1)                  # [K - 1]
        Delta_f, dDelta_f = np.zeros((K, K)), np.zeros((K, K))
        for i in range(K):
            for j in range(i + 1, K):
                Delta_f[i, j] = seg[i:j].sum()
                Delta_f[j, i] = -Delta_f[i, j]
                dDelta_f[i, j] = dDelta_f[j, i] = np.sqrt(sB[1, i] ** 2 + np.sum(sB[2, i + 1:j] ** 2) + sB[0, j] ** 2)
        return dict(names=names, lambdas=lambdas, mean=mean, sigma=sigma, Delta_f=Delta_f, dDelta_f=dDelta_f)


class ReplicaExchangeAnalyzer(MultiStateSamplerAnalyzer):
    """replicaexchange.py:427-439."""


class ParallelTemperingAnalyzer(ReplicaExchangeAnalyzer):
    """paralleltempering.py:240-252."""


class SAMSAnalyzer(MultiStateSamplerAnalyzer):
    """sams.py:694-704."""


class MultiPhaseAnalyzer:
    """multistateanalyzer.py:2224-2570: several phases combined with signs (``complex - solvent``); an observable of the
    combination is the signed sum of each phase's value between its ``reference_states``, errors added in quadrature (the
    default registry's free_energy / entropy / enthalpy, :304-340)."""

    def __init__(self, phases):
        self._phases, self._names, self._signs = list(phases['phases']), list(phases['names']), list(phases['signs'])
        shared = [o for o in MultiStateSamplerAnalyzer.observables if all(o in getattr(p, 'observables', ()) for p in self._phases)]
        if not shared:
            raise RuntimeError('There are no shared computable observable between the phases, combining them will do nothing.')
        self._observables = tuple(shared)
        for name in shared:
            setattr(self, 'get_' + name, (lambda n: (lambda: self._compute_observable(n)))(name))

    observables = property(lambda self: self._observables)
    phases = property(lambda self: self._phases)
    names = property(lambda self: self._names)
    signs = property(lambda self: self._signs)

    def clear(self):
        for phase in self._phases:
            phase.clear()

    def _combine_phases(self, other, operator='+'):
        phases, names, signs = list(self._phases), list(self._names), list(self._signs)
        flip = lambda sign: '-' if ((operator == '-') != (sign == '-')) else '+'
        if isinstance(other, MultiPhaseAnalyzer):
            for phase, name, sign in zip(other.phases, other.names, other.signs):
                names.append(generate_phase_name(name, [n for n in other.names if n != name] + names))
                signs.append(flip(sign))
                phases.append(phase)
        elif isinstance(other, MultiStateSamplerAnalyzer):
            names.append(generate_phase_name(other.name, names))
            signs.append(flip(other._sign))
            other._sign = '+'
            phases.append(other)
        else:
            raise TypeError("cannot %s 'MultiPhaseAnalyzer' and '%s' objects" % ('add' if operator == '+' else 'subtract', type(other)))
        return MultiPhaseAnalyzer(dict(phases=phases, names=names, signs=signs))

    def __add__(self, other):
        return self._combine_phases(other, '+')

    def __sub__(self, other):
        return self._combine_phases(other, '-')

    def __neg__(self):
        import copy
        out = copy.copy(self)
        out._signs = ['-' if s == '+' else '+' for s in self._signs]
        return out

    def __str__(self):
        return 'MultiPhaseAnalyzer <' + ' '.join('%s%s' % (s, n) for s, n in zip(self._signs, self._names)) + '>'

    def _compute_observable(self, name):
        value, error = 0.0, 0.0
        for phase, sign in zip(self._phases, self._signs):
            v, e = getattr(phase, 'get_' + name)()
            if not isinstance(phase, MultiPhaseAnalyzer):
                i, j = phase.reference_states
                v, e = v[i, j], e[i, j]
            value = value + v if sign == '+' else value - v
            error = (error ** 2 + e ** 2) ** 0.5
        return value, error
