"""The cases of tests/golden/analysis_device_bits.npz: what the analysis extensions (csrc/timeseries.hip, energy_store.hip, mbar.hip)
return on the device, as arrays that are compared to the bit.  tests/golden/make_golden_analysis_device_bits.py recorded the file from
the commit before the extensions got one shared inefficiency pass and one scaffold; tests/test_timeseries_gpu.py and
tests/test_energy_store_gpu.py compute the same dictionaries again and compare.  Every input comes from the seeded generators of the
tests, so the file holds results only: per family ('single', 'several', 'mbar', 'energy_store') one uint64 vector, the arrays of the
family in the order of their sorted names.  A double is stored as its uint64 view (a NaN compares by its bit pattern), status and the
last lag (never negative) as their values."""
import os
import numpy as np
from openmmtools_amd._engine import DeviceMBAR, DeviceTimeseries, DeviceEnergyStore, series_inefficiency_multiple
import timeseries_cases as tc
import energy_store_oracle as eo
import mbar_cases as mc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'analysis_device_bits.npz')
SETTINGS = [(fast, mintime) for fast in (False, True) for mintime in (0, 3)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64)


def _counts(a):
    a = np.atleast_1d(np.asarray(a))
    assert (a >= 0).all()
    return a.astype(np.uint64)


def _single(out, key, A, origins):
    ts = DeviceTimeseries(A)
    for fast, mintime in SETTINGS:
        g, status, last = ts.inefficiency(origins, fast=fast, mintime=mintime)
        k = '%s/fast%d/mintime%d/' % (key, fast, mintime)
        out[k + 'g'], out[k + 'status'], out[k + 'last_lag'] = _bits(g), _counts(status), _counts(last)
    ts.close()


def single_series(chunk):
    """DeviceTimeseries.inefficiency on the series, sizes and origins of tests/test_timeseries_gpu.py"""
    out = {}
    for kind in ('ar05', 'alternating', 'ar05_plus_1e6'):
        for N in (2, 3, 100, chunk - 1, chunk + 1, 3 * chunk + 7):
            _single(out, 'single/%s/%d' % (kind, N), tc.series(kind, N), tc.origins(N, chunk))
    _single(out, 'single/ar099/4000', tc.series('ar099', 4000), [0, 7, 1000])
    _single(out, 'single/constant_suffix', np.concatenate([tc.series('ar05', 100), np.full(100, 2.5)]), [0, 50, 100, 150, 198])
    return out


def _several(out, key, A):
    for fast, mintime in SETTINGS:
        g, status, last = series_inefficiency_multiple(A, fast=fast, mintime=mintime)[:3]
        k = '%s/fast%d/mintime%d/' % (key, fast, mintime)
        out[k + 'g'], out[k + 'status'], out[k + 'last_lag'] = _bits(g), _counts(status), _counts(last)


def several_series(chunk):
    """series_inefficiency_multiple on the sets of tests/test_energy_store_gpu.py"""
    out = {}
    for K in (1, 3, 24):
        for N in (2, 3, 100, chunk + 1):
            _several(out, 'several/%dx%d' % (K, N), eo.series(K, N))
    rng = np.random.default_rng(11)
    _several(out, 'several/ar099_3x4000', np.stack([eo.ar1(4000, 0.99, rng) for _ in range(3)]))
    _several(out, 'several/constant_3x50', np.full((3, 50), 2.5))
    return out


def mbar_and_energy_store():
    """one case per kernel family of mbar.hip (column, row and Gram pass at a fixed unconverged f_k; of the long case the per-sample
    log_den is held through its sum phi and through the two passes that read it) and the effective energy with SAMS weights"""
    out = {}
    for name in ('5x1000_alternating', '3x9001_three_chunks'):
        u_kn, N_k, _ = mc.harmonic_case(*mc.CASES[name])
        f = np.random.default_rng(5).normal(scale=0.7, size=u_kn.shape[0])
        d = DeviceMBAR(u_kn, N_k)
        log_den, phi = d.log_denominator(f)
        k = 'mbar/%s/' % name
        out[k + 'phi'] = _bits(phi)
        if log_den.size <= 1000:
            out[k + 'log_den'] = _bits(log_den)
        out[k + 'self_consistent'], out[k + 'gram'] = _bits(d.self_consistent(f)), _bits(d.gram(f))
        d.close()
    T, R, S = 65, 24, 24
    e, _, st = eo.synthetic_store(T, R, S, 0, 'shared')
    lw, f_l = eo.log_weights_case(T, S)
    store = DeviceEnergyStore(e, None, st)
    out['energy_store/effective_energy_sams_65x24x24'] = _bits(store.effective_energy(lw, f_l))
    store.close()
    return out


def pack(now):
    return np.concatenate([now[k] for k in sorted(now)])


def assert_same_bits(now, family):
    """the arrays of ``now``, all of one family, against the recorded vector of that family"""
    assert all(k.startswith(family + '/') for k in now)
    gold = np.load(GOLDEN)[family]
    vec = pack(now)
    assert vec.dtype == gold.dtype and vec.shape == gold.shape
    at = np.cumsum([0] + [now[k].size for k in sorted(now)])
    differ = [k for k, lo, hi in zip(sorted(now), at, at[1:]) if not np.array_equal(vec[lo:hi], gold[lo:hi])]
    print('%d arrays of %s, %d differ from the recorded bits %s' % (len(now), family, len(differ), differ[:8]))
    assert not differ
