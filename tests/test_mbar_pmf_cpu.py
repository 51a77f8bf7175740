"""MBAR.compute_pmf with the numpy solver, bin_samples and the analyzer's get_pmf: no GPU.  The reference is the class's own dense
route: compute_perturbed_free_energies with one perturbed state per bin, whose row is u_n inside the bin and +inf outside.  Bounds
between the two routes are the project's between its MBAR paths: 1e-10 on free energies, 1e-8 relative on errors."""
import functools
import os
import numpy as np
import pytest
from openmmtools_amd import _engine
from openmmtools_amd.multistate import analysis as an
import oracle
import mbar_cases as mc
import test_unbias_restraint_cpu as ur

CPU_LIB = os.path.join(os.path.dirname(os.path.abspath(oracle.__file__)), '_build', 'libremd_cpu.so')
SEED = 0x5EEDB007C0FFEE
CASES = ['2x65', '5x1000_alternating', '17x1037']
NBINS = [1, 3, 11]
MODES = ['from-lowest', 'from-specified', 'from-normalization', 'all-differences']


@functools.lru_cache(maxsize=None)
def _mbar(name, B=0):
    K, N_k = mc.CASES[name]
    u_kn, N_k, _ = mc.harmonic_case(K, N_k)
    u_kn.setflags(write=False)
    return an.MBAR(u_kn, N_k, n_bootstraps=B, bootstrap_seed=SEED)


@functools.lru_cache(maxsize=None)
def _binned(name, nbins):
    """(u_n, bin_n): the state half way between the first and the last one, and every sample in a bin: a seeded permutation dealt
    round over the bins, so that none is empty"""
    m = _mbar(name)
    bin_n = np.random.default_rng(1000 + nbins).permutation(m.N) % nbins
    u_n = 0.5 * (m.u_kn[0] + m.u_kn[-1])
    u_n.setflags(write=False)
    bin_n.setflags(write=False)
    return u_n, bin_n


def dense_rows(u_n, bin_n, nbins, with_z=False):
    rows = np.where(bin_n[None, :] == np.arange(nbins)[:, None], u_n[None, :], np.inf)
    if with_z:
        rows = np.concatenate([rows, np.where(bin_n >= 0, u_n, np.inf)[None, :]], axis=0)
    return rows


def close_errors(a, b):
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a)
    assert np.all(np.abs(a[ok] - b[ok]) <= 1e-8 * np.abs(b[ok]) + 1e-13), np.max(np.abs(a[ok] - b[ok]))


# ---- against the dense path --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nbins', NBINS)
@pytest.mark.parametrize('name', CASES)
def test_all_differences_are_the_dense_paths(name, nbins):
    m = _mbar(name)
    u_n, bin_n = _binned(name, nbins)
    r = m.compute_pmf(u_n, bin_n, nbins, uncertainties='all-differences')
    dense = m.compute_perturbed_free_energies(dense_rows(u_n, bin_n, nbins))
    f = r['f_i']
    assert f.shape == (nbins,) and r['df_i'].shape == (nbins, nbins) and f.min() == 0.0
    assert np.max(np.abs((f[None, :] - f[:, None]) - dense['Delta_f'])) <= 1e-10
    close_errors(r['df_i'], dense['dDelta_f'])
    assert np.array_equal(r['n_i'], np.bincount(bin_n, minlength=nbins))


@pytest.mark.parametrize('nbins', NBINS)
@pytest.mark.parametrize('name', CASES)
def test_bootstrap_errors_are_the_dense_paths(name, nbins):
    m = _mbar(name, 8)
    u_n, bin_n = _binned(name, nbins)
    r = m.compute_pmf(u_n, bin_n, nbins, uncertainties='all-differences', uncertainty_method='bootstrap')
    dense = m.compute_perturbed_free_energies(dense_rows(u_n, bin_n, nbins), uncertainty_method='bootstrap')   # (refuses an empty replicate)
    f = r['f_i']
    assert np.max(np.abs((f[None, :] - f[:, None]) - dense['Delta_f'])) <= 1e-10
    close_errors(r['df_i'], dense['dDelta_f'])
    if nbins > 1:
        assert np.all(r['df_i'][~np.eye(nbins, dtype=bool)] > 0.0)


# ---- mode algebra --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('method', [None, 'bootstrap'])
@pytest.mark.parametrize('name, nbins', [('2x65', 3), ('17x1037', 11)])
def test_modes_are_rows_of_all_differences(name, nbins, method):
    m = _mbar(name, 8)
    u_n, bin_n = _binned(name, nbins)
    full = m.compute_pmf(u_n, bin_n, nbins, uncertainties='all-differences', uncertainty_method=method)
    low = m.compute_pmf(u_n, bin_n, nbins, uncertainty_method=method)
    j = int(np.argmin(full['f_i']))
    assert np.array_equal(low['f_i'], full['f_i']) and low['f_i'][j] == 0.0
    close_errors(low['df_i'], full['df_i'][j])
    ref = (j + 1) % nbins
    spec = m.compute_pmf(u_n, bin_n, nbins, uncertainties='from-specified', pmf_reference=ref, uncertainty_method=method)
    assert np.array_equal(spec['f_i'], full['f_i'])
    close_errors(spec['df_i'], full['df_i'][ref])
    assert spec['df_i'][ref] == 0.0


@pytest.mark.parametrize('name, nbins', [('2x65', 3), ('5x1000_alternating', 11), ('17x1037', 1)])
def test_normalization(name, nbins):
    m = _mbar(name, 8)
    u_n, bin_n = _binned(name, nbins)
    bin_n = bin_n.copy()
    bin_n[::7] = -1                                                  # z runs over the binned samples only
    r = m.compute_pmf(u_n, bin_n, nbins, uncertainties='from-normalization')
    assert abs(np.sum(np.exp(-r['f_i'])) - 1.0) <= 1e-12
    rows = dense_rows(u_n, bin_n, nbins, with_z=True)
    dense = m.compute_perturbed_free_energies(rows)
    assert np.max(np.abs(r['f_i'] - dense['Delta_f'][nbins, :nbins])) <= 1e-10
    close_errors(r['df_i'], dense['dDelta_f'][:nbins, nbins])
    rb = m.compute_pmf(u_n, bin_n, nbins, uncertainties='from-normalization', uncertainty_method='bootstrap')
    close_errors(rb['df_i'], m.compute_perturbed_free_energies(rows, uncertainty_method='bootstrap')['dDelta_f'][:nbins, nbins])


# ---- edges ---------------------------------------------------------------------------------------------------------------------------
def test_empty_bins_and_unbinned_samples():
    m = _mbar('17x1037', 8)
    u_n, _ = _binned('17x1037', 3)
    rng = np.random.default_rng(5)
    used = np.array([0, 2, 3, 6])                                   # of 8 bins; 1, 4, 5, 7 hold nothing
    bin_n = used[rng.integers(0, used.size, m.N)]
    bin_n[:9] = -1
    bin_n[-9:] = -1
    bin_n[500] = 5                                                   # a bin whose only sample has weight 0 is empty too
    u = u_n.copy()
    u[500] = np.inf
    empty = np.array([1, 4, 5, 7])
    for mode in MODES:
        for method in (None, 'bootstrap'):
            r = m.compute_pmf(u, bin_n, 8, uncertainties=mode, pmf_reference=3, uncertainty_method=method)
            assert np.all(np.isposinf(r['f_i'][empty])) and np.all(np.isfinite(r['f_i'][used]))
            df = r['df_i']
            if mode == 'all-differences':
                assert np.all(np.isnan(df[empty])) and np.all(np.isnan(df[:, empty])) and np.all(np.isfinite(df[np.ix_(used, used)]))
            else:
                assert np.all(np.isnan(df[empty])) and np.all(np.isfinite(df[used]))
            assert r['n_i'][5] == 1 and r['n_i'].sum() == m.N - 18
    # the empty bins and the samples outside take no part: the same surface over the used bins alone
    keep = bin_n >= 0
    keep[500] = False
    compact = np.where(keep, np.searchsorted(used, np.where(keep, bin_n, 0)), -1)
    a = m.compute_pmf(u, bin_n, 8, uncertainties='all-differences')
    b = m.compute_pmf(u, compact, 4, uncertainties='all-differences')
    assert np.max(np.abs(a['f_i'][used] - b['f_i'])) <= 1e-10
    close_errors(a['df_i'][np.ix_(used, used)], b['df_i'])
    dense = m.compute_perturbed_free_energies(dense_rows(u, compact, 4))
    close_errors(b['df_i'], dense['dDelta_f'])


def test_one_sample_bins_and_more_bins_than_samples():
    m = _mbar('2x65')
    u_n, _ = _binned('2x65', 3)
    bin_n = np.arange(m.N) * 3                                      # 65 samples, each alone in its bin, over 200 bins
    r = m.compute_pmf(u_n, bin_n, 200, uncertainties='all-differences')
    assert np.array_equal(np.isfinite(r['f_i']), np.bincount(bin_n, minlength=200) == 1)
    log_w = -u_n - m._log_denominator(m.f_k)
    assert np.max(np.abs((r['f_i'][bin_n] - r['f_i'][bin_n].min()) - (log_w.max() - log_w))) <= 1e-10
    dense = m.compute_perturbed_free_energies(dense_rows(u_n, bin_n, 200)[bin_n])
    close_errors(r['df_i'][np.ix_(bin_n, bin_n)], dense['dDelta_f'])


def test_one_state_and_unsampled_states():
    u_kn, N_k, _ = mc.harmonic_case(1, [40])
    m = an.MBAR(u_kn, N_k, n_bootstraps=4, bootstrap_seed=3)
    bin_n = np.arange(40) % 3
    u_n = 0.5 * u_kn[0]
    for method in (None, 'bootstrap'):
        r = m.compute_pmf(u_n, bin_n, 3, uncertainties='all-differences', uncertainty_method=method)
        dense = m.compute_perturbed_free_energies(dense_rows(u_n, bin_n, 3), uncertainty_method=method)
        assert np.max(np.abs((r['f_i'][None, :] - r['f_i'][:, None]) - dense['Delta_f'])) <= 1e-10
        close_errors(r['df_i'], dense['dDelta_f'])
    m = _mbar('5x1000_alternating')                                  # N_k = 0, 300, 0, 700, 0
    u_n, bin_n = _binned('5x1000_alternating', 3)
    r = m.compute_pmf(m.u_kn[2], bin_n, 3, uncertainties='all-differences')        # the surface at an unsampled state
    close_errors(r['df_i'], m.compute_perturbed_free_energies(dense_rows(m.u_kn[2], bin_n, 3))['dDelta_f'])


def test_weights_spanning_600_in_one_bin_stay_finite():
    m = _mbar('2x65')
    u_n = np.linspace(0.0, 600.0, m.N)
    bin_n = np.zeros(m.N, dtype=np.int64)
    bin_n[::2] = 1
    for mode in MODES:
        r = m.compute_pmf(u_n, bin_n, 2, uncertainties=mode, pmf_reference=0)
        assert np.all(np.isfinite(r['f_i'])) and np.all(np.isfinite(r['df_i']))
    log_w = -u_n - m._log_denominator(m.f_k)
    f = np.array([-an._logsumexp(log_w[bin_n == i]) for i in range(2)])
    r = m.compute_pmf(u_n, bin_n, 2)
    assert np.max(np.abs(r['f_i'] - (f - f.min()))) <= 1e-10


def test_refusals():
    m = _mbar('2x65')
    plain = _mbar('2x65', 0)
    u_n, bin_n = _binned('2x65', 3)
    for bad in (np.nan, -np.inf):
        u = u_n.copy()
        u[7] = bad
        with pytest.raises(an.ParameterError, match='u_n'):
            m.compute_pmf(u, bin_n, 3)
    with pytest.raises(an.ParameterError, match='u_n'):
        m.compute_pmf(u_n[:-1], bin_n, 3)
    with pytest.raises(an.ParameterError, match='every bin is empty'):
        m.compute_pmf(np.full(m.N, np.inf), bin_n, 3)
    with pytest.raises(an.ParameterError, match='every bin is empty'):
        m.compute_pmf(u_n, np.full(m.N, -1), 3)
    for bad in (bin_n[:-1], np.where(np.arange(m.N) == 4, 3, bin_n), np.where(np.arange(m.N) == 4, -2, bin_n), bin_n.astype(np.float64)):
        with pytest.raises(ValueError, match='bin_n'):
            m.compute_pmf(u_n, bad, 3)
    for bad in (0, -1, 65537, 2.5, True):
        with pytest.raises(ValueError, match='nbins'):
            m.compute_pmf(u_n, np.zeros(m.N, dtype=np.int64), bad)
    assert an.MBAR.PMF_MAX_BINS == _engine.MBAR_PMF_MAX_BINS == 65536 and an.MBAR.PMF_MAX_COLUMNS == 4096
    with pytest.raises(ValueError, match='uncertainties'):
        m.compute_pmf(u_n, bin_n, 3, uncertainties='from-highest')
    holed = np.where(bin_n == 1, -1, bin_n)
    for bad in (None, -1, 3, 1.0, 1):                                # (bin 1 is empty)
        with pytest.raises(ValueError, match='pmf_reference'):
            m.compute_pmf(u_n, holed, 3, uncertainties='from-specified', pmf_reference=bad)
    with pytest.raises(ValueError, match='uncertainty_method'):
        m.compute_pmf(u_n, bin_n, 3, uncertainty_method='jackknife')
    with pytest.raises(an.ParameterError, match='without any bootstraps'):
        plain.compute_pmf(u_n, bin_n, 3, uncertainty_method='bootstrap')


def test_the_asymptotic_errors_stop_at_their_column_limit_and_name_the_bootstrap():
    u_kn, N_k, _ = mc.harmonic_case(2, [2100, 2100])
    m = an.MBAR(u_kn, N_k, n_bootstraps=2, bootstrap_seed=1)
    bin_n = np.arange(m.N)                                           # 4200 bins of one sample: 2 + 4200 + 1 columns
    with pytest.raises(ValueError, match="uncertainty_method='bootstrap'"):
        m.compute_pmf(u_kn[0], bin_n, m.N)
    r = m.compute_pmf(u_kn[0], bin_n, m.N, uncertainty_method='bootstrap')
    assert np.all(np.isfinite(r['f_i'])) and r['df_i'].shape == (m.N,)


def test_a_bin_empty_in_a_replicate_leaves_that_replicate_out():
    m = _mbar('2x65', 8)
    u_n, _ = _binned('2x65', 3)
    counts = np.stack([m._bootstrap_counts(b) for b in range(8)])
    n = int(np.flatnonzero((counts == 0).sum(axis=0) >= 1)[0])       # a sample that some replicate did not draw: alone in bin 1
    missing = counts[:, n] == 0
    assert 0 < missing.sum() < 7
    bin_n = np.where(np.arange(m.N) == n, 1, 0)
    r = m.compute_pmf(u_n, bin_n, 2, uncertainties='all-differences', uncertainty_method='bootstrap')
    f_b = m._bootstrap_pmf(u_n, bin_n, 2)
    assert np.array_equal(np.isposinf(f_b[:, 1]), missing) and np.all(np.isfinite(f_b[:, 0]))
    expect = np.std((f_b[:, 1] - f_b[:, 0])[~missing])
    assert abs(r['df_i'][0, 1] - expect) <= 1e-12 * expect and r['df_i'][0, 1] == r['df_i'][1, 0]
    # fewer than two replicates with both bins: NaN
    lone = np.where(missing)[0]
    m2 = an.MBAR(m.u_kn, m.N_k, n_bootstraps=1, bootstrap_seed=SEED)
    assert np.all(np.isnan(m2.compute_pmf(u_n, bin_n, 2, uncertainty_method='bootstrap')['df_i'])) and lone.size


# ---- physics -------------------------------------------------------------------------------------------------------------------------
def test_a_flat_coordinate_under_harmonic_umbrellas_comes_out_flat():
    """5 harmonic windows u_k(x) = (x - c_k)^2 / 2 (kT) over a flat coordinate, exact Gaussian samples; the surface at u = 0 over
    bins of equal width is flat.  The error bars set the margin: every bin within 5 of its own df_i of the lowest."""
    rng = np.random.default_rng(20260)
    c = np.arange(5.0)
    x = np.concatenate([rng.normal(ck, 1.0, size=400) for ck in c])
    u_kn = 0.5 * (x[None, :] - c[:, None]) ** 2
    m = an.MBAR(u_kn, [400] * 5)
    bin_n, nbins = an.bin_samples(x, np.linspace(-0.5, 4.5, 11))
    r = m.compute_pmf(np.zeros(x.size), bin_n, nbins)
    assert nbins == 10 and r['n_i'].min() >= 20, r['n_i']
    assert np.all(np.isfinite(r['df_i'])) and np.all(r['df_i'][r['f_i'] > 0.0] > 0.0)
    assert np.all(r['f_i'] <= 5.0 * r['df_i']), (r['f_i'], r['df_i'])
    # and the same data do show a surface that is not flat: the first window's own potential
    tilted = m.compute_pmf(u_kn[0], bin_n, nbins)
    assert np.any(tilted['f_i'] > 5.0 * tilted['df_i'])


# ---- bin_samples ---------------------------------------------------------------------------------------------------------------------
def test_bin_samples_one_dimension():
    e = np.array([0.0, 0.5, 1.5, 2.0])
    v = np.array([0.0, 0.25, 0.5, 1.4999, 1.5, 2.0, 2.0000001, -1e-9, np.nan, np.inf, -np.inf, 1.0])
    bin_n, nbins = an.bin_samples(v, e)
    assert nbins == 3 and bin_n.tolist() == [0, 0, 1, 1, 2, 2, -1, -1, -1, -1, -1, 1]
    assert an.bin_samples(v, [e])[0].tolist() == bin_n.tolist() and an.bin_samples(v[:, None], [e])[0].tolist() == bin_n.tolist()
    inside = bin_n >= 0
    assert np.array_equal(bin_n[inside], np.minimum(np.digitize(v[inside], e) - 1, 2))
    assert np.array_equal(np.bincount(bin_n[inside], minlength=3), np.histogram(v[np.isfinite(v)], bins=e)[0])


@pytest.mark.parametrize('D', [2, 3])
def test_bin_samples_is_histogramdd_with_the_first_dimension_fastest(D):
    rng = np.random.default_rng(D)
    edges = [np.array([-1.0, 0.0, 0.25, 1.0]), np.linspace(-1.0, 1.0, 6), np.array([-0.5, 0.5])][:D]
    v = rng.uniform(-1.2, 1.2, size=(500, D))
    v[:D] = [e[-1] for e in edges]                                   # right edges: inside the last interval
    v[D:2 * D] = np.diag([e[1] for e in edges])                      # an inner edge opens its interval
    v[10, 0] = np.nan
    bin_n, nbins = an.bin_samples(v, edges)
    shape = [e.size - 1 for e in edges]
    assert nbins == int(np.prod(shape))
    H = np.histogramdd(v[~np.isnan(v).any(axis=1)], bins=edges)[0]
    assert np.array_equal(np.bincount(bin_n[bin_n >= 0], minlength=nbins), H.reshape(-1, order='F').astype(np.int64))
    assert bin_n[0] == nbins - 1 and bin_n[10] == -1
    idx = np.unravel_index(bin_n[bin_n >= 0], shape, order='F')
    for d, e in enumerate(edges):
        x = v[bin_n >= 0, d]
        assert np.all(e[idx[d]] <= x) and np.all(x <= e[idx[d] + 1])
    outside = np.any([(v[:, d] < e[0]) | (v[:, d] > e[-1]) for d, e in enumerate(edges)], axis=0)
    assert np.array_equal(bin_n == -1, outside | np.isnan(v).any(axis=1))


def test_bin_samples_refusals():
    for values, edges in ((np.zeros((3, 4)), [[0, 1]] * 4), (np.zeros((3, 2)), [[0, 1]]), (np.zeros(3), [0.0]), (np.zeros(3), [0.0, 0.0, 1.0]),
                          (np.zeros((2, 2, 2)), [[0, 1]] * 2)):
        with pytest.raises(ValueError):
            an.bin_samples(values, edges)


# ---- the analyzer --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def walk_store(tmp_path_factory):
    rng = np.random.default_rng(78)
    sts = ur._states(ur._pair_system(ur.CUT_K_R), ur.CUT_T, lambdas=[1.0, 1.0, 1.0])
    e, si, x, d = ur._gaussian_pair_run(rng, ur.CUT_T, 121, ur.K_B + ur.CUT_K_R, ur.CUT_K_R, None, walk=True)
    return ur._write_store(tmp_path_factory.mktemp('pmf') / 'store', sts, e, si, x), d.astype(np.float64)


@pytest.mark.parametrize('cutoff', [None, 2.0])
def test_get_pmf_bins_the_analyzers_own_columns(walk_store, cutoff):
    rep, d = walk_store
    kw = dict(n_equilibration_iterations=1, statistical_inefficiency=2.0, unbias_restraint=True, restraint_distance_cutoff=None)
    a = an.MultiStateSamplerAnalyzer(rep, restraint_energy_cutoff=cutoff, analysis_kwargs={'n_bootstraps': 4, 'bootstrap_seed': 11}, **kw)
    values = d[:, :, 0]                                              # [n_iterations + 1][n_replicas]
    edges = np.linspace(-0.06, 0.06, 7)
    f_i, df_i, n_i = a.get_pmf(values, edges, state=1)
    # by hand: the selected iterations, replica by replica, less the frames the cutoff dropped
    iterations = a._decorrelated_selection()[3]
    assert 1 < iterations.size < 120
    mbar = a.mbar
    v = values[iterations].T.reshape(-1)
    if cutoff is not None:
        full = an.MultiStateSamplerAnalyzer(rep, restraint_energy_cutoff=None, **kw)
        u_full = full._compute_mbar_unbiased_energies()[0]
        where = [int(np.flatnonzero(np.all(u_full[1:-1] == mbar.u_kn[1:-1, [n]], axis=0))[0]) for n in range(mbar.N)]
        assert 0 < len(where) < v.size
        v = v[where]
    assert v.size == mbar.N and mbar.K == 5
    bin_n, nbins = an.bin_samples(v, edges)
    r = mbar.compute_pmf(mbar.u_kn[2], bin_n, nbins)                 # sampled state 1 behind the end row in front
    assert np.array_equal(f_i, r['f_i']) and np.array_equal(df_i, r['df_i'], equal_nan=True) and np.array_equal(n_i, r['n_i'])
    assert n_i.sum() == np.count_nonzero(bin_n >= 0) > 0.9 * v.size and np.isfinite(f_i).sum() >= 4
    # two dimensions, another mode, the analyzer's uncertainty method
    a.uncertainty_method = 'bootstrap'
    f2, df2, n2 = a.get_pmf(d[:, :, :2], [edges, np.array([-1.0, 0.0, 1.0])], state=0, uncertainties='from-normalization')
    v2 = d[iterations][:, :, :2].swapaxes(0, 1).reshape(-1, 2)
    if cutoff is not None:
        v2 = v2[where]
    b2, nb2 = an.bin_samples(v2, [edges, np.array([-1.0, 0.0, 1.0])])
    r2 = mbar.compute_pmf(mbar.u_kn[1], b2, nb2, uncertainties='from-normalization', uncertainty_method='bootstrap')
    assert nb2 == 12 and np.array_equal(f2, r2['f_i']) and np.array_equal(df2, r2['df_i'], equal_nan=True) and np.array_equal(n2, r2['n_i'])
    assert a._mbar is mbar


def test_get_pmf_refusals(walk_store):
    rep, d = walk_store
    a = an.MultiStateSamplerAnalyzer(rep, n_equilibration_iterations=1, statistical_inefficiency=2.0)
    edges = np.linspace(-0.06, 0.06, 7)
    for bad in (d[:-1, :, 0], d[:, :2, 0], d[:, :, 0].T, d[:, :, 0].reshape(-1), d[:, :, :, None]):
        with pytest.raises(ValueError, match=r'\[n_iterations \+ 1\]\[n_replicas\] = \[121\]\[3\]'):
            a.get_pmf(bad, edges)
    for bad in (-1, 3, 1.0, None):
        with pytest.raises(ValueError, match='state'):
            a.get_pmf(d[:, :, 0], edges, state=bad)


# ---- no device -----------------------------------------------------------------------------------------------------------------------
def test_compute_pmf_on_the_cpu_port_names_the_header():
    assert os.path.exists(CPU_LIB), 'build() makes oracle/_build/libremd_cpu.so; without it this check would not run'
    lists = [getattr(_engine, n) for n in dir(_engine) if n.endswith('EXPORTS') and n != 'MBAR_PMF_EXPORTS']
    assert len(lists) > 10 and all(set(_engine.MBAR_PMF_EXPORTS).isdisjoint(x) for x in lists)
    assert _engine.MBAR_PMF_EXPORTS == ['remd_mbar_pmf_chunk', 'remd_mbar_pmf', 'remd_mbar_bootstrap_pmf']

    class WithoutPmf:                                                # a library of the GPU build before these entry points
        def __getattr__(self, name):
            if name in _engine.MBAR_PMF_EXPORTS:
                raise AttributeError(name)
            return lambda *a: 0
    d = _engine.DeviceMBAR.__new__(_engine.DeviceMBAR)
    d.lib, d.h, d.K, d.N = WithoutPmf(), None, 2, 65
    u_n, bin_n = _binned('2x65', 3)
    with pytest.raises(NotImplementedError, match='remd_mbar_pmf_chunk.*include/remd_hip_mbar.h'):
        d.pmf_chunk()
    with pytest.raises(NotImplementedError, match='include/remd_hip_mbar.h'):
        d.pmf(np.zeros(2), u_n, bin_n, 3)
    with pytest.raises(NotImplementedError, match='include/remd_hip_mbar.h'):
        d.bootstrap_pmf([0], np.zeros((1, 2)), u_n, bin_n, 3)
    # the estimator hands the refusal on
    m = an.MBAR.__new__(an.MBAR)
    m.__dict__.update(_mbar('2x65').__dict__)
    m._dev = d
    with pytest.raises(NotImplementedError, match='include/remd_hip_mbar.h'):
        m.compute_pmf(u_n, bin_n, 3)
    # the CPU port of the ABI exports none of them
    import ctypes
    lib = ctypes.CDLL(CPU_LIB)
    assert not any(hasattr(lib, name) for name in _engine.MBAR_PMF_EXPORTS)
