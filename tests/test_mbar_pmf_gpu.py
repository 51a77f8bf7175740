"""Free energy surfaces over binned samples on the device (include/remd_hip_mbar.h remd_mbar_pmf, remd_mbar_bootstrap_pmf,
openmmtools_amd/csrc/mbar_pmf.hip, analysis.MBAR(solver='device').compute_pmf) against the numpy solver.  Bounds as between the
project's MBAR paths: 1e-10 on free energies, 1e-8 relative on errors; 1e-12 relative between two device routes to one sum.
The shapes are the smallest that reach the kernels' edges: N no multiple of 64, bins one above and exactly at the samples one
workgroup reduces, one bin with everything, 4096 bins for 1037 samples, a bin scattered over the whole index range, -1 at both ends."""
import functools
import numpy as np
import pytest
from openmmtools_amd.multistate import analysis as an
import mbar_cases as mc

pytestmark = pytest.mark.gpu

SEED = 0x5EEDB007C0FFEE
B = 8
MODES = ['from-lowest', 'from-specified', 'from-normalization', 'all-differences']


@functools.lru_cache(maxsize=None)
def _case(name):
    if name == '1x70':
        K, N_k = 1, [70]
    elif name == '17x915_two_unsampled':
        K, N_k = 17, [0 if k in (3, 11) else 61 for k in range(17)]
    else:
        K, N_k = mc.CASES[name]
    u_kn, N_k, _ = mc.harmonic_case(K, N_k)
    u_kn.setflags(write=False)
    return u_kn, N_k


@functools.lru_cache(maxsize=None)
def _numpy(name):
    return an.MBAR(*_case(name), n_bootstraps=B, bootstrap_seed=SEED)


@functools.lru_cache(maxsize=None)
def _device(name):
    return an.MBAR(*_case(name), solver='device', n_bootstraps=B, bootstrap_seed=SEED)


CHUNK = 256                                                          # asserted against the device's answer below


@functools.lru_cache(maxsize=None)
def _layout(name, layout):
    """(u_n, bin_n, nbins, pmf_reference)"""
    m = _numpy(name)
    N = m.N
    rng = np.random.default_rng(41)
    u_n = 0.5 * (m.u_kn[0] + m.u_kn[-1])
    if layout == 'chunk_edges':                                      # bin 0: CHUNK + 1 samples, bin 1: CHUNK, both scattered; -1 at both ends
        inner = rng.permutation(np.arange(3, N - 3))
        bin_n = np.full(N, -1)
        bin_n[inner[:CHUNK + 1]] = 0
        bin_n[inner[CHUNK + 1:2 * CHUNK + 1]] = 1
        bin_n[inner[2 * CHUNK + 1:]] = 2 + np.arange(inner.size - 2 * CHUNK - 1) % 3
        nbins, ref = 5, 1
    elif layout == 'one_bin':
        bin_n, nbins, ref = np.zeros(N, dtype=np.int64), 1, 0
    elif layout == 'sparse_4096':
        bin_n, nbins = rng.integers(0, 4096, N), 4096
        ref = int(bin_n[N // 2])
    elif layout == 'thirds':                                         # small cases: three bins dealt round, -1 at both ends, one +inf
        bin_n = rng.permutation(N) % 3
        bin_n[0] = bin_n[-1] = -1
        u_n = u_n.copy()
        u_n[N // 2] = np.inf
        nbins, ref = 3, 2
    u_n.setflags(write=False)
    bin_n.setflags(write=False)
    return u_n, bin_n, nbins, ref


LAYOUTS = [('17x1037', 'chunk_edges'), ('17x1037', 'one_bin'), ('17x1037', 'sparse_4096'), ('2x65', 'thirds'), ('5x1000_alternating', 'thirds'),
           ('1x70', 'thirds'), ('17x915_two_unsampled', 'thirds'), ('17x915_two_unsampled', 'chunk_edges')]


def close_errors(a, b, rel=1e-8):
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a)
    if ok.any():
        print('largest error difference / bound: %.3g' % np.max(np.abs(a[ok] - b[ok]) / (rel * np.abs(b[ok]) + 1e-13)))
    assert np.all(np.abs(a[ok] - b[ok]) <= rel * np.abs(b[ok]) + 1e-13)


def close_f(a, b):
    assert np.array_equal(np.isposinf(a), np.isposinf(b))
    ok = np.isfinite(b)
    print('largest f_i difference: %.3g' % np.max(np.abs(a[ok] - b[ok])))
    assert np.all(np.abs(a[ok] - b[ok]) <= 1e-10)


def test_the_samples_per_workgroup():
    assert _device('2x65')._dev.pmf_chunk() == CHUNK


@pytest.mark.parametrize('name, layout', LAYOUTS)
def test_the_pass_is_the_numpy_pass_at_the_same_f_k(name, layout):
    """f_i, cross, diag and the parts of the column z at the numpy solver's f_k: one sum in two orders"""
    ref, dev = _numpy(name), _device(name)._dev
    u_n, bin_n, nbins, _ = _layout(name, layout)
    f_i, cross, diag, parts = dev.pmf(ref.f_k, u_n, bin_n, nbins, want_all=True)
    e_f, e_cross, e_diag, e_parts = ref._pmf_parts(np.asarray(u_n), np.asarray(bin_n), nbins, True)
    close_f(f_i, e_f)
    close_errors(cross, e_cross, rel=1e-10)
    close_errors(diag, e_diag, rel=1e-10)
    assert abs(parts[0] - e_parts[0]) <= 1e-10
    close_errors(parts[1:], e_parts[1:], rel=1e-10)
    empty = ~np.isfinite(e_f)
    assert np.all(diag[empty] == 0.0) and np.all(cross[:, empty] == 0.0)
    # bit for bit the same from call to call
    again = dev.pmf(ref.f_k, u_n, bin_n, nbins, want_all=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip((f_i, cross, diag, parts), again))
    assert dev.last_ms() > 0.0


@pytest.mark.parametrize('name, layout', LAYOUTS)
def test_compute_pmf_device_against_numpy(name, layout):
    ref, dev = _numpy(name), _device(name)
    u_n, bin_n, nbins, reference = _layout(name, layout)
    for mode in MODES:
        for method in (None, 'bootstrap'):
            if mode == 'all-differences' and nbins == 4096 and method == 'bootstrap':
                continue                                             # (8 x 4096 x 4096 differences on the host: the vector modes cover it)
            e = ref.compute_pmf(u_n, bin_n, nbins, uncertainties=mode, pmf_reference=reference, uncertainty_method=method)
            g = dev.compute_pmf(u_n, bin_n, nbins, uncertainties=mode, pmf_reference=reference, uncertainty_method=method)
            close_f(g['f_i'], e['f_i'])
            close_errors(g['df_i'], e['df_i'])
            assert np.array_equal(g['n_i'], e['n_i'])


def test_cross_and_diag_are_the_dense_augmented_gram_entries():
    ref, dev = _numpy('2x65'), _device('2x65')._dev
    u_n, bin_n, nbins, _ = _layout('2x65', 'thirds')
    rows = np.where(np.asarray(bin_n)[None, :] == np.arange(nbins)[:, None], np.asarray(u_n)[None, :], np.inf)
    f_l, _, G = dev.augmented_gram(ref.f_k, u_ln=rows)
    f_i, cross, diag, _ = dev.pmf(ref.f_k, u_n, bin_n, nbins)
    K = ref.K
    assert np.all(np.abs(f_i - f_l) <= 1e-12 * np.maximum(1.0, np.abs(f_l)))
    close_errors(cross, G[:K, K:], rel=1e-12)
    close_errors(diag, np.diag(G)[K:], rel=1e-12)
    off = G[K:, K:][~np.eye(nbins, dtype=bool)]
    assert np.all(off == 0.0)                                        # what the bin-bin block never has to be computed for


def test_a_replicate_alone_is_the_replicate_in_its_batch():
    m = _device('17x1037')
    dev = m._dev
    u_n, bin_n, nbins, _ = _layout('17x1037', 'chunk_edges')
    dev.bootstrap_draw(SEED, 0, B, m.sample_states)
    batch = dev.bootstrap_pmf(np.arange(B), m.f_k_boots, u_n, bin_n, nbins)
    assert batch.shape == (B, nbins) and np.all(np.isfinite(batch))
    alone = dev.bootstrap_pmf([5], m.f_k_boots[5:6], u_n, bin_n, nbins)
    assert alone.tobytes() == batch[5:6].tobytes()
    some = dev.bootstrap_pmf([6, 2], m.f_k_boots[[6, 2]], u_n, bin_n, nbins)
    assert some.tobytes() == batch[[6, 2]].tobytes()
    assert dev.bootstrap_pmf(np.arange(B), m.f_k_boots, u_n, bin_n, nbins).tobytes() == batch.tobytes()
    expect = _numpy('17x1037')._bootstrap_pmf(np.asarray(u_n), np.asarray(bin_n), nbins)
    assert np.max(np.abs(batch - expect)) <= 1e-10


def test_a_bin_without_a_drawn_sample_is_empty_in_that_replicate():
    ref, m = _numpy('2x65'), _device('2x65')
    u_n = 0.5 * (ref.u_kn[0] + ref.u_kn[-1])
    counts = np.stack([ref._bootstrap_counts(b) for b in range(B)])
    n = int(np.flatnonzero((counts == 0).sum(axis=0) >= 1)[0])
    missing = counts[:, n] == 0
    assert 0 < missing.sum() < B - 1
    bin_n = np.where(np.arange(ref.N) == n, 1, 0)
    m._dev.bootstrap_draw(SEED, 0, B, None)
    f_b = m._dev.bootstrap_pmf(np.arange(B), m.f_k_boots, u_n, bin_n, 2)
    assert np.array_equal(np.isposinf(f_b[:, 1]), missing) and np.all(np.isfinite(f_b[:, 0]))
    for mode in MODES:
        e = ref.compute_pmf(u_n, bin_n, 2, uncertainties=mode, pmf_reference=0, uncertainty_method='bootstrap')
        g = m.compute_pmf(u_n, bin_n, 2, uncertainties=mode, pmf_reference=0, uncertainty_method='bootstrap')
        close_f(g['f_i'], e['f_i'])
        close_errors(g['df_i'], e['df_i'])


def test_refusals_leave_the_problem_usable():
    m = _device('2x65')
    dev = m._dev
    u_n, bin_n, nbins, _ = _layout('2x65', 'thirds')
    u_n, bin_n = np.asarray(u_n), np.asarray(bin_n)
    good = dev.pmf(m.f_k, u_n, bin_n, nbins)
    dev.bootstrap_draw(SEED, 2, 4, None)
    f_b = m.f_k_boots[2:6]
    good_b = dev.bootstrap_pmf([2, 3, 4, 5], f_b, u_n, bin_n, nbins)
    bad_u, bad_inf = u_n.copy(), u_n.copy()
    bad_u[3], bad_inf[3] = np.nan, -np.inf
    bad_f = m.f_k.copy()
    bad_f[1] = np.inf
    for args, message in (((m.f_k, u_n, np.where(np.arange(65) == 9, nbins, bin_n), nbins), r'bin_n\[9\] = 3 is outside -1 \.\.\. 2'),
                          ((m.f_k, u_n, np.where(np.arange(65) == 9, -2, bin_n), nbins), r'bin_n\[9\] = -2'),
                          ((m.f_k, u_n, np.full(65, -1), 0), 'nbins = 0 is outside 1 ... REMD_MBAR_PMF_MAX_BINS = 65536'),
                          ((m.f_k, u_n, bin_n, 65537), 'nbins = 65537 is outside'),
                          ((m.f_k, bad_u, bin_n, nbins), r'u_n\[3\] is a NaN or -inf'),
                          ((m.f_k, bad_inf, bin_n, nbins), r'u_n\[3\] is a NaN or -inf'),
                          ((bad_f, u_n, bin_n, nbins), r'f_k\[1\] is not finite')):
        with pytest.raises(RuntimeError, match='remd_mbar_pmf failed.*' + message):
            dev.pmf(*args)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(good[:3], dev.pmf(m.f_k, u_n, bin_n, nbins)[:3]))
    bad_fb = f_b.copy()
    bad_fb[2, 0] = np.nan
    for args, message in ((([2, 3, 4, 6], f_b, u_n, bin_n, nbins), 'replicate 6 is outside the drawn range 2 ... 5'),
                          (([1], f_b[:1], u_n, bin_n, nbins), 'replicate 1 is outside the drawn range'),
                          (([2, 3, 4, 5], bad_fb, u_n, bin_n, nbins), 'f_b of replicate 4 holds a non-finite value'),
                          (([2, 3, 4, 5], f_b, bad_u, bin_n, nbins), r'u_n\[3\] is a NaN or -inf'),
                          (([2, 3, 4, 5], f_b, u_n, np.where(np.arange(65) == 9, nbins, bin_n), nbins), r'bin_n\[9\] = 3'),
                          (([2, 3, 4, 5], f_b, u_n, bin_n, 65537), 'nbins = 65537')):
        with pytest.raises(RuntimeError, match='remd_mbar_bootstrap_pmf failed.*' + message):
            dev.bootstrap_pmf(*args)
        assert dev.bootstrap_pmf([2, 3, 4, 5], f_b, u_n, bin_n, nbins).tobytes() == good_b.tobytes()
    # the largest nbins is taken
    wide = dev.pmf(m.f_k, u_n, np.where(bin_n >= 0, bin_n * 30000, -1), 65536)[0]
    assert np.array_equal(wide[[0, 30000, 60000]], good[0]) and np.isposinf(wide).sum() == 65533
