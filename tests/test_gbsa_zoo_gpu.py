"""The implicit-solvent kernels (csrc/gbsa.hip) on the zoo of tests/gbsa_zoo.py, against the f64 oracles (autograd forces, so independent
of the kernels' hand-derived force through the Born radii): every branch of H(r; or_i, sr_j) -- zero, partial, far, engulfed -- in the
one-launch kernel and in the three tiled launches, the atom counts at which the kernels change path (the small/tiled switch, one live
lane in the last tile, one staging block exactly, a second block of one atom and a partly filled one), alchemical scale factors beyond
one tile with the u_kl columns, the CutoffPeriodic model with overlapping pairs across the box faces, and bit-reproducibility.
tests/test_gbsa_zoo_cpu.py shows without a GPU that the cases reach what they claim.  Bounds: the project's GB tolerances (gbsa_zoo.ENERGY_RTOL, FORCE_TOL, ROWS_RTOL)."""
import numpy as np
import pytest

import gbsa_zoo as zoo
from openmmtools_amd.system import system_to_desc

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 128, 129, 1024, 1025, 1100)
# (n, spread, REMD_GB_SMALL): up to 64 atoms under both settings ('0': the three tiled launches)
ZOO_CASES = [(n, spread, small) for n in SIZES for spread in (1.0, zoo.DILUTE) for small in (('1', '0') if n <= 64 else ('1',))]


def _replicas(n):
    return 3 if n < 1000 else 2


@pytest.mark.parametrize('small', ['1', '0'])
@pytest.mark.parametrize('k', range(len(zoo.PAIR_SETS)))
def test_two_atoms_through_every_regime_and_border(hip_engine_factory, monkeypatch, k, small):
    """energy and both atoms' forces at every distance of the scan; the two forces are opposite to the bit"""
    monkeypatch.setenv('REMD_GB_SMALL', small)
    system, x, r, dropped = zoo.pair_scan(k)
    assert dropped == 0
    U, f = zoo.check_against_oracle(hip_engine_factory(), system_to_desc(system), x, zoo.ENERGY_RTOL, zoo.FORCE_TOL, name='pair scan %d small=%s' % (k, small))
    worst = np.abs(f[:, 0] + f[:, 1]).max()
    print('pair scan %d small=%s: max |F_0 + F_1| = %.3g' % (k, small, worst))
    assert np.array_equal(f[:, 0], -f[:, 1]), worst


@pytest.mark.parametrize('n,spread,small', ZOO_CASES)
def test_overlap_zoo_at_the_atom_count_edges(hip_engine_factory, monkeypatch, n, spread, small):
    monkeypatch.setenv('REMD_GB_SMALL', small)
    system, x0, (q, radius, scale) = zoo.overlap_zoo(n, spread=spread)
    X = zoo.replica_positions(x0, _replicas(n))
    if n >= 63:
        assert all(v > 0 for v in zoo.regimes(X[0], radius, scale).values())
    zoo.check_against_oracle(hip_engine_factory(), system_to_desc(system), X, zoo.ENERGY_RTOL, zoo.FORCE_TOL, name='zoo %d x%g small=%s' % (n, spread, small))


@pytest.mark.parametrize('spread', [1.0, zoo.DILUTE])
@pytest.mark.parametrize('n', [150, 1100])
def test_alchemical_zoo_rows_and_forces_beyond_one_tile(hip_engine_factory, n, spread):
    """every third atom alchemical: the u_kl row of each replica at every state's lambda (the columns with one lambda for all replicas),
    the potential and the forces at the replica's own"""
    system, x0, (q, radius, scale) = zoo.alchemical_zoo(n, spread=spread)
    desc = system_to_desc(system)
    assert desc['gbsa']['alchemical'].tolist() == [1 if i % 3 == 0 else 0 for i in range(n)]
    zoo.check_against_oracle(hip_engine_factory(), desc, zoo.replica_positions(x0, 3), zoo.ENERGY_RTOL, zoo.FORCE_TOL, ladder=True, rows_rtol=zoo.ROWS_RTOL,
                             name='alchemical zoo %d x%g' % (n, spread))


@pytest.mark.parametrize('spread', [1.0, zoo.DILUTE])
@pytest.mark.parametrize('n', [63, 64])
def test_alchemical_zoo_on_the_small_and_on_the_tiled_path(hip_engine_factory, monkeypatch, n, spread):
    """both paths against the oracle and against each other.  They evaluate the same pair expressions and give wavefront w the same
    partners j = w (mod 16) in the same order; what differs is the compiler's contraction of each kernel and that the tiled launches
    round the pair force and the force through the Born radii to fixed point one after the other: a few f32 ulp (6e-8) per term --
    1e-6 of the energies and 1e-5 of the largest force component are ten and twenty times tighter than the bounds against the oracle."""
    system, x0, _ = zoo.alchemical_zoo(n, spread=spread)
    desc = system_to_desc(system)
    out = []
    for small in ('1', '0'):
        monkeypatch.setenv('REMD_GB_SMALL', small)
        eng = hip_engine_factory()
        zoo.check_against_oracle(eng, desc, zoo.replica_positions(x0, 3), zoo.ENERGY_RTOL, zoo.FORCE_TOL, ladder=True, rows_rtol=zoo.ROWS_RTOL,
                                 name='alchemical zoo %d x%g small=%s' % (n, spread, small))
        rows, U, _, f, _ = zoo.evaluate(eng, desc, zoo.replica_positions(x0, 3), ladder=True)
        out.append((rows, U, f))
    (rows1, U1, f1), (rows0, U0, f0) = out
    print('alchemical zoo %d x%g small against tiled: rows %.3g U %.3g forces %.3g of %.6g' %
          (n, spread, np.abs(rows1 - rows0).max(), np.abs(U1 - U0).max(), np.abs(f1 - f0).max(), np.abs(f0).max()))
    assert np.allclose(rows1, rows0, rtol=1e-6, atol=1e-6 * np.abs(rows0).max()) and np.allclose(U1, U0, rtol=1e-6, atol=1e-6 * np.abs(U0).max())
    assert np.abs(f1 - f0).max() < 1e-5 * np.abs(f0).max()


def test_periodic_zoo_with_overlaps_across_the_box_faces(hip_engine_factory):
    system, x0, box, (q, radius, scale), _ = zoo.periodic_zoo()
    desc = system_to_desc(system)
    assert desc['gbsa']['method'] == 2
    X = zoo.periodic_replicas(x0, 3, box[0])
    masks = zoo.regime_masks(X[0], radius, scale, box=box, cutoff=1.4)
    across = zoo.straddling(X[0], box)
    assert all(int((m & across).sum()) > 0 for m in masks.values())
    U, _ = zoo.check_against_oracle(hip_engine_factory(), desc, X, zoo.ENERGY_RTOL, zoo.FORCE_TOL, box=box, name='periodic zoo')
    assert np.ptp(U) > 0.1                                      # the replicas see different GB energies


@pytest.mark.parametrize('spread', [1.0, zoo.DILUTE])
def test_two_evaluations_of_1100_atoms_on_fresh_handles_agree_to_the_bit(hip_engine_factory, spread):
    """the sums have a fixed order: wavefront partial sums added in wavefront order, forces in fixed point, energies per tile"""
    system, x0, _ = zoo.alchemical_zoo(1100, spread=spread)
    desc = system_to_desc(system)
    X = zoo.replica_positions(x0, 3)
    out = [zoo.evaluate(hip_engine_factory(), desc, X, ladder=True) for _ in range(2)]
    assert np.all(np.isfinite(out[0][0])) and np.abs(out[0][3]).max() > 1.0
    for a, b, what in zip(out[0], out[1], ('rows', 'U', 'positions', 'forces', 'labels')):
        assert np.array_equal(a, b), what
