"""The implicit-solvent zoo (tests/gbsa_zoo.py) without a GPU: the cases reach the branches of H(r; or_i, sr_j) they claim, the f64
oracles' autograd forces agree with central differences in every regime, and the C++ port of the ABI (oracle/cpu/remd_cpu.cpp, its own
analytic gb_H) agrees with the oracle on the two-atom scan and on the NoCutoff zoo at every atom count the GPU file uses.  The periodic
model is not in the C++ port: that case is checked against tests/custom_gb_oracle.py by central differences only."""
import os

import numpy as np
import pytest

import oracle
import gbsa_zoo as zoo
from oracle.forcefield import ForceFieldOracle
from oracle.alchemical_regions import total_state_energies, total_energy_forces
from openmmtools_amd.system import system_to_desc
from openmmtools_amd._engine import HipEngine

CPU_LIB = os.path.join(os.path.dirname(os.path.abspath(oracle.__file__)), '_build', 'libremd_cpu.so')
SIZES = (1, 2, 63, 64, 65, 128, 129, 1024, 1025, 1100)
# central differences of an f64 energy of E ~ 1e3 .. 1e4 kJ/mol with this step: rounding 1e-16 E / h ~ 1e-6 kJ/mol/nm, truncation
# h^2 f''' far below it; the step is below twice ZOO_BORDER_GUARD, so no pair crosses a kink of dH.  Forces are ~1e3: 1e-7 of the
# largest has two decades of room.
FD_STEP, FD_TOL = 1e-6, 1e-7


@pytest.fixture(scope='module')
def cpu_lib():
    if not os.path.exists(CPU_LIB):
        oracle.build()
    return CPU_LIB


def _all_four(counts):
    return all(counts[k] > 0 for k in ('zero', 'partial', 'far', 'engulfed'))


def test_regimes_counts_the_four_branches_of_hand_placed_pairs():
    # or = 0.441 / 0.041, sr = 0.5292 / 0.03485: at r = 0.1 the small atom is engulfed and the large one sees nothing of it
    x = np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0]])
    assert zoo.regimes(x, [0.05, 0.45], [0.85, 1.2]) == dict(zero=1, partial=0, far=0, engulfed=1)
    m = zoo.regime_masks(x, [0.05, 0.45], [0.85, 1.2])
    assert m['engulfed'][0, 1] and m['zero'][1, 0]
    assert zoo.regimes(x * 1.5, [0.2, 0.2], [0.85, 0.85]) == dict(zero=0, partial=2, far=0, engulfed=0)
    assert zoo.regimes(x * 9.0, [0.2, 0.2], [0.85, 0.85]) == dict(zero=0, partial=0, far=2, engulfed=0)
    # through a face of a 3 nm box the pair at 2.9 nm is the pair at 0.1 nm; out of range it is in no regime
    box = np.full(3, 3.0)
    assert zoo.regimes(x * 29.0, [0.05, 0.45], [0.85, 1.2], box=box, cutoff=1.4) == dict(zero=1, partial=0, far=0, engulfed=1)
    assert sum(zoo.regimes(x * 15.0, [0.05, 0.45], [0.85, 1.2], box=box, cutoff=1.4).values()) == 0


SPREADS = (1.0, zoo.DILUTE)


@pytest.mark.parametrize('spread', SPREADS)
@pytest.mark.parametrize('n', SIZES + (96, 150))
def test_overlap_zoo_reaches_every_regime_and_keeps_its_guards(n, spread):
    system, x0, (q, radius, scale) = zoo.overlap_zoo(n, spread=spread)
    assert set(radius) <= set(zoo.RADII) and set(scale) <= set(zoo.SCALES) and x0.min() >= 0.0 and x0.max() <= spread * zoo.zoo_edge(n)
    assert np.isclose(n / zoo.zoo_edge(n) ** 3, zoo.CELL_ATOMS / zoo.CELL ** 3) or n <= 200
    for x in zoo.replica_positions(x0, zoo.MAX_REPLICAS):
        counts = zoo.regimes(x, radius, scale)
        assert sum(counts.values()) == n * (n - 1)
        assert _all_four(counts) or n <= 2, counts
        if n > 1:
            d = np.linalg.norm(x[:, None] - x[None], axis=-1) + np.eye(n)
            assert d.min() >= zoo.MIN_DISTANCE
            assert zoo.border_margin(x, radius, scale) >= zoo.ZOO_BORDER_GUARD
        if n > 200:
            assert d.max() > 2.5                               # "far" pairs at several nm
    gb = system_to_desc(system)['gbsa']
    e, f, = zoo.gb_reference(gb, x0)
    assert np.isfinite(e) and np.all(np.isfinite(f))


@pytest.mark.parametrize('n', [63, 64, 65, 96, 128, 129, 150, 1024, 1025, 1100])
def test_the_dense_zoo_saturates_the_tanh_and_the_dilute_one_leaves_atoms_on_its_slope(n):
    """saturated atoms stay in the cases; but where 1 - tanh^2 vanishes so does the force through the Born radii, and H and dH are out of
    sight: every size also runs DILUTE, where a quarter of the atoms or more are on the slope"""
    _, x0, (q, radius, scale) = zoo.overlap_zoo(n)
    psi, slope = zoo.born_saturation(x0, radius, scale)
    assert psi.max() > 5.0 and np.sum(slope < 1e-6) > n // 3
    _, x0, (q, radius, scale) = zoo.overlap_zoo(n, spread=zoo.DILUTE)
    psi, slope = zoo.born_saturation(x0, radius, scale)
    assert np.sum(slope > 1e-3) >= n // 4 and np.sum(slope < 1e-6) > 0 and psi.max() > 1.5, (np.sum(slope > 1e-3), np.sum(slope < 1e-6), psi.max())


def _central_difference(energy, x, i, c):
    xp, xm = x.copy(), x.copy()
    xp[i, c] += FD_STEP; xm[i, c] -= FD_STEP
    return -(energy(xp) - energy(xm)) / (2.0 * FD_STEP)


def _atoms_of_each_regime(masks, per_regime=3):
    """(regime, atom) of a few ordered pairs (i, j) of every regime: both atoms of each pair"""
    out = []
    for k, m in masks.items():
        ii, jj = np.nonzero(m)
        assert len(ii) > 0, k
        for t in np.linspace(0, len(ii) - 1, per_regime).astype(int):
            out += [(k, int(ii[t])), (k, int(jj[t]))]
    return out


@pytest.mark.parametrize('spread', SPREADS)
@pytest.mark.parametrize('n,lam', [(96, 1.0), (150, 0.4), (1100, 1.0)])
def test_oracle_autograd_forces_are_central_differences_in_every_regime(n, lam, spread):
    system, x, par = zoo.alchemical_zoo(n, spread=spread) if lam != 1.0 else zoo.overlap_zoo(n, spread=spread)
    gb = system_to_desc(system)['gbsa']
    assert (gb['alchemical'].sum() > 0) == (lam != 1.0)
    _, f = zoo.gb_reference(gb, x, lam)
    atoms = _atoms_of_each_regime(zoo.regime_masks(x, gb['radius'], gb['scale']), per_regime=3 if n < 1000 else 1)
    for q, (k, i) in enumerate(atoms):
        c = q % 3
        fd = _central_difference(lambda y: zoo.gb_reference(gb, y, lam, forces=False)[0], x, i, c)
        assert abs(fd - f[i, c]) < FD_TOL * np.abs(f).max(), (k, i, c, fd, f[i, c])


@pytest.mark.parametrize('k', range(len(zoo.PAIR_SETS)))
def test_pair_scan_covers_every_regime_and_border_and_drops_nothing(k):
    system, x, r, dropped = zoo.pair_scan(k)
    p = zoo.PAIR_SETS[k]
    borders = np.array(zoo.pair_borders(p))
    assert dropped == 0 and len(r) == 40 + 2 * len(borders) and len(borders) == 6
    assert np.diff(r).min() > 0.0 and r[0] == zoo.MIN_DISTANCE and np.isclose(r[-1], 1.5)
    assert min(np.abs(rr - borders).min() for rr in r) >= zoo.BORDER_GUARD
    for b in borders:                                           # the two points next to every border
        assert np.sum(np.isclose(r, b - zoo.BORDER_STEP, atol=1e-12)) == 1 and np.sum(np.isclose(r, b + zoo.BORDER_STEP, atol=1e-12)) == 1
    assert np.allclose(np.linalg.norm(x[:, 1] - x[:, 0], axis=-1), r, rtol=1e-14)
    total = dict(zero=0, partial=0, far=0, engulfed=0)
    seen = set()
    for xx in x:
        m = zoo.regime_masks(xx, (p[0], p[2]), (p[1], p[3]))
        for name in total:
            total[name] += int(m[name].sum())
        seen.add(tuple(name for i, j in ((0, 1), (1, 0)) for name in total if m[name][i, j]))
    assert _all_four(total), total
    assert len(seen) >= 4                                       # the two orderings change regime at different borders
    # autograd of the oracle against central differences at every r (the scan is what the analytic dH of both ports is held to)
    gb = system_to_desc(system)['gbsa']
    for xx in x:
        _, f = zoo.gb_reference(gb, xx)
        fd = _central_difference(lambda y: zoo.gb_reference(gb, y, forces=False)[0], xx, 1, 2)
        assert abs(fd - f[1, 2]) < 1e-7 * max(np.abs(f).max(), 1.0), (np.linalg.norm(xx[1]), fd, f[1, 2])
        assert np.allclose(f[0], -f[1], rtol=1e-12, atol=1e-12)


def test_the_other_oracles_see_nothing_in_a_zoo_system():
    for system, x in (zoo.overlap_zoo(150)[:2], zoo.alchemical_zoo(150)[:2]):
        desc = system_to_desc(system)
        zoo.gb_is_the_only_term(desc)
        d0 = dict(desc); d0.pop('gbsa')
        if 'alch_regions' in desc:
            assert not np.any(total_state_energies(d0, x, None, zoo.LADDER_S, zoo.LADDER_E))
            e, f = total_energy_forces(d0, x, None, zoo.LADDER_S[1], zoo.LADDER_E[1])
        else:
            e, f = ForceFieldOracle(d0).energy_forces(x, None)
        assert e == 0.0 and not np.any(f)
    system, x, box = zoo.periodic_zoo()[:3]
    d0 = dict(system_to_desc(system)); d0.pop('gbsa')
    e, f = ForceFieldOracle(d0).energy_forces(x, box)
    assert e == 0.0 and not np.any(f)


@pytest.mark.parametrize('k', range(len(zoo.PAIR_SETS)))
def test_cpu_port_follows_the_oracle_along_the_pair_scan(cpu_lib, k):
    system, x, r, _ = zoo.pair_scan(k)
    eng = HipEngine(lib_path=cpu_lib)
    U, f = zoo.check_against_oracle(eng, system_to_desc(system), x, 1e-9, 1e-8, name='pair scan %d' % k)
    assert np.array_equal(f[:, 0], -f[:, 1])
    eng.close()


@pytest.mark.parametrize('spread', SPREADS)
@pytest.mark.parametrize('n', SIZES)
def test_cpu_port_follows_the_oracle_on_the_overlap_zoo(cpu_lib, n, spread):
    system, x0, _ = zoo.overlap_zoo(n, spread=spread)
    eng = HipEngine(lib_path=cpu_lib)
    zoo.check_against_oracle(eng, system_to_desc(system), zoo.replica_positions(x0, 3 if n < 1000 else 2), 1e-9, 1e-8, name='zoo %d x%g' % (n, spread))
    eng.close()


@pytest.mark.parametrize('spread', SPREADS)
@pytest.mark.parametrize('n', [150, 1100])
def test_cpu_port_follows_the_oracle_on_the_alchemical_zoo(cpu_lib, n, spread):
    system, x0, _ = zoo.alchemical_zoo(n, spread=spread)
    desc = system_to_desc(system)
    assert desc['gbsa']['alchemical'].tolist() == [1 if i % 3 == 0 else 0 for i in range(n)]
    eng = HipEngine(lib_path=cpu_lib)
    zoo.check_against_oracle(eng, desc, zoo.replica_positions(x0, 3), 1e-9, 1e-8, ladder=True, rows_rtol=1e-9, name='alchemical zoo %d x%g' % (n, spread))
    eng.close()


def test_periodic_zoo_straddles_the_faces_in_every_regime_and_keeps_its_guards():
    system, x0, box, (q, radius, scale), redrawn = zoo.periodic_zoo()
    gb = system_to_desc(system)['gbsa']
    assert gb['method'] == 2 and gb['cutoff'] == 1.4 and len(x0) == 130 and set(radius) <= set(zoo.RADII) and set(scale) <= set(zoo.SCALES)
    X = zoo.periodic_replicas(x0, zoo.MAX_REPLICAS, box[0])
    assert X.min() >= 0.0 and X.max() < box[0] and np.abs(X[2] - X[0]).max() > 0.7
    for r, x in enumerate(X):
        assert zoo.cutoff_margin(x, box, 1.4) >= zoo.CUTOFF_GUARD             # none remains next to the cutoff
        assert zoo.border_margin(x, radius, scale, box=box) >= zoo.ZOO_BORDER_GUARD
        masks = zoo.regime_masks(x, radius, scale, box=box, cutoff=1.4)
        assert _all_four({k: int(m.sum()) for k, m in masks.items()})
        across = zoo.straddling(x, box)
        if r == 0:                                               # the hand-placed pairs: joined only by the minimum image
            assert masks['engulfed'][0, 1] and masks['zero'][1, 0] and masks['partial'][2, 3] and masks['partial'][3, 2]
            assert masks['zero'][4, 5] and masks['partial'][5, 4] and across[0, 1] and across[2, 3] and across[4, 5]
            assert all(int((m & across).sum()) > 0 for m in masks.values())
            assert np.linalg.norm(x[0] - x[1]) > 2.5
    assert redrawn > 0                                           # the guards did re-draw atoms


def test_periodic_oracle_forces_are_central_differences_in_every_regime():
    system, x0, box, _, _ = zoo.periodic_zoo()
    gb = system_to_desc(system)['gbsa']
    for r, x in enumerate(zoo.periodic_replicas(x0, 2, box[0])):
        _, f = zoo.gb_reference(gb, x, 1.0, box)
        masks = zoo.regime_masks(x, gb['radius'], gb['scale'], box=box, cutoff=1.4)
        if r == 0:                                               # (the shifted replica has other pairs at the faces, not of every regime)
            masks = {k: m & zoo.straddling(x, box) for k, m in masks.items()}
        atoms = _atoms_of_each_regime(masks, per_regime=2) + [('face', i) for i in range(6)]
        for q, (k, i) in enumerate(atoms):
            c = q % 3
            fd = _central_difference(lambda y: zoo.gb_reference(gb, y, 1.0, box, forces=False)[0], x, i, c)
            assert abs(fd - f[i, c]) < FD_TOL * np.abs(f).max(), (k, i, c, fd, f[i, c])


@pytest.mark.parametrize('case', ['zoo 64', 'alchemical 65', 'periodic'])
def test_f32_restatement_is_the_oracles_formula(case):
    """the helper that measures what f32 costs computes the oracle's energy and forces: to f32 accuracy with room (1e-4 of the energy,
    1e-3 of the largest force component -- it is a check of the formulas, any slip in one is of order one)"""
    if case == 'periodic':
        system, x, box = zoo.periodic_zoo()[:3]
        lam = 1.0
    else:
        n = int(case.split()[1])
        system, x, _ = zoo.alchemical_zoo(n) if case.startswith('alch') else zoo.overlap_zoo(n)
        box, lam = None, (0.4 if case.startswith('alch') else 1.0)
    e_err, f_err = zoo.f32_error(system_to_desc(system)['gbsa'], x, lam, box)
    print(case, 'f32 restatement: energy rel %.3g, force %.3g of the largest component' % (e_err, f_err))
    assert e_err < 1e-4 and f_err < 1e-3
