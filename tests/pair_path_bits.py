"""The cases of tests/golden/pair_path_bits.npz: what the direct-space pair path of csrc/forces.hip (molecule order, gather, cluster-pair
lists, pair kernel, scatter) gives through the C ABI, compared to the bit.  tests/golden/make_golden_pair_path_bits.py recorded the file
from the commit before the host side of that path got one owner per sorted system (nb_sorted); the device code of the two commits is
byte-identical, so tests/test_pair_path_bits_gpu.py holds every later commit that leaves the kernels alone to these bits, and a commit
that changes them on purpose records the file again.  Two runs of one binary cannot see an argument that is wrong in both; this can.

Every input comes from the seeded helpers of tests/test_forcefield_parity.py, so the file holds results only: one uint64 vector per
case, the arrays of the case in the order of their sorted names.  A double is stored as its uint64 view.  Of an array with a row per
atom ([R][N][3]) the file keeps the SHA-256 of its bytes (4 words) and the bit view of every 16th atom row, so that a difference
still points somewhere; energies are kept whole."""
import contextlib
import hashlib
import os
import numpy as np
from openmmtools_amd import testsystems as ts, alchemy, unit
from openmmtools_amd.system import system_to_desc
from test_forcefield_parity import _engine_for

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pair_path_bits.npz')
CASES = ('split', 'split_alchemical', 'one_system', 'tiles', 'reaction_field', 'phases')
STEPS = 45          # a re-sort of the molecule order (every 40 evaluations) falls inside the run
MD = dict(splitting='V R R O R R V', dt=0.002, n_steps=STEPS)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64)


def _per_atom(out, key, a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    assert a.ndim == 3 and a.shape[2] == 3
    out[key + '/sha256'] = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint64).copy()
    out[key + '/every16th'] = _bits(a[:, ::16])


def _forces_and_energies(out, key, eng):
    rows, U = eng.compute_energies(want_potential=True)
    out[key + 'u_kl'], out[key + 'potential'] = _bits(rows), _bits(U)
    _per_atom(out, key + 'forces', eng.get_forces())


def _propagated(out, key, eng):
    assert not eng.propagate(0).any()
    x, v = eng.get_replicas()[:2]
    _per_atom(out, key + 'x_after_%d_steps' % STEPS, x)
    _per_atom(out, key + 'v_after_%d_steps' % STEPS, v)


@contextlib.contextmanager
def _env(**kw):
    """the engine's switches are read when a handle is made"""
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _alanine():
    al = ts.AlanineDipeptideExplicit()
    return al, system_to_desc(al.system, ewald_split='auto')


def split(make):
    """AlanineDipeptideExplicit, PME at the rebalanced Ewald split, R = 3: two-system gather and list, nonbonded_sci2_kernel, the combined
    scatter; 45 steps through a re-sort; then the SAME handle with R = 2 (everything sized by R is made again)"""
    al, desc = _alanine()
    eng = make(ewald_split='auto')
    _, x, box = _engine_for(eng, al.system, al.positions, R=3, jitter=0.002, desc=desc, **MD)
    out = {}
    _forces_and_energies(out, 'split/R3/', eng)
    _propagated(out, 'split/R3/', eng)
    eng.set_replicas(2, 0, x[:2], None, box[:2], np.arange(2))
    _forces_and_energies(out, 'split/then_R2/', eng)
    return out


def split_alchemical(make):
    """the same system with its first 10 atoms alchemical on a lambda_sterics ladder: the ALCH instantiations and d_rep_lam"""
    al = ts.AlanineDipeptideExplicit()
    system = alchemy.AbsoluteAlchemicalFactory().create_alchemical_system(al.system, alchemy.AlchemicalRegion(alchemical_atoms=range(10)))
    eng = make(ewald_split='auto')
    _engine_for(eng, system, al.positions, R=3, lam_s=np.array([1.0, 0.7, 0.3, 0.0]), labels=[0, 1, 3], jitter=0.002,
                desc=system_to_desc(system, ewald_split='auto'), **MD)
    out = {}
    _forces_and_energies(out, 'split_alchemical/', eng)
    return out


def one_system(make):
    """LennardJonesFluid(500), R = 2, regular launches instead of the resident small-system kernel: gather_positions_kernel,
    build_sci_list_kernel, nonbonded_sci_kernel, the one-system scatter"""
    lj = ts.LennardJonesFluid(nparticles=500)
    with _env(REMD_RESIDENT='0'):
        eng = make()
    _engine_for(eng, lj.system, lj.positions, R=2, jitter=0.01, **MD)
    out = {}
    _forces_and_energies(out, 'one_system/', eng)
    _propagated(out, 'one_system/', eng)
    return out


def tiles(make):
    """the split case on the 64-atom tile kernel (what a list overflow falls back to): it reads the main system's sorted buffers"""
    al, desc = _alanine()
    with _env(REMD_NB_TILES='1'):
        eng = make(ewald_split='auto')
    _engine_for(eng, al.system, al.positions, R=3, jitter=0.002, desc=desc, **MD)
    out = {}
    _forces_and_energies(out, 'tiles/', eng)
    return out


# the smallest box WaterBox fills for a cutoff: its edge has to exceed two cutoffs (0.6 nm, the shortest the suite uses)
RF_EDGE, RF_CUTOFF = 1.25, 0.6


def reaction_field(make):
    """a CutoffPeriodic TIP3P box (charges everywhere, Lennard-Jones on the oxygens only): the split path under NB_RF"""
    box = ts.WaterBox(box_edge=RF_EDGE * unit.nanometers, cutoff=RF_CUTOFF * unit.nanometers, nonbondedMethod=ts.NonbondedForce.CutoffPeriodic)
    eng = make()
    _engine_for(eng, box.system, box.positions, R=2, jitter=0.002, **MD)
    out = {}
    _forces_and_energies(out, 'reaction_field/', eng)
    return out


def phases(make):
    """the split case as two blocks of replicas (set_phases(2), R = 4): the child contexts own their sorted state"""
    al, desc = _alanine()
    eng = make(ewald_split='auto')
    _engine_for(eng, al.system, al.positions, R=4, jitter=0.002, desc=desc, **MD)
    eng.set_phases(2)
    out = {}
    _propagated(out, 'phases/', eng)
    assert eng.phases_active() == 2
    return out


def pack(now):
    return np.concatenate([now[k] for k in sorted(now)])


def assert_same_bits(now, case):
    """the arrays of ``now``, all of one case, against the recorded vector of that case"""
    assert all(k.startswith(case + '/') for k in now)
    gold = np.load(GOLDEN)[case]
    vec = pack(now)
    assert vec.dtype == gold.dtype and vec.shape == gold.shape
    at = np.cumsum([0] + [now[k].size for k in sorted(now)])
    differ = [k for k, lo, hi in zip(sorted(now), at, at[1:]) if not np.array_equal(vec[lo:hi], gold[lo:hi])]
    print('%d arrays of %s, %d differ from the recorded bits %s' % (len(now), case, len(differ), differ[:8]))
    assert not differ
