"""The cases of tests/golden/listed_terms_bits.npz: what the listed terms (harmonic bonds and angles, periodic torsions, 1-4 exceptions,
the Ewald exclusion correction) give through the C ABI at every place they are evaluated, compared to the bit.
tests/golden/make_golden_listed_terms_bits.py recorded the file from the commit before the kernels with energies (csrc/forces.hip)
were moved onto the arithmetic of csrc/listed_terms.h; the softened bonded terms of general alchemical regions (csrc/alch_regions.hip)
are recorded with them.  tests/test_listed_terms_bits_gpu.py holds every later commit to these bits; a commit that changes a term on
purpose records the file again.

The file holds results only, packed as in tests/pair_path_bits.py: one uint64 vector per case, an array with a row per atom as its
SHA-256 and the bit view of every 16th atom row, energies whole.  Where several organisations of the same arithmetic must agree (the
listed launch per term or per atom entry, the three places its workgroups can run) there is ONE record: the case evaluates all of them
and requires equal arrays before it returns the first."""
import os
import numpy as np
from openmmtools_amd import testsystems as ts, alchemy
from openmmtools_amd.system import system_to_desc
from pair_path_bits import _bits, _per_atom, _env, pack
from test_forcefield_parity import KB, SEED
from test_alchemical_regions import _alanine_two_regions, LADDER_S, LADDER_E

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'listed_terms_bits.npz')
CASES = ('classes', 'alchemical', 'placement', 'resident', 'regions')
# force groups of (external, bonds, angles, torsions, direct space, reciprocal space): each bonded class and the nonbonded force in a group
# of its own
GROUPS = [0, 1, 2, 3, 4, 4]
MASKS = {'bonds': 1 << 1, 'angles': 1 << 2, 'torsions': 1 << 3, 'nonbonded': 1 << 4,
         'bonds+torsions': (1 << 1) | (1 << 3),         # idle angle lanes inside an atom's run of entries: the segmented scan's hard case
         'all': 0x1f}


def _handle(eng, system, positions, R, n_steps, lam_s=None, lam_e=None, labels=None, splitting='V R R O R R V', ewald_split='auto'):
    """test_forcefield_parity._engine_for with a lambda_electrostatics ladder and velocities that are kept (reassign_velocities=False)"""
    eng.set_system(system_to_desc(system, ewald_split=ewald_split))
    K = R if lam_s is None else len(lam_s)
    eng.set_states(np.full(K, 1.0 / (KB * 300.0)), lam_s, lam_e, None)
    eng.set_integrator(splitting, 0.002, 1.0, n_steps, False, 1e-8)
    eng.seed(SEED)
    rng = np.random.default_rng(3)
    x = np.stack([positions + 0.002 * rng.normal(size=positions.shape) * (r > 0) for r in range(R)])
    box = np.tile(np.diag(system.getDefaultPeriodicBoxVectors()), (R, 1))
    eng.set_replicas(R, 0, x, None, box, np.arange(R) % K if labels is None else labels)
    eng.set_force_groups(GROUPS)
    return eng


def _group_forces(eng):
    return {name: eng.get_forces(groups=mask) for name, mask in MASKS.items()}


def _same(a, b, what):
    differ = [k for k in a if not np.array_equal(a[k], b[k])]
    assert not differ, '%s: %s differ' % (what, differ)


def _with_energies(out, key, eng):
    """every energy of one evaluation, then one step whose first kick takes the forces that evaluation left (their only way out)"""
    rows, U = eng.compute_energies(want_potential=True)
    out[key + 'u_kl'], out[key + 'potential'] = _bits(rows), _bits(U)
    comp = eng.energy_components()
    out[key + 'components'] = _bits([[c[n] for n in sorted(c)] for c in comp])
    assert all(len(c) == 9 for c in comp)
    assert not eng.propagate(0).any()
    x, v = eng.get_replicas()[:2]
    _per_atom(out, key + 'x_one_step_behind', x)
    _per_atom(out, key + 'v_one_step_behind', v)


def _forces_both_ways(out, key, make, *args, **kw):
    """the groups' force-only evaluations, one (term, slot) entry per thread (the default) and one term per thread"""
    eng = _handle(make(ewald_split='auto'), *args, **kw)
    with _env(REMD_LISTED_ATOMS='0'):
        per_term = _handle(make(ewald_split='auto'), *args, **kw)
    f = _group_forces(eng)
    _same(f, _group_forces(per_term), 'REMD_LISTED_ATOMS=0')
    for name in f:
        assert np.abs(f[name]).max() > 1.0
        _per_atom(out, key + 'forces/' + name, f[name])
    return eng


def classes(make):
    """AlanineDipeptideExplicit, PME, R = 2: each class alone, bonds + torsions, everything; then the evaluation with energies"""
    al = ts.AlanineDipeptideExplicit()
    out = {}
    eng = _forces_both_ways(out, 'classes/', make, al.system, al.positions, 2, 1)
    _with_energies(out, 'classes/', eng)
    return out


def alchemical(make):
    """its first 10 atoms alchemical, four states on which both lambdas fall, every replica in another one: the soft-core exception
    (one alchemical atom), the exception charge x lambda_electrostatics, the exclusion correction x lambda or lambda^2"""
    al = ts.AlanineDipeptideExplicit()
    system = alchemy.AbsoluteAlchemicalFactory().create_alchemical_system(al.system, alchemy.AlchemicalRegion(alchemical_atoms=range(10)))
    ladder = dict(lam_s=np.array([1.0, 0.8, 0.5, 0.2]), lam_e=np.array([0.9, 0.6, 0.35, 0.1]), labels=[3, 1, 2])
    out = {}
    eng = _forces_both_ways(out, 'alchemical/', make, system, al.positions, 3, 1, **ladder)
    _with_energies(out, 'alchemical/', eng)
    return out


def placement(make):
    """five steps of the first case with the listed workgroups riding in the spreading launch, in a launch of their own behind the mesh
    launches, and behind the pair kernel: one trajectory"""
    al = ts.AlanineDipeptideExplicit()
    runs = {}
    for name, env in (('ride', dict(REMD_NB_PRIO='1')), ('main', dict(REMD_NB_PRIO='1', REMD_LISTED_RIDE='0')), ('direct', dict(REMD_LISTED_MAIN='0'))):
        with _env(**env):
            eng = _handle(make(ewald_split='auto'), al.system, al.positions, 2, 5)
        assert not eng.propagate(0).any()
        runs[name] = dict(zip('xv', eng.get_replicas()[:2]))
    _same(runs['ride'], runs['main'], 'REMD_LISTED_RIDE=0')
    _same(runs['ride'], runs['direct'], 'REMD_LISTED_MAIN=0')
    out = {}
    _per_atom(out, 'placement/x_after_5_steps', runs['ride']['x'])
    _per_atom(out, 'placement/v_after_5_steps', runs['ride']['v'])
    return out


def resident(make):
    """AlanineDipeptideVacuum, R = 2, ten steps in the resident small-molecule kernel: the listed terms on positions in LDS"""
    al = ts.AlanineDipeptideVacuum()
    eng = _handle(make(ewald_split='reference'), al.system, al.positions, 2, 10, ewald_split='reference')
    assert not eng.propagate(0).any()
    x, v = eng.get_replicas()[:2]
    out = {}
    _per_atom(out, 'resident/x_after_10_steps', x)
    _per_atom(out, 'resident/v_after_10_steps', v)
    return out


# lambda_bonds, lambda_angles, lambda_torsions of the dipeptide's region on the six states of LADDER_S; the replicas sit in states 1, 2, 3
REGION_BONDED = np.array([[1.0, 0.9, 0.7, 0.5, 0.2, 0.0], [1.0, 0.95, 0.8, 0.6, 0.3, 0.1], [1.0, 0.55, 0.45, 0.25, 0.0, 0.0]])
REGION_LABELS = [1, 2, 3]


def regions(make):
    """the softened-bonded row of tests/test_alchemical_regions.py: every angle and proper torsion of the dipeptide and three of its bonds
    scaled by their region's lambdas, none of them 0 or 1 where a replica sits"""
    own = REGION_BONDED[:, REGION_LABELS]
    assert np.all((own > 0) & (own < 1)) and len(set(own.reshape(-1))) == own.size
    al, system, _ = _alanine_two_regions(dict(), frozenset(), alchemical_torsions=True, alchemical_angles=True, alchemical_bonds=[0, 2, 5])
    desc = system_to_desc(system, ewald_split='reference')
    terms = desc['alch_regions']
    assert len(terms['torsion_atoms']) > 10 and len(terms['angle_atoms']) > 10 and len(terms['bond_atoms']) == 3
    eng = make(ewald_split='reference')
    eng.set_system(desc)
    K, R = len(LADDER_S), len(REGION_LABELS)
    eng.set_states(np.full(K, 1.0 / (KB * 300.0)))
    eng.set_region_lambdas(LADDER_S, LADDER_E)
    bonded = np.ones((3, K, 2))
    bonded[:, :, 0] = REGION_BONDED
    eng.set_region_bonded_lambdas(*bonded)
    eng.set_integrator('V R R O R R V', 0.002, 1.0, 5, True, 1e-8)
    eng.seed(SEED)
    x = np.stack([al.positions + 0.001 * r * np.random.default_rng(r).normal(size=al.positions.shape) for r in range(R)])
    box = np.tile(np.diag(system.getDefaultPeriodicBoxVectors()), (R, 1))
    eng.set_replicas(R, 0, x, None, box, np.array(REGION_LABELS))
    out = {}
    rows, U = eng.compute_energies(want_potential=True)
    out['regions/u_kl'], out['regions/potential'] = _bits(rows), _bits(U)
    _per_atom(out, 'regions/forces', eng.get_forces())
    return out


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
