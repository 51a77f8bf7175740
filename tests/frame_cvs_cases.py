"""The case table of the collective variables of stored frames, shared by tests/test_frame_cvs_cpu.py (frame_cvs_numpy), by
tests/test_frame_cvs_gpu.py (_engine.frame_cvs) and by tools/record_frame_cv_errors.py.  Every case is seeded; its reference
(tests/frame_cvs_oracle.py) is computed once per process and shared.

Bounds.  A case in general position holds device and numpy within GENERAL_BOUND = 1e-10 (nm, rad) of the oracle: the project's
standing bar for f64 sums in a fixed order.  The degenerate families -- angles within 1e-6 of 0 or pi, where acos amplifies the rounding
of the cosine by 1 / theta; dihedrals at the branch cut, compared modulo 2 pi; an RMSD at the floor -- are bounded at 4 x the largest error
of the DEVICE against the oracle that tools/record_frame_cv_errors.py recorded for the family on an MI355X
(profiles/frame_cv_errors.txt).  The yardstick is the oracle throughout, never the output of the code under test."""
import functools
import os

import numpy as np

import frame_cvs_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERRORS_FILE = os.path.join(ROOT, 'profiles', 'frame_cv_errors.txt')
GENERAL_BOUND = 1e-10
FAMILIES = ('angle-end', 'dihedral-cut', 'rmsd-floor')
SIZES = (1, 2, 63, 64, 65, 257)             # lane-stride edges of the wavefront kernel; 257: past the RMSD kernel's block of 256


class Case:
    """name, pos [F][n_atoms][3] f32, box [F][3] f32 or None, masses [n_atoms], variables (the oracle's plain tuples),
    family: None (general position) or one of FAMILIES"""

    def __init__(self, name, pos, box, masses, variables, family=None):
        self.name, self.pos, self.box, self.masses, self.variables, self.family = name, pos, box, masses, variables, family

    @property
    def modulo_2pi(self):
        return self.family == 'dihedral-cut'

    def descriptors(self, an):
        """the variables as descriptors of multistate.analysis"""
        out = []
        for var in self.variables:
            if var[0] == 'rmsd':
                out.append(an.RMSDCV(var[1], var[2]))
                continue
            kind, groups, weights, periodic = var
            if kind == 'distance':
                out.append(an.DistanceCV(groups[0], groups[1], weights1=weights[0], weights2=weights[1], periodic=periodic))
            elif kind == 'angle':
                out.append(an.AngleCV(*groups, weights=None if all(w is None for w in weights) else weights, periodic=periodic))
            else:
                out.append(an.DihedralCV(*groups, weights=None if all(w is None for w in weights) else weights, periodic=periodic))
        return out


def _sizes(periodic, F):
    """Nine mixed variables over groups of 1, 2, 63, 64, 65 and 257 atoms scattered through the atom list, per-frame boxes that
    differ, every atom of a centroid group wrapped into the box one by one (the group of 63 sits on the x face and is split by it);
    weights None (masses), explicit and unequal."""
    rng = np.random.default_rng(20250117)
    n_atoms = sum(SIZES) + 257 + 3 + 10
    order = rng.permutation(n_atoms)
    g, at = {}, 0
    for n in SIZES:
        g[n] = [int(a) for a in order[at:at + n]]; at += n
    r257 = [int(a) for a in order[at:at + 257]]; at += 257
    r3 = [int(a) for a in order[at:at + 3]]
    masses = rng.uniform(1.0, 32.0, n_atoms)
    reference = rng.uniform(-0.8, 0.8, (n_atoms, 3))
    box = (np.array([3.0, 3.3, 2.8]) + rng.uniform(-0.1, 0.1, (9, 3))).astype(np.float32)
    pos = rng.uniform(0.0, 2.5, (9, n_atoms, 3))
    frac = {n: rng.uniform(0.1, 0.9, 3) for n in SIZES}
    for f in range(9):
        L = box[f].astype(np.float64)
        for n in SIZES:
            centre = frac[n] * L + rng.normal(size=3) * 0.1
            if n == 63:
                centre[0] = L[0] - 0.05
            x = centre + rng.uniform(-0.3, 0.3, (n, 3))
            pos[f, g[n]] = x - L * np.floor(x / L)
        for atoms in (r257, r3):
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            q = q * np.sign(np.linalg.det(q))
            pos[f, atoms] = 0.5 * L + reference[atoms] @ q.T + rng.normal(size=(len(atoms), 3)) * 0.05
    w = lambda n: [float(v) for v in rng.uniform(0.5, 2.0, n)]
    variables = [
        ('distance', [g[1], g[257]], [None, None], periodic),
        ('distance', [g[2], g[63]], [[1.0, 3.0], w(63)], periodic),
        ('distance', [g[64], g[65]], [None, None], periodic),
        ('angle', [g[1], g[64], g[65]], [None, None, None], periodic),
        ('angle', [g[2], g[63], g[257]], [None, w(63), w(257)], periodic),
        ('dihedral', [g[1], g[2], g[63], g[64]], [None, None, None, None], periodic),
        ('dihedral', [g[65], g[257], g[64], g[63]], [w(65), None, w(64), None], periodic),
        ('rmsd', reference, r257),
        ('rmsd', reference, r3),
    ]
    name = 'sizes' if periodic else 'sizes-unimaged'
    return Case(name, pos[:F].astype(np.float32), box[:F], masses, variables)


def _far():
    """groups 40 nm from the origin, where an f32 position has a spacing of 4e-6 nm: nothing is lost to the offset"""
    rng = np.random.default_rng(40)
    n_atoms = 20
    pos = (40.0 + rng.uniform(-0.4, 0.4, (3, n_atoms, 3))).astype(np.float32)
    reference = rng.uniform(-0.4, 0.4, (n_atoms, 3))
    variables = [('distance', [list(range(0, 10)), list(range(10, 15))], [None, None], False),
                 ('angle', [[0, 1], [5, 6, 7], [12]], [None, None, None], False),
                 ('dihedral', [[0], [5], [10], [15]], [None, None, None, None], False),
                 ('rmsd', reference, list(range(3, 13)))]
    return Case('far', pos, None, rng.uniform(1.0, 16.0, n_atoms), variables)


def _exact():
    """One frame (F = 1): a dihedral at exactly 0 (cis, planar), coincident atoms and two identical groups (distance exactly 0)"""
    pos = np.zeros((1, 12, 3), dtype=np.float32)
    pos[0, :4] = [[1, 0, 0], [0, 0, 0], [0, 1, 0], [1, 1, 0]]
    pos[0, 4] = pos[0, 5] = [0.25, -1.5, 2.0]
    pos[0, 6:12] = np.random.default_rng(3).uniform(-1.0, 1.0, (6, 3))
    variables = [('dihedral', [[0], [1], [2], [3]], [None] * 4, False),
                 ('distance', [[4], [5]], [None, None], False),
                 ('distance', [[6, 7, 8], [6, 7, 8]], [None, None], False),
                 ('distance', [[6, 7, 8], [9, 10, 11]], [[1.0, 2.0, 3.0], None], False)]
    return Case('exact', pos, None, np.linspace(1.0, 12.0, 12), variables)


def _rmsd_shapes():
    """RMSDs of 3 particles and of mirrored, planar and collinear sets (the two largest eigenvalues of Horn's matrix coincide for the
    planar and the collinear set: any vector of their eigenspace gives the same superposition)"""
    rng = np.random.default_rng(77)
    n_atoms = 3 + 20 + 12 + 8
    reference = rng.uniform(-0.6, 0.6, (n_atoms, 3))
    three, mirrored, planar, collinear = list(range(0, 3)), list(range(3, 23)), list(range(23, 35)), list(range(35, 43))
    reference[planar, 2] = 0.0
    reference[collinear] = np.outer(np.linspace(-0.7, 0.9, 8) ** 3, [1.0, 0.0, 0.0])
    pos = np.zeros((3, n_atoms, 3))
    for f in range(3):
        for atoms in (three, mirrored, planar, collinear):
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            q = q * np.sign(np.linalg.det(q))
            y = reference[atoms].copy()
            if atoms is mirrored:
                y[:, 0] = -y[:, 0]
            noise = rng.normal(size=y.shape) * 0.03
            if atoms is planar:
                noise[:, 2] = 0.0                        # (the set stays planar)
            if atoms is collinear:
                noise[:, 1:] = 0.0                       # (and this one on its line)
            pos[f, atoms] = (y + noise) @ q.T + rng.uniform(-1.0, 1.0, 3)
    variables = [('rmsd', reference, three), ('rmsd', reference, mirrored), ('rmsd', reference, planar), ('rmsd', reference, collinear)]
    return Case('rmsd-shapes', pos.astype(np.float32), None, np.ones(n_atoms), variables)


def _angle_end():
    """angles of three atoms at exactly 0 and exactly pi (collinear), and within 1e-6 of either end"""
    rng = np.random.default_rng(5)
    F = 18
    pos = np.zeros((F, 3, 3), dtype=np.float32)
    pos[:, 0] = [1.0, 0.0, 0.0]
    pos[0, 2] = [2.0, 0.0, 0.0]
    pos[1, 2] = [-2.0, 0.0, 0.0]
    for f in range(2, F):
        theta, phi = rng.uniform(1e-7, 9e-7), rng.uniform(0.0, 2.0 * np.pi)
        pos[f, 2] = [2.0 if f < 10 else -2.0, 2.0 * theta * np.cos(phi), 2.0 * theta * np.sin(phi)]
    return Case('angle-end', pos, None, np.ones(3), [('angle', [[0], [1], [2]], [None] * 3, False)], family='angle-end')


def _dihedral_cut():
    """dihedrals of four atoms at +pi (trans, planar: the closed end of the range), at -pi + 1e-9, and within 1e-6 of the cut on
    either side"""
    rng = np.random.default_rng(6)
    F = 12
    pos = np.zeros((F, 4, 3), dtype=np.float32)
    pos[:, 0] = [1.0, 0.0, 0.0]
    pos[:, 2] = [0.0, 1.0, 0.0]
    pos[:, 3] = [-1.0, 1.0, 0.0]
    pos[1, 3, 2] = 1e-9
    for f in range(2, F):
        pos[f, 3, 2] = rng.uniform(1e-9, 1e-6) * (1.0 if f % 2 else -1.0)
    return Case('dihedral-cut', pos, None, np.ones(4), [('dihedral', [[0], [1], [2], [3]], [None] * 4, False)], family='dihedral-cut')


def _rmsd_floor():
    """a copy of the reference, turned by a quarter about z and translated, all exactly representable, and the reference itself: the mean
    square deviation is rounding alone, far below 1e-20 nm^2, and the RMSD is 0 through the floor"""
    rng = np.random.default_rng(8)
    n_atoms = 24
    reference = rng.integers(-64, 65, (n_atoms, 3)) / 64.0
    turned = np.stack([-reference[:, 1], reference[:, 0], reference[:, 2]], axis=1) + np.array([2.0, -3.0, 0.5])
    pos = np.stack([turned, reference]).astype(np.float32)
    return Case('rmsd-floor', pos, None, np.ones(n_atoms), [('rmsd', reference, list(range(2, 22)))], family='rmsd-floor')


@functools.lru_cache(maxsize=None)
def all_cases():
    return (_sizes(True, 9), _sizes(False, 2), _far(), _exact(), _rmsd_shapes(), _angle_end(), _dihedral_cut(), _rmsd_floor())


def case(name):
    return {c.name: c for c in all_cases()}[name]


@functools.lru_cache(maxsize=None)
def reference(name):
    """the oracle's values [F][n] of a case (mpmath numbers; floats for an RMSD), computed once per process"""
    c = case(name)
    return oracle.evaluate(c.variables, c.pos, c.box, c.masses)


def errors(name, values):
    """|values - oracle| [F][n] of a case"""
    return oracle.errors(values, reference(name), modulo_2pi=case(name).modulo_2pi)


@functools.lru_cache(maxsize=None)
def recorded():
    """{family: the largest recorded error of the device against the oracle} from profiles/frame_cv_errors.txt"""
    out = {}
    with open(ERRORS_FILE) as fh:
        for line in fh:
            parts = line.split()
            if parts and parts[0] == 'row':
                out[parts[2]] = max(out.get(parts[2], 0.0), float(parts[3]))
    missing = [f for f in FAMILIES if f not in out]
    assert not missing, 'profiles/frame_cv_errors.txt records no error for %s' % missing
    return out


def bound(name):
    c = case(name)
    return GENERAL_BOUND if c.family is None else 4.0 * recorded()[c.family]


# ---- a small store for the analyzer's round trip ---------------------------------------------------------------------------------
STORE_ANALYSIS_PARTICLES = (7, 2, 9, 4, 0, 5)          # a strict, unsorted subset of the ten particles


def write_store(path, periodic=True, n_it=25, analysis_particles=STORE_ANALYSIS_PARTICLES, position_interval=1):
    """A hand-written store of three replicas that walk three states over ten particles of unequal masses, the analysis particles a
    strict, unsorted subset, per-frame boxes that differ: (reporter, System, positions [it][R][10][3] f32, box [it][R][3] f32 or None)"""
    from openmmtools_amd import states, unit
    from openmmtools_amd.system import System, HarmonicBondForce
    from openmmtools_amd.multistate import MultiStateReporter
    rng = np.random.default_rng(99)
    R = K = 3
    system = System()
    for m in (12.0, 1.0, 16.0, 14.0, 12.0, 1.0, 32.0, 12.0, 16.0, 1.0):
        system.addParticle(m)
    bond = HarmonicBondForce()
    bond.addBond(0, 1, 0.1, 1000.0)
    system.addForce(bond)
    sts = [states.ThermodynamicState(system, T * unit.kelvin) for T in (300.0, 330.0, 360.0)]
    positions = rng.uniform(0.0, 2.0, (n_it, R, 10, 3)).astype(np.float32)
    box = (2.0 + rng.uniform(-0.2, 0.2, (n_it, R, 3))).astype(np.float32) if periodic else None
    E = rng.exponential(2.0, (n_it, R))
    energies = E[:, :, None] * np.array([1.0, 300.0 / 330.0, 300.0 / 360.0])[None, None, :]
    state_indices = np.stack([rng.permutation(K) for _ in range(n_it)])
    rep = MultiStateReporter(str(path), open_mode='w', checkpoint_interval=50, analysis_particle_indices=analysis_particles,
                             position_interval=position_interval, layout='records')
    rep.initialize(R, K, 0, 10)
    rep.write_thermodynamic_states(sts, [])
    for it in range(n_it):
        rep.write_sampler_states([states.SamplerState(positions[it, r].astype(np.float64),
                                                      box_vectors=None if box is None else np.diag(box[it, r].astype(np.float64)))
                                  for r in range(R)], it)
        rep.write_replica_thermodynamic_states(state_indices[it], it)
        rep.write_energies(energies[it], np.ones((R, K), dtype=np.int8), np.zeros((R, 0)), it)
        rep.write_mixing_statistics(np.zeros((K, K), dtype=np.int32), np.zeros((K, K), dtype=np.int32), it)
        rep.write_timestamp(it)
        rep.write_last_iteration(it)
    return rep, system, positions, box


def store_variables(an, periodic=True):
    """four variables over the analysis particles of write_store, in System numbering"""
    reference = np.random.default_rng(100).uniform(-0.5, 0.5, (10, 3))
    return [an.DihedralCV(0, 4, 5, 9, periodic=periodic), an.DistanceCV([7, 2], [9, 4, 0], periodic=periodic),
            an.AngleCV([2, 5], 7, [0, 9], weights=[[1.0, 2.0], None, None], periodic=periodic), an.RMSDCV(reference, [5, 2, 7, 4])]
