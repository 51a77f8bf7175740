"""The benchmark test systems of BASELINE.json, built on the System shim.

Mirrors the constructor logic of openmmtools/testsystems.py for
  HarmonicOscillator        :685-802
  LennardJonesFluid         :1872-2030 (+ subrandom_particle_positions :236-289 and the Sobol'
                            generator it calls, sobol.i4_sobol_generate(3, N, 1))
  AlanineDipeptideExplicit  :3465-3527   HostGuestExplicit :3789-3857   DHFRExplicit :3863-3923
The Amber-built systems are loaded from compact .npz system descriptions under
openmmtools_amd/data/, produced from the reference's prmtop/inpcrd files by
tools/convert_amber.py with the parser in openmmtools_amd/amber.py.
"""
import os
import numpy as np
from . import unit
from .system import (System, NonbondedForce, CustomExternalForce, HarmonicBondForce, HarmonicAngleForce,
                     PeriodicTorsionForce, CMMotionRemover, CustomNonbondedForce, CustomBondForce)

DEFAULT_EWALD_ERROR_TOLERANCE = 1.0e-5            # testsystems.py:69
DEFAULT_CUTOFF_DISTANCE = 10.0 * unit.angstroms   # :70
DEFAULT_SWITCH_WIDTH = 1.5 * unit.angstroms       # :71

_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'data')


class TestSystem:
    __test__ = False     # not a pytest class

    def __init__(self, **kwargs):
        self.system = None
        self.positions = None
        self.topology = None


class HarmonicOscillator(TestSystem):
    """3D harmonic oscillator: one particle in U = K/2 ((x-x0)^2 + y^2 + z^2) + U0 (testsystems.py:761-802)."""

    def __init__(self, K=100.0 * unit.kilocalories_per_mole / unit.angstroms ** 2, mass=39.948 * unit.amu,
                 U0=0.0 * unit.kilojoules_per_mole, **kwargs):
        super().__init__(**kwargs)
        system = System()
        system.addParticle(mass)
        positions = np.zeros([1, 3], np.float32).astype(np.float64)
        edge = 1000.0 * unit.nanometers
        system.setDefaultPeriodicBoxVectors([edge, 0, 0], [0, edge, 0], [0, 0, edge])
        force = CustomExternalForce(CustomExternalForce.HARMONIC_EXPRESSION)
        force.addGlobalParameter('testsystems_HarmonicOscillator_K', K)
        force.addGlobalParameter('testsystems_HarmonicOscillator_x0', 0.0)
        force.addGlobalParameter('testsystems_HarmonicOscillator_U0', U0)
        force.addParticle(0, [])
        system.addForce(force)
        self.K, self.mass, self.U0 = K, mass, U0
        self.system, self.positions = system, positions
        self.ndof = 3

    def get_potential_expectation(self, state):
        from .constants import kB
        return 1.5 * kB * state.temperature          # testsystems.py:820


def sobol3(n_points):
    """First n points (seeds 0..n-1) of the 3-D Sobol' sequence in Gray-code order, 30-bit.

    Equivalent to the reference's sobol.i4_sobol_generate(3, n, 1) (sobol.py:136-169, 171-436):
    Bratley-Fox direction numbers, dimension 1 = van der Corput, dimension 2 from x+1 with m = (1),
    dimension 3 from x^2+x+1 with m = (1, 1).  Checked against tests/golden/sobol_512x3.npy.
    """
    bits = 30
    m = np.zeros((3, bits), dtype=np.int64)
    m[0, :] = 1
    m[1, 0] = 1
    for i in range(1, bits):
        m[1, i] = (2 * m[1, i - 1]) ^ m[1, i - 1]
    m[2, 0] = m[2, 1] = 1
    for i in range(2, bits):
        m[2, i] = (2 * m[2, i - 1]) ^ (4 * m[2, i - 2]) ^ m[2, i - 2]
    v = m * (2 ** (bits - 1 - np.arange(bits)))[None, :]          # direction numbers scaled to 2^30
    out = np.zeros((3, n_points))
    q = np.zeros(3, dtype=np.int64)
    for n in range(n_points):
        out[:, n] = q / float(2 ** bits)
        l = 0                                # position of the lowest zero bit of n
        k = n
        while k & 1:
            k >>= 1
            l += 1
        q ^= v[:, l]
    return out


def subrandom_particle_positions(nparticles, box_vectors):
    """testsystems.py:236-289 (method='sobol'): float32 positions, x[dim] * L[dim]."""
    x = np.array(sobol3(nparticles), np.float32)
    positions = np.zeros([nparticles, 3], np.float32)
    for dim in range(3):
        l = np.float32(box_vectors[dim][dim])
        positions[:, dim] = x[dim, :] * l
    return positions.astype(np.float64)


class LennardJonesFluid(TestSystem):
    """Periodic argon-like LJ fluid (testsystems.py:1939-2030): CutoffPeriodic (zero charge), switching
    function from cutoff - switch_width, analytic long-range dispersion correction, Sobol' positions."""

    def __init__(self, nparticles=1000, reduced_density=0.05, mass=39.9 * unit.amu, sigma=3.4 * unit.angstrom,
                 epsilon=0.238 * unit.kilocalories_per_mole, cutoff=None, switch_width=3.4 * unit.angstrom,
                 shift=False, dispersion_correction=True, lattice=False, charge=None, ewaldErrorTolerance=None,
                 **kwargs):
        super().__init__(**kwargs)
        if shift or lattice or charge is not None:
            raise NotImplementedError('shift / lattice / charged LJ fluids are not part of the benchmark configs')
        if cutoff is None:
            cutoff = 3.0 * sigma                                           # :1957-1958
        system = System()
        number_density = reduced_density / sigma ** 3                      # :1970
        volume = nparticles / number_density
        box_edge = volume ** (1.0 / 3.0)
        system.setDefaultPeriodicBoxVectors([box_edge, 0, 0], [0, box_edge, 0], [0, 0, box_edge])
        nb = NonbondedForce()
        nb.setNonbondedMethod(NonbondedForce.CutoffPeriodic)
        nb.setCutoffDistance(cutoff)
        nb.setUseDispersionCorrection(dispersion_correction)
        nb.setUseSwitchingFunction(False)
        if switch_width is not None:
            nb.setUseSwitchingFunction(True)
            nb.setSwitchingDistance(cutoff - switch_width)                 # :1987-1989
        for _ in range(nparticles):
            system.addParticle(mass)
            nb.addParticle(0.0, sigma, epsilon)
        positions = subrandom_particle_positions(nparticles, system.getDefaultPeriodicBoxVectors())
        system.addForce(nb)
        self.system, self.positions = system, positions
        self.ndof = 3 * nparticles


class CustomLennardJonesFluidMixture(TestSystem):
    """testsystems.py:2169-2305: the argon fluid of LennardJonesFluid split between a NonbondedForce and a CustomNonbondedForce with the
    Lennard-Jones string (sigma and epsilon written into it as definitions; the per-particle parameters charge, sigma, epsilon are
    carried and not read).  The first nparticles // 2 particles have their epsilon in the custom force and zero in the NonbondedForce,
    the others the reverse.  Both forces share the cutoff, the switch and the long-range correction."""

    def __init__(self, nparticles=1000, reduced_density=0.05, mass=39.9 * unit.amu, sigma=3.4 * unit.angstrom,
                 epsilon=0.238 * unit.kilocalories_per_mole, cutoff=None, switch_width=None, dispersion_correction=True, **kwargs):
        super().__init__(**kwargs)
        charge = 0.0
        if cutoff is None:
            cutoff = 3.0 * sigma                                           # :2233-2234
        ncustom = int(nparticles / 2)                                      # :2237
        system = System()
        number_density = reduced_density / sigma ** 3
        volume = nparticles / number_density
        box_edge = volume ** (1.0 / 3.0)
        system.setDefaultPeriodicBoxVectors([box_edge, 0, 0], [0, box_edge, 0], [0, 0, box_edge])
        nb = NonbondedForce()
        nb.setNonbondedMethod(NonbondedForce.CutoffPeriodic)
        nb.setCutoffDistance(cutoff)
        nb.setUseDispersionCorrection(dispersion_correction)
        nb.setUseSwitchingFunction(False)
        if switch_width is not None:
            nb.setUseSwitchingFunction(True)
            nb.setSwitchingDistance(cutoff - switch_width)
        system.addForce(nb)
        energy_expression = '4*epsilon*((sigma/r)^12 - (sigma/r)^6);'      # :2265-2267 ('%f': six decimals, as the reference writes them)
        energy_expression += 'sigma = %f;' % sigma
        energy_expression += 'epsilon = %f;' % epsilon
        cnb = CustomNonbondedForce(energy_expression)
        cnb.addPerParticleParameter('charge')
        cnb.addPerParticleParameter('sigma')
        cnb.addPerParticleParameter('epsilon')
        cnb.setNonbondedMethod(CustomNonbondedForce.CutoffPeriodic)
        cnb.setUseLongRangeCorrection(dispersion_correction)
        cnb.setCutoffDistance(cutoff)
        cnb.setUseSwitchingFunction(False)
        if switch_width is not None:
            cnb.setUseSwitchingFunction(True)
            cnb.setSwitchingDistance(cutoff - switch_width)
        system.addForce(cnb)
        for atom_index in range(nparticles):
            system.addParticle(mass)
            if atom_index < ncustom:
                cnb.addParticle([charge, sigma, epsilon])
                nb.addParticle(0.0, sigma, 0.0)
            else:
                cnb.addParticle([0.0, sigma, 0.0])
                nb.addParticle(charge, sigma, epsilon)
        self.system = system
        self.positions = subrandom_particle_positions(nparticles, system.getDefaultPeriodicBoxVectors())
        self.ndof = 3 * nparticles


class WCAFluid(TestSystem):
    """testsystems.py:2312-2386: a Weeks-Chandler-Andersen fluid.  No NonbondedForce: the only pair interaction is a CustomNonbondedForce
    with the shifted Lennard-Jones string cut at its minimum 2^(1/6) sigma (CutoffPeriodic, no switch, no long-range correction).  As in
    the reference the box edge is (nparticles / density)^(1/3) nm, rounded to f32 -- the density is not scaled by sigma^3 there."""

    def __init__(self, nparticles=216, density=0.96, mass=39.9 * unit.amu, epsilon=None, sigma=3.4 * unit.angstrom, **kwargs):
        super().__init__(**kwargs)
        from .constants import kB
        if epsilon is None:
            epsilon = 120.0 * unit.kelvin * kB                             # :2314
        system = System()
        volume = nparticles / density
        length = float(np.float32(1.0) * volume ** (1.0 / 3.0))             # (:2342-2346: the box vectors are f32 arrays)
        system.setDefaultPeriodicBoxVectors([length, 0, 0], [0, length, 0], [0, 0, length])
        for _ in range(nparticles):
            system.addParticle(mass)
        energy_expression = '4.0*epsilon*((sigma/r)^12 - (sigma/r)^6) + epsilon;'      # :2354-2356
        energy_expression += 'sigma = %f;' % sigma
        energy_expression += 'epsilon = %f;' % epsilon
        force = CustomNonbondedForce(energy_expression)
        for _ in range(nparticles):
            force.addParticle([])
        force.setNonbondedMethod(CustomNonbondedForce.CutoffPeriodic)
        rmin = 2.0 ** (1.0 / 6.0) * sigma
        force.setCutoffDistance(rmin)
        system.addForce(force)
        self.system = system
        self.positions = subrandom_particle_positions(nparticles, system.getDefaultPeriodicBoxVectors())
        self.ndof = 3 * nparticles


class StillingerWeberFluid(TestSystem):
    """A Stillinger-Weber fluid on a simple cubic lattice at liquid density.  NOT one of the reference's test systems: it exists to
    exercise CustomManyParticleForce.  model='mW' is monatomic water (Molinero and Moore, J. Phys. Chem. B 113, 4008 (2009)): epsilon
    = 6.189 kcal/mol, sigma = 0.23925 nm, A = 7.049556277, B = 0.6022245584, p = 4, q = 0, gamma = 1.2, a = 1.8, lambda = 23.15,
    cos(theta0) = -1/3, one particle of 18.015 amu per molecule at 33.4 molecules per nm^3.  The two-body term
    A eps (B (sigma/r)^p - (sigma/r)^q) exp(sigma / (r - a sigma)) is a CustomNonbondedForce and the three-body term
    lambda eps (cos theta_jik - cos theta0)^2 exp(gamma sigma / (r_ij - a sigma)) exp(gamma sigma / (r_ik - a sigma)) a
    CustomManyParticleForce in UniqueCentralParticle mode, both CutoffPeriodic with the cutoff a sigma (where every term vanishes with
    all its derivatives).  nparticles must be a cube (64, 512, 4096, ...)."""
    MODELS = dict(mW=dict(epsilon=6.189 * 4.184, sigma=0.23925, A=7.049556277, B=0.6022245584, p=4, q=0, gamma=1.2, a=1.8, lam=23.15,
                          cos0=-1.0 / 3.0, mass=18.015, density=33.4))

    def __init__(self, nparticles=512, model='mW', **kwargs):
        super().__init__(**kwargs)
        from .system import CustomManyParticleForce
        if model not in self.MODELS:
            raise ValueError('StillingerWeberFluid: model %r (the models are %s)' % (model, ', '.join(self.MODELS)))
        m = self.MODELS[model]
        n = int(round(nparticles ** (1.0 / 3.0)))
        if n ** 3 != nparticles:
            raise ValueError('StillingerWeberFluid: nparticles must be a cube, not %d' % nparticles)
        length = float(np.float32((nparticles / m['density']) ** (1.0 / 3.0)))
        cutoff = m['a'] * m['sigma']
        system = System()
        system.setDefaultPeriodicBoxVectors([length, 0, 0], [0, length, 0], [0, 0, length])
        for _ in range(nparticles):
            system.addParticle(m['mass'])
        constants = 'A=%r; B=%r; eps=%r; sigma=%r; a=%r; gamma=%r; lam=%r; cos0=%r' % (m['A'], m['B'], m['epsilon'], m['sigma'], m['a'], m['gamma'],
                                                                                       m['lam'], m['cos0'])
        two = CustomNonbondedForce('A*eps*(B*(sigma/r)^%d-(sigma/r)^%d)*exp(sigma/(r-a*sigma)); %s' % (m['p'], m['q'], constants))
        three = CustomManyParticleForce(3, 'lam*eps*(cos(angle(p2,p1,p3))-cos0)^2*exp(gamma*sigma/(distance(p1,p2)-a*sigma))'
                                           '*exp(gamma*sigma/(distance(p1,p3)-a*sigma)); %s' % constants)
        three.setPermutationMode(CustomManyParticleForce.UniqueCentralParticle)
        for _ in range(nparticles):
            two.addParticle([])
            three.addParticle([], 0)
        for f in (two, three):
            f.setNonbondedMethod(f.CutoffPeriodic)
            f.setCutoffDistance(cutoff)
            system.addForce(f)
        self.system = system
        grid = (np.arange(n) + 0.5) * (length / n)
        self.positions = np.array([[x, y, z] for x in grid for y in grid for z in grid], dtype=np.float64)
        self.ndof = 3 * nparticles


class DoubleWellDimer_WCAFluid(WCAFluid):
    """testsystems.py:2393-2533: ``ndimers`` pairs (2k, 2k + 1) of the WCA fluid joined by the double-well CustomBondForce
    h (1 - ((r - r0 - w) / w)^2)^2.  The reference puts that force in force group 1; here it stays in group 0 beside the WCA force,
    because the engine keeps every custom force of a System in one force group (custom_expr.custom_terms_desc).  As in the reference the bonded pairs keep their WCA interaction (it adds no
    exclusions) and the positions stay in the fluid's order (its reordering step returns them unchanged)."""

    def __init__(self, ndimers=1, nparticles=216, density=0.96, mass=39.9 * unit.amu, epsilon=None, sigma=3.4 * unit.angstrom, h=None,
                 r0=2.0 ** (1.0 / 6.0) * 3.4 * unit.angstrom, w=0.3 * 3.4 * unit.angstrom, **kwargs):
        from .constants import kB
        if h is None:
            h = self._default_h(kB)
        if not (0 <= ndimers <= self._max_bonds(nparticles)):
            raise ValueError("Can't create %s bonds with %s particles" % (str(ndimers), str(nparticles)))
        super().__init__(nparticles, density, mass, epsilon, sigma, **kwargs)
        self.dw_dimer = CustomBondForce('h*(1 - ((r-r0-w)/w)^2)^2')        # :2477-2483
        self.dw_dimer.addPerBondParameter('h')
        self.dw_dimer.addPerBondParameter('r0')
        self.dw_dimer.addPerBondParameter('w')
        self.system.addForce(self.dw_dimer)
        for a, b in self._bond_pairs(ndimers):
            self.dw_dimer.addBond(a, b, [h, r0, w])

    @staticmethod
    def _default_h(kB):
        return 6.0 * 0.824 * 120 * unit.kelvin * kB                        # :2397

    @staticmethod
    def _max_bonds(nparticles):
        return nparticles / 2

    def _bond_pairs(self, nbonds):
        for bond_idx in range(nbonds):
            yield (2 * bond_idx, 2 * bond_idx + 1)


class DoubleWellChain_WCAFluid(DoubleWellDimer_WCAFluid):
    """testsystems.py:2540-2623: a chain of ``nchained`` particles 0, 1, 2, ... joined by double-well bonds in the WCA fluid (nchained 0
    or 1: the plain fluid).  The reference's default barrier here is 6 x 0.824 K kB (without the dimer's factor 120)."""

    def __init__(self, nchained=3, nparticles=216, density=0.96, mass=39.9 * unit.amu, epsilon=None, sigma=3.4 * unit.angstrom, h=None,
                 r0=2.0 ** (1.0 / 6.0) * 3.4 * unit.angstrom, w=0.3 * 3.4 * unit.angstrom, **kwargs):
        nchained = 1 if nchained == 0 else nchained
        super().__init__(nchained - 1, nparticles, density, mass, epsilon, sigma, h, r0, w, **kwargs)

    @staticmethod
    def _default_h(kB):
        return 6.0 * 0.824 * unit.kelvin * kB                              # :2543

    @staticmethod
    def _max_bonds(nparticles):
        return nparticles - 1

    def _bond_pairs(self, nbonds):
        for bond_idx in range(nbonds):
            yield (bond_idx, bond_idx + 1)


class IdealGas(TestSystem):
    """testsystems.py:2631-2735: non-interacting particles in a periodic box of volume N kT / p with a null periodic
    NonbondedForce (so that a barostat can act): <V> = (N + 1) kT / p under the Monte Carlo barostat, <U> = 0."""

    def __init__(self, nparticles=216, mass=39.9 * unit.amu, temperature=298.0 * unit.kelvin, pressure=1.0 * unit.atmosphere,
                 volume=None, **kwargs):
        super().__init__(**kwargs)
        from . import constants
        if volume is None:
            volume = nparticles * constants.kB * float(unit.to_md(temperature)) / float(unit.to_md(pressure))      # nm^3, :2664-2665
        length = float(unit.to_md(volume)) ** (1.0 / 3.0)
        system = System()
        system.setDefaultPeriodicBoxVectors([length, 0, 0], [0, length, 0], [0, 0, length])
        nb = NonbondedForce()
        nb.setNonbondedMethod(NonbondedForce.CutoffPeriodic)                # :2678-2682: charge 0, sigma 1 nm, epsilon 0
        nb.setCutoffDistance(min(1.0, 0.45 * length))
        nb.setUseDispersionCorrection(False)
        for _ in range(nparticles):
            system.addParticle(mass)
            nb.addParticle(0.0, 1.0, 0.0)
        system.addForce(nb)
        self.system, self.positions = system, subrandom_particle_positions(nparticles, system.getDefaultPeriodicBoxVectors())
        self.ndof = 3 * nparticles


def _load_npz_system(name):
    path = os.path.join(_DATA, name + '.npz')
    if not os.path.exists(path):
        raise FileNotFoundError('%s missing: run tools/convert_amber.py where the reference data exists' % path)
    z = np.load(path)
    system = System()
    for m in z['mass']:
        system.addParticle(float(m))
    box = z['box']
    system.setDefaultPeriodicBoxVectors([box[0], 0, 0], [0, box[1], 0], [0, 0, box[2]])
    bf = HarmonicBondForce()
    for (i, j), (r0, k) in zip(z['bond_atoms'], z['bond_params']):
        bf.addBond(i, j, r0, k)
    af = HarmonicAngleForce()
    for (i, j, k3), (th, k) in zip(z['angle_atoms'], z['angle_params']):
        af.addAngle(i, j, k3, th, k)
    tf = PeriodicTorsionForce()
    for (i, j, k3, l), (n, ph, k) in zip(z['torsion_atoms'], z['torsion_params']):
        tf.addTorsion(i, j, k3, l, int(n), ph, k)
    nb = NonbondedForce()
    for q, s, e in zip(z['charge'], z['sigma'], z['epsilon']):
        nb.addParticle(q, s, e)
    nb.exceptions = [(int(a), int(b), float(p[0]), float(p[1]), float(p[2]))
                     for (a, b), p in zip(z['exception_atoms'], z['exception_params'])]
    for (i, j), d in zip(z['constraint_atoms'], z['constraint_dist']):
        system.addConstraint(i, j, d)
    for f in (bf, af, tf, nb):
        system.addForce(f)
    system.addForce(CMMotionRemover(1))            # prmtop.createSystem default removeCMMotion=True
    positions = z['positions'].astype(np.float64)
    velocities = z['velocities'].astype(np.float64) if 'velocities' in z.files else None
    return system, nb, positions, velocities, z


class _AmberExplicit(TestSystem):
    _name = None

    def __init__(self, constraints='HBonds', rigid_water=True, nonbondedCutoff=DEFAULT_CUTOFF_DISTANCE,
                 use_dispersion_correction=True, nonbondedMethod='PME', hydrogenMass=None,
                 switch_width=DEFAULT_SWITCH_WIDTH, ewaldErrorTolerance=DEFAULT_EWALD_ERROR_TOLERANCE, **kwargs):
        super().__init__(**kwargs)
        if constraints != 'HBonds' or not rigid_water or hydrogenMass is not None:
            raise NotImplementedError('only constraints=HBonds, rigid_water=True, no HMR (the testsystem defaults)')
        system, nb, positions, velocities, z = _load_npz_system(self._name)
        method = {'PME': NonbondedForce.PME, 'CutoffPeriodic': NonbondedForce.CutoffPeriodic}[nonbondedMethod]
        nb.setNonbondedMethod(method)
        nb.setCutoffDistance(nonbondedCutoff)
        nb.setUseDispersionCorrection(use_dispersion_correction)
        nb.setEwaldErrorTolerance(ewaldErrorTolerance)
        if switch_width is not None:                                       # testsystems.py:3515-3517
            nb.setUseSwitchingFunction(True)
            nb.setSwitchingDistance(nonbondedCutoff - switch_width)
        self.system, self.positions, self.velocities = system, positions, velocities
        self.residue_names = [str(s) for s in z['residue_names']] if 'residue_names' in z.files else None


class AlanineDipeptideExplicit(_AmberExplicit):
    """testsystems.py:3465-3527: ACE-ALA-NME + 749 TIP3P waters, 2269 atoms, PME."""
    _name = 'alanine-dipeptide-explicit'


class AlanineDipeptideVacuum(TestSystem):
    """testsystems.py:3352-3388: ACE-ALA-NME (22 atoms) without solvent -- prmtop.createSystem(implicitSolvent=None, constraints=HBonds,
    nonbondedCutoff=None): NonbondedForce with NoCutoff, no periodic box, CMMotionRemover."""

    def __init__(self, constraints='HBonds', hydrogenMass=None, **kwargs):
        super().__init__(**kwargs)
        if constraints != 'HBonds' or hydrogenMass is not None:
            raise NotImplementedError('only constraints=HBonds, no HMR (the testsystem defaults)')
        system, nb, positions, velocities, z = _load_npz_system('alanine-dipeptide-vacuum')
        nb.setNonbondedMethod(NonbondedForce.NoCutoff)
        self.system, self.positions, self.velocities = system, positions, None
        self.residue_names = [str(s) for s in z['residue_names']] if 'residue_names' in z.files else None


class HostGuestVacuum(TestSystem):
    """testsystems.py:3660-3712: CB7 host + B2 guest (156 atoms) without solvent -- prmtop.createSystem(implicitSolvent=None,
    constraints=HBonds, nonbondedMethod=NoCutoff)."""

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        system, nb, positions, velocities, z = _load_npz_system('cb7-b2-vacuum')
        nb.setNonbondedMethod(NonbondedForce.NoCutoff)
        self.system, self.positions, self.velocities = system, positions, None
        self.residue_names = [str(s) for s in z['residue_names']] if 'residue_names' in z.files else None


class AlanineDipeptideImplicit(AlanineDipeptideVacuum):
    """testsystems.py:3424-3462: the vacuum dipeptide + Generalized-Born implicit solvent.  The reference's default is app.OBC1, which
    current OpenMM builds as a CustomGBForce from its own expression library (not in the reference's tree); what is built here is
    ``implicitSolvent='OBC2'`` = openmm.GBSAOBCForce -- the force the reference's alchemical factory spells out term by term
    (alchemy.py:2144-2225) -- with the topology's own GB radii and screening factors (prmtop RADII / SCREEN, mbondi2), solvent
    dielectric 78.5, solute dielectric 1, ACE surface term.

    ``implicitSolvent='HCT'`` is the Hawkins-Cramer-Truhlar model as a CustomGBForce whose strings are written here: the same
    integral I, B = 1 / (1 / or - I), the self and pair terms of the OBC strings and the ACE surface term.  It uses the same radii and
    screening factors, the file's mbondi2 ones -- not the radii set openmm.app pairs with HCT.  The engine compiles it for the custom
    forces' stack machine (custom_gb.compile_custom_gb)."""

    def __init__(self, implicitSolvent='OBC2', constraints='HBonds', hydrogenMass=None, **kwargs):
        if implicitSolvent not in ('OBC2', 'HCT'):
            raise NotImplementedError("implicitSolvent=%r: only 'OBC2' (openmm.GBSAOBCForce) and 'HCT' (a CustomGBForce) are built" % (implicitSolvent,))
        super().__init__(constraints=constraints, hydrogenMass=hydrogenMass, **kwargs)
        from .system import GBSAOBCForce, CustomGBForce
        z = np.load(os.path.join(_DATA, 'alanine-dipeptide-vacuum.npz'))
        if implicitSolvent == 'HCT':
            gb = CustomGBForce()
            for name in ('charge', 'radius', 'scale'):
                gb.addPerParticleParameter(name)
            gb.addGlobalParameter('solventDielectric', 78.5)
            gb.addGlobalParameter('soluteDielectric', 1.0)
            gb.addComputedValue('I', 'step(r+sr2-or1)*0.5*(1/L-1/U+0.25*(r-sr2^2/r)*(1/(U^2)-1/(L^2))+0.5*log(L/U)/r+C);'
                                'U=r+sr2; C=2*(1/or1-1/L)*step(sr2-r-or1); L=max(or1,D); D=abs(r-sr2); sr2=scale2*or2;'
                                'or1=radius1-0.009; or2=radius2-0.009', CustomGBForce.ParticlePairNoExclusions)
            gb.addComputedValue('B', '1/(1/or-I); or=radius-0.009', CustomGBForce.SingleParticle)
            gb.addEnergyTerm('28.3919551*(radius+0.14)^2*(radius/B)^6-0.5*138.935485*(1/soluteDielectric-1/solventDielectric)*charge^2/B',
                             CustomGBForce.SingleParticle)
            gb.addEnergyTerm('-138.935485*(1/soluteDielectric-1/solventDielectric)*charge1*charge2/f; f=sqrt(r^2+B1*B2*exp(-r^2/(4*B1*B2)))',
                             CustomGBForce.ParticlePairNoExclusions)
            for q, r, sc in zip(z['charge'], z['gb_radii'], z['gb_screen']):
                gb.addParticle([q, r, sc])
            self.system.addForce(gb)
            return
        gb = GBSAOBCForce()
        for q, r, sc in zip(z['charge'], z['gb_radii'], z['gb_screen']):
            gb.addParticle(q, r, sc)
        self.system.addForce(gb)


class HostGuestExplicit(_AmberExplicit):
    """testsystems.py:3789-3857: CB7 + B2 guest + 1445 TIP3P waters, 4491 atoms."""
    _name = 'cb7-b2-explicit'


class DHFRExplicit(_AmberExplicit):
    """testsystems.py:3863-3923: DHFR (JAC benchmark), 23558 atoms, positions and velocities from JAC.inpcrd."""
    _name = 'dhfr-explicit'


class CustomGBForceSystem(TestSystem):
    """A periodic system of ions with a CustomGBForce (testsystems.py:4279-4389, after OpenMM's TestReferenceCustomGBForce.cpp): 70 pairs
    of +1 / -1 particles of 39.9 amu in a 10 nm box, a CutoffPeriodic NonbondedForce and an OBC2 CustomGBForce, both with a 2 nm cutoff;
    radius 0.2 / 0.1 nm, scale 0.5 for the first half of the particles and 0.8 for the rest; Sobol' positions."""

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        from .system import CustomGBForce
        n_molecules = 70
        n_particles = n_molecules * 2
        box_size = 10.0 * unit.nanometers
        mass = 39.9 * unit.amu
        sigma = 3.350 * unit.angstrom
        epsilon = 0.001603 * unit.kilojoule_per_mole
        cutoff = 2.0 * unit.nanometers
        system = System()
        for _ in range(n_particles):
            system.addParticle(mass)
        system.setDefaultPeriodicBoxVectors([box_size, 0.0, 0.0], [0.0, box_size, 0.0], [0.0, 0.0, box_size])
        nonbonded = NonbondedForce()
        nonbonded.setNonbondedMethod(NonbondedForce.CutoffPeriodic)
        nonbonded.setCutoffDistance(cutoff)
        custom = CustomGBForce()
        custom.setNonbondedMethod(CustomGBForce.CutoffPeriodic)
        custom.setCutoffDistance(cutoff)
        custom.addPerParticleParameter("charge")
        custom.addPerParticleParameter("radius")
        custom.addPerParticleParameter("scale")
        custom.addGlobalParameter("testsystems_CustomGBForceSystem_solventDielectric", 80.0)
        custom.addGlobalParameter("testsystems_CustomGBForceSystem_soluteDielectric", 1.0)
        custom.addComputedValue("I", "step(r+sr2-or1)*0.5*(1/L-1/U+0.25*(1/U^2-1/L^2)*(r-sr2*sr2/r)+0.5*log(L/U)/r+C);"
                                "U=r+sr2;"
                                "C=2*(1/or1-1/L)*step(sr2-r-or1);"
                                "L=max(or1, D);"
                                "D=abs(r-sr2);"
                                "sr2 = scale2*or2;"
                                "or1 = radius1-0.009; or2 = radius2-0.009", CustomGBForce.ParticlePairNoExclusions)
        custom.addComputedValue("B", "1/(1/or-tanh(1*psi-0.8*psi^2+4.85*psi^3)/radius);"
                                "psi=I*or; or=radius-0.009", CustomGBForce.SingleParticle)
        energy_expression = '28.3919551*(radius+0.14)^2*(radius/B)^6-0.5*138.935485*(1/soluteDielectric-1/solventDielectric)*charge^2/B;'
        energy_expression += 'solventDielectric = testsystems_CustomGBForceSystem_solventDielectric;'
        energy_expression += 'soluteDielectric = testsystems_CustomGBForceSystem_soluteDielectric;'
        custom.addEnergyTerm(energy_expression, CustomGBForce.SingleParticle)
        energy_expression = '-138.935485*(1/soluteDielectric-1/solventDielectric)*charge1*charge2/f;'
        energy_expression += 'f=sqrt(r^2+B1*B2*exp(-r^2/(4*B1*B2)));'
        energy_expression += 'solventDielectric = testsystems_CustomGBForceSystem_solventDielectric;'
        energy_expression += 'soluteDielectric = testsystems_CustomGBForceSystem_soluteDielectric;'
        custom.addEnergyTerm(energy_expression, CustomGBForce.ParticlePairNoExclusions)
        for i in range(n_molecules):
            scale = 0.5 if i < n_molecules / 2 else 0.8
            for charge, radius in ((1.0 * unit.elementary_charge, 0.2 * unit.nanometers), (-1.0 * unit.elementary_charge, 0.1 * unit.nanometers)):
                nonbonded.addParticle(charge, sigma, epsilon)
                custom.addParticle([charge, radius, scale])
        system.addForce(nonbonded)
        system.addForce(custom)
        self.system, self.positions = system, subrandom_particle_positions(n_particles, system.getDefaultPeriodicBoxVectors())


# ---- water boxes (testsystems.py:2828-3170) --------------------------------------------------------------------------------------
# The published rigid geometries and parameters of the water models, as data (nm, degrees, e, kJ/mol, amu).  No openmm.app here: the
# box is built on a lattice at liquid density.  r_OM: distance of the TIP4P-Ew charge site from the oxygen along the HOH bisector;
# r_OL / LOL: distance of a TIP5P lone pair from the oxygen and the angle between the two (Horn et al. 2004; Mahoney & Jorgensen 2000).
WATER_MODELS = {
    'tip3p':   dict(r_OH=0.09572, HOH=104.52, q_H=0.417, sigma_O=0.31507524065751241, eps_O=0.635968),
    'spce':    dict(r_OH=0.1, HOH=109.47, q_H=0.4238, sigma_O=0.31657195050398818, eps_O=0.6497752),
    'tip4pew': dict(r_OH=0.09572, HOH=104.52, q_H=0.52422, sigma_O=0.316435, eps_O=0.680946, r_OM=0.0125),
    'tip5p':   dict(r_OH=0.09572, HOH=104.52, q_H=0.241, sigma_O=0.312, eps_O=0.66944, r_OL=0.07, LOL=109.47),
}
WATER_MASS_O, WATER_MASS_H = 15.99943, 1.007947
WATER_NUMBER_DENSITY = 33.4        # molecules per nm^3 (0.997 g/cm^3)


def water_site_weights(model):
    """The virtual sites of one water of ``model`` as (class name, weights) from the published geometry: () for the three-site
    models; TIP4P-Ew: a three-particle average over (O, H1, H2) with w_H = r_OM / (2 r_OH cos(HOH/2)), w_O = 1 - 2 w_H; TIP5P: two
    out-of-plane sites with w12 = w13 = -r_OL cos(LOL/2) / (2 r_OH cos(HOH/2)) and wcross = +- r_OL sin(LOL/2) / (r_OH^2 sin HOH)."""
    m = WATER_MODELS[model]
    half = 0.5 * m['HOH'] * unit.degrees
    if 'r_OM' in m:
        w_h = m['r_OM'] / (2.0 * m['r_OH'] * np.cos(half))
        return (('ThreeParticleAverageSite', (1.0 - 2.0 * w_h, w_h, w_h)),)
    if 'r_OL' in m:
        lone = 0.5 * m['LOL'] * unit.degrees
        w = -m['r_OL'] * np.cos(lone) / (2.0 * m['r_OH'] * np.cos(half))
        wc = m['r_OL'] * np.sin(lone) / (m['r_OH'] ** 2 * np.sin(2.0 * half))
        return (('OutOfPlaneSite', (w, w, wc)), ('OutOfPlaneSite', (w, w, -wc)))
    return ()


class WaterBox(TestSystem):
    """testsystems.py:2828-2976: a periodic box of rigid water, ``model`` one of 'tip3p', 'spce', 'tip4pew' (four sites) and 'tip5p'
    (five sites); the reference's constructor arguments and defaults.  The charge site of TIP4P-Ew and the lone pairs of TIP5P are
    virtual sites (System.setVirtualSite).  The reference fills the box with openmm.app's Modeller; here round(33.4 V) molecules
    sit on a cubic lattice, each turned so that its hydrogens keep away from the molecules placed before -- minimise before running.
    Not built here: flexible water (constrained=False) and ions (ionic_strength != 0).  ``ndof`` counts 6 per rigid water: the
    sites are no degrees of freedom."""

    def __init__(self, box_edge=25.0 * unit.angstroms, cutoff=DEFAULT_CUTOFF_DISTANCE, model='tip3p', switch_width=DEFAULT_SWITCH_WIDTH,
                 constrained=True, dispersion_correction=True, nonbondedMethod=NonbondedForce.PME,
                 ewaldErrorTolerance=DEFAULT_EWALD_ERROR_TOLERANCE, positive_ion='Na+', negative_ion='Cl-', ionic_strength=0.0, **kwargs):
        super().__init__(**kwargs)
        from .system import ThreeParticleAverageSite, OutOfPlaneSite
        if model not in WATER_MODELS:
            raise Exception("Specified water model '{}' is not in list of supported models: {}".format(model, str(sorted(WATER_MODELS))))
        if not constrained:
            raise NotImplementedError('WaterBox(constrained=False): flexible water is not built here')
        if ionic_strength != 0.0:
            raise NotImplementedError('WaterBox(ionic_strength=%r): ions are not built here' % (ionic_strength,))
        m = WATER_MODELS[model]
        box_edge, cutoff = float(unit.to_md(box_edge)), float(unit.to_md(cutoff))
        sites = water_site_weights(model)
        per = 3 + len(sites)
        n_waters = max(1, int(round(WATER_NUMBER_DENSITY * box_edge ** 3)))
        half = 0.5 * m['HOH'] * unit.degrees
        d_hh = 2.0 * m['r_OH'] * np.sin(half)
        q_site = -2.0 * m['q_H'] / len(sites) if sites else 0.0
        system = System()
        system.setDefaultPeriodicBoxVectors([box_edge, 0, 0], [0, box_edge, 0], [0, 0, box_edge])
        nb = NonbondedForce()
        nb.setNonbondedMethod(nonbondedMethod)
        nb.setCutoffDistance(cutoff)
        nb.setUseSwitchingFunction(False)
        if switch_width is not None:
            nb.setUseSwitchingFunction(True)
            nb.setSwitchingDistance(cutoff - float(unit.to_md(switch_width)))
        nb.setUseDispersionCorrection(bool(dispersion_correction))
        nb.setEwaldErrorTolerance(ewaldErrorTolerance)
        for w in range(n_waters):
            o = system.addParticle(WATER_MASS_O)
            h1, h2 = system.addParticle(WATER_MASS_H), system.addParticle(WATER_MASS_H)
            nb.addParticle(0.0 if sites else -2.0 * m['q_H'], m['sigma_O'], m['eps_O'])
            nb.addParticle(m['q_H'], 1.0, 0.0)
            nb.addParticle(m['q_H'], 1.0, 0.0)
            system.addConstraint(o, h1, m['r_OH'])
            system.addConstraint(o, h2, m['r_OH'])
            system.addConstraint(h1, h2, d_hh)
            for (cls, weights) in sites:
                s = system.addParticle(0.0)
                nb.addParticle(q_site, 1.0, 0.0)
                system.setVirtualSite(s, ThreeParticleAverageSite(o, h1, h2, *weights) if cls == 'ThreeParticleAverageSite'
                                      else OutOfPlaneSite(o, h1, h2, *weights))
            for a in range(o, o + per):
                for b in range(a + 1, o + per):
                    nb.addException(a, b, 0.0, 1.0, 0.0)
        system.addForce(nb)
        self.system = system
        self.model, self.n_waters, self.sites_per_water = model, n_waters, len(sites)
        self.positions = self._lattice_positions(m, sites, n_waters, box_edge)
        self.ndof = 6 * n_waters

    @staticmethod
    def _lattice_positions(m, sites, n_waters, box_edge):
        from . import virtual_sites
        half = 0.5 * m['HOH'] * unit.degrees
        # one water: O at the origin, the hydrogens in the xy plane about the x axis
        local = np.array([[0.0, 0.0, 0.0], [m['r_OH'] * np.cos(half), m['r_OH'] * np.sin(half), 0.0],
                          [m['r_OH'] * np.cos(half), -m['r_OH'] * np.sin(half), 0.0]])
        side = int(np.ceil(n_waters ** (1.0 / 3.0) - 1e-9))
        cell = box_edge / side
        rng = np.random.RandomState(20041001)
        per = 3 + len(sites)
        pos = np.zeros((n_waters * per, 3))
        placed = np.zeros((0, 3))
        for w in range(n_waters):
            centre = (np.array([w % side, (w // side) % side, w // (side * side)]) + 0.5) * cell
            best, best_d = None, -1.0
            for _ in range(24):
                q = rng.normal(size=4)
                q /= np.linalg.norm(q)
                a, b, c, d = q
                rot = np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                                [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                                [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])
                trial = centre + local @ rot.T
                if len(placed) == 0:
                    best = trial
                    break
                delta = trial[1:, None, :] - placed[None, :, :]
                delta -= box_edge * np.round(delta / box_edge)
                dmin = np.sqrt((delta ** 2).sum(axis=2)).min()
                if dmin > best_d:
                    best, best_d = trial, dmin
            pos[w * per:w * per + 3] = best
            placed = np.vstack([placed, best])
            for k, (cls, weights) in enumerate(sites):
                pos[w * per + 3 + k] = virtual_sites.place(cls, best, weights)
        return pos


class FourSiteWaterBox(WaterBox):
    """testsystems.py:3099-3125: a TIP4P-Ew water box."""

    def __init__(self, *args, **kwargs):
        super().__init__(model='tip4pew', *args, **kwargs)


class FiveSiteWaterBox(WaterBox):
    """testsystems.py:3128-3154: a TIP5P water box."""

    def __init__(self, *args, **kwargs):
        super().__init__(model='tip5p', *args, **kwargs)
