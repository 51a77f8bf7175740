"""Minimal stand-in for ``openmm.System`` and the Force classes the benchmark test systems use.

The reference's input contract is an ``openmm.System`` wrapped in a ``ThermodynamicState``
(openmmtools/states.py:1494 hashes its XML).  OpenMM is not importable in the build
environment, so this module mirrors the subset of the OpenMM API (same method names and
argument order, md-unit floats instead of Quantities) that openmmtools/testsystems.py uses
for HarmonicOscillator (:761-802), LennardJonesFluid (:1939-2030) and the Amber-built
explicit-solvent systems (:3496-3527, :3818-3857, :3892-3923).  ``system_to_desc`` flattens a
System into the arrays behind ``remd_system_desc`` (include/remd_hip.h).  A real
``openmm.System`` can be converted with ``from_openmm`` where OpenMM exists.
"""
import hashlib
import math
import types
import numpy as np


class Force:
    def __init__(self):
        self._group = 0

    def getForceGroup(self):
        return self._group

    def setForceGroup(self, g):
        self._group = int(g)


class HarmonicBondForce(Force):
    def __init__(self):
        super().__init__()
        self.bonds = []

    def addBond(self, i, j, length, k):
        self.bonds.append((int(i), int(j), float(length), float(k)))
        return len(self.bonds) - 1

    def getNumBonds(self):
        return len(self.bonds)

    def getBondParameters(self, idx):
        return self.bonds[idx]


class HarmonicAngleForce(Force):
    def __init__(self):
        super().__init__()
        self.angles = []

    def addAngle(self, i, j, k, angle, kf):
        self.angles.append((int(i), int(j), int(k), float(angle), float(kf)))
        return len(self.angles) - 1

    def getNumAngles(self):
        return len(self.angles)

    def getAngleParameters(self, idx):
        return self.angles[idx]


class PeriodicTorsionForce(Force):
    def __init__(self):
        super().__init__()
        self.torsions = []

    def addTorsion(self, i, j, k, l, periodicity, phase, kf):
        self.torsions.append((int(i), int(j), int(k), int(l), int(periodicity), float(phase), float(kf)))
        return len(self.torsions) - 1

    def getNumTorsions(self):
        return len(self.torsions)

    def getTorsionParameters(self, idx):
        return self.torsions[idx]


class NonbondedForce(Force):
    NoCutoff, CutoffNonPeriodic, CutoffPeriodic, Ewald, PME = 0, 1, 2, 3, 4

    def __init__(self):
        super().__init__()
        self.particles = []
        self.exceptions = []
        self._method = NonbondedForce.NoCutoff
        self._cutoff = 1.0
        self._use_switch = False
        self._switch = -1.0
        self._dispersion = True
        self._rf_dielectric = 78.3
        self._ewald_tol = 5e-4
        self._pme_params = None
        self._recip_group = -1

    def getReciprocalSpaceForceGroup(self):
        return self._recip_group

    def setReciprocalSpaceForceGroup(self, g):
        """-1 (default): the reciprocal-space part acts in the force group of the force itself."""
        self._recip_group = int(g)

    def addParticle(self, charge, sigma, epsilon):
        self.particles.append((float(charge), float(sigma), float(epsilon)))
        return len(self.particles) - 1

    def getNumParticles(self):
        return len(self.particles)

    def getParticleParameters(self, idx):
        return self.particles[idx]

    def setParticleParameters(self, idx, charge, sigma, epsilon):
        self.particles[idx] = (float(charge), float(sigma), float(epsilon))

    def addException(self, i, j, chargeProd, sigma, epsilon, replace=False):
        i, j = int(i), int(j)
        for n, e in enumerate(self.exceptions):
            if {e[0], e[1]} == {i, j}:
                if not replace:
                    raise ValueError('exception between %d and %d already exists' % (i, j))
                self.exceptions[n] = (i, j, float(chargeProd), float(sigma), float(epsilon))
                return n
        self.exceptions.append((i, j, float(chargeProd), float(sigma), float(epsilon)))
        return len(self.exceptions) - 1

    def getNumExceptions(self):
        return len(self.exceptions)

    def getExceptionParameters(self, idx):
        return self.exceptions[idx]

    def setNonbondedMethod(self, m):
        self._method = int(m)

    def getNonbondedMethod(self):
        return self._method

    def setCutoffDistance(self, d):
        self._cutoff = float(d)

    def getCutoffDistance(self):
        return self._cutoff

    def setUseSwitchingFunction(self, flag):
        self._use_switch = bool(flag)

    def getUseSwitchingFunction(self):
        return self._use_switch

    def setSwitchingDistance(self, d):
        self._switch = float(d)

    def getSwitchingDistance(self):
        return self._switch

    def setUseDispersionCorrection(self, flag):
        self._dispersion = bool(flag)

    def getUseDispersionCorrection(self):
        return self._dispersion

    def setReactionFieldDielectric(self, e):
        self._rf_dielectric = float(e)

    def getReactionFieldDielectric(self):
        return self._rf_dielectric

    def setEwaldErrorTolerance(self, tol):
        self._ewald_tol = float(tol)

    def getEwaldErrorTolerance(self):
        return self._ewald_tol

    def setPMEParameters(self, alpha, nx, ny, nz):
        self._pme_params = (float(alpha), int(nx), int(ny), int(nz))

    def usesPeriodicBoundaryConditions(self):
        return self._method in (NonbondedForce.CutoffPeriodic, NonbondedForce.Ewald, NonbondedForce.PME)


class Continuous1DFunction:
    """openmm.Continuous1DFunction: ``values`` are samples at n uniformly spaced points over [min, max]; the function is the natural
    cubic spline through them (second derivative zero at both ends) or, with ``periodic``, the periodic cubic spline with the argument
    wrapped into [min, max).  Outside [min, max] a function that is not periodic has the value 0 and the derivative 0 (OpenMM's
    reference platform); at exactly min and max the end intervals' own value and one-sided derivative apply.  At least 2 values (3
    when periodic, the first equal to the last), at most custom_expr.MAX_TABLE_POINTS where a custom force's expression calls it."""

    def __init__(self, values, min, max, periodic=False):
        self._periodic = bool(periodic)
        self.setFunctionParameters(values, min, max)

    def setFunctionParameters(self, values, min, max):
        values = np.array(values, dtype=np.float64).reshape(-1)
        lo, hi = float(min), float(max)
        least = 3 if self._periodic else 2
        if len(values) < least:
            raise ValueError('Continuous1DFunction: %d values (a %s function needs at least %d)'
                             % (len(values), 'periodic' if self._periodic else 'continuous', least))
        if not (np.isfinite(lo) and np.isfinite(hi)):
            raise ValueError('Continuous1DFunction: the bounds min = %r, max = %r are not finite' % (lo, hi))
        if lo >= hi:
            raise ValueError('Continuous1DFunction: min = %r is not below max = %r' % (lo, hi))
        if not np.isfinite(values).all():
            raise ValueError('Continuous1DFunction: value %d is not finite' % int(np.flatnonzero(~np.isfinite(values))[0]))
        if self._periodic and values[0] != values[-1]:
            raise ValueError('Continuous1DFunction: a periodic function needs values[0] == values[-1] (%r and %r)' % (values[0], values[-1]))
        self._values, self._min, self._max = values, lo, hi

    def getFunctionParameters(self):
        return self._values.tolist(), self._min, self._max

    def getPeriodic(self):
        return self._periodic

    def Copy(self):
        return Continuous1DFunction(self._values, self._min, self._max, self._periodic)


class Discrete1DFunction:
    """openmm.Discrete1DFunction: the value is values[round(x)], halves rounded away from zero as C's round does; the derivative is 0.
    An index outside 0 ... n - 1 gives NaN: OpenMM throws there, the device cannot, and a NaN energy is what the sampler's NaN check
    catches."""

    def __init__(self, values):
        self.setFunctionParameters(values)

    def setFunctionParameters(self, values):
        values = np.array(values, dtype=np.float64).reshape(-1)
        if len(values) < 1:
            raise ValueError('Discrete1DFunction: no values')
        if not np.isfinite(values).all():
            raise ValueError('Discrete1DFunction: value %d is not finite' % int(np.flatnonzero(~np.isfinite(values))[0]))
        self._values = values

    def getFunctionParameters(self):
        return self._values.tolist()

    def Copy(self):
        return Discrete1DFunction(self._values)


def _grid_values(cls, sizes, values, least):
    """the flat values of a function on a grid of ``sizes`` (first index fastest), checked as the 1D classes check theirs"""
    sizes = tuple(int(n) for n in sizes)
    values = np.array(values, dtype=np.float64).reshape(-1)
    for axis, n in zip('xyz', sizes):
        if n < least:
            raise ValueError('%s: %ssize = %d (at least %d)' % (cls, axis, n, least))
    if len(values) != int(np.prod(sizes)):
        raise ValueError('%s: %d values for a grid of %s (%d)' % (cls, len(values), ' x '.join(str(n) for n in sizes), int(np.prod(sizes))))
    if not np.isfinite(values).all():
        raise ValueError('%s: value %d is not finite' % (cls, int(np.flatnonzero(~np.isfinite(values))[0])))
    return sizes, values


class Continuous2DFunction:
    """openmm.Continuous2DFunction: ``values[i + xsize*j]`` are samples f(x_i, y_j) on uniform grids of xsize points over [xmin, xmax]
    and ysize points over [ymin, ymax]; the function is the bicubic Hermite interpolant whose node derivatives are those of the 1D
    cubic splines through the rows and columns (natural, or with ``periodic`` periodic in both directions with both arguments
    wrapped; definition: include/remd_hip_custom.h).  Outside either range a function that is not periodic has the value 0 and both
    derivatives 0.  Both sizes at least 2; a periodic function needs its last row and column equal to the first; at most
    custom_expr.MAX_TABLE_CELLS values where a custom force's expression calls it.  (Continuous3DFunction does not exist here: the
    custom forces refuse it by name, like any foreign object.)"""

    def __init__(self, xsize, ysize, values, xmin, xmax, ymin, ymax, periodic=False):
        self._periodic = bool(periodic)
        self.setFunctionParameters(xsize, ysize, values, xmin, xmax, ymin, ymax)

    def setFunctionParameters(self, xsize, ysize, values, xmin, xmax, ymin, ymax):
        (nx, ny), values = _grid_values('Continuous2DFunction', (xsize, ysize), values, 2)
        bounds = tuple(float(v) for v in (xmin, xmax, ymin, ymax))
        for axis, lo, hi in (('x', bounds[0], bounds[1]), ('y', bounds[2], bounds[3])):
            if not (np.isfinite(lo) and np.isfinite(hi)):
                raise ValueError('Continuous2DFunction: the bounds %smin = %r, %smax = %r are not finite' % (axis, lo, axis, hi))
            if lo >= hi:
                raise ValueError('Continuous2DFunction: %smin = %r is not below %smax = %r' % (axis, lo, axis, hi))
        grid = values.reshape(ny, nx)
        if self._periodic and not (np.array_equal(grid[0], grid[-1]) and np.array_equal(grid[:, 0], grid[:, -1])):
            raise ValueError('Continuous2DFunction: a periodic function needs its last row and column equal to the first')
        self._nx, self._ny, self._values, self._bounds = nx, ny, values, bounds

    def getFunctionParameters(self):
        return (self._nx, self._ny, self._values.tolist()) + self._bounds

    def getPeriodic(self):
        return self._periodic

    def Copy(self):
        return Continuous2DFunction(self._nx, self._ny, self._values, *self._bounds, periodic=self._periodic)


class Discrete2DFunction:
    """openmm.Discrete2DFunction: the value is values[round(x) + xsize*round(y)], halves rounded away from zero; the derivatives are
    0.  An index outside its range gives NaN (see Discrete1DFunction)."""

    def __init__(self, xsize, ysize, values):
        self.setFunctionParameters(xsize, ysize, values)

    def setFunctionParameters(self, xsize, ysize, values):
        (self._nx, self._ny), self._values = _grid_values('Discrete2DFunction', (xsize, ysize), values, 1)

    def getFunctionParameters(self):
        return self._nx, self._ny, self._values.tolist()

    def Copy(self):
        return Discrete2DFunction(self._nx, self._ny, self._values)


class Discrete3DFunction:
    """openmm.Discrete3DFunction: values[round(x) + xsize*round(y) + xsize*ysize*round(z)]; otherwise as Discrete2DFunction."""

    def __init__(self, xsize, ysize, zsize, values):
        self.setFunctionParameters(xsize, ysize, zsize, values)

    def setFunctionParameters(self, xsize, ysize, zsize, values):
        (self._nx, self._ny, self._nz), self._values = _grid_values('Discrete3DFunction', (xsize, ysize, zsize), values, 1)

    def getFunctionParameters(self):
        return self._nx, self._ny, self._nz, self._values.tolist()

    def Copy(self):
        return Discrete3DFunction(self._nx, self._ny, self._nz, self._values)


class _CustomForce(Force):
    """What OpenMM's custom forces share: the energy string, global parameters with default values, per-term parameter names, the
    periodic-boundary flag and tabulated functions (Continuous1DFunction, Discrete1DFunction, Continuous2DFunction, Discrete2DFunction
    and Discrete3DFunction; the engine refuses every other kind, Continuous3DFunction among them)."""

    def __init__(self, energy):
        super().__init__()
        self._energy = str(energy)
        self._globals = []                    # [name, default]
        self._per_bond = []                   # per-term parameter names (per bond / angle / torsion / particle)
        self._periodic = False
        self._functions = []                  # (name, function)
        self._derivatives = []                # global parameter names (addEnergyParameterDerivative)
        self._in_engine = None                # id(self) once system_to_desc has read the force (a copy is another object and starts afresh)

    def getEnergyFunction(self):
        return self._energy

    def setEnergyFunction(self, energy):
        self._energy = str(energy)

    def addGlobalParameter(self, name, defaultValue):
        self._globals.append([str(name), float(defaultValue)])
        return len(self._globals) - 1

    def getNumGlobalParameters(self):
        return len(self._globals)

    def getGlobalParameterName(self, index):
        return self._globals[index][0]

    def getGlobalParameterDefaultValue(self, index):
        return self._globals[index][1]

    def setGlobalParameterDefaultValue(self, index, defaultValue):
        self._globals[index][1] = float(defaultValue)

    def addEnergyParameterDerivative(self, name):
        """openmm's addEnergyParameterDerivative: ask for dE/d(global parameter ``name``) of this force
        (HipEngine.custom_energy_parameter_derivatives).  Only a force that declared a parameter contributes to its derivative."""
        cls, name = type(self).__name__, str(name)
        if getattr(self, '_in_engine', None) == id(self):
            raise NotImplementedError('%s: adding an energy parameter derivative (%r) after set_system is not supported: the engine keeps '
                                      'the declarations it was given, build the states again' % (cls, name))
        if name not in [g[0] for g in self._globals]:
            raise ValueError('%s: addEnergyParameterDerivative(%r): the force has no global parameter of that name (%s)'
                             % (cls, name, ', '.join(g[0] for g in self._globals) or 'it has none'))
        if name in self._derivatives:
            raise ValueError('%s: addEnergyParameterDerivative(%r): the derivative with respect to that parameter was already added' % (cls, name))
        self._derivatives.append(name)
        return len(self._derivatives) - 1

    def getNumEnergyParameterDerivatives(self):
        return len(getattr(self, '_derivatives', ()))

    def getEnergyParameterDerivativeName(self, index):
        return self._derivatives[index]

    def addPerBondParameter(self, name):
        self._per_bond.append(str(name))
        return len(self._per_bond) - 1

    def getNumPerBondParameters(self):
        return len(self._per_bond)

    def getPerBondParameterName(self, index):
        return self._per_bond[index]

    def setUsesPeriodicBoundaryConditions(self, periodic):
        self._periodic = bool(periodic)

    def usesPeriodicBoundaryConditions(self):
        return self._periodic

    def addTabulatedFunction(self, name, function):
        self._functions.append((str(name), function))
        return len(self._functions) - 1

    def getNumTabulatedFunctions(self):
        return len(self._functions)

    def getTabulatedFunctionName(self, index):
        return self._functions[index][0]

    def getTabulatedFunction(self, index):
        return self._functions[index][1]


def _term_arrays(terms, width, n_params, what):
    """atoms int32 [n][width] and params float64 [n][n_params] of a custom force's terms ((atoms..., parameters) tuples)."""
    for t in terms:
        if len(t[-1]) != n_params:
            raise ValueError('%s: a term carries %d parameters, the force declares %d' % (what, len(t[-1]), n_params))
    atoms = np.array([t[:width] for t in terms], dtype=np.int32).reshape(-1, width)
    params = np.array([t[-1] for t in terms], dtype=np.float64).reshape(len(terms), n_params)
    return atoms, params


class CustomBondForce(_CustomForce):
    """openmm.CustomBondForce: bonds between two particles, the energy a function of their distance r, of per-bond and of global
    parameters.  The restraint forms of forces.py go to csrc/restraints.hip, every other expression to csrc/custom_terms.hip."""

    def __init__(self, energy):
        super().__init__(energy)
        self._bonds = []                      # (p1, p2, parameters)

    def addBond(self, particle1, particle2, parameters=()):
        self._bonds.append((int(particle1), int(particle2), [float(p) for p in parameters]))
        return len(self._bonds) - 1

    def getNumBonds(self):
        return len(self._bonds)

    def getBondParameters(self, index):
        p1, p2, parameters = self._bonds[index]
        return p1, p2, list(parameters)

    def setBondParameters(self, index, particle1, particle2, parameters=()):
        self._bonds[index] = (int(particle1), int(particle2), [float(p) for p in parameters])

    def _term_arrays(self):
        return _term_arrays(self._bonds, 2, len(self._per_bond), 'CustomBondForce')


class CustomAngleForce(_CustomForce):
    """openmm.CustomAngleForce: the energy a function of the angle theta (radians, 0 ... pi) at the middle one of three particles."""

    def __init__(self, energy):
        super().__init__(energy)
        self._angles = []                     # (p1, p2, p3, parameters)

    addPerAngleParameter = _CustomForce.addPerBondParameter
    getNumPerAngleParameters = _CustomForce.getNumPerBondParameters
    getPerAngleParameterName = _CustomForce.getPerBondParameterName

    def addAngle(self, particle1, particle2, particle3, parameters=()):
        self._angles.append((int(particle1), int(particle2), int(particle3), [float(p) for p in parameters]))
        return len(self._angles) - 1

    def getNumAngles(self):
        return len(self._angles)

    def getAngleParameters(self, index):
        p1, p2, p3, parameters = self._angles[index]
        return p1, p2, p3, list(parameters)

    def setAngleParameters(self, index, particle1, particle2, particle3, parameters=()):
        self._angles[index] = (int(particle1), int(particle2), int(particle3), [float(p) for p in parameters])

    def _term_arrays(self):
        return _term_arrays(self._angles, 3, len(self._per_bond), 'CustomAngleForce')


class CustomTorsionForce(_CustomForce):
    """openmm.CustomTorsionForce: the energy a function of the dihedral theta (radians, -pi ... pi, the sign convention of
    PeriodicTorsionForce) of four particles."""

    def __init__(self, energy):
        super().__init__(energy)
        self._torsions = []                   # (p1, p2, p3, p4, parameters)

    addPerTorsionParameter = _CustomForce.addPerBondParameter
    getNumPerTorsionParameters = _CustomForce.getNumPerBondParameters
    getPerTorsionParameterName = _CustomForce.getPerBondParameterName

    def addTorsion(self, particle1, particle2, particle3, particle4, parameters=()):
        self._torsions.append((int(particle1), int(particle2), int(particle3), int(particle4), [float(p) for p in parameters]))
        return len(self._torsions) - 1

    def getNumTorsions(self):
        return len(self._torsions)

    def getTorsionParameters(self, index):
        p1, p2, p3, p4, parameters = self._torsions[index]
        return p1, p2, p3, p4, list(parameters)

    def setTorsionParameters(self, index, particle1, particle2, particle3, particle4, parameters=()):
        self._torsions[index] = (int(particle1), int(particle2), int(particle3), int(particle4), [float(p) for p in parameters])

    def _term_arrays(self):
        return _term_arrays(self._torsions, 4, len(self._per_bond), 'CustomTorsionForce')


class CustomCompoundBondForce(_CustomForce):
    """openmm.CustomCompoundBondForce: bonds between ``numParticles`` particles, the energy a function of their coordinates
    x1 y1 z1 ... and of distance(p1,p2), angle(p1,p2,p3), dihedral(p1,p2,p3,p4) and pointdistance(x1,y1,z1,x2,y2,z2) between them, of
    per-bond and of global parameters (Boresch restraints are one six-particle bond).  Every expression goes to
    csrc/custom_compound.hip."""

    def __init__(self, numParticles, energy):
        super().__init__(energy)
        self._n_particles = int(numParticles)
        self._bonds = []                      # (p1, ..., pP, parameters)

    def getNumParticlesPerBond(self):
        return self._n_particles

    def _bond(self, particles, parameters):
        particles = [int(p) for p in particles]
        if len(particles) != self._n_particles:
            raise ValueError('CustomCompoundBondForce: a bond of %d particles, the force declares %d' % (len(particles), self._n_particles))
        return tuple(particles) + ([float(p) for p in parameters],)

    def addBond(self, particles, parameters=()):
        self._bonds.append(self._bond(particles, parameters))
        return len(self._bonds) - 1

    def getNumBonds(self):
        return len(self._bonds)

    def getBondParameters(self, index):
        bond = self._bonds[index]
        return list(bond[:-1]), list(bond[-1])

    def setBondParameters(self, index, particles, parameters=()):
        self._bonds[index] = self._bond(particles, parameters)

    def _term_arrays(self):
        return _term_arrays(self._bonds, self._n_particles, len(self._per_bond), 'CustomCompoundBondForce')


class CustomCentroidBondForce(_CustomForce):
    """openmm.CustomCentroidBondForce: bonds between ``numGroups`` groups of particles, the energy a compound-bond expression of the
    groups' weighted centroids: their coordinates x1 y1 z1 ..., distance(g1,g2), angle(g1,g2,g3), dihedral(g1,g2,g3,g4) and
    pointdistance(x1,y1,z1,x2,y2,z2), per-bond and global parameters.  A group without weights is weighted by its particles' masses.
    Every expression goes to csrc/custom_centroid.hip; the radially symmetric restraints of forces.py, which build on a class of
    their own (forces.CustomCentroidBondForce), keep csrc/restraints.hip."""

    def __init__(self, numGroups, energy):
        super().__init__(energy)
        self._n_groups_per_bond = int(numGroups)
        self._groups = []                     # (particles, weights or None)
        self._bonds = []                      # (g1, ..., gP, parameters)

    def getNumGroupsPerBond(self):
        return self._n_groups_per_bond

    @staticmethod
    def _checked_group(particles, weights):
        particles = [int(p) for p in particles]
        weights = None if weights is None or len(weights) == 0 else [float(w) for w in weights]
        if weights is not None and len(weights) != len(particles):
            raise ValueError('CustomCentroidBondForce: a group of %d particles with %d weights' % (len(particles), len(weights)))
        return particles, weights

    def addGroup(self, particles, weights=None):
        self._groups.append(self._checked_group(particles, weights))
        return len(self._groups) - 1

    def getNumGroups(self):
        return len(self._groups)

    def getGroupParameters(self, index):
        particles, weights = self._groups[index]
        return list(particles), ([] if weights is None else list(weights))

    def setGroupParameters(self, index, particles, weights=None):
        self._groups[index] = self._checked_group(particles, weights)

    def _bond(self, groups, parameters):
        groups = [int(g) for g in groups]
        if len(groups) != self._n_groups_per_bond:
            raise ValueError('CustomCentroidBondForce: a bond of %d groups, the force declares %d' % (len(groups), self._n_groups_per_bond))
        return tuple(groups) + ([float(p) for p in parameters],)

    def addBond(self, groups, parameters=()):
        self._bonds.append(self._bond(groups, parameters))
        return len(self._bonds) - 1

    def getNumBonds(self):
        return len(self._bonds)

    def getBondParameters(self, index):
        bond = self._bonds[index]
        return list(bond[:-1]), list(bond[-1])

    def setBondParameters(self, index, groups, parameters=()):
        self._bonds[index] = self._bond(groups, parameters)

    def _term_arrays(self):
        """the bonds' group numbers int32 [n][groups per bond] and parameters float64 [n][p]"""
        return _term_arrays(self._bonds, self._n_groups_per_bond, len(self._per_bond), 'CustomCentroidBondForce')


class RMSDForce(Force):
    """openmm.RMSDForce: the root-mean-square deviation (nm, numerically kJ/mol) of ``particles`` from ``referencePositions`` after
    the optimal superposition.  ``referencePositions`` is [N][3] for ALL particles of the System (nm, or a unit Quantity); only the
    rows of ``particles`` are used, and an empty list means every particle.  No periodic boundary conditions (OpenMM's rule).  Meant
    as a collective variable of a CustomCVForce; added to a System on its own it acts as CustomCVForce('v') with itself as v
    (csrc/custom_cv.hip)."""

    def __init__(self, referencePositions, particles=()):
        super().__init__()
        self.setReferencePositions(referencePositions)
        self.setParticles(particles)

    def getReferencePositions(self):
        return self._reference.copy()

    def setReferencePositions(self, positions):
        from .unit import to_md
        ref = np.array(to_md(positions), dtype=np.float64)
        if ref.ndim != 2 or ref.shape[1] != 3:
            raise ValueError('RMSDForce: reference positions of shape %s (one row of x, y, z per particle of the System)' % (ref.shape,))
        self._reference = ref

    def getParticles(self):
        return list(self._particles)

    def setParticles(self, particles):
        self._particles = [int(p) for p in particles]

    def usesPeriodicBoundaryConditions(self):
        return False

    def updateParametersInContext(self, context=None):
        raise NotImplementedError('RMSDForce: changing the reference positions or the particles after set_system (updateParametersInContext) '
                                  'is not supported: the engine keeps the reference it was given, build the states again')


class CustomCVForce(_CustomForce):
    """openmm.CustomCVForce: the energy an expression of collective variables, each the energy of a Force of its own, of global
    parameters and of tabulated functions.  The engine takes one to three collective variables, each an RMSDForce
    (csrc/custom_cv.hip); the variables keep the objects they were given, as in OpenMM."""

    def __init__(self, energy):
        super().__init__(energy)
        self._variables = []                  # (name, force)

    def addCollectiveVariable(self, name, force):
        self._variables.append((str(name), force))
        return len(self._variables) - 1

    def getNumCollectiveVariables(self):
        return len(self._variables)

    def getCollectiveVariableName(self, index):
        return self._variables[index][0]

    def getCollectiveVariable(self, index):
        return self._variables[index][1]

    def usesPeriodicBoundaryConditions(self):
        return False

    def addEnergyParameterDerivative(self, name):
        raise NotImplementedError('CustomCVForce: energy parameter derivatives (addEnergyParameterDerivative %r) are not supported' % (name,))

    def getNumEnergyParameterDerivatives(self):
        return 0


class CMAPTorsionForce(Force):
    """openmm.CMAPTorsionForce: the energy of a pair of dihedrals read from a map -- the backbone phi / psi correction of CHARMM22/36
    and Amber ff19SB.  A map is ``size * size`` energies in kJ/mol, ``energy[i + size*j]`` at the first angle 2 pi i / size and the
    second 2 pi j / size, periodic in both; between the nodes it is the bicubic patch whose node derivatives come from periodic cubic
    splines (OpenMM's CMAPTorsionForceImpl::calcMapDerivatives; custom_expr.cmap_block builds it).  A torsion pair names a map and two
    quadruples of particles, which usually share three; each dihedral has the sign and range of PeriodicTorsionForce.  Off by
    default, setUsesPeriodicBoundaryConditions makes every difference inside a dihedral a minimum image.  The force counts among the
    custom forces of a System (one force group, custom_expr.MAX_FORCES) and runs in csrc/cmap.hip; size 2 ... MAX_SIZE and at most
    MAX_MAPS maps are the engine's limits."""
    MAX_MAPS = 64                             # REMD_CUSTOM_MAX_MAPS
    MAX_SIZE = 255                            # (size + 1)^2 node values must stay within custom_expr.MAX_TABLE_CELLS

    def __init__(self):
        super().__init__()
        self._maps = []                       # (size, energies float64 [size * size])
        self._torsions = []                   # (map, a1, a2, a3, a4, b1, b2, b3, b4)
        self._periodic = False

    @staticmethod
    def _map(size, energy):
        from .unit import to_md
        if int(size) != size or int(size) < 2:
            raise ValueError('CMAPTorsionForce: a map of size %r (at least 2)' % (size,))
        size = int(size)
        energy = np.array(to_md(energy), dtype=np.float64).reshape(-1)
        if len(energy) != size * size:
            raise ValueError('CMAPTorsionForce: a map of size %d needs %d energies, not %d' % (size, size * size, len(energy)))
        if not np.isfinite(energy).all():
            raise ValueError('CMAPTorsionForce: a map energy that is not finite')
        if size > CMAPTorsionForce.MAX_SIZE:
            raise NotImplementedError('CMAPTorsionForce: a map of size %d (the engine takes 2 ... %d)' % (size, CMAPTorsionForce.MAX_SIZE))
        return size, energy

    def addMap(self, size, energy):
        entry = self._map(size, energy)
        if len(self._maps) >= self.MAX_MAPS:
            raise NotImplementedError('CMAPTorsionForce: more than %d maps in one force' % self.MAX_MAPS)
        self._maps.append(entry)
        return len(self._maps) - 1

    def getNumMaps(self):
        return len(self._maps)

    def getMapParameters(self, index):
        size, energy = self._maps[index]
        return size, energy.tolist()

    def setMapParameters(self, index, size, energy):
        self._maps[index] = self._map(size, energy)

    @staticmethod
    def _torsion(map, a, b):
        for name, quad in (('first', a), ('second', b)):
            if len(set(quad)) != 4:
                raise ValueError('CMAPTorsionForce: the %s dihedral (%s) names particle %d twice'
                                 % (name, ', '.join(str(p) for p in quad), [p for p in quad if quad.count(p) > 1][0]))
        return (int(map),) + tuple(a) + tuple(b)

    def addTorsion(self, map, a1, a2, a3, a4, b1, b2, b3, b4):
        self._torsions.append(self._torsion(map, [int(p) for p in (a1, a2, a3, a4)], [int(p) for p in (b1, b2, b3, b4)]))
        return len(self._torsions) - 1

    def getNumTorsions(self):
        return len(self._torsions)

    def getTorsionParameters(self, index):
        return self._torsions[index]

    def setTorsionParameters(self, index, map, a1, a2, a3, a4, b1, b2, b3, b4):
        self._torsions[index] = self._torsion(map, [int(p) for p in (a1, a2, a3, a4)], [int(p) for p in (b1, b2, b3, b4)])

    def setUsesPeriodicBoundaryConditions(self, periodic):
        self._periodic = bool(periodic)

    def usesPeriodicBoundaryConditions(self):
        return self._periodic

    def updateParametersInContext(self, context=None):
        raise NotImplementedError('CMAPTorsionForce: changing a map or a torsion after set_system (updateParametersInContext) is not '
                                  'supported: the engine keeps the maps it was given, build the states again')


class CustomExternalForce(_CustomForce):
    """openmm.CustomExternalForce: the energy a function of a particle's x, y, z, of per-particle and of global parameters.  The
    harmonic-well expression of testsystems.HarmonicOscillator (testsystems.py:779-786) keeps the engine's own kernel (ext_K / ext_x0 /
    ext_U0 of remd_system_desc); every other expression goes to csrc/custom_terms.hip."""

    HARMONIC_EXPRESSION = ('(K/2.0) * ((x-x0)^2 + y^2 + z^2) + U0;'
                           'K = testsystems_HarmonicOscillator_K;'
                           'x0 = testsystems_HarmonicOscillator_x0;'
                           'U0 = testsystems_HarmonicOscillator_U0;')

    def __init__(self, energy_expression):
        super().__init__(energy_expression)
        self._particles = []                  # (index, parameters)

    addPerParticleParameter = _CustomForce.addPerBondParameter
    getNumPerParticleParameters = _CustomForce.getNumPerBondParameters
    getPerParticleParameterName = _CustomForce.getPerBondParameterName

    energy_expression = property(lambda self: self._energy)
    globals = property(lambda self: dict((n, v) for n, v in self._globals))       # {name: default value}
    particles = property(lambda self: [p[0] for p in self._particles])            # particle indices

    def is_harmonic_oscillator(self):
        return self._energy.replace(' ', '') == self.HARMONIC_EXPRESSION.replace(' ', '') and not self._per_bond

    def getGlobalParameter(self, name):
        return self.globals[name]

    def addParticle(self, index, params=()):
        self._particles.append((int(index), [float(p) for p in params]))
        return len(self._particles) - 1

    def getNumParticles(self):
        return len(self._particles)

    def getParticleParameters(self, index):
        p, parameters = self._particles[index]
        return p, list(parameters)

    def setParticleParameters(self, index, particle, parameters=()):
        self._particles[index] = (int(particle), [float(p) for p in parameters])

    def _term_arrays(self):
        return _term_arrays(self._particles, 1, len(self._per_bond), 'CustomExternalForce')


class CustomNonbondedForce(_CustomForce):
    """openmm.CustomNonbondedForce: the energy a function of the distance r of two particles, of their per-particle parameters (a
    parameter p appears as p1 and p2) and of global parameters, summed over every pair that no exclusion names and, with a cutoff,
    that lies inside it.  Every expression goes to csrc/custom_nonbonded.hip (one wavefront per tile of 64 x 64 particles: the cost is
    quadratic in the particle count).  Interaction groups, energy parameter derivatives and the long-range correction of an expression
    that calls a tabulated function are refused."""
    NoCutoff, CutoffNonPeriodic, CutoffPeriodic = 0, 1, 2

    def __init__(self, energy):
        super().__init__(energy)
        self._particles = []                  # per-particle parameter lists
        self._exclusions = []                 # (i, j)
        self._method = CustomNonbondedForce.NoCutoff
        self._cutoff = 1.0
        self._use_switch = False
        self._switch = -1.0
        self._lrc = False

    addPerParticleParameter = _CustomForce.addPerBondParameter
    getNumPerParticleParameters = _CustomForce.getNumPerBondParameters
    getPerParticleParameterName = _CustomForce.getPerBondParameterName

    def addParticle(self, parameters=()):
        self._particles.append([float(p) for p in parameters])
        return len(self._particles) - 1

    def getNumParticles(self):
        return len(self._particles)

    def getParticleParameters(self, index):
        return list(self._particles[index])

    def setParticleParameters(self, index, parameters=()):
        self._particles[index] = [float(p) for p in parameters]

    def addExclusion(self, particle1, particle2):
        self._exclusions.append((int(particle1), int(particle2)))
        return len(self._exclusions) - 1

    def getNumExclusions(self):
        return len(self._exclusions)

    def getExclusionParticles(self, index):
        return self._exclusions[index]

    def createExclusionsFromBonds(self, bonds, bondCutoff):
        """OpenMM's rule: every pair of particles joined by at most ``bondCutoff`` of the bonds (pairs of particle indices) becomes an
        exclusion, each pair once, in the order of the lower particle."""
        if bondCutoff < 1:
            return
        n = len(self._particles)
        for a, b in bonds:
            if not (0 <= a < n and 0 <= b < n):
                raise ValueError('CustomNonbondedForce.createExclusionsFromBonds: a bond names particle %d (the force has %d)' % (max(a, b) if min(a, b) >= 0 else min(a, b), n))
        near = [set() for _ in range(n)]
        for a, b in bonds:
            near[a].add(int(b)); near[b].add(int(a))
        reach = [set(s) for s in near]
        for _ in range(int(bondCutoff) - 1):
            reach = [set(r).union(*[near[k] for k in r]) for r in reach]
        for i in range(n):
            for j in sorted(reach[i]):
                if j < i:
                    self.addExclusion(j, i)

    def setNonbondedMethod(self, method):
        if int(method) not in (0, 1, 2):
            raise ValueError('CustomNonbondedForce: nonbonded method %r (NoCutoff, CutoffNonPeriodic or CutoffPeriodic)' % (method,))
        self._method = int(method)

    def getNonbondedMethod(self):
        return self._method

    def setCutoffDistance(self, distance):
        self._cutoff = float(distance)

    def getCutoffDistance(self):
        return self._cutoff

    def setUseSwitchingFunction(self, use):
        self._use_switch = bool(use)

    def getUseSwitchingFunction(self):
        return self._use_switch

    def setSwitchingDistance(self, distance):
        self._switch = float(distance)

    def getSwitchingDistance(self):
        return self._switch

    def setUseLongRangeCorrection(self, use):
        self._lrc = bool(use)

    def getUseLongRangeCorrection(self):
        return self._lrc

    def usesPeriodicBoundaryConditions(self):
        return self._method == CustomNonbondedForce.CutoffPeriodic

    def setUsesPeriodicBoundaryConditions(self, periodic):
        raise ValueError('CustomNonbondedForce: periodic boundary conditions follow the nonbonded method (setNonbondedMethod(CutoffPeriodic))')

    def addInteractionGroup(self, set1, set2):
        raise NotImplementedError('CustomNonbondedForce: interaction groups (addInteractionGroup) are not supported')

    def getNumInteractionGroups(self):
        return 0

    def addEnergyParameterDerivative(self, name):
        raise NotImplementedError('CustomNonbondedForce: energy parameter derivatives (addEnergyParameterDerivative) are not supported')

    def getNumEnergyParameterDerivatives(self):
        return 0


class CustomHbondForce(_CustomForce):
    """openmm.CustomHbondForce: donors (up to three particles d1 d2 d3) and acceptors (a1 a2 a3), the energy an expression of
    distance(), angle() and dihedral() among the six, of per-donor, per-acceptor and global parameters and of tabulated functions,
    summed over every (donor, acceptor) pair that no exclusion names and, with a cutoff, whose distance(d1, a1) is below it.  -1 marks
    an unused second or third particle; the expression may name only particles every donor and acceptor has.  Every expression goes
    to csrc/custom_hbond.hip (one wavefront per tile of 64 donors x 64 acceptors: the cost is proportional to donors x acceptors).
    A non-excluded pair that shares a particle is refused, as are raw coordinates and pointdistance / pointangle / pointdihedral."""
    NoCutoff, CutoffNonPeriodic, CutoffPeriodic = 0, 1, 2

    def __init__(self, energy):
        super().__init__(energy)
        self._per_acceptor = []               # per-acceptor parameter names (_per_bond holds the per-donor ones)
        self._donors = []                     # (d1, d2, d3, parameters)
        self._acceptors = []                  # (a1, a2, a3, parameters)
        self._exclusions = []                 # (donor, acceptor)
        self._method = CustomHbondForce.NoCutoff
        self._cutoff = 1.0

    addPerDonorParameter = _CustomForce.addPerBondParameter
    getNumPerDonorParameters = _CustomForce.getNumPerBondParameters
    getPerDonorParameterName = _CustomForce.getPerBondParameterName

    def addPerAcceptorParameter(self, name):
        self._per_acceptor.append(str(name))
        return len(self._per_acceptor) - 1

    def getNumPerAcceptorParameters(self):
        return len(self._per_acceptor)

    def getPerAcceptorParameterName(self, index):
        return self._per_acceptor[index]

    @staticmethod
    def _row(p1, p2, p3, parameters):
        return (int(p1), int(p2), int(p3), [float(p) for p in parameters])

    def addDonor(self, d1, d2, d3, parameters=()):
        self._donors.append(self._row(d1, d2, d3, parameters))
        return len(self._donors) - 1

    def getNumDonors(self):
        return len(self._donors)

    def getDonorParameters(self, index):
        d1, d2, d3, parameters = self._donors[index]
        return d1, d2, d3, list(parameters)

    def setDonorParameters(self, index, d1, d2, d3, parameters=()):
        self._donors[index] = self._row(d1, d2, d3, parameters)

    def addAcceptor(self, a1, a2, a3, parameters=()):
        self._acceptors.append(self._row(a1, a2, a3, parameters))
        return len(self._acceptors) - 1

    def getNumAcceptors(self):
        return len(self._acceptors)

    def getAcceptorParameters(self, index):
        a1, a2, a3, parameters = self._acceptors[index]
        return a1, a2, a3, list(parameters)

    def setAcceptorParameters(self, index, a1, a2, a3, parameters=()):
        self._acceptors[index] = self._row(a1, a2, a3, parameters)

    def addExclusion(self, donor, acceptor):
        self._exclusions.append((int(donor), int(acceptor)))
        return len(self._exclusions) - 1

    def getNumExclusions(self):
        return len(self._exclusions)

    def getExclusionParticles(self, index):
        return self._exclusions[index]

    def setExclusionParticles(self, index, donor, acceptor):
        self._exclusions[index] = (int(donor), int(acceptor))

    def setNonbondedMethod(self, method):
        if int(method) not in (0, 1, 2):
            raise ValueError('CustomHbondForce: nonbonded method %r (NoCutoff, CutoffNonPeriodic or CutoffPeriodic)' % (method,))
        self._method = int(method)

    def getNonbondedMethod(self):
        return self._method

    def setCutoffDistance(self, distance):
        self._cutoff = float(distance)

    def getCutoffDistance(self):
        return self._cutoff

    def usesPeriodicBoundaryConditions(self):
        return self._method == CustomHbondForce.CutoffPeriodic

    def setUsesPeriodicBoundaryConditions(self, periodic):
        raise ValueError('CustomHbondForce: periodic boundary conditions follow the nonbonded method (setNonbondedMethod(CutoffPeriodic))')

    def updateParametersInContext(self, context=None):
        raise NotImplementedError('CustomHbondForce: changing donors, acceptors or exclusions after set_system (updateParametersInContext) is not '
                                  'supported: build the System again')


class CustomManyParticleForce(_CustomForce):
    """openmm.CustomManyParticleForce with three particles per set: the energy an expression of distance(), angle() and dihedral()
    among p1 p2 p3, of per-particle parameters (a parameter sigma appears as sigma1, sigma2 and sigma3, the slot appended), of global
    parameters and of tabulated functions, summed over sets of three distinct particles none of whose pairs is excluded.
    SinglePermutation: every unordered set once, with a cutoff all three distances below it.  UniqueCentralParticle: every set once per
    choice of its central particle p1, the other two unordered, with a cutoff only the two distances to p1 below it.  A type filter on
    slot s admits a set only under an assignment that puts a particle of an allowed type into slot s; where several assignments pass,
    OpenMM leaves the choice open: here it is the first in lexicographic order of the atom indices (p1, p2, p3) -- over six
    assignments in SinglePermutation, over the two with p1 fixed in UniqueCentralParticle.  Every expression goes to
    csrc/custom_manyparticle.hip (a neighbour row of at most 128 entries per particle, then one wavefront per central particle).
    Sets of another size, raw coordinates and pointdistance / pointangle / pointdihedral are refused."""
    NoCutoff, CutoffNonPeriodic, CutoffPeriodic = 0, 1, 2
    SinglePermutation, UniqueCentralParticle = 0, 1

    def __init__(self, particlesPerSet, energy):
        super().__init__(energy)
        if int(particlesPerSet) != 3:
            raise NotImplementedError('CustomManyParticleForce: sets of %d particles (sets of 3 particles are supported)' % int(particlesPerSet))
        self._per_set = 3
        self._particles = []                  # (parameters, type)
        self._exclusions = []                 # (i, j)
        self._method = CustomManyParticleForce.NoCutoff
        self._cutoff = 1.0
        self._mode = CustomManyParticleForce.SinglePermutation
        self._filters = {}                    # slot -> sorted types

    addPerParticleParameter = _CustomForce.addPerBondParameter
    getNumPerParticleParameters = _CustomForce.getNumPerBondParameters
    getPerParticleParameterName = _CustomForce.getPerBondParameterName

    def getNumParticlesPerSet(self):
        return self._per_set

    @staticmethod
    def _particle(parameters, type):
        if not 0 <= int(type) <= 31:
            raise ValueError('CustomManyParticleForce: particle type %d (the types are 0 ... 31)' % int(type))
        return ([float(p) for p in parameters], int(type))

    def addParticle(self, parameters=(), type=0):
        self._particles.append(self._particle(parameters, type))
        return len(self._particles) - 1

    def getNumParticles(self):
        return len(self._particles)

    def getParticleParameters(self, index):
        parameters, type = self._particles[index]
        return list(parameters), type

    def setParticleParameters(self, index, parameters=(), type=0):
        self._particles[index] = self._particle(parameters, type)

    def addExclusion(self, particle1, particle2):
        self._exclusions.append((int(particle1), int(particle2)))
        return len(self._exclusions) - 1

    def getNumExclusions(self):
        return len(self._exclusions)

    def getExclusionParticles(self, index):
        return self._exclusions[index]

    def setExclusionParticles(self, index, particle1, particle2):
        self._exclusions[index] = (int(particle1), int(particle2))

    createExclusionsFromBonds = CustomNonbondedForce.createExclusionsFromBonds

    def setNonbondedMethod(self, method):
        if int(method) not in (0, 1, 2):
            raise ValueError('CustomManyParticleForce: nonbonded method %r (NoCutoff, CutoffNonPeriodic or CutoffPeriodic)' % (method,))
        self._method = int(method)

    def getNonbondedMethod(self):
        return self._method

    def setCutoffDistance(self, distance):
        self._cutoff = float(distance)

    def getCutoffDistance(self):
        return self._cutoff

    def setPermutationMode(self, mode):
        if int(mode) not in (0, 1):
            raise ValueError('CustomManyParticleForce: permutation mode %r (SinglePermutation or UniqueCentralParticle)' % (mode,))
        self._mode = int(mode)

    def getPermutationMode(self):
        return self._mode

    def setTypeFilter(self, index, types):
        if not 0 <= int(index) <= 2:
            raise ValueError('CustomManyParticleForce: type filter index %d (the particles of a set are 0 ... 2)' % int(index))
        types = sorted({int(t) for t in types})
        for t in types:
            if not 0 <= t <= 31:
                raise ValueError('CustomManyParticleForce: type filter %d names type %d (the types are 0 ... 31)' % (int(index), t))
        self._filters[int(index)] = types

    def getTypeFilter(self, index):
        """the allowed types of slot ``index``; an empty list: no filter (OpenMM's convention)"""
        if not 0 <= int(index) <= 2:
            raise ValueError('CustomManyParticleForce: type filter index %d (the particles of a set are 0 ... 2)' % int(index))
        return list(self._filters.get(int(index), ()))

    def usesPeriodicBoundaryConditions(self):
        return self._method == CustomManyParticleForce.CutoffPeriodic

    def setUsesPeriodicBoundaryConditions(self, periodic):
        raise ValueError('CustomManyParticleForce: periodic boundary conditions follow the nonbonded method (setNonbondedMethod(CutoffPeriodic))')

    def updateParametersInContext(self, context=None):
        raise NotImplementedError('CustomManyParticleForce: changing particles, exclusions or filters after set_system (updateParametersInContext) is '
                                  'not supported: build the System again')


class GBSAOBCForce(Force):
    """openmm.GBSAOBCForce: OBC2 Born radii + ACE surface term (the form the reference's alchemical factory spells out, alchemy.py:2144-2225).
    NoCutoff only."""
    NoCutoff, CutoffNonPeriodic, CutoffPeriodic = 0, 1, 2

    def __init__(self):
        super().__init__()
        self.particles = []                 # (charge, radius nm, scale)
        self._solvent, self._solute, self._sa, self._method = 78.5, 1.0, 2.25936, 0

    def addParticle(self, charge, radius, scalingFactor):
        self.particles.append((float(charge), float(radius), float(scalingFactor)))
        return len(self.particles) - 1

    def getNumParticles(self): return len(self.particles)
    def getParticleParameters(self, idx): return self.particles[idx]
    def setParticleParameters(self, idx, charge, radius, scalingFactor): self.particles[idx] = (float(charge), float(radius), float(scalingFactor))
    def getSolventDielectric(self): return self._solvent
    def setSolventDielectric(self, v): self._solvent = float(v)
    def getSoluteDielectric(self): return self._solute
    def setSoluteDielectric(self, v): self._solute = float(v)
    def getSurfaceAreaEnergy(self): return self._sa
    def setSurfaceAreaEnergy(self, v): self._sa = float(v)
    def getNonbondedMethod(self): return self._method
    def setNonbondedMethod(self, m): self._method = int(m)


class CustomGBForce(Force):
    """openmm.CustomGBForce: per-particle parameters, global parameters, computed values and energy terms given as expression strings.
    The OBC family (openmmtools_amd/custom_gb.py recognises it: the CustomGBForceSystem strings of testsystems.py:4332-4351, the
    alchemical factory's GBSA strings, and both after _alchemically_modify_CustomGBForce), with NoCutoff or CutoffPeriodic, goes to
    csrc/gbsa.hip; every other force is compiled for the custom forces' stack machine (custom_gb.compile_custom_gb, csrc/custom_gb.hip):
    at most 4 computed values, the first a pair sum and the others SingleParticle, at most 8 energy terms, tabulated functions,
    exclusions, the three nonbonded methods; global parameters take their default values."""
    NoCutoff, CutoffNonPeriodic, CutoffPeriodic = 0, 1, 2
    SingleParticle, ParticlePair, ParticlePairNoExclusions = 0, 1, 2

    def __init__(self):
        super().__init__()
        self.per_particle = []              # names
        self.globals = []                   # [name, default]
        self.computed = []                  # (name, expression, type)
        self.energy_terms = []              # (expression, type)
        self.particles = []                 # tuples of floats
        self.exclusions = []                # (i, j)
        self.functions = []                 # (name, function): tabulated functions (the general path evaluates them)
        self._method, self._cutoff = 0, 1.0

    def addPerParticleParameter(self, name):
        self.per_particle.append(str(name)); return len(self.per_particle) - 1
    def getNumPerParticleParameters(self): return len(self.per_particle)
    def getPerParticleParameterName(self, idx): return self.per_particle[idx]
    def addGlobalParameter(self, name, defaultValue):
        self.globals.append([str(name), float(defaultValue)]); return len(self.globals) - 1
    def getNumGlobalParameters(self): return len(self.globals)
    def getGlobalParameterName(self, idx): return self.globals[idx][0]
    def getGlobalParameterDefaultValue(self, idx): return self.globals[idx][1]
    def setGlobalParameterDefaultValue(self, idx, defaultValue): self.globals[idx][1] = float(defaultValue)
    def addComputedValue(self, name, expression, computationType):
        self.computed.append((str(name), str(expression), int(computationType))); return len(self.computed) - 1
    def getNumComputedValues(self): return len(self.computed)
    def getComputedValueParameters(self, idx): return self.computed[idx]
    def addEnergyTerm(self, expression, computationType):
        self.energy_terms.append((str(expression), int(computationType))); return len(self.energy_terms) - 1
    def getNumEnergyTerms(self): return len(self.energy_terms)
    def getEnergyTermParameters(self, idx): return self.energy_terms[idx]
    def addParticle(self, parameters=()):
        self.particles.append(tuple(float(v) for v in parameters)); return len(self.particles) - 1
    def getNumParticles(self): return len(self.particles)
    def getParticleParameters(self, idx): return list(self.particles[idx])
    def setParticleParameters(self, idx, parameters): self.particles[idx] = tuple(float(v) for v in parameters)
    def addExclusion(self, particle1, particle2):
        self.exclusions.append((int(particle1), int(particle2))); return len(self.exclusions) - 1
    def getNumExclusions(self): return len(self.exclusions)
    def getExclusionParticles(self, idx): return list(self.exclusions[idx])
    def addTabulatedFunction(self, name, function):
        self.functions.append((str(name), function)); return len(self.functions) - 1
    def getNumTabulatedFunctions(self): return len(self.functions)
    def getTabulatedFunctionName(self, idx): return self.functions[idx][0]
    def getTabulatedFunction(self, idx): return self.functions[idx][1]
    def getNonbondedMethod(self): return self._method
    def setNonbondedMethod(self, m): self._method = int(m)
    def getCutoffDistance(self): return self._cutoff
    def setCutoffDistance(self, d): self._cutoff = float(d)
    def usesPeriodicBoundaryConditions(self): return self._method == CustomGBForce.CutoffPeriodic

    def addEnergyParameterDerivative(self, name):
        raise NotImplementedError('CustomGBForce: energy parameter derivatives (addEnergyParameterDerivative %r) are not supported: the '
                                  'global parameters of a CustomGBForce are folded into its constants' % (name,))

    def getNumEnergyParameterDerivatives(self):
        return 0

    def updateParametersInContext(self, context=None):
        raise NotImplementedError('CustomGBForce: changing particles, exclusions or functions after set_system (updateParametersInContext) is '
                                  'not supported: the engine keeps the tables it was given, build the states again')


class CMMotionRemover(Force):
    def __init__(self, frequency=1):
        super().__init__()
        self.frequency = int(frequency)

    def getFrequency(self):
        return self.frequency


class MonteCarloAnisotropicBarostat(Force):
    """openmm.MonteCarloAnisotropicBarostat: a Monte Carlo barostat that changes one box edge per attempt, among the axes whose scale
    flag is set.  Pressure (three components) in kJ/mol/nm^3 (``p * unit.bar``), temperature in K.  Carries no energy: the engine's
    per-axis barostat (include/remd_hip_barostat.h) makes the moves, for the states of a ThermodynamicState on this System."""

    def __init__(self, defaultPressure, defaultTemperature, scaleX=True, scaleY=True, scaleZ=True, frequency=25):
        super().__init__()
        self.setDefaultPressure(defaultPressure)
        self.setDefaultTemperature(defaultTemperature)
        self._scale = (bool(scaleX), bool(scaleY), bool(scaleZ))
        self.setFrequency(frequency)

    def getDefaultPressure(self): return self._pressure
    def setDefaultPressure(self, pressure):
        from .unit import to_md
        p = tuple(float(v) for v in np.asarray(to_md(pressure), dtype=np.float64).reshape(-1))
        if len(p) != 3:
            raise ValueError('MonteCarloAnisotropicBarostat takes the pressure along the three axes')
        self._pressure = p
    def getDefaultTemperature(self): return self._temperature
    def setDefaultTemperature(self, temperature):
        from .unit import to_md
        self._temperature = float(to_md(temperature))
    def getScaleX(self): return self._scale[0]
    def getScaleY(self): return self._scale[1]
    def getScaleZ(self): return self._scale[2]
    def getFrequency(self): return self._frequency
    def setFrequency(self, frequency): self._frequency = int(frequency)
    def usesPeriodicBoundaryConditions(self): return False      # (as OpenMM's barostats answer: the other forces decide)


class MonteCarloMembraneBarostat(Force):
    """openmm.MonteCarloMembraneBarostat: pressure (kJ/mol/nm^3, ``p * unit.bar``) and surface tension (kJ/mol/nm^2,
    ``g * unit.bar * unit.nanometer``) on a box whose xy plane holds a membrane; ``xymode`` couples or frees the two in-plane edges,
    ``zmode`` frees or fixes z or ties it to the plane at constant volume.  Carries no energy, like the anisotropic barostat."""
    XYIsotropic, XYAnisotropic = 0, 1
    ZFree, ZFixed, ConstantVolume = 0, 1, 2

    def __init__(self, defaultPressure, defaultSurfaceTension, defaultTemperature, xymode, zmode, frequency=25):
        super().__init__()
        self.setDefaultPressure(defaultPressure)
        self.setDefaultSurfaceTension(defaultSurfaceTension)
        self.setDefaultTemperature(defaultTemperature)
        self.setXYMode(xymode)
        self.setZMode(zmode)
        self.setFrequency(frequency)

    def getDefaultPressure(self): return self._pressure
    def setDefaultPressure(self, pressure):
        from .unit import to_md
        self._pressure = float(to_md(pressure))
    def getDefaultSurfaceTension(self): return self._surface_tension
    def setDefaultSurfaceTension(self, surfaceTension):
        from .unit import to_md
        self._surface_tension = float(to_md(surfaceTension))
    def getDefaultTemperature(self): return self._temperature
    def setDefaultTemperature(self, temperature):
        from .unit import to_md
        self._temperature = float(to_md(temperature))
    def getXYMode(self): return self._xymode
    def setXYMode(self, mode):
        if int(mode) not in (self.XYIsotropic, self.XYAnisotropic):
            raise ValueError('unknown xy mode %r' % (mode,))
        self._xymode = int(mode)
    def getZMode(self): return self._zmode
    def setZMode(self, mode):
        if int(mode) not in (self.ZFree, self.ZFixed, self.ConstantVolume):
            raise ValueError('unknown z mode %r' % (mode,))
        self._zmode = int(mode)
    def getFrequency(self): return self._frequency
    def setFrequency(self, frequency): self._frequency = int(frequency)
    def usesPeriodicBoundaryConditions(self): return False      # (as OpenMM's barostats answer: the other forces decide)


class VirtualSite:
    """A massless particle whose position is a fixed function of its parents' (OpenMM's VirtualSite; csrc/virtual_sites.hip)."""
    kind = -1

    def __init__(self, particles, weights):
        self._particles = tuple(int(p) for p in particles)
        self._weights = tuple(float(w) for w in weights)
        if any(not math.isfinite(w) for w in self._weights):
            raise ValueError('%s: a weight is not finite' % type(self).__name__)

    def getNumParticles(self):
        return len(self._particles)

    def getParticle(self, particle):
        return self._particles[particle]

    def __eq__(self, other):
        return type(self) is type(other) and self._particles == other._particles and self._weights == other._weights

    def __hash__(self):
        return hash((type(self).__name__, self._particles, self._weights))


class TwoParticleAverageSite(VirtualSite):
    """x = w1 x1 + w2 x2."""
    kind = 0

    def __init__(self, particle1, particle2, weight1, weight2):
        super().__init__((particle1, particle2), (weight1, weight2))

    def getWeight(self, particle):
        return self._weights[particle]


class ThreeParticleAverageSite(VirtualSite):
    """x = w1 x1 + w2 x2 + w3 x3."""
    kind = 1

    def __init__(self, particle1, particle2, particle3, weight1, weight2, weight3):
        super().__init__((particle1, particle2, particle3), (weight1, weight2, weight3))

    def getWeight(self, particle):
        return self._weights[particle]


class OutOfPlaneSite(VirtualSite):
    """x = x1 + w12 r12 + w13 r13 + wcross (r12 x r13), r12 = x2 - x1, r13 = x3 - x1."""
    kind = 2

    def __init__(self, particle1, particle2, particle3, weight12, weight13, weightCross):
        super().__init__((particle1, particle2, particle3), (weight12, weight13, weightCross))

    def getWeight12(self):
        return self._weights[0]

    def getWeight13(self):
        return self._weights[1]

    def getWeightCross(self):
        return self._weights[2]


class System:
    # particle index -> VirtualSite.  An instance gets a dict of its own with its first setVirtualSite: a System without sites
    # pickles as it always did (the stores' bytes are pinned).
    virtual_sites = types.MappingProxyType({})

    def __init__(self):
        self.masses = []
        self.forces = []
        self.constraints = []
        self._box = ((2.0, 0.0, 0.0), (0.0, 2.0, 0.0), (0.0, 0.0, 2.0))
        self.alchemical_region = None     # set by alchemy.AbsoluteAlchemicalFactory (one region on the pair kernels' own path)
        self.alchemical_regions = None    # ... general regions: the factory's force split (alchemical_region_terms, csrc/alch_regions.hip)

    def addParticle(self, mass):
        self.masses.append(float(mass))
        return len(self.masses) - 1

    def getNumParticles(self):
        return len(self.masses)

    def getParticleMass(self, i):
        return self.masses[i]

    def addForce(self, force):
        self.forces.append(force)
        return len(self.forces) - 1

    def getNumForces(self):
        return len(self.forces)

    def getForce(self, i):
        return self.forces[i]

    def getForces(self):
        return list(self.forces)

    def addConstraint(self, i, j, distance):
        self.constraints.append((int(i), int(j), float(distance)))
        return len(self.constraints) - 1

    def getNumConstraints(self):
        return len(self.constraints)

    def getConstraintParameters(self, idx):
        return self.constraints[idx]

    def setVirtualSite(self, index, virtualSite):
        """Make particle ``index`` (mass 0) a virtual site; what the System cannot run is refused by system_to_desc."""
        index = int(index)
        if not 0 <= index < len(self.masses):
            raise ValueError('setVirtualSite: particle index %d out of range' % index)
        if not isinstance(virtualSite, VirtualSite):
            raise NotImplementedError('setVirtualSite: %s is not supported (TwoParticleAverageSite, ThreeParticleAverageSite and '
                                      'OutOfPlaneSite are)' % type(virtualSite).__name__)
        if 'virtual_sites' not in self.__dict__:
            self.virtual_sites = {}
        self.virtual_sites[index] = virtualSite

    def isVirtualSite(self, index):
        return int(index) in self.virtual_sites

    def getVirtualSite(self, index):
        if int(index) not in self.virtual_sites:
            raise ValueError('getVirtualSite: particle %d is not a virtual site' % int(index))
        return self.virtual_sites[int(index)]

    def setDefaultPeriodicBoxVectors(self, a, b, c):
        self._box = (tuple(float(v) for v in a), tuple(float(v) for v in b), tuple(float(v) for v in c))

    def getDefaultPeriodicBoxVectors(self):
        return np.array(self._box, dtype=np.float64)

    def usesPeriodicBoundaryConditions(self):
        return any(getattr(f, 'usesPeriodicBoundaryConditions', lambda: False)() for f in self.forces)

    def fingerprint(self):
        """Stable hash of the system's content (stand-in for the XML hash, states.py:1492-1495)."""
        hsh = hashlib.sha1()

        def feed(d):
            for key in sorted(d):
                v = d[key]
                hsh.update(key.encode())
                if isinstance(v, dict):
                    feed(v)
                else:
                    hsh.update(np.ascontiguousarray(v).tobytes() if isinstance(v, np.ndarray) else repr(v).encode())
        feed(system_to_desc(self))
        return hsh.hexdigest()


# ---------------------------------------------------------------------------------------------

def ewald_parameters(cutoff, tolerance, box):
    """alpha and mesh size from the Ewald error tolerance.

    alpha = sqrt(-ln(2 tol))/r_c (the formula the reference quotes at alchemy.py:1528-1532);
    mesh >= 2 alpha L / (3 tol^(1/5)) per axis, rounded up to a product of 2, 3, 5 (the radices of the
    in-tree FFT).
    """
    alpha = math.sqrt(-math.log(2.0 * tolerance)) / cutoff
    grid = []
    for L in box:
        n = int(math.ceil(2.0 * alpha * L / (3.0 * tolerance ** 0.2)))
        n = max(n, 6)
        while True:
            m = n
            for p in (2, 3, 5):
                while m % p == 0:
                    m //= p
            if m == 1:
                break
            n += 1
        grid.append(n)
    return alpha, grid


def rebalanced_coulomb_cutoff(cutoff, tolerance, box, max_extension=1.25, min_edge=None):
    """Range of the Ewald direct-space sum that the device engine prefers for this box (``ewald_split='auto'``), or ``cutoff``.

    The Ewald sum does not depend on where it is split; OpenMM ties the split to the NonbondedForce cutoff
    (alpha = sqrt(-ln 2 tol) / r_c, the rule quoted at alchemy.py:1528-1532), which for AlanineDipeptideExplicit means a
    75 x 75 x 72 mesh.  On the MI355X the mesh chain (spread -> planes -> gather) is the critical path of an MD step and the
    plane pass quantises badly: an nx x ny plane of complex f32 must fit the LDS several times per CU, and power-of-two lines
    need a third fewer butterfly stages.  So the Coulomb range is stretched, by at most ``max_extension``, to the shortest
    range >= cutoff for which the SAME tolerance rule asks for a mesh whose largest edge is one of the plane-friendly sizes
    below; Lennard-Jones terms keep ``cutoff``.  Measured on 24 x alanine dipeptide: profiles/r04_ewald_split_sweep.txt.
    """
    friendly = (32, 40, 48, 64, 80, 96, 128)
    root = math.sqrt(-math.log(2.0 * tolerance))
    lmax = max(float(L) for L in box)
    # (min_edge: the shortest box edge the run may see -- the smallest starting box of an ensemble, less a margin under a barostat;
    # twice the stretched range must stay below it)
    lmin = min(float(L) for L in box) if min_edge is None else min(float(min_edge), min(float(L) for L in box))
    n_ref = max(ewald_parameters(cutoff, tolerance, box)[1])
    best = cutoff
    for n in friendly:
        if n >= n_ref:
            break
        # largest alpha whose rule mesh is <= n on the longest edge, a hair inside the ceil()
        alpha = (n - 1e-6) * 3.0 * tolerance ** 0.2 / (2.0 * lmax)
        rcc = root / alpha
        if cutoff < rcc <= max_extension * cutoff and 2.0 * rcc < lmin:
            best = rcc
    return best


def _classify_constraints(system):
    """Split distance constraints into rigid 3-site waters (SETTLE) and X-H star clusters (SHAKE)."""
    n = system.getNumParticles()
    adj = [[] for _ in range(n)]
    for (i, j, d) in system.constraints:
        adj[i].append((j, d))
        adj[j].append((i, d))
    seen = [False] * n
    settle, shake, shake_d = [], [], []
    for a in range(n):
        if seen[a] or not adj[a]:
            continue
        comp, stack = [], [a]
        seen[a] = True
        while stack:
            u = stack.pop()
            comp.append(u)
            for (w, _) in adj[u]:
                if not seen[w]:
                    seen[w] = True
                    stack.append(w)
        comp.sort()
        ncons = sum(len(adj[u]) for u in comp) // 2
        if len(comp) == 3 and ncons == 3:
            # triangle: the heavy atom is the one with the largest mass
            o = max(comp, key=lambda u: system.masses[u])
            hs = [u for u in comp if u != o]
            d_oh = [d for (w, d) in adj[o] if w == hs[0]][0]
            d_oh2 = [d for (w, d) in adj[o] if w == hs[1]][0]
            d_hh = [d for (w, d) in adj[hs[0]] if w == hs[1]][0]
            if abs(d_oh - d_oh2) > 1e-9 or abs(system.masses[hs[0]] - system.masses[hs[1]]) > 1e-9:
                raise NotImplementedError('asymmetric rigid triangle constraints are not supported')
            settle.append((o, hs[0], hs[1], d_oh, d_hh))
        else:
            centre = max(comp, key=lambda u: len(adj[u]))
            if ncons != len(comp) - 1 or len(adj[centre]) != ncons or len(comp) > 4:
                raise NotImplementedError('constraint topology must be rigid water or X-H(1..3) star clusters')
            hs = [w for (w, _) in adj[centre]]
            ds = [d for (_, d) in adj[centre]]
            shake.append([centre] + hs + [-1] * (3 - len(hs)))
            shake_d.append(ds + [0.0] * (3 - len(ds)))
    # the engine's analytic solve takes its centre of mass from ONE set of masses, the first water's (remd_build_constraints)
    for s in settle:
        if any(abs(system.masses[s[k]] - system.masses[settle[0][k]]) > 1e-9 for k in range(3)):
            raise NotImplementedError('all rigid waters must share one set of masses (a D2O or 18-O water among H2O is not supported)')
    return settle, shake, shake_d


def _virtual_site_table(system, d):
    """The site table of remd_set_virtual_sites (include/remd_hip_vsites.h) or None, and every refusal that needs the whole System.

    ``molecule``: per site, the smallest particle index of the molecule it is counted into -- its parents'.  Molecules are the
    connected components of bonds, constraints and exceptions (the engine's molecule table takes exceptions and constraints), a
    site joined to its parents."""
    sites = getattr(system, 'virtual_sites', None) or {}
    n = system.getNumParticles()
    for i, m in enumerate(system.masses):
        if m == 0.0 and i not in sites:
            raise ValueError('massless particles are not supported: particle %d has mass 0 and is not a virtual site' % i)
    if not sites:
        return None
    constrained = {p for (i, j, _) in system.constraints for p in (i, j)}
    for s, site in sorted(sites.items()):
        if not isinstance(site, VirtualSite) or site.kind not in (0, 1, 2):
            raise NotImplementedError('virtual site %d: %s is not supported (TwoParticleAverageSite, ThreeParticleAverageSite and '
                                      'OutOfPlaneSite are)' % (s, type(site).__name__))
        if system.masses[s] != 0.0:
            raise ValueError('virtual site %d has mass %g: a virtual site must have mass 0' % (s, system.masses[s]))
        if s in constrained:
            raise ValueError('virtual site %d takes part in a constraint' % s)
        parents = [site.getParticle(k) for k in range(site.getNumParticles())]
        for p in parents:
            if not 0 <= p < n:
                raise ValueError('virtual site %d: parent index %d out of range' % (s, p))
            if p in sites:
                raise NotImplementedError('virtual site %d: parent %d is itself a virtual site (sites on top of sites are not supported)' % (s, p))
        if len(set(parents)) != len(parents):
            raise ValueError('virtual site %d: a parent is named twice %r' % (s, tuple(parents)))
    # molecules without the sites' own links: the parents of a site must already lie in one
    root = list(range(n))

    def find(a):
        while root[a] != a:
            root[a] = root[root[a]]
            a = root[a]
        return a

    def unite(a, b):
        a, b = find(a), find(b)
        if a != b:
            root[max(a, b)] = min(a, b)
    for (i, j, _) in system.constraints:
        unite(i, j)
    for k in range(len(d['bond_atoms'])):
        unite(int(d['bond_atoms'][k][0]), int(d['bond_atoms'][k][1]))
    exc = [(int(e[0]), int(e[1])) for e in d['exception_atoms']]
    for (i, j) in exc:
        if i not in sites and j not in sites:
            unite(i, j)
    periodic = d['nb_method'] in (1, 2) or system.usesPeriodicBoundaryConditions()
    linked = {s: set() for s in sites}
    for (i, j) in exc:
        if i in sites:
            linked[i].add(j)
        if j in sites:
            linked[j].add(i)
    order = sorted(sites)
    molecule = []
    for s in order:
        site = sites[s]
        parents = [site.getParticle(k) for k in range(site.getNumParticles())]
        mols = {find(p) for p in parents}
        if periodic and len(mols) != 1:
            raise ValueError('virtual site %d: its parents %r lie in different molecules of a periodic System (positions are taken '
                             'without minimum images; a molecule is kept whole)' % (s, tuple(parents)))
        if periodic and d['nb_method'] in (1, 2) and not (linked[s] & set(parents)):
            raise ValueError('virtual site %d has no exception with any of its parents: the engine counts it into their molecule '
                             'through the exceptions of the NonbondedForce' % s)
        molecule.append(min(mols))
    width = np.full((len(order), 3), -1, dtype=np.int32)
    weight = np.zeros((len(order), 3), dtype=np.float64)
    for row, s in enumerate(order):
        site = sites[s]
        for k in range(site.getNumParticles()):
            width[row, k] = site.getParticle(k)
        weight[row, :len(site._weights)] = site._weights
    return dict(site=np.array(order, dtype=np.int32), kind=np.array([sites[s].kind for s in order], dtype=np.int32),
                parent=width, weight=weight, molecule=np.array(molecule, dtype=np.int32))


def _is_restraint(force):
    from .forces import is_restraint_force
    return is_restraint_force(force)


def _is_custom_term(force):
    from .custom_expr import is_custom_term_force
    return is_custom_term_force(force)


def system_to_desc(system, box=None, ewald_split=None, min_edge=None):
    """Flatten a System into the arrays of remd_system_desc (include/remd_hip.h).

    ewald_split: None / 'reference' = OpenMM's rule (alpha and mesh from the NonbondedForce cutoff); 'auto' = the Coulomb range
    of ``rebalanced_coulomb_cutoff``; a number = that Coulomb range in nm.  With a range beyond the cutoff the descriptor
    carries ``coulomb_cutoff`` (-> remd_set_coulomb_cutoff) and the alpha / mesh that the same tolerance rule gives for it.
    """
    n = system.getNumParticles()
    d = dict(n_atoms=n, mass=np.array(system.masses, dtype=np.float64))
    d.update(n_ext=0, ext_atoms=np.zeros(0, np.int32), ext_K=0.0, ext_x0=0.0, ext_U0=0.0)
    bonds, angles, torsions = [], [], []
    nb = None
    gb = None
    cmm = 0
    restraints = []                     # receptor-ligand restraints (forces.py): remd_set_restraints, include/remd_hip_restraints.h
    custom = []                         # custom bond / angle / torsion / external expressions: remd_set_custom_terms, include/remd_hip_custom.h
    # force groups of (external, bonds, angles, torsions, nonbonded direct, PME reciprocal): remd_set_force_groups
    fg = [0, 0, 0, 0, 0, 0]
    for f in system.forces:
        g = f.getForceGroup() if hasattr(f, 'getForceGroup') else 0
        if isinstance(f, CustomExternalForce):
            if f.is_harmonic_oscillator():
                fg[0] = g
        elif isinstance(f, HarmonicBondForce):
            fg[1] = g
        elif isinstance(f, HarmonicAngleForce):
            fg[2] = g
        elif isinstance(f, PeriodicTorsionForce):
            fg[3] = g
        elif isinstance(f, NonbondedForce):
            fg[4] = g
            fg[5] = g if f.getReciprocalSpaceForceGroup() < 0 else f.getReciprocalSpaceForceGroup()
    d['force_groups'] = np.array(fg, dtype=np.int32)
    for f in system.forces:
        if _is_custom_term(f):
            custom.append(f)
        elif isinstance(f, CustomExternalForce):
            if getattr(f, '_derivatives', None):
                raise NotImplementedError('CustomExternalForce: energy parameter derivatives (addEnergyParameterDerivative %r) of the built-in '
                                          'harmonic oscillator form are not supported' % (f._derivatives[0],))
            d['n_ext'] = len(f.particles)
            d['ext_atoms'] = np.array(f.particles, dtype=np.int32)
            d['ext_K'] = f.globals['testsystems_HarmonicOscillator_K']
            d['ext_x0'] = f.globals['testsystems_HarmonicOscillator_x0']
            d['ext_U0'] = f.globals['testsystems_HarmonicOscillator_U0']
        elif isinstance(f, HarmonicBondForce):
            bonds += f.bonds
        elif isinstance(f, HarmonicAngleForce):
            angles += f.angles
        elif isinstance(f, PeriodicTorsionForce):
            torsions += f.torsions
        elif isinstance(f, NonbondedForce):
            if nb is not None:
                raise NotImplementedError('more than one NonbondedForce')
            nb = f
        elif isinstance(f, CMMotionRemover):
            cmm = f.frequency
        elif isinstance(f, (GBSAOBCForce, CustomGBForce)):
            if gb is not None:
                raise NotImplementedError('more than one implicit-solvent force (%s and %s)' % (type(gb).__name__, type(f).__name__))
            gb = f
        elif isinstance(f, (MonteCarloAnisotropicBarostat, MonteCarloMembraneBarostat)):
            pass        # no energy: the ThermodynamicState reads it (states.py) and the sampler hands it to the engine's barostat
        elif _is_restraint(f):
            if getattr(f, '_derivatives', None):
                raise NotImplementedError('%s: energy parameter derivatives (addEnergyParameterDerivative %r) of a restraint force are not '
                                          'supported' % (type(f).__name__, f._derivatives[0]))
            from .forces import restraint_terms
            restraints.append(restraint_terms(f, system.masses))
        else:
            raise NotImplementedError('unsupported force %r' % type(f).__name__)
    d['bond_atoms'] = np.array([b[:2] for b in bonds], dtype=np.int32).reshape(-1, 2)
    d['bond_params'] = np.array([b[2:] for b in bonds], dtype=np.float64).reshape(-1, 2)
    d['angle_atoms'] = np.array([a[:3] for a in angles], dtype=np.int32).reshape(-1, 3)
    d['angle_params'] = np.array([a[3:] for a in angles], dtype=np.float64).reshape(-1, 2)
    d['torsion_atoms'] = np.array([t[:4] for t in torsions], dtype=np.int32).reshape(-1, 4)
    d['torsion_params'] = np.array([t[4:] for t in torsions], dtype=np.float64).reshape(-1, 3)
    d.update(nb_method=0, cutoff=0.0, switch_distance=-1.0, rf_dielectric=78.3, ewald_alpha=0.0,
             pme_grid=np.zeros(3, np.int32), use_dispersion_correction=0,
             charge=np.zeros(n), sigma=np.zeros(n), epsilon=np.zeros(n),
             exception_atoms=np.zeros((0, 2), np.int32), exception_params=np.zeros((0, 3)))
    if nb is not None:
        if nb.getNumParticles() != n:
            raise ValueError('NonbondedForce has %d particles, system has %d' % (nb.getNumParticles(), n))
        method = nb.getNonbondedMethod()
        if method == NonbondedForce.CutoffPeriodic:
            d['nb_method'] = 1
        elif method == NonbondedForce.PME:
            d['nb_method'] = 2
        elif method == NonbondedForce.NoCutoff:
            d['nb_method'] = 3                      # REMD_NB_NOCUTOFF: every pair, no box (the vacuum test systems; csrc/nocutoff.hip)
        else:
            raise NotImplementedError('nonbonded method %d (only NoCutoff, CutoffPeriodic and PME are supported)' % method)
        nocut = d['nb_method'] == 3                 # OpenMM ignores cutoff, switching function and dispersion correction without a cutoff
        d['cutoff'] = 0.0 if nocut else nb.getCutoffDistance()
        d['switch_distance'] = nb.getSwitchingDistance() if (nb.getUseSwitchingFunction() and not nocut) else -1.0
        d['rf_dielectric'] = nb.getReactionFieldDielectric()
        d['use_dispersion_correction'] = int(nb.getUseDispersionCorrection() and not nocut)
        p = np.array(nb.particles, dtype=np.float64).reshape(-1, 3)
        d['charge'], d['sigma'], d['epsilon'] = p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()
        d['exception_atoms'] = np.array([e[:2] for e in nb.exceptions], dtype=np.int32).reshape(-1, 2)
        d['exception_params'] = np.array([e[2:] for e in nb.exceptions], dtype=np.float64).reshape(-1, 3)
        if d['nb_method'] == 2:
            if box is None:
                box = np.diag(system.getDefaultPeriodicBoxVectors())
            if nb._pme_params is not None:
                d['ewald_alpha'] = nb._pme_params[0]
                d['pme_grid'] = np.array(nb._pme_params[1:], dtype=np.int32)
            else:
                tol = nb.getEwaldErrorTolerance()
                rcc = d['cutoff']
                if ewald_split == 'auto':
                    rcc = rebalanced_coulomb_cutoff(d['cutoff'], tol, box, min_edge=min_edge)
                elif ewald_split not in (None, 'reference'):
                    rcc = float(ewald_split)
                    if rcc < d['cutoff']:
                        raise ValueError('ewald_split: the Coulomb range cannot be shorter than the nonbonded cutoff')
                alpha, grid = ewald_parameters(rcc, tol, box)
                d['ewald_alpha'] = alpha
                d['pme_grid'] = np.array(grid, dtype=np.int32)
                if rcc > d['cutoff']:
                    d['coulomb_cutoff'] = rcc
    sites = _virtual_site_table(system, d)          # (in front of the constraint classification: a site takes no part in it)
    if sites is not None:
        d['virtual_sites'] = sites
    settle, shake, shake_d = _classify_constraints(system)
    d['settle_atoms'] = np.array([s[:3] for s in settle], dtype=np.int32).reshape(-1, 3)
    d['settle_dOH'] = settle[0][3] if settle else 0.0
    d['settle_dHH'] = settle[0][4] if settle else 0.0
    for s in settle:
        if abs(s[3] - d['settle_dOH']) > 1e-9 or abs(s[4] - d['settle_dHH']) > 1e-9:
            raise NotImplementedError('all rigid waters must share one geometry')
    d['shake_atoms'] = np.array(shake, dtype=np.int32).reshape(-1, 4)
    d['shake_dist'] = np.array(shake_d, dtype=np.float64).reshape(-1, 3)
    d['cmm_frequency'] = cmm
    region = getattr(system, 'alchemical_region', None)
    if region is not None:
        d['alch_atoms'] = np.array(sorted(region.alchemical_atoms), dtype=np.int32)
        d['softcore'] = (region.softcore_alpha, region.softcore_a, region.softcore_b, region.softcore_c)
        d['annihilate_sterics'] = bool(region.annihilate_sterics)          # -> remd_set_alchemical_options
    else:
        d['alch_atoms'] = np.zeros(0, np.int32)
        d['softcore'] = (0.5, 1.0, 1.0, 6.0)
        d['annihilate_sterics'] = False
    if isinstance(gb, CustomGBForce):
        # a CustomGBForce of the OBC family: remd_set_gbsa + remd_set_gb_model (include/remd_hip_gb.h)
        from .custom_gb import custom_gb_to_desc
        if box is None:
            box = np.diag(system.getDefaultPeriodicBoxVectors())
        gbsa = custom_gb_to_desc(gb, n, d['nb_method'], box)
        if gbsa is None:                    # not of the OBC templates: the general path, one of the custom forces (csrc/custom_gb.hip)
            custom.append(gb)
        else:
            d['gbsa'] = gbsa
    elif gb is not None:
        # implicit solvent: remd_set_gbsa (csrc/gbsa.hip).  The surface term is the ACE one with OpenMM's default energy (28.3919551 = 4 pi x
        # 2.25936 kJ/mol/nm^2 in the factory's expression, alchemy.py:2207); 0 switches it off
        if d['nb_method'] != 3 or gb.getNonbondedMethod() != GBSAOBCForce.NoCutoff:
            raise NotImplementedError('GBSAOBCForce with a cutoff (only NoCutoff implicit-solvent systems are supported)')
        if gb.getNumParticles() != n:
            raise ValueError('GBSAOBCForce has %d particles, system has %d' % (gb.getNumParticles(), n))
        if gb.getSurfaceAreaEnergy() not in (0.0, 2.25936):
            raise NotImplementedError('GBSAOBCForce surface area energy %r (OpenMM\'s default 2.25936 kJ/mol/nm^2 or 0)' % gb.getSurfaceAreaEnergy())
        gp = np.array(gb.particles, dtype=np.float64).reshape(-1, 3)
        alch = np.zeros(n, dtype=np.int32)
        regions = getattr(system, 'alchemical_regions', None)
        if regions is not None:                       # the factory's alchemical GBSA: one region (alchemy.py:2168-2171)
            alch[regions[0].alchemical_atoms] = 1
        from .custom_gb import OBC2_MODEL
        d['gbsa'] = dict(charge=gp[:, 0].copy(), radius=gp[:, 1].copy(), scale=gp[:, 2].copy(), alchemical=alch,
                         solute_dielectric=gb.getSoluteDielectric(), solvent_dielectric=gb.getSolventDielectric(),
                         surface_area=int(gb.getSurfaceAreaEnergy() != 0.0), **OBC2_MODEL)
    if getattr(system, 'rf_unshifted_switch_width', None) is not None and d['nb_method'] == 1:
        # the reaction field as the alchemical factory re-writes it for the WHOLE system (alchemical_rf_treatment='switched'): remd_set_reaction_field
        d['rf_unshifted_switch_width'] = float(system.rf_unshifted_switch_width)
    if restraints:
        # keyed by position ('000', '001', ...): the fingerprint hashes every array of a nested dict
        d['restraints'] = {'%03d' % k: r for k, r in enumerate(restraints)}
    if custom:
        from .custom_expr import custom_terms_desc
        terms = custom_terms_desc(custom, system.masses, box_vectors=system.getDefaultPeriodicBoxVectors())
        for f in custom:                     # (what an engine is given does not follow a later addEnergyParameterDerivative)
            if hasattr(f, '_derivatives'):
                f._in_engine = id(f)
        if terms:
            from .custom_expr import check_cv_molecules, check_hbond_molecules
            check_cv_molecules(d, terms)
            check_hbond_molecules(d, terms)
            d['custom_terms'] = terms
            # the handle's global-parameter columns, once (every entry above repeats them for remd_custom_force_desc)
            first = terms['000']
            d['custom_globals'] = dict(names=list(first['global_names']), defaults=first['global_defaults'].copy())
    if getattr(system, 'alchemical_regions', None) is not None:
        # general regions: this descriptor is the NonbondedForce the factory leaves behind, the custom forces follow through
        # remd_set_alchemical_regions (alchemy.AbsoluteAlchemicalFactory._region_terms)
        d['alch_regions'] = dict(system.alchemical_region_terms)
    return d


def virtual_site_from_openmm(site):
    """An OpenMM virtual site as the class of the same name here; by the object's class name and getters, so that no OpenMM is needed."""
    name = type(site).__name__
    p = [int(site.getParticle(k)) for k in range(site.getNumParticles())] if hasattr(site, 'getNumParticles') else []
    if name == 'TwoParticleAverageSite':
        return TwoParticleAverageSite(p[0], p[1], site.getWeight(0), site.getWeight(1))
    if name == 'ThreeParticleAverageSite':
        return ThreeParticleAverageSite(p[0], p[1], p[2], site.getWeight(0), site.getWeight(1), site.getWeight(2))
    if name == 'OutOfPlaneSite':
        return OutOfPlaneSite(p[0], p[1], p[2], site.getWeight12(), site.getWeight13(), site.getWeightCross())
    raise NotImplementedError('virtual site class %s is not supported (TwoParticleAverageSite, ThreeParticleAverageSite and '
                              'OutOfPlaneSite are)' % name)


def _functions_from_openmm(f, g, cls_name):
    """the tabulated functions of ``f`` added to ``g``: taken over as they are when they are this module's classes, rebuilt from
    getFunctionParameters() by class name otherwise"""
    functions = dict(Continuous1DFunction=Continuous1DFunction, Discrete1DFunction=Discrete1DFunction, Continuous2DFunction=Continuous2DFunction,
                     Discrete2DFunction=Discrete2DFunction, Discrete3DFunction=Discrete3DFunction)
    for i in range(f.getNumTabulatedFunctions()):
        fn, name = f.getTabulatedFunction(i), f.getTabulatedFunctionName(i)
        cls = type(fn).__name__
        if cls not in functions:
            raise NotImplementedError('%s: tabulated function %r is a %s (Continuous1DFunction, Discrete1DFunction, '
                                      'Continuous2DFunction, Discrete2DFunction and Discrete3DFunction are supported)' % (cls_name, name, cls))
        if not isinstance(fn, tuple(functions.values())):
            args = list(fn.getFunctionParameters())
            fn = functions[cls](*args, **(dict(periodic=bool(fn.getPeriodic())) if hasattr(fn, 'getPeriodic') else {}))
        g.addTabulatedFunction(name, fn)


def _derivatives_from_openmm(f, g):
    """the energy parameter derivatives ``f`` declares, declared on ``g`` (an object without the getters declares none)"""
    for i in range(f.getNumEnergyParameterDerivatives() if hasattr(f, 'getNumEnergyParameterDerivatives') else 0):
        g.addEnergyParameterDerivative(f.getEnergyParameterDerivativeName(i))


def manyparticle_force_from_openmm(f):
    """An openmm.CustomManyParticleForce as the class of the same name here; by the object's getters, so that no OpenMM is needed.
    The cutoff may carry a unit (anything with value_in_unit_system) or be a number in nm; an empty type filter means none."""
    g = CustomManyParticleForce(f.getNumParticlesPerSet(), f.getEnergyFunction())
    for i in range(f.getNumPerParticleParameters()):
        g.addPerParticleParameter(f.getPerParticleParameterName(i))
    for i in range(f.getNumGlobalParameters()):
        g.addGlobalParameter(f.getGlobalParameterName(i), f.getGlobalParameterDefaultValue(i))
    _functions_from_openmm(f, g, 'CustomManyParticleForce')
    for i in range(f.getNumParticles()):
        parameters, type = f.getParticleParameters(i)
        g.addParticle(parameters, type)
    for i in range(f.getNumExclusions()):
        g.addExclusion(*f.getExclusionParticles(i))
    g.setNonbondedMethod(int(f.getNonbondedMethod()))
    cutoff = f.getCutoffDistance()
    if hasattr(cutoff, 'value_in_unit_system'):
        from .unit import to_md
        cutoff = to_md(cutoff)
    g.setCutoffDistance(cutoff)
    g.setPermutationMode(int(f.getPermutationMode()))
    for s in range(3):
        types = list(f.getTypeFilter(s))
        if types:
            g.setTypeFilter(s, types)
    _derivatives_from_openmm(f, g)
    g.setForceGroup(int(f.getForceGroup()))
    return g


def gb_force_from_openmm(f):
    """An openmm.CustomGBForce as the class of the same name here; by the object's getters, so that no OpenMM is needed.  The cutoff may
    carry a unit (anything with value_in_unit_system) or be a number in nm; functions are taken over as they are when they are this
    module's classes and rebuilt from getFunctionParameters() by class name otherwise (a GBn / GBn2 System brings its neck tables)."""
    g = CustomGBForce()
    for i in range(f.getNumPerParticleParameters()):
        g.addPerParticleParameter(f.getPerParticleParameterName(i))
    for i in range(f.getNumGlobalParameters()):
        g.addGlobalParameter(f.getGlobalParameterName(i), f.getGlobalParameterDefaultValue(i))
    _functions_from_openmm(f, g, 'CustomGBForce')
    for i in range(f.getNumComputedValues()):
        name, expression, kind = f.getComputedValueParameters(i)
        g.addComputedValue(name, expression, int(kind))
    for i in range(f.getNumEnergyTerms()):
        expression, kind = f.getEnergyTermParameters(i)
        g.addEnergyTerm(expression, int(kind))
    for i in range(f.getNumParticles()):
        g.addParticle(list(f.getParticleParameters(i)))
    for i in range(f.getNumExclusions()):
        g.addExclusion(*f.getExclusionParticles(i))
    g.setNonbondedMethod(int(f.getNonbondedMethod()))
    cutoff = f.getCutoffDistance()
    if hasattr(cutoff, 'value_in_unit_system'):
        from .unit import to_md
        cutoff = to_md(cutoff)
    g.setCutoffDistance(cutoff)
    _derivatives_from_openmm(f, g)          # (a CustomGBForce refuses them by name)
    g.setForceGroup(int(f.getForceGroup()))
    return g


def hbond_force_from_openmm(f):
    """An openmm.CustomHbondForce as the class of the same name here; by the object's getters, so that no OpenMM is needed.  The cutoff
    may carry a unit (anything with value_in_unit) or be a number in nm; functions are taken over as they are when they are this
    module's classes and rebuilt from getFunctionParameters() by class name otherwise."""
    g = CustomHbondForce(f.getEnergyFunction())
    for i in range(f.getNumPerDonorParameters()):
        g.addPerDonorParameter(f.getPerDonorParameterName(i))
    for i in range(f.getNumPerAcceptorParameters()):
        g.addPerAcceptorParameter(f.getPerAcceptorParameterName(i))
    for i in range(f.getNumGlobalParameters()):
        g.addGlobalParameter(f.getGlobalParameterName(i), f.getGlobalParameterDefaultValue(i))
    _functions_from_openmm(f, g, 'CustomHbondForce')
    for i in range(f.getNumDonors()):
        d1, d2, d3, parameters = f.getDonorParameters(i)
        g.addDonor(d1, d2, d3, parameters)
    for i in range(f.getNumAcceptors()):
        a1, a2, a3, parameters = f.getAcceptorParameters(i)
        g.addAcceptor(a1, a2, a3, parameters)
    for i in range(f.getNumExclusions()):
        g.addExclusion(*f.getExclusionParticles(i))
    g.setNonbondedMethod(int(f.getNonbondedMethod()))
    cutoff = f.getCutoffDistance()
    if hasattr(cutoff, 'value_in_unit_system'):
        from .unit import to_md
        cutoff = to_md(cutoff)
    g.setCutoffDistance(cutoff)
    _derivatives_from_openmm(f, g)
    g.setForceGroup(int(f.getForceGroup()))
    return g


def from_openmm(omm_system):
    """Convert a real ``openmm.System`` (only where OpenMM is importable; not exercised in CI here)."""
    import openmm
    from openmm import unit as u
    s = System()
    for i in range(omm_system.getNumParticles()):
        s.addParticle(omm_system.getParticleMass(i).value_in_unit(u.amu))
    a, b, c = omm_system.getDefaultPeriodicBoxVectors()
    s.setDefaultPeriodicBoxVectors(*[v.value_in_unit(u.nanometer) for v in (a, b, c)])
    for i in range(omm_system.getNumConstraints()):
        p, q, dist = omm_system.getConstraintParameters(i)
        s.addConstraint(p, q, dist.value_in_unit(u.nanometer))
    for i in range(omm_system.getNumParticles()):
        if getattr(omm_system, 'isVirtualSite', lambda index: False)(i):
            s.setVirtualSite(i, virtual_site_from_openmm(omm_system.getVirtualSite(i)))
    for f in omm_system.getForces():
        if isinstance(f, openmm.HarmonicBondForce):
            g = HarmonicBondForce()
            for k in range(f.getNumBonds()):
                p, q, r0, kk = f.getBondParameters(k)
                g.addBond(p, q, r0.value_in_unit(u.nanometer), kk.value_in_unit(u.kilojoule_per_mole / u.nanometer ** 2))
        elif isinstance(f, openmm.HarmonicAngleForce):
            g = HarmonicAngleForce()
            for k in range(f.getNumAngles()):
                p, q, r, th, kk = f.getAngleParameters(k)
                g.addAngle(p, q, r, th.value_in_unit(u.radian), kk.value_in_unit(u.kilojoule_per_mole / u.radian ** 2))
        elif isinstance(f, openmm.PeriodicTorsionForce):
            g = PeriodicTorsionForce()
            for k in range(f.getNumTorsions()):
                p, q, r, t, per, ph, kk = f.getTorsionParameters(k)
                g.addTorsion(p, q, r, t, per, ph.value_in_unit(u.radian), kk.value_in_unit(u.kilojoule_per_mole))
        elif isinstance(f, openmm.NonbondedForce):
            g = NonbondedForce()
            for k in range(f.getNumParticles()):
                q, sig, eps = f.getParticleParameters(k)
                g.addParticle(q.value_in_unit(u.elementary_charge), sig.value_in_unit(u.nanometer),
                              eps.value_in_unit(u.kilojoule_per_mole))
            for k in range(f.getNumExceptions()):
                p, q, qq, sig, eps = f.getExceptionParameters(k)
                g.addException(p, q, qq.value_in_unit(u.elementary_charge ** 2), sig.value_in_unit(u.nanometer),
                               eps.value_in_unit(u.kilojoule_per_mole))
            g.setNonbondedMethod(f.getNonbondedMethod())
            g.setCutoffDistance(f.getCutoffDistance().value_in_unit(u.nanometer))
            g.setUseSwitchingFunction(f.getUseSwitchingFunction())
            g.setSwitchingDistance(f.getSwitchingDistance().value_in_unit(u.nanometer))
            g.setUseDispersionCorrection(f.getUseDispersionCorrection())
            g.setReactionFieldDielectric(f.getReactionFieldDielectric())
            g.setEwaldErrorTolerance(f.getEwaldErrorTolerance())
        elif isinstance(f, openmm.CMMotionRemover):
            g = CMMotionRemover(f.getFrequency())
        elif isinstance(f, openmm.CMAPTorsionForce):
            g = CMAPTorsionForce()
            for k in range(f.getNumMaps()):
                size, energy = f.getMapParameters(k)
                g.addMap(size, energy.value_in_unit(u.kilojoule_per_mole))
            for k in range(f.getNumTorsions()):
                g.addTorsion(*f.getTorsionParameters(k))
            g.setUsesPeriodicBoundaryConditions(f.usesPeriodicBoundaryConditions())
            g.setForceGroup(f.getForceGroup())
        elif type(f).__name__ == 'CustomHbondForce':
            g = hbond_force_from_openmm(f)
        elif type(f).__name__ == 'CustomManyParticleForce':
            g = manyparticle_force_from_openmm(f)
        elif type(f).__name__ == 'CustomGBForce':
            g = gb_force_from_openmm(f)
        else:
            raise NotImplementedError('unsupported OpenMM force %s' % type(f).__name__)
        s.addForce(g)
    return s
