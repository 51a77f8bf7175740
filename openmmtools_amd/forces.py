"""Receptor-ligand restraint forces (openmmtools/forces.py:44-1108).

The reference builds its restraints on ``openmm.CustomCentroidBondForce`` / ``openmm.CustomBondForce``; OpenMM is absent here, so
``CustomCentroidBondForce`` and ``CustomBondForce`` below mirror the subset of their API the restraints use (global parameters,
per-bond parameters, groups with weights, the periodic-boundary flag) on this package's own ``Force`` hierarchy (system.py).  The
energy strings are the reference's, verbatim; the engine evaluates them with a kernel of its own (csrc/restraints.hip), and
``system.system_to_desc`` refuses any other expression.

Quantities are md-unit floats (nm, kJ/mol, kJ/mol/nm^2), as everywhere in this package.
"""
import collections
import inspect
import math
import re
import zlib

import numpy as np

from .system import Force, _CustomForce, CustomBondForce
from .unit import to_md

# 1 L / (N_A mol) in nm^3 (openmmtools/constants.py:18)
STANDARD_STATE_VOLUME = 1.0e24 / 6.02214076e23


class MultipleForcesError(Exception):
    """Error raised when multiple forces of the same class are found."""
    pass


class NoForceFoundError(Exception):
    """Error raised when no forces matching the given criteria are found."""
    pass


# ---- the OpenMM custom forces the restraints build on: CustomBondForce is system.py's, CustomCentroidBondForce as far as they use it ----
class CustomCentroidBondForce(_CustomForce):
    """openmm.CustomCentroidBondForce: groups of particles (weights None = the particles' masses) and bonds between groups."""

    def __init__(self, numGroups, energy):
        super().__init__(energy)
        self._n_groups_per_bond = int(numGroups)
        self._groups = []                     # (particles, weights or None)
        self._bonds = []                      # (groups, parameters)

    def getNumGroupsPerBond(self):
        return self._n_groups_per_bond

    def addGroup(self, particles, weights=None):
        self._groups.append((list(int(p) for p in particles), None if weights is None or len(weights) == 0 else [float(w) for w in weights]))
        return len(self._groups) - 1

    def getNumGroups(self):
        return len(self._groups)

    def getGroupParameters(self, index):
        particles, weights = self._groups[index]
        return list(particles), ([] if weights is None else list(weights))

    def setGroupParameters(self, index, particles, weights=None):
        self._groups[index] = (list(int(p) for p in particles), None if weights is None or len(weights) == 0 else [float(w) for w in weights])

    def addBond(self, groups, parameters=()):
        self._bonds.append((list(int(g) for g in groups), [float(p) for p in parameters]))
        return len(self._bonds) - 1

    def getNumBonds(self):
        return len(self._bonds)

    def getBondParameters(self, index):
        groups, parameters = self._bonds[index]
        return list(groups), list(parameters)

    def setBondParameters(self, index, groups, parameters=()):
        self._bonds[index] = (list(int(g) for g in groups), [float(p) for p in parameters])


# ---- restorable class hash (openmmtools/utils/utils.py:830, 912, 1023-1037) ----------------------------------------------------
_HASH_PARAMETER = '_restorable_force__class_hash'


def _class_hash(cls):
    return float(zlib.adler32(cls.__name__.encode()))


def restore_interface(force):
    """utils.RestorableOpenMMObject.restore_interface: a custom force whose first global parameter is the class hash of one of the
    restraint classes becomes an instance of that class again (a document written by the reference, or by system_xml).  Returns
    True when the interface was restored."""
    if not isinstance(force, _CustomForce) or force.getNumGlobalParameters() == 0 or force.getGlobalParameterName(0) != _HASH_PARAMETER:
        return False
    if isinstance(force, RadiallySymmetricRestraintForce):
        return True
    h = force.getGlobalParameterDefaultValue(0)
    for cls in _RESTRAINT_CLASSES:
        base = CustomCentroidBondForce if issubclass(cls, CustomCentroidBondForce) else CustomBondForce
        if _class_hash(cls) == h and type(force) is base:
            force.__class__ = cls
            return True
    return False


def iterate_forces(system):
    """Iterate over and restore the Python interface of the forces in the system."""
    for force in system.getForces():
        restore_interface(force)
        yield force
    return


def find_forces(system, force_type, only_one=False, include_subclasses=False):
    """forces.py:63-166: the forces of ``system`` of type ``force_type`` (a class, or a regular expression matched against the class
    name), as an OrderedDict {force index: force}; with ``only_one`` the single (index, force) pair, NoForceFoundError /
    MultipleForcesError otherwise."""
    re_pattern = None
    if not inspect.isclass(force_type):
        re_pattern = re.compile(force_type)
    forces = {}
    for force_idx, force in enumerate(iterate_forces(system)):
        if re_pattern is not None:
            if re_pattern.match(force.__class__.__name__):
                forces[force_idx] = force
        elif type(force) is force_type or (include_subclasses and isinstance(force, force_type)):
            forces[force_idx] = force
    if include_subclasses and re_pattern is not None:
        matched_force_classes = [force.__class__ for force in forces.values()]
        for force_idx, force in enumerate(iterate_forces(system)):
            if force_idx in forces:
                continue
            for matched_force_class in matched_force_classes:
                if isinstance(force, matched_force_class):
                    forces[force_idx] = force
    forces = collections.OrderedDict(sorted(forces.items()))
    if only_one is True:
        if len(forces) == 0:
            raise NoForceFoundError(f'No force of type {force_type} could be found.')
        if len(forces) > 1:
            raise MultipleForcesError(f'Found multiple forces of type {force_type}')
        return forces.popitem(last=False)
    return forces


def _compute_sphere_volume(radius):
    """Compute the volume of a square well restraint."""
    return 4.0 / 3 * np.pi * radius ** 3


def _compute_harmonic_volume(radius, spring_constant, beta):
    """forces.py:174-205: volume (nm^3) of exp(-beta K r^2 / 2) from 0 to radius."""
    bk = beta * spring_constant
    bk_2 = bk / 2
    bkr2_2 = bk_2 * radius ** 2
    volume = math.sqrt(math.pi / 2) * math.erf(math.sqrt(bkr2_2)) / bk ** (3.0 / 2)
    volume -= math.exp(-bkr2_2) * radius / bk
    return 4 * math.pi * volume


def _compute_harmonic_radius(spring_constant, potential_energy):
    """forces.py:208-228: the radius at which (K/2) r^2 equals the energy."""
    return math.sqrt(2 * potential_energy / spring_constant)


# ---- restraints ---------------------------------------------------------------------------------------------------------------
class RadiallySymmetricRestraintForce(Force):
    """forces.py:234-669: base class of restraints whose energy depends only on the distance between two groups of atoms.  The first
    global parameter is the restorable class hash, the second the controlling parameter."""

    def __init__(self, restraint_parameters, restrained_atom_indices1, restrained_atom_indices2, controlling_parameter_name,
                 *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.addGlobalParameter(_HASH_PARAMETER, _class_hash(type(self)))
        assert len(restraint_parameters) == 1 or isinstance(restraint_parameters, collections.OrderedDict)
        parameter_names, parameter_values = zip(*restraint_parameters.items())
        self._create_bond([float(to_md(v)) for v in parameter_values], restrained_atom_indices1, restrained_atom_indices2)
        assert self.getNumGlobalParameters() == 1
        self.addGlobalParameter(controlling_parameter_name, 1.0)
        for parameter in parameter_names:
            self.addPerBondParameter(parameter)

    def _create_bond(self, bond_parameter_values, restrained_atom_indices1, restrained_atom_indices2):
        raise NotImplementedError()

    def addEnergyParameterDerivative(self, name):
        raise NotImplementedError('%s: energy parameter derivatives (addEnergyParameterDerivative %r) of a restraint force are not '
                                  'supported (csrc/restraints.hip has no such path)' % (type(self).__name__, name))

    def getNumEnergyParameterDerivatives(self):
        return 0

    @property
    def restraint_parameters(self):
        """OrderedDict: The restraint parameters in dictionary form."""
        parameter_values = self.getBondParameters(0)[-1]
        return collections.OrderedDict((self.getPerBondParameterName(i), v) for i, v in enumerate(parameter_values))

    @property
    def controlling_parameter_name(self):
        """str: The name of the global parameter controlling the energy function (read-only)."""
        return self.getGlobalParameterName(1)

    def distance_at_energy(self, potential_energy):
        """The distance (nm) at which the potential energy (kJ/mol) is ``potential_energy``."""
        raise NotImplementedError()

    def energy_of_distance(self, r):
        """The restraint's energy (kJ/mol) at the distance r (nm) with the controlling parameter at its default value: what the
        reference reads from an OpenMM Reference Context of two particles (forces.py:531-555)."""
        lam = self.getGlobalParameterDefaultValue(1)
        p = self.restraint_parameters
        return lam * self._energy_at(float(r), p['K'], p.get('r0', 0.0))

    def compute_standard_state_correction(self, thermodynamic_state, square_well=False, radius_cutoff=None, energy_cutoff=None,
                                          max_volume=None):
        """forces.py:367-459: - log(V_standard / V_restraint), V_restraint bounded by the volume of the periodic box."""
        is_npt = thermodynamic_state.pressure is not None
        if max_volume == 'system':
            max_volume = thermodynamic_state.get_volume(ignore_ensemble=True)
        elif max_volume is None and not is_npt:
            max_volume = thermodynamic_state.volume
        elif max_volume is None:
            raise TypeError('max_volume must be provided with NPT ensemble')
        else:
            max_volume = float(to_md(max_volume))
        if radius_cutoff is not None:
            radius_cutoff = float(to_md(radius_cutoff))
        if (not thermodynamic_state.is_periodic and square_well is True and
                radius_cutoff is None and energy_cutoff is None and max_volume is None):
            raise TypeError('One between radius_cutoff, energy_cutoff, or max_volume '
                            'must be provided when reweighting non-periodic thermodynamic '
                            'states to a square-well restraint.')
        if square_well is True and energy_cutoff is None and radius_cutoff is None:
            restraint_volume = max_volume
        elif square_well is True and radius_cutoff is not None:
            restraint_volume = _compute_sphere_volume(radius_cutoff)
        else:
            restraint_volume = self._compute_restraint_volume(thermodynamic_state, square_well, radius_cutoff, energy_cutoff)
        if max_volume is not None and restraint_volume > max_volume:
            restraint_volume = max_volume
        return -math.log(STANDARD_STATE_VOLUME / restraint_volume)

    def _compute_restraint_volume(self, thermodynamic_state, square_well, radius_cutoff, energy_cutoff):
        return self._integrate_restraint_volume(thermodynamic_state, square_well, radius_cutoff, energy_cutoff)

    def _integrate_restraint_volume(self, thermodynamic_state, square_well, radius_cutoff, energy_cutoff):
        """forces.py:496-589, the potential from ``energy_of_distance`` instead of an OpenMM Reference Context."""
        import scipy.integrate
        beta = thermodynamic_state.beta

        def restraint_potential_func(r):
            return beta * self.energy_of_distance(r)

        def integrand(r):
            potential = restraint_potential_func(r)
            if energy_cutoff is not None and potential > energy_cutoff:
                return 0.0
            if square_well:
                potential = 0.0
            return 4.0 * math.pi * r ** 2 * math.exp(-potential)

        r_min, r_max, analytical_volume = self._determine_integral_limits(thermodynamic_state, radius_cutoff, energy_cutoff,
                                                                          restraint_potential_func)
        restraint_volume, _ = scipy.integrate.quad(integrand, r_min, r_max)
        return restraint_volume + analytical_volume

    def _determine_integral_limits(self, thermodynamic_state, radius_cutoff, energy_cutoff, potential_energy_func):
        """forces.py:592-669."""
        r_min = 0.0
        r_max = float('inf')
        analytical_volume = 0.0
        if radius_cutoff is not None:
            r_max = min(r_max, radius_cutoff)
        if energy_cutoff is not None:
            try:
                energy_cutoff_distance = self.distance_at_energy(energy_cutoff * thermodynamic_state.kT)
            except NotImplementedError:
                potential = 0.0
                energy_cutoff_distance = 0.0
                while potential <= energy_cutoff and energy_cutoff_distance < r_max:
                    energy_cutoff_distance += 0.1
                    potential = potential_energy_func(energy_cutoff_distance)
            r_max = min(r_max, energy_cutoff_distance)
        if r_max == float('inf'):
            if thermodynamic_state.is_periodic:
                r_max = 3.0 * float(np.max(thermodynamic_state.default_box_vectors))
            else:
                r_max = 100.0
        return r_min, r_max, analytical_volume


class RadiallySymmetricCentroidRestraintForce(RadiallySymmetricRestraintForce, CustomCentroidBondForce):
    """forces.py:672-746: a restraint between the mass-weighted centroids of two groups of atoms."""

    def __init__(self, energy_function, restraint_parameters, restrained_atom_indices1, restrained_atom_indices2,
                 controlling_parameter_name='lambda_restraints'):
        energy_function = controlling_parameter_name + ' * (' + energy_function + ')'
        super().__init__(restraint_parameters, restrained_atom_indices1, restrained_atom_indices2, controlling_parameter_name,
                         2, energy_function)

    @property
    def restrained_atom_indices1(self):
        return list(self.getGroupParameters(0)[0])

    @restrained_atom_indices1.setter
    def restrained_atom_indices1(self, atom_indices):
        self.setGroupParameters(0, atom_indices)

    @property
    def restrained_atom_indices2(self):
        return list(self.getGroupParameters(1)[0])

    @restrained_atom_indices2.setter
    def restrained_atom_indices2(self, atom_indices):
        self.setGroupParameters(1, atom_indices)

    def _create_bond(self, bond_parameter_values, restrained_atom_indices1, restrained_atom_indices2):
        self.addGroup(restrained_atom_indices1)
        self.addGroup(restrained_atom_indices2)
        self.addBond([0, 1], bond_parameter_values)


class RadiallySymmetricBondRestraintForce(RadiallySymmetricRestraintForce, CustomBondForce):
    """forces.py:749-803: the same between two single atoms."""

    def __init__(self, energy_function, restraint_parameters, restrained_atom_index1, restrained_atom_index2,
                 controlling_parameter_name='lambda_restraints'):
        energy_function = energy_function.replace('distance(g1,g2)', 'r')
        energy_function = controlling_parameter_name + ' * (' + energy_function + ')'
        super().__init__(restraint_parameters, [restrained_atom_index1], [restrained_atom_index2], controlling_parameter_name,
                         energy_function)

    @property
    def restrained_atom_indices1(self):
        return [self.getBondParameters(0)[0]]

    @restrained_atom_indices1.setter
    def restrained_atom_indices1(self, atom_indices):
        assert len(atom_indices) == 1
        atom1, atom2, parameters = self.getBondParameters(0)
        self.setBondParameters(0, atom_indices[0], atom2, parameters)

    @property
    def restrained_atom_indices2(self):
        return [self.getBondParameters(0)[1]]

    @restrained_atom_indices2.setter
    def restrained_atom_indices2(self, atom_indices):
        assert len(atom_indices) == 1
        atom1, atom2, parameters = self.getBondParameters(0)
        self.setBondParameters(0, atom1, atom_indices[0], parameters)

    def _create_bond(self, bond_parameter_values, restrained_atom_indices1, restrained_atom_indices2):
        self.addBond(restrained_atom_indices1[0], restrained_atom_indices2[0], bond_parameter_values)


class HarmonicRestraintForceMixIn:
    """forces.py:806-851: E = lambda (K/2) r^2."""
    ENERGY_FUNCTION = '(K/2)*distance(g1,g2)^2'

    def __init__(self, spring_constant, *args, **kwargs):
        restraint_parameters = collections.OrderedDict([('K', spring_constant)])
        super().__init__(self.ENERGY_FUNCTION, restraint_parameters, *args, **kwargs)

    @staticmethod
    def _energy_at(r, K, r0):
        return (K / 2) * r ** 2

    @property
    def spring_constant(self):
        """kJ/mol/nm^2"""
        return self.getBondParameters(0)[-1][0]

    def distance_at_energy(self, potential_energy):
        return _compute_harmonic_radius(self.spring_constant, float(to_md(potential_energy)))

    def _compute_restraint_volume(self, thermodynamic_state, square_well, radius_cutoff, energy_cutoff):
        if energy_cutoff is None:
            energy_cutoff = 100.0  # kT
        radius = self.distance_at_energy(energy_cutoff * thermodynamic_state.kT)
        if radius_cutoff is not None:
            radius = min(radius, radius_cutoff)
        if square_well:
            return _compute_sphere_volume(radius)
        return _compute_harmonic_volume(radius, self.spring_constant, thermodynamic_state.beta)


class HarmonicRestraintForce(HarmonicRestraintForceMixIn, RadiallySymmetricCentroidRestraintForce):
    """forces.py:854-899: ``E = controlling_parameter * (K/2)*r^2`` between the mass-weighted centroids of two groups.

    Parameters: spring_constant (kJ/mol/nm^2), restrained_atom_indices1, restrained_atom_indices2,
    controlling_parameter_name='lambda_restraints'."""
    pass


class HarmonicRestraintBondForce(HarmonicRestraintForceMixIn, RadiallySymmetricBondRestraintForce):
    """forces.py:902-936: the harmonic restraint between two atoms."""
    pass


class FlatBottomRestraintForceMixIn:
    """forces.py:939-1010: E = lambda step(r - r0) (K/2) (r - r0)^2."""
    ENERGY_FUNCTION = 'step(distance(g1,g2)-r0) * (K/2)*(distance(g1,g2)-r0)^2'

    def __init__(self, spring_constant, well_radius, *args, **kwargs):
        restraint_parameters = collections.OrderedDict([('K', spring_constant), ('r0', well_radius)])
        super().__init__(self.ENERGY_FUNCTION, restraint_parameters, *args, **kwargs)

    @staticmethod
    def _energy_at(r, K, r0):
        return (1.0 if r - r0 >= 0 else 0.0) * (K / 2) * (r - r0) ** 2

    @property
    def spring_constant(self):
        """kJ/mol/nm^2"""
        return self.getBondParameters(0)[-1][0]

    @property
    def well_radius(self):
        """nm"""
        return self.getBondParameters(0)[-1][1]

    def distance_at_energy(self, potential_energy):
        potential_energy = float(to_md(potential_energy))
        if potential_energy == 0.0:
            raise ValueError('Cannot compute the distance at this potential energy.')
        return self.well_radius + _compute_harmonic_radius(self.spring_constant, potential_energy)

    def _compute_restraint_volume(self, thermodynamic_state, square_well, radius_cutoff, energy_cutoff):
        if square_well:
            _, r_max, _ = self._determine_integral_limits(thermodynamic_state, radius_cutoff, energy_cutoff)
            return _compute_sphere_volume(r_max)
        return self._integrate_restraint_volume(thermodynamic_state, square_well, radius_cutoff, energy_cutoff)

    def _determine_integral_limits(self, thermodynamic_state, radius_cutoff, energy_cutoff, potential_energy_func=None):
        if energy_cutoff is None:
            energy_cutoff = 100.0  # kT
        energy_cutoff = energy_cutoff * thermodynamic_state.kT
        r_max = _compute_harmonic_radius(self.spring_constant, energy_cutoff)
        r_max += self.well_radius
        if radius_cutoff is not None:
            r_max = min(r_max, radius_cutoff)
        r_min = min(r_max, self.well_radius)
        analytical_volume = _compute_sphere_volume(r_min)
        return r_min, r_max, analytical_volume


class FlatBottomRestraintForce(FlatBottomRestraintForceMixIn, RadiallySymmetricCentroidRestraintForce):
    """forces.py:1013-1066: ``E = controlling_parameter * step(r-r0) * (K/2)*(r-r0)^2`` between two group centroids.

    Parameters: spring_constant (kJ/mol/nm^2), well_radius (nm), restrained_atom_indices1, restrained_atom_indices2,
    controlling_parameter_name='lambda_restraints'."""
    pass


class FlatBottomRestraintBondForce(FlatBottomRestraintForceMixIn, RadiallySymmetricBondRestraintForce):
    """forces.py:1069-1107: the flat-bottom restraint between two atoms."""
    pass


_RESTRAINT_CLASSES = (HarmonicRestraintForce, HarmonicRestraintBondForce, FlatBottomRestraintForce, FlatBottomRestraintBondForce)
_BODIES = {HarmonicRestraintForceMixIn.ENERGY_FUNCTION: 0, FlatBottomRestraintForceMixIn.ENERGY_FUNCTION: 1}


def _match_restraint_form(force):
    """(kind 0 harmonic / 1 flat bottom, controlling parameter name) of a custom force whose energy is '<global> * (<restraint body>)',
    else (None, None).  The one place that decides which kernel a CustomBondForce reaches (restraint_terms, is_restraint_form)."""
    restore_interface(force)
    energy = force.getEnergyFunction().replace(' ', '')
    names = [force.getGlobalParameterName(i) for i in range(force.getNumGlobalParameters())]
    kind = parameter = None
    is_centroid = isinstance(force, CustomCentroidBondForce)
    for body, k in _BODIES.items():
        # a centroid force speaks of distance(g1,g2), a bond force of r (forces.py:763): each only in its own form
        form = body if is_centroid else body.replace('distance(g1,g2)', 'r')
        for name in names:
            if energy == (name + '*(' + form + ')').replace(' ', ''):
                kind, parameter = k, name
    return kind, parameter


def restraint_terms(force, masses):
    """What the engine needs of one restraint force (system.system_to_desc): dict(kind 0 harmonic / 1 flat bottom, K, r0, the two
    groups with their centroid weights -- masses where the group gives none --, periodic flag, controlling parameter name, force
    group).  NotImplementedError for a custom force whose energy is not one of the four restraint forms."""
    kind, parameter = _match_restraint_form(force)
    is_centroid = isinstance(force, CustomCentroidBondForce)
    if kind is None or (is_centroid and force.getNumGroupsPerBond() != 2):
        raise NotImplementedError('unsupported custom force %r (energy %r): only the restraint forms of openmmtools.forces are supported'
                                  % (type(force).__name__, force.getEnergyFunction()))
    if force.getNumBonds() != 1:
        raise NotImplementedError('a restraint force with %d bonds (one is supported)' % force.getNumBonds())
    per_bond = [force.getPerBondParameterName(i) for i in range(force.getNumPerBondParameters())]
    if is_centroid:
        gidx, values = force.getBondParameters(0)
        groups = [force.getGroupParameters(g) for g in gidx]
    else:
        a1, a2, values = force.getBondParameters(0)
        groups = [([a1], []), ([a2], [])]
    params = dict(zip(per_bond, values))
    out = dict(kind=kind, K=float(params['K']), r0=float(params.get('r0', 0.0)), periodic=int(force.usesPeriodicBoundaryConditions()),
               parameter=parameter, force_group=int(force.getForceGroup()))
    for n, (atoms, weights) in enumerate(groups, start=1):
        atoms = np.array(atoms, dtype=np.int32)
        w = np.array(weights, dtype=np.float64) if len(weights) else np.array([masses[a] for a in atoms], dtype=np.float64)
        out['atoms%d' % n], out['weights%d' % n] = atoms, w
    return out


def is_restraint_form(force):
    """Whether a custom force carries one of the restraint forms (csrc/restraints.hip evaluates it): restraint_terms' own matcher."""
    return _match_restraint_form(force)[0] is not None


def is_restraint_force(force):
    """The forces restraint_terms takes: a CustomCentroidBondForce (refused there unless it is a restraint form) and a CustomBondForce
    in one of the restraint forms; any other CustomBondForce expression takes the expression path (custom_expr.py)."""
    if isinstance(force, CustomCentroidBondForce):
        return True
    return isinstance(force, CustomBondForce) and is_restraint_form(force)
