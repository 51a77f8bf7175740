"""ThermodynamicState / SamplerState: the input contract of the replica-exchange engine.

Mirrors the parts of openmmtools/states.py the hot path touches:
  ThermodynamicState   states.py:331-1930  (system, temperature, pressure, beta, reduced potential
                       algebra :1908-1917, compatibility :994-1050)
  SamplerState         states.py:1933-2521 (positions, velocities, box_vectors, cached energies)
  CompoundThermodynamicState + GlobalParameterState (lambda_sterics / lambda_electrostatics)
                       states.py:2524-3046, alchemy.AlchemicalState alchemy.py:86-410
Quantities are md-unit floats / numpy arrays (see unit.py).
"""
import copy
import inspect
import numpy as np
from . import constants
from .unit import to_md


class _CodedError(Exception):
    """The reference's state errors carry a `code` (class constants, numbered in declaration order) and take their message from a table
    indexed by it (states.py:300-337, 366-377): user code tests `err.code == ThermodynamicsError.NO_THERMOSTAT`."""
    _table = ()

    def __init__(self, code, *args):
        super().__init__(self.error_messages[code].format(*args))
        self.code = code

    def __init_subclass__(cls, **kw):
        super().__init_subclass__(**kw)
        cls.error_messages = {}
        for number, (name, message) in enumerate(cls._table):
            setattr(cls, name, number)
            cls.error_messages[number] = message


class ThermodynamicsError(_CodedError):
    """states.py:272-337 (names, numbers and messages are the reference's: tests/test_signatures.py holds them to its source)."""
    _table = (('MULTIPLE_THERMOSTATS', 'System has multiple thermostats.'),
              ('NO_THERMOSTAT', 'System does not have a thermostat specifying the temperature.'),
              ('NONE_TEMPERATURE', 'Cannot set temperature of the thermodynamic state to None.'),
              ('INCONSISTENT_THERMOSTAT', 'System thermostat is inconsistent with thermodynamic state.'),
              ('MULTIPLE_BAROSTATS', 'System has multiple barostats.'),
              ('NO_BAROSTAT', 'System does not have a barostat specifying the pressure.'),
              ('UNSUPPORTED_BAROSTAT', 'Found unsupported barostat {} in system.'),
              ('UNSUPPORTED_ANISOTROPIC_BAROSTAT', 'MonteCarloAnisotropicBarostat is only supported if the pressure along all scaled axes is the same.'),
              ('SURFACE_TENSION_NOT_SUPPORTED', 'Surface tension can only be set for states that have a system with a MonteCarloMembraneBarostat.'),
              ('INCONSISTENT_BAROSTAT', 'System barostat is inconsistent with thermodynamic state.'),
              ('BAROSTATED_NONPERIODIC', 'Non-periodic systems cannot have a barostat.'),
              ('INCONSISTENT_INTEGRATOR', 'Integrator is coupled to a heat bath at a different temperature.'),
              ('INCOMPATIBLE_SAMPLER_STATE', 'The sampler state has a different number of particles.'),
              ('INCOMPATIBLE_ENSEMBLE', 'Cannot apply to a context in a different thermodynamic ensemble.'))


class SamplerStateError(_CodedError):
    """states.py:340-382."""
    _table = (('INCONSISTENT_VELOCITIES', 'Velocities have different length than positions.'),
              ('INCONSISTENT_POSITIONS', 'Specified positions with inconsistent number of particles.'))


def create_thermodynamic_state_protocol(system, protocol, constants=None, composable_states=None):
    """states.py:39-141: one state per entry of the protocol -- ``protocol`` maps attribute names (temperature, pressure,
    lambda_sterics, ...) to equally long value lists, ``constants`` to values shared by every state; ``system`` is a System
    (then a temperature must be among them) or a ThermodynamicState; ``composable_states`` wrap it into a
    CompoundThermodynamicState first."""
    protocol = dict(protocol)
    if len(protocol) == 0:
        raise ValueError('No protocol has been specified.')
    lengths = {len(v) for v in protocol.values()}
    if len(lengths) != 1:
        raise ValueError('The protocol parameter values have different lengths!\n{}'.format(protocol))
    n = lengths.pop()
    constants_ = dict(constants or {})
    if set(constants_) & set(protocol):
        raise ValueError('Some parameters have been specified both in constants and protocol.')
    for key, value in constants_.items():
        protocol[key] = [value] * n
    if isinstance(system, ThermodynamicState):
        thermo_state = system
    else:
        if 'temperature' in constants_:
            temperature = constants_['temperature']
        elif 'temperature' in protocol:
            temperature = protocol['temperature'][0]
        else:
            raise ValueError('If a System is passed the list of constants must specify the temperature.')
        thermo_state = ThermodynamicState(system, temperature=temperature)
    if composable_states is not None:
        if not isinstance(composable_states, (list, tuple)):
            composable_states = [composable_states]
        thermo_state = CompoundThermodynamicState(thermo_state, composable_states)
    out = [copy.deepcopy(thermo_state) for _ in range(n)]
    for k, state in enumerate(out):
        for key, values in protocol.items():
            if not hasattr(state, key):
                raise AttributeError('{} object does not have protocol attribute {}'.format(type(state), key))
            setattr(state, key, values[k])
    return out


class MonteCarloBarostatSettings:
    """The accessors of openmm.MonteCarloBarostat the reference's code and tests read from ``ThermodynamicState.barostat``."""

    def __init__(self, pressure, temperature, frequency):
        self._pressure, self._temperature, self._frequency = float(pressure), float(temperature), int(frequency)

    def getDefaultPressure(self):
        return self._pressure                     # kJ/mol/nm^3 (``pressure / unit.bar`` gives bar)

    def getDefaultTemperature(self):
        return self._temperature

    def getFrequency(self):
        return self._frequency


class ThermodynamicState:
    _SUPPORTED_BAROSTATS = {'MonteCarloBarostat', 'MonteCarloAnisotropicBarostat', 'MonteCarloMembraneBarostat'}       # states.py:1656
    _surface_tension = None                 # (states pickled before the NPgammaT ensemble was carried)

    def __init__(self, system, temperature=None, pressure=None, surface_tension=None):
        """states.py:507-508, 1314-1353.  A System here carries no thermostat force a temperature could be read from: no temperature
        is the reference's NO_THERMOSTAT.  A MonteCarloAnisotropicBarostat or MonteCarloMembraneBarostat among the System's forces
        (system.py) makes the state an NPT / NPgammaT one of that kind: pressure and surface tension are inferred from it when not
        given; a surface tension without a membrane barostat is the reference's INCOMPATIBLE_ENSEMBLE."""
        self._system = system
        barostat = self._find_barostat(system)
        is_membrane = type(barostat).__name__ == 'MonteCarloMembraneBarostat'
        if surface_tension is not None and not is_membrane:
            raise ThermodynamicsError(ThermodynamicsError.INCOMPATIBLE_ENSEMBLE)          # states.py:1330-1331
        if temperature is None:
            raise ThermodynamicsError(ThermodynamicsError.NO_THERMOSTAT)                  # states.py:1336-1339
        self.temperature = temperature
        if pressure is None and barostat is not None:
            pressure = self._get_barostat_pressure(barostat)                              # states.py:1319-1324
        # NPT: the reference adds an openmm.MonteCarloBarostat (frequency 25) to the System (states.py:1177-1181); here the
        # pressure (kJ/mol/nm^3, i.e. `p * unit.bar`) and the frequency are handed to the engine's barostat
        self.pressure = pressure                                                 # Quantity -> kJ/mol/nm^3 (md units)
        self.barostat_frequency = 25 if barostat is None else int(barostat.getFrequency())
        if is_membrane:                       # kJ/mol/nm^2, i.e. `g * unit.bar * unit.nanometer` (states.py:1326-1333)
            self._surface_tension = float(barostat.getDefaultSurfaceTension() if surface_tension is None else to_md(surface_tension))

    @classmethod
    def _find_barostat(cls, system):
        """states.py:1658-1696: the System's barostat force or None; more than one, an unknown one, or an anisotropic one the
        reduced potential cannot describe (no scaled axis, or different pressures along the scaled axes) are errors."""
        found = [f for f in system.getForces() if 'Barostat' in type(f).__name__]
        if len(found) > 1:
            raise ThermodynamicsError(ThermodynamicsError.MULTIPLE_BAROSTATS)
        if not found:
            return None
        barostat = found[0]
        if type(barostat).__name__ not in cls._SUPPORTED_BAROSTATS:
            raise ThermodynamicsError(ThermodynamicsError.UNSUPPORTED_BAROSTAT, type(barostat).__name__)
        if type(barostat).__name__ == 'MonteCarloAnisotropicBarostat':
            scaled = [barostat.getScaleX(), barostat.getScaleY(), barostat.getScaleZ()]
            if sum(scaled) == 0:
                raise ThermodynamicsError(ThermodynamicsError.UNSUPPORTED_ANISOTROPIC_BAROSTAT)
            active = [p for p, on in zip(barostat.getDefaultPressure(), scaled) if on]
            if any(abs(p - active[0]) > 0 for p in active):
                raise ThermodynamicsError(ThermodynamicsError.UNSUPPORTED_ANISOTROPIC_BAROSTAT)
        return barostat

    @staticmethod
    def _get_barostat_pressure(barostat):
        """states.py:1794-1802: an anisotropic barostat's pressure is the one along its first scaled axis."""
        if type(barostat).__name__ == 'MonteCarloAnisotropicBarostat':
            scaled = [barostat.getScaleX(), barostat.getScaleY(), barostat.getScaleZ()]
            return barostat.getDefaultPressure()[scaled.index(True)]
        return barostat.getDefaultPressure()

    def _system_barostat(self):
        """the System's barostat force while the state is at constant pressure (None at constant volume)"""
        return None if self._pressure is None else self._find_barostat(self._system)

    def _barostat_signature(self):
        """what two states' barostats must share to run in one Context (states.py:1716-1721 compares the types; modes and scale
        flags are part of the standard System the reference hashes): None at constant volume."""
        if self._pressure is None:
            return None
        b = self._system_barostat()
        name = type(b).__name__
        if name == 'MonteCarloAnisotropicBarostat':
            return (name, bool(b.getScaleX()), bool(b.getScaleY()), bool(b.getScaleZ()))
        if name == 'MonteCarloMembraneBarostat':
            return (name, int(b.getXYMode()), int(b.getZMode()))
        return ('MonteCarloBarostat',)

    def _is_barostat_type_consistent(self, barostat):
        """states.py:1716-1721."""
        return type(barostat) is type(self._system_barostat())

    @property
    def pressure(self):
        return self._pressure

    @pressure.setter
    def pressure(self, value):
        """states.py:680-703."""
        if value is not None and not self._system.usesPeriodicBoundaryConditions():
            raise ThermodynamicsError(ThermodynamicsError.BAROSTATED_NONPERIODIC)            # states.py:1764-1766
        self._pressure = None if value is None else float(to_md(value))

    @property
    def barostat(self):
        """states.py:705-727: a copy of the System's barostat force carrying this state's pressure, surface tension and temperature;
        for a System without one (plain NPT: the reference adds an openmm.MonteCarloBarostat) the three numbers that barostat would
        carry (pressure of this state, its temperature, the attempt frequency); None at constant volume."""
        if self._pressure is None:
            return None
        force = self._system_barostat()
        if force is None:
            return MonteCarloBarostatSettings(self._pressure, self._temperature, self.barostat_frequency)
        force = copy.deepcopy(force)
        if type(force).__name__ == 'MonteCarloAnisotropicBarostat':
            force.setDefaultPressure((self._pressure,) * 3)                                  # states.py:1780-1781
        else:
            force.setDefaultPressure(self._pressure)
        force.setDefaultTemperature(self._temperature)
        if self._surface_tension is not None:
            force.setDefaultSurfaceTension(self._surface_tension)
        return force

    @property
    def surface_tension(self):
        """states.py:806-816: the surface tension (kJ/mol/nm^2) of a state whose System has a MonteCarloMembraneBarostat, else None."""
        return self._surface_tension

    @surface_tension.setter
    def surface_tension(self, gamma):
        if (self._surface_tension is None) != (gamma is None):                               # states.py:813-814
            raise ThermodynamicsError(ThermodynamicsError.SURFACE_TENSION_NOT_SUPPORTED)
        self._surface_tension = None if gamma is None else float(to_md(gamma))

    def get_volume(self, ignore_ensemble=False):
        """states.py:773-794: volume of the System's default periodic box (nm^3); None when the volume fluctuates (a pressure is set,
        unless ignore_ensemble) or the System is not periodic."""
        if self._pressure is not None and not ignore_ensemble:
            return None
        if not self._system.usesPeriodicBoundaryConditions():
            return None
        return float(abs(np.linalg.det(np.array(self._system.getDefaultPeriodicBoxVectors(), dtype=np.float64).reshape(3, 3))))

    @property
    def volume(self):
        """states.py:763-771."""
        return self.get_volume()

    @property
    def system(self):
        return self._system

    def get_system(self, remove_thermostat=False, remove_barostat=False):
        """states.py:836-870.  A System here holds neither a thermostat nor a barostat force (temperature and pressure live on the
        state and go to the engine), so there is nothing to remove: the two flags are accepted for the caller's sake."""
        return self._system

    @property
    def temperature(self):
        return self._temperature

    @temperature.setter
    def temperature(self, value):
        if value is None:
            raise ThermodynamicsError(ThermodynamicsError.NONE_TEMPERATURE)                  # states.py:664-666
        value = float(to_md(value))                    # float kelvin or an openmm.unit.Quantity
        if not value > 0:
            raise ValueError('temperature must be positive')
        self._temperature = value

    @property
    def kT(self):
        return constants.kB * self._temperature

    @property
    def beta(self):
        return 1.0 / (constants.kB * self._temperature)

    @property
    def n_particles(self):
        return self._system.getNumParticles()

    @property
    def is_periodic(self):
        return self._system.usesPeriodicBoundaryConditions()

    @property
    def default_box_vectors(self):
        return self._system.getDefaultPeriodicBoxVectors()

    # lambda parameters: a plain ThermodynamicState is the fully interacting end state
    lambda_sterics = 1.0
    lambda_electrostatics = 1.0

    def region_lambdas(self, names):
        return [1.0] * len(names), [1.0] * len(names)

    def global_parameter(self, name):
        """no composable state controls a global parameter of a plain ThermodynamicState (CompoundThermodynamicState.global_parameter)"""
        return None

    def region_bonded_lambdas(self, names):
        return [1.0] * len(names), [1.0] * len(names), [1.0] * len(names)

    def __setstate__(self, state):
        """States pickled before ``pressure`` / ``temperature`` became properties (storage format 'openmmtools_amd-records-1'
        of earlier revisions) carry the plain attribute names: map them onto the backing fields so that old stores resume."""
        state = dict(state)
        for old, new in (('pressure', '_pressure'), ('temperature', '_temperature'), ('system', '_system')):
            if old in state and new not in state:
                state[new] = state.pop(old)
        state.setdefault('_pressure', None)
        state.setdefault('barostat_frequency', 25)
        self.__dict__.update(state)

    @staticmethod
    def _compute_reduced_potential(potential_energy, temperature, volume=None, pressure=None, area_xy=None, surface_tension=None):
        """states.py:1908-1917: u = beta (U + p V - gamma A_xy); energies per mole, so N_A is already folded in."""
        beta = 1.0 / (constants.kB * temperature)
        reduced = potential_energy
        if pressure is not None:
            reduced = reduced + pressure * volume
        if area_xy is not None and surface_tension is not None:
            reduced = reduced - surface_tension * area_xy
        return beta * reduced

    def reduced_potential(self, context_state):
        """states.py:932-992.  Reduced potential of a SamplerState with a cached potential energy, or of an energy in kJ/mol (the
        reference also takes an openmm.Context there, hence the argument's name)."""
        sampler_state_or_energy = context_state
        if isinstance(sampler_state_or_energy, SamplerState):
            energy = sampler_state_or_energy.potential_energy
            volume = sampler_state_or_energy.volume
            area_xy = sampler_state_or_energy.area_xy
            if energy is None:
                raise ValueError('SamplerState has no cached potential energy')
        else:
            energy, volume, area_xy = float(sampler_state_or_energy), None, None
        return self._compute_reduced_potential(energy, self._temperature, volume, self.pressure, area_xy, self.surface_tension)

    def is_state_compatible(self, thermodynamic_state):
        """states.py:994-1050: same standard system and same ensemble."""
        other = thermodynamic_state
        return (self._system is other._system or self._system.fingerprint() == other._system.fingerprint()) \
            and (self.pressure is None) == (other.pressure is None) and self._barostat_signature() == other._barostat_signature()

    def __deepcopy__(self, memo):
        # Systems are treated as immutable once wrapped (the reference deep-copies and re-hashes)
        new = copy.copy(self)
        return new


class AlchemicalStateError(ValueError):
    """alchemy.py:60-62 (a ValueError here as well: what this class raised before it had a name of its own)."""


class AlchemicalState:
    """lambda_sterics / lambda_electrostatics carrier (alchemy.py:86-410, only these two).  ``parameters_name_suffix`` (states.py:3149-3181,
    alchemy.py:203-231): the state of the alchemical region of that name -- its parameters are then also reachable as
    ``lambda_sterics_<suffix>`` / ``lambda_electrostatics_<suffix>``, the names the factory gives the region's global parameters
    (alchemy.py:1360-1377)."""

    _PARAMETERS = ('lambda_sterics', 'lambda_electrostatics', 'lambda_bonds', 'lambda_angles', 'lambda_torsions')

    def __init__(self, lambda_sterics=1.0, lambda_electrostatics=1.0, lambda_bonds=1.0, lambda_angles=1.0, lambda_torsions=1.0,
                 parameters_name_suffix=None, **kwargs):
        object.__setattr__(self, 'parameters_name_suffix', parameters_name_suffix)
        values = dict(lambda_sterics=lambda_sterics, lambda_electrostatics=lambda_electrostatics, lambda_bonds=lambda_bonds,
                      lambda_angles=lambda_angles, lambda_torsions=lambda_torsions)
        for key, value in kwargs.items():                       # lambda_sterics_<suffix>=... as the reference's constructor takes them
            base = self._base_name(key)
            if base not in self._PARAMETERS:
                raise AlchemicalStateError('Unknown parameters %r' % key)                    # states.py:3170-3172
            values[base] = value
        # lambda_bonds / angles / torsions act on the bonded terms a region names (AlchemicalRegion.alchemical_bonds ..., alchemy.py:196-199);
        # None = "the System does not define it" (alchemy.py:94-99) is the interacting value here
        for name, value in values.items():
            setattr(self, name, 1.0 if value is None else float(value))
        # the bonded parameters this state was GIVEN (the reference keeps the others at None = "not defined", alchemy.py:94-99, and
        # set_alchemical_parameters leaves those alone, :247-262)
        given = {self._base_name(k) for k in kwargs}
        object.__setattr__(self, '_defined', {k for k in ('lambda_bonds', 'lambda_angles', 'lambda_torsions')
                                              if k in given or (values[k] is not None and float(values[k]) != 1.0)})

    parameters_name_suffix = None
    lambda_bonds = lambda_angles = lambda_torsions = 1.0          # (states pickled before these were carried)
    _defined = frozenset()

    def _base_name(self, name):
        sfx = self.parameters_name_suffix
        if sfx is not None and name.endswith('_' + sfx):
            return name[:-len(sfx) - 1]
        return name

    def __getattr__(self, name):                      # only reached for names that are not plain attributes
        base = self._base_name(name) if not name.startswith('__') else name
        if base != name and base in self._PARAMETERS:
            return self.__dict__[base]
        raise AttributeError(name)

    def __setattr__(self, name, value):
        base = self._base_name(name)
        object.__setattr__(self, base if base in self._PARAMETERS else name, float(value) if base in self._PARAMETERS else value)

    def set_alchemical_parameters(self, new_value):
        """alchemy.py:247-262: every alchemical parameter this state controls to ``new_value``."""
        v = float(new_value)
        if not 0.0 <= v <= 1.0:
            raise ValueError('{} must be between 0 and 1.'.format('lambda_sterics'))     # alchemy.py:216-218: the first parameter's validator speaks
        self.lambda_sterics = v
        self.lambda_electrostatics = v
        for k in sorted(self.__dict__.get('_defined', ())):
            setattr(self, k, v)

    @staticmethod
    def _has_region(system, suffix):
        regions = getattr(system, 'alchemical_regions', None)
        if regions is not None:
            return any(r.name == suffix for r in regions)
        region = getattr(system, 'alchemical_region', None)
        return region is not None and (region.name == suffix or suffix is None or region.name is None)

    @classmethod
    def from_system(cls, system, *args, parameters_name_suffix=None, **kwargs):
        """alchemy.py:203-231: the state a System's alchemical parameters stand at (those written by apply_to_system, else the
        interacting end state the factory creates); a System without an alchemical region (of that name) has none."""
        if not cls._has_region(system, parameters_name_suffix):
            raise AlchemicalStateError('system has no alchemical region' + ('' if parameters_name_suffix is None else ' named %r' % parameters_name_suffix))
        stored = (getattr(system, 'alchemical_parameters', None) or {}).get(parameters_name_suffix, {})
        state = cls(*args, parameters_name_suffix=parameters_name_suffix, **dict({k: stored.get(k, 1.0) for k in cls._PARAMETERS}, **kwargs))
        # lambda_bonds / angles / torsions are defined where the region names softened terms (alchemy.py:1170-1197, 1252-1275, 1331-1354)
        regions = getattr(system, 'alchemical_regions', None) or [getattr(system, 'alchemical_region', None)]
        for r in regions:
            if r is not None and (r.name == parameters_name_suffix or len(regions) == 1):
                state._defined.update('lambda_' + k for k in ('bonds', 'angles', 'torsions') if getattr(r, 'alchemical_' + k, None))
        return state

    def apply_to_system(self, system):
        """alchemy.py:354-373: the System's own alchemical parameters (what a state read back with from_system starts from) set to
        this state's.  The engine takes lambdas from the thermodynamic states, not from the System."""
        if not self._has_region(system, self.parameters_name_suffix):
            raise AlchemicalStateError('system has no alchemical region')
        stored = dict(getattr(system, 'alchemical_parameters', None) or {})
        stored[self.parameters_name_suffix] = {k: float(getattr(self, k)) for k in self._PARAMETERS}
        system.alchemical_parameters = stored

    def check_system_consistency(self, system):
        """alchemy.py:375-393: AlchemicalStateError unless the System's alchemical parameters equal this state's."""
        other = type(self).from_system(system, parameters_name_suffix=self.parameters_name_suffix)
        for k in self._PARAMETERS:
            if float(getattr(other, k)) != float(getattr(self, k)):
                raise AlchemicalStateError('system has %s = %r, the state %r' % (k, getattr(other, k), getattr(self, k)))


class ComposableStateError(Exception):
    """states.py:2524-2530: error raised by a composable state."""
    pass


class GlobalParameterError(ComposableStateError):
    """Exception raised by ``GlobalParameterState``."""
    pass


class GlobalParameterFunction:
    """states.py:3058-3097: a function of global parameters, evaluated with ``utils.math_eval`` on the state's function variables."""

    def __init__(self, expression):
        self._expression = expression

    def __call__(self, variables):
        from .utils import math_eval
        return math_eval(self._expression, variables)


class GlobalParameterState:
    """states.py:3100-3935: a composable state controlling global parameters of a System's forces (here the controlling parameters
    of the restraint forces, forces.py).  Subclasses declare their parameters with the ``GlobalParameter`` descriptor; parameters
    left undefined read as None.  ``apply_to_context`` has no counterpart: the engine handle stands in for a Context, the sampler
    hands it every state's values."""

    _GLOBAL_PARAMETER_ERROR = GlobalParameterError

    def __init__(self, parameters_name_suffix=None, **kwargs):
        self._initialize(parameters_name_suffix=parameters_name_suffix, **kwargs)

    @classmethod
    def from_system(cls, system, parameters_name_suffix=None):
        """The state whose parameters are the values the System's forces define (their default values)."""
        state_parameters = {}
        for force, parameter_name, parameter_id in cls._get_system_controlled_parameters(system, parameters_name_suffix):
            parameter_value = force.getGlobalParameterDefaultValue(parameter_id)
            if parameter_name in state_parameters:
                if state_parameters[parameter_name] != parameter_value:
                    err_msg = ('Parameter {} has been found twice (Force {}) with two values: '
                               '{} and {}').format(parameter_name, force.__class__.__name__,
                                                   parameter_value, state_parameters[parameter_name])
                    raise cls._GLOBAL_PARAMETER_ERROR(err_msg)
            else:
                state_parameters[parameter_name] = parameter_value
        if len(state_parameters) == 0:
            err_msg = 'System has no global parameters controlled by this state.'
            raise cls._GLOBAL_PARAMETER_ERROR(err_msg)
        state = cls(parameters_name_suffix)
        for parameter_name, parameter_value in state_parameters.items():
            setattr(state, parameter_name, parameter_value)
        return state

    def get_function_variable(self, variable_name):
        try:
            variable_value = self._function_variables[variable_name]
        except KeyError:
            err_msg = f'Unknown function variable {variable_name}'
            raise self._GLOBAL_PARAMETER_ERROR(err_msg)
        return variable_value

    def set_function_variable(self, variable_name, new_value):
        forbidden_variable_names = set(self._parameters)
        if variable_name in forbidden_variable_names:
            err_msg = ('Cannot have an function variable with the same name '
                       'of the predefined global parameter {}.'.format(variable_name))
            raise self._GLOBAL_PARAMETER_ERROR(err_msg)
        if not (np.isreal(new_value) and np.isscalar(new_value)):
            err_msg = 'Only integers and floats can be assigned to a function variable.'
            raise self._GLOBAL_PARAMETER_ERROR(err_msg)
        self._function_variables[variable_name] = new_value

    def __eq__(self, other):
        if not isinstance(other, GlobalParameterState):
            return False
        if not set(self._parameters) == set(other._parameters):
            return False
        return all(getattr(self, p) == getattr(other, p) for p in self._parameters)

    def __ne__(self, other):
        return not self == other

    def __str__(self):
        return str(self._parameters)

    class GlobalParameter:
        """Descriptor for a global parameter (states.py:3434-3482): name, value in the standard state, optional validator
        ``validator(descriptor, instance, new_value) -> validated_value``."""

        def __init__(self, parameter_name, standard_value, validator=None):
            self.parameter_name = parameter_name
            self.standard_value = standard_value
            self.validator_func = validator

        def __get__(self, instance, owner_class=None):
            if instance is None:
                return self
            self._check_controlled(instance)
            return instance._get_global_parameter_value(self.parameter_name, self)

        def __set__(self, instance, new_value):
            self._check_controlled(instance)
            instance._set_global_parameter_value(self.parameter_name, new_value, self)

        def validator(self, validator):
            return self.__class__(self.parameter_name, self.standard_value, validator)

        def _check_controlled(self, instance):
            if instance._parameters_name_suffix is not None:
                suffixed_parameter_name = self.parameter_name + '_' + instance._parameters_name_suffix
                err_msg = 'This state does not control {} but {}.'.format(self.parameter_name, suffixed_parameter_name)
                raise AttributeError(err_msg)

    def apply_to_system(self, system):
        """Set the System's global parameters (the forces' default values) to this state's."""
        parameters_applied = set()
        for force, parameter_name, parameter_id in self._get_system_controlled_parameters(system, self._parameters_name_suffix):
            parameter_value = getattr(self, parameter_name)
            if parameter_value is None:
                err_msg = 'The system parameter {} is not defined in this state.'
                raise self._GLOBAL_PARAMETER_ERROR(err_msg.format(parameter_name))
            parameters_applied.add(parameter_name)
            force.setGlobalParameterDefaultValue(parameter_id, parameter_value)
        for parameter_name in self._get_controlled_parameters(self._parameters_name_suffix):
            if self._parameters[parameter_name] is not None and parameter_name not in parameters_applied:
                err_msg = 'Could not find global parameter {} in the system.'
                raise self._GLOBAL_PARAMETER_ERROR(err_msg.format(parameter_name))

    def check_system_consistency(self, system):
        system_state = self.__class__.from_system(system, self._parameters_name_suffix)
        if self != system_state:
            err_msg = ('Consistency check failed:\n'
                       '\tSystem parameters {}\n'
                       '\t{} parameters {}')
            raise self._GLOBAL_PARAMETER_ERROR(err_msg.format(system_state, self.__class__.__name__, self))

    def apply_to_context(self, context):
        raise NotImplementedError('GlobalParameterState.apply_to_context: there is no openmm.Context here; the sampler hands every '
                                  "state's global parameters to the engine handle")

    @classmethod
    def _get_controlled_parameters(cls, parameters_name_suffix=None):
        suffix = '' if parameters_name_suffix is None else '_' + parameters_name_suffix
        return {name + suffix: descriptor for c in inspect.getmro(cls)
                for name, descriptor in c.__dict__.items() if isinstance(descriptor, cls.GlobalParameter)}

    def _validate_global_parameter(self, parameter_name, parameter_value, descriptor=None):
        if descriptor is None:
            descriptor = self._get_controlled_parameters(self._parameters_name_suffix)[parameter_name]
        if descriptor.validator_func is not None:
            parameter_value = descriptor.validator_func(descriptor, self, parameter_value)
        return parameter_value

    def _get_global_parameter_value(self, parameter_name, descriptor=None, resolve_function=True):
        parameter_value = self._parameters[parameter_name]
        if resolve_function and isinstance(parameter_value, GlobalParameterFunction):
            parameter_value = parameter_value(self._function_variables)
            parameter_value = self._validate_global_parameter(parameter_name, parameter_value, descriptor)
        return parameter_value

    def _set_global_parameter_value(self, parameter_name, new_value, descriptor=None):
        if parameter_name not in self._parameters:
            raise KeyError(parameter_name)
        if not isinstance(new_value, GlobalParameterFunction):
            new_value = self._validate_global_parameter(parameter_name, new_value, descriptor)
        self._parameters[parameter_name] = new_value

    def __getattr__(self, key):
        if key.startswith('__') or key in ('_parameters', '_function_variables', '_parameters_name_suffix'):
            raise AttributeError(key)
        try:
            return self._get_global_parameter_value(key)
        except KeyError:
            raise AttributeError(key)

    def __setattr__(self, key, value):
        if '_parameters_name_suffix' in self.__dict__ and self._parameters_name_suffix is not None:
            try:
                self._set_global_parameter_value(key, value)
            except KeyError:
                pass
            else:
                return
        super().__setattr__(key, value)

    @classmethod
    def _get_system_controlled_parameters(cls, system, parameters_name_suffix):
        searched_parameters = cls._get_controlled_parameters(parameters_name_suffix)
        for force in system.getForces():
            try:
                n_global_parameters = force.getNumGlobalParameters()
            except AttributeError:
                continue
            for parameter_id in range(n_global_parameters):
                parameter_name = force.getGlobalParameterName(parameter_id)
                if parameter_name in searched_parameters:
                    if type(force).__name__ == 'CustomGBForce':      # the engine reads a CustomGBForce's globals at their default values
                        raise cls._GLOBAL_PARAMETER_ERROR('global parameter {} of a CustomGBForce cannot be controlled by a '
                                                          'state'.format(parameter_name))
                    yield force, parameter_name, parameter_id

    def __getstate__(self):
        serialization = dict(parameters={}, function_variables=self._function_variables.copy(),
                             parameters_name_suffix=self._parameters_name_suffix)
        suffix = '' if self._parameters_name_suffix is None else '_' + self._parameters_name_suffix
        for parameter_name in self._get_controlled_parameters():
            parameter_value = self._parameters[parameter_name + suffix]
            if isinstance(parameter_value, GlobalParameterFunction):
                parameter_value = parameter_value._expression
            serialization['parameters'][parameter_name] = parameter_value
        return serialization

    def __setstate__(self, serialization):
        parameters = dict(serialization['parameters'])
        parameters_name_suffix = serialization.get('parameters_name_suffix', None)
        function_variables = serialization.get('function_variables', {})
        global_parameter_functions = {}
        for parameter_name, value in parameters.items():
            if isinstance(value, str):
                global_parameter_functions[parameter_name] = value
                parameters[parameter_name] = None
        self._initialize(parameters_name_suffix=parameters_name_suffix, **parameters)
        for variable_name, value in function_variables.items():
            self.set_function_variable(variable_name, value)
        suffix = '' if parameters_name_suffix is None else '_' + parameters_name_suffix
        for parameter_name, expression in global_parameter_functions.items():
            setattr(self, parameter_name + suffix, GlobalParameterFunction(expression))

    def _initialize(self, parameters_name_suffix=None, **kwargs):
        self._function_variables = {}
        controlled_parameters = set(self._get_controlled_parameters())
        unknown_parameters = set(kwargs) - controlled_parameters
        if len(unknown_parameters) > 0:
            err_msg = f"Unknown parameters {unknown_parameters}"
            raise self._GLOBAL_PARAMETER_ERROR(err_msg)
        if parameters_name_suffix is not None:
            kwargs = {key + '_' + parameters_name_suffix: value for key, value in kwargs.items()}
            controlled_parameters = {key + '_' + parameters_name_suffix for key in controlled_parameters}
        self._parameters = dict.fromkeys(controlled_parameters, None)
        self._parameters_name_suffix = parameters_name_suffix
        for parameter_name, value in kwargs.items():
            setattr(self, parameter_name, value)

    def __deepcopy__(self, memo):
        new = object.__new__(type(self))
        new.__setstate__(self.__getstate__())
        return new

    def __copy__(self):
        return self.__deepcopy__({})

    def __reduce__(self):
        # a pickled state names no class outside this package (a store opens only this package's classes, multistatereporter.py):
        # it comes back as a StoredGlobalParameterState that controls the same parameters under the same class name
        spec = {name: d.standard_value for name, d in type(self)._get_controlled_parameters().items()}
        return (StoredGlobalParameterState, (), dict(class_name=type(self).__name__, spec=spec, state=self.__getstate__()))


_STORED_CLASSES = {}


def stored_global_parameter_class(class_name, spec):
    """The GlobalParameterState subclass named ``class_name`` that controls the parameters of ``spec`` ({name: standard value}): what
    a store gives back for a user's subclass it cannot import (one class per name and parameter set)."""
    key = (str(class_name), tuple(sorted((str(k), v) for k, v in spec.items())))
    cls = _STORED_CLASSES.get(key)
    if cls is None:
        attrs = {name: GlobalParameterState.GlobalParameter(name, standard_value=v) for name, v in key[1]}
        attrs['__module__'] = __name__
        cls = _STORED_CLASSES[key] = type(key[0], (StoredGlobalParameterState,), attrs)
    return cls


class StoredGlobalParameterState(GlobalParameterState):
    """A GlobalParameterState read back from a store: the class the store recorded (its name and parameters), without validators."""

    def __setstate__(self, serialization):
        if 'spec' in serialization:
            object.__setattr__(self, '__class__', stored_global_parameter_class(serialization['class_name'], serialization['spec']))
            serialization = serialization['state']
        GlobalParameterState.__setstate__(self, serialization)


class CompoundThermodynamicState(ThermodynamicState):
    """states.py:2524-3046 restricted to AlchemicalState composable states: one (any suffix), or one per named alchemical region."""

    def __init__(self, thermodynamic_state, composable_states):
        super().__init__(thermodynamic_state.system, thermodynamic_state.temperature, thermodynamic_state.pressure,
                         thermodynamic_state.surface_tension)
        if len(composable_states) < 1 or not all(isinstance(c, (AlchemicalState, GlobalParameterState)) for c in composable_states):
            raise NotImplementedError('only AlchemicalState and GlobalParameterState composable states are supported')
        alchs = [c for c in composable_states if isinstance(c, AlchemicalState)]
        globs = [c for c in composable_states if isinstance(c, GlobalParameterState)]
        suffixes = [c.parameters_name_suffix for c in alchs]
        names = [p for g in globs for p in g._parameters]
        if len(set(suffixes)) != len(suffixes) or len(set(names)) != len(names):
            raise ValueError('composable states control the same parameters')                 # states.py:2574-2590
        object.__setattr__(self, '_alchs', [copy.copy(c) for c in alchs])
        # GlobalParameterStates (states.py:3100-3935, e.g. lambda_restraints of the restraint forces): parameters by their (suffixed) names
        object.__setattr__(self, '_globals', [copy.deepcopy(c) for c in globs])

    _globals = ()

    @property
    def _alch(self):
        return self._alchs[0]

    def _owner(self, name):
        """the composable state that answers to the attribute ``name`` (plain or suffixed), or None"""
        for g in self.__dict__.get('_globals', ()):
            if name in g._parameters:
                return g, name
        for c in self.__dict__.get('_alchs', ()):
            sfx = c.parameters_name_suffix
            if name in AlchemicalState._PARAMETERS and (sfx is None or len(self._alchs) == 1):
                return c, name
            if sfx is not None and name.endswith('_' + sfx) and name[:-len(sfx) - 1] in AlchemicalState._PARAMETERS:
                return c, name[:-len(sfx) - 1]
        return None

    # (the plain names shadow the end-state class attributes of ThermodynamicState)
    @property
    def lambda_sterics(self):
        hit = self._owner('lambda_sterics')
        return 1.0 if hit is None else getattr(hit[0], hit[1])

    @property
    def lambda_electrostatics(self):
        hit = self._owner('lambda_electrostatics')
        return 1.0 if hit is None else getattr(hit[0], hit[1])

    def __getattr__(self, name):
        if not name.startswith('_'):
            hit = self._owner(name)
            if hit is not None:
                return getattr(hit[0], hit[1])
        raise AttributeError(name)

    def __setattr__(self, name, value):
        hit = None if name.startswith('_') else self._owner(name)
        if hit is not None:
            setattr(hit[0], hit[1], value if isinstance(hit[0], GlobalParameterState) else float(value))
        else:
            object.__setattr__(self, name, value)

    def _state_of_region(self, nm, n_names):
        c = next((c for c in self._alchs if c.parameters_name_suffix == nm), None)
        if c is None and len(self._alchs) == 1 and n_names == 1:
            c = self._alchs[0]
        return c

    def region_lambdas(self, names):
        """(lambda_sterics, lambda_electrostatics) of the alchemical regions ``names`` at this state: the composable state with that
        suffix (a single unsuffixed state answers for a single region)."""
        cs = [self._state_of_region(nm, len(names)) for nm in names]
        return [1.0 if c is None else c.lambda_sterics for c in cs], [1.0 if c is None else c.lambda_electrostatics for c in cs]

    def region_bonded_lambdas(self, names):
        """(lambda_bonds, lambda_angles, lambda_torsions) of the regions ``names``"""
        cs = [self._state_of_region(nm, len(names)) for nm in names]
        return tuple([1.0 if c is None else getattr(c, k) for c in cs] for k in ('lambda_bonds', 'lambda_angles', 'lambda_torsions'))

    def __deepcopy__(self, memo):
        new = copy.copy(self)
        object.__setattr__(new, '_alchs', [copy.copy(c) for c in self._alchs])
        object.__setattr__(new, '_globals', [copy.deepcopy(c) for c in self.__dict__.get('_globals', ())])
        return new

    def global_parameter(self, name):
        """The value of the global parameter ``name`` at this state: the GlobalParameterState that controls it, None if none does
        (or it leaves the parameter undefined)."""
        for g in self.__dict__.get('_globals', ()):
            if name in g._parameters:
                return g._get_global_parameter_value(name)
        return None

    def __setstate__(self, state):
        state = dict(state)
        if '_alch' in state and '_alchs' not in state:           # stores written before several composable states were carried
            state['_alchs'] = [state.pop('_alch')]
        super().__setstate__(state)


class SamplerState:
    def __init__(self, positions, velocities=None, box_vectors=None):
        # plain arrays in nm / nm ps^-1, or openmm.unit.Quantity of arrays / Vec3 lists (states.py:1975-2010)
        self.positions = np.array(to_md(positions), dtype=np.float64).reshape(-1, 3)
        self.velocities = None if velocities is None else np.array(to_md(velocities), dtype=np.float64).reshape(-1, 3)
        if self.velocities is not None and self.velocities.shape != self.positions.shape:
            raise SamplerStateError(SamplerStateError.INCONSISTENT_VELOCITIES)               # states.py:2397-2399
        if box_vectors is not None and not hasattr(box_vectors, 'value_in_unit_system'):
            box_vectors = [to_md(b) for b in box_vectors] if isinstance(box_vectors, (list, tuple)) else box_vectors
        self.box_vectors = None if box_vectors is None else np.array(to_md(box_vectors), dtype=np.float64).reshape(3, 3)
        self.potential_energy = None
        self.kinetic_energy = None

    @property
    def n_particles(self):
        return self.positions.shape[0]

    @property
    def total_energy(self):
        """states.py:2170-2174: potential + kinetic energy when both are cached, else None."""
        if self.potential_energy is None or self.kinetic_energy is None:
            return None
        return self.potential_energy + self.kinetic_energy

    @property
    def area_xy(self):
        """states.py:2180-2184: area of the box in the xy plane (None without a box)."""
        if self.box_vectors is None:
            return None
        return float(abs(np.cross(self.box_vectors[0], self.box_vectors[1])[2]))

    def __getitem__(self, item):
        """states.py:2296-2325: the sampler state of a subset of particles (an index, a slice or a sequence of indices): copies
        of their positions and velocities, the same box, no energies (undefined for a subset)."""
        if np.issubdtype(type(item), np.integer):
            item = [int(item)]
        sub = SamplerState(np.array(self.positions[item], dtype=np.float64),
                           velocities=None if self.velocities is None else np.array(self.velocities[item], dtype=np.float64),
                           box_vectors=None if self.box_vectors is None else self.box_vectors.copy())
        return sub

    def has_nan(self):
        """states.py:2281-2293: any NaN among the positions (what the reference checks) or the velocities."""
        return bool(np.isnan(self.positions).any() or (self.velocities is not None and np.isnan(self.velocities).any()))

    @property
    def volume(self):
        if self.box_vectors is None:
            return None
        return float(abs(np.linalg.det(self.box_vectors)))

    @property
    def box_edges(self):
        """Orthorhombic edge lengths; triclinic boxes are not supported by the engine."""
        if self.box_vectors is None:
            return None
        off = self.box_vectors - np.diag(np.diag(self.box_vectors))
        if np.abs(off).max() > 1e-9:
            raise NotImplementedError('triclinic periodic boxes are not supported')
        return np.diag(self.box_vectors).copy()

    def __getstate__(self):
        return dict(positions=self.positions, velocities=self.velocities, box_vectors=self.box_vectors,
                    potential_energy=self.potential_energy, kinetic_energy=self.kinetic_energy)

    def __setstate__(self, s):
        self.__dict__.update(s)


def reduced_potential_at_states(sampler_state, thermodynamic_states, context_cache=None, engine=None):
    """states.py:144-183: the reduced potentials of ONE configuration at a list of thermodynamic states (grouped by compatible
    System: one set of device tables per group, every state of a group from one evaluation where only the temperature or
    lambda differs).  The engine's u_kl row for a single replica: ``engine`` is the engine object to use (default: a HipEngine
    on the GPU; ``context_cache.make_engine()`` when a cache is given)."""
    from .multistate import MultiStateSampler
    from . import mcmc
    if engine is None and context_cache is not None and hasattr(context_cache, 'make_engine'):
        engine = context_cache.make_engine()
    row = MultiStateSampler(mcmc_moves=mcmc.LangevinDynamicsMove(n_steps=1), number_of_iterations=0, engine=engine,
                            online_analysis_interval=None)
    row.create(list(thermodynamic_states), [sampler_state], storage=None)
    row._compute_energies()
    return np.array(row.energy_thermodynamic_states[0], dtype=np.float64)


def group_by_compatibility(states):
    """states.py:186-217."""
    groups, indices = [], []
    for i, s in enumerate(states):
        for g, idx in zip(groups, indices):
            if s.is_state_compatible(g[0]):
                g.append(s)
                idx.append(i)
                break
        else:
            groups.append([s])
            indices.append([i])
    return groups, indices
