"""Compiler of OpenMM energy expressions for the custom bond, angle, torsion, external, compound-bond and centroid-bond forces
(system.CustomBondForce, CustomAngleForce, CustomTorsionForce, CustomExternalForce, CustomCompoundBondForce, CustomCentroidBondForce):
an energy string becomes the postfix program of include/remd_hip_custom.h, which csrc/custom_terms.hip, csrc/custom_compound.hip and
csrc/custom_centroid.hip run on a forward-mode stack machine (every stack slot a value and its partial derivatives with respect to
the force's variables).

A compound-bond force of P particles (1 ... MAX_PARTICLES) has the variables x1 y1 z1 ... xP yP zP (operand 3*(i-1)+c) and the
functions distance(pi,pj), angle(pi,pj,pk) and dihedral(pi,pj,pk,pl), whose operand packs the zero-based particle slots in 4-bit
fields, first argument lowest; the particle names p1 ... pP are legal only there.  pointdistance(x1,y1,z1,x2,y2,z2) is the
periodicdistance opcode (the engine images it only where the force is periodic); pointangle and pointdihedral are refused.

A centroid-bond force of P groups per bond is the same thing over the groups' centroids: the same variables, the same functions with
the names g1 ... gP in place of p1 ... pP, the same program.  Its descriptor carries the groups beside it (custom_terms_desc).

Grammar: numbers (exponent notation included), ``+ - * / ^``, unary minus, parentheses, function calls, and ``;``-separated
definitions ``name = expr`` in any order, substituted where they are used.  ``^`` binds tighter than unary minus and groups to the
right, as in OpenMM's Lepton.  A constant integer exponent up to +-64 becomes REMD_CX_POWI (multiplications: defined for a negative
base); every other power is REMD_CX_POW.

The limits are the engine's (include/remd_hip_custom.h); what is over them, an unknown name, an unknown or tabulated function is
refused with NotImplementedError naming the force and the item.
"""
import re

import numpy as np

MAX_PROGRAM, MAX_STACK, MAX_PARAMS, MAX_GLOBALS, MAX_FORCES = 256, 16, 16, 16, 8
MAX_INTEGER_POWER = 64
MAX_PARTICLES = 8                               # particles per bond of a compound-bond force

KIND_BOND, KIND_ANGLE, KIND_TORSION, KIND_EXTERNAL, KIND_COMPOUND, KIND_CENTROID = 0, 1, 2, 3, 4, 5
KIND_OF_CLASS = {'CustomBondForce': KIND_BOND, 'CustomAngleForce': KIND_ANGLE, 'CustomTorsionForce': KIND_TORSION,
                 'CustomExternalForce': KIND_EXTERNAL, 'CustomCompoundBondForce': KIND_COMPOUND, 'CustomCentroidBondForce': KIND_CENTROID}
VARIABLES = {KIND_BOND: ('r',), KIND_ANGLE: ('theta',), KIND_TORSION: ('theta',), KIND_EXTERNAL: ('x', 'y', 'z')}


def compound_variables(n_particles):
    """x1 y1 z1 ... xP yP zP: the variables of a compound-bond force in operand order"""
    return tuple('%s%d' % (c, i) for i in range(1, n_particles + 1) for c in 'xyz')


# opcodes (include/remd_hip_custom.h)
(CONST, VAR, PARAM, GLOBAL, ADD, SUB, MUL, DIV, NEG, POWI, POW, SQRT, EXP, LOG, SIN, COS, TAN, ASIN, ACOS, ATAN, ATAN2, SINH, COSH,
 TANH, ERF, ERFC, ABS, MIN, MAX, STEP, DELTA, SELECT, FLOOR, CEIL, PERIODICDISTANCE, DISTANCE, ANGLE, DIHEDRAL) = range(38)

# name -> (opcode, number of arguments)
FUNCTIONS = dict(sqrt=(SQRT, 1), exp=(EXP, 1), log=(LOG, 1), sin=(SIN, 1), cos=(COS, 1), tan=(TAN, 1), asin=(ASIN, 1), acos=(ACOS, 1),
                 atan=(ATAN, 1), atan2=(ATAN2, 2), sinh=(SINH, 1), cosh=(COSH, 1), tanh=(TANH, 1), erf=(ERF, 1), erfc=(ERFC, 1),
                 abs=(ABS, 1), min=(MIN, 2), max=(MAX, 2), step=(STEP, 1), delta=(DELTA, 1), select=(SELECT, 3), floor=(FLOOR, 1),
                 ceil=(CEIL, 1), periodicdistance=(PERIODICDISTANCE, 6))
_BINARY = {'+': ADD, '-': SUB, '*': MUL, '/': DIV}
# slots an opcode takes from the stack (it pushes one)
POPS = {CONST: 0, VAR: 0, PARAM: 0, GLOBAL: 0, ADD: 2, SUB: 2, MUL: 2, DIV: 2, POW: 2, ATAN2: 2, MIN: 2, MAX: 2, SELECT: 3,
        PERIODICDISTANCE: 6, DISTANCE: 0, ANGLE: 0, DIHEDRAL: 0}
# the functions of particles of a compound-bond force: name -> (opcode, number of particles)
PARTICLE_FUNCTIONS = dict(distance=(DISTANCE, 2), angle=(ANGLE, 3), dihedral=(DIHEDRAL, 4))
# the names of a bond's particles: p1 ... of a compound-bond force, g1 ... of a centroid-bond force (prefix -> pattern, noun)
_PARTICLE_NAMES = {'p': (re.compile(r'p([1-9][0-9]*)'), 'particle'), 'g': (re.compile(r'g([1-9][0-9]*)'), 'group')}

_TOKEN = re.compile(r'\s*(?:(\d+\.?\d*(?:[eE][+-]?\d+)?|\.\d+(?:[eE][+-]?\d+)?)|([A-Za-z_][A-Za-z_0-9]*)|(.))')


class _Parser:
    """Recursive descent: expr := term (('+' | '-') term)*; term := unary (('*' | '/') unary)*; unary := '-' unary | power;
    power := atom ('^' unary)?; atom := number | name | name '(' expr (',' expr)* ')' | '(' expr ')'."""

    def __init__(self, text, where):
        self.where, self.text = where, text
        self.tokens = []
        pos = 0
        while pos < len(text):
            m = _TOKEN.match(text, pos)
            if m is None or m.end() == pos:
                break
            pos = m.end()
            if m.group(1) is not None:
                self.tokens.append(('num', float(m.group(1))))
            elif m.group(2) is not None:
                self.tokens.append(('name', m.group(2)))
            elif m.group(3) is not None and not m.group(3).isspace():
                self.tokens.append(('op', m.group(3)))
        self.i = 0

    def fail(self, what):
        raise NotImplementedError('%s: %s in %r' % (self.where, what, self.text))

    def peek(self):
        return self.tokens[self.i] if self.i < len(self.tokens) else ('end', None)

    def take(self, kind=None, value=None):
        tok = self.peek()
        if (kind is not None and tok[0] != kind) or (value is not None and tok[1] != value):
            self.fail('expected %s, found %r' % (value or kind, tok[1]))
        self.i += 1
        return tok

    def parse(self):
        e = self.expr()
        if self.peek()[0] != 'end':
            self.fail('unexpected %r' % (self.peek()[1],))
        return e

    def expr(self):
        e = self.term()
        while self.peek() in (('op', '+'), ('op', '-')):
            op = self.take()[1]
            e = ('bin', op, e, self.term())
        return e

    def term(self):
        e = self.unary()
        while self.peek() in (('op', '*'), ('op', '/')):
            op = self.take()[1]
            e = ('bin', op, e, self.unary())
        return e

    def unary(self):
        if self.peek() == ('op', '-'):
            self.take()
            return ('neg', self.unary())
        if self.peek() == ('op', '+'):
            self.take()
            return self.unary()
        return self.power()

    def power(self):
        base = self.atom()
        if self.peek() == ('op', '^'):
            self.take()
            return ('pow', base, self.unary())
        return base

    def atom(self):
        kind, value = self.peek()
        if kind == 'num':
            self.take()
            return ('num', value)
        if kind == 'name':
            self.take()
            if self.peek() == ('op', '('):
                self.take()
                args = [self.expr()]
                while self.peek() == ('op', ','):
                    self.take()
                    args.append(self.expr())
                self.take('op', ')')
                return ('call', value, args)
            return ('name', value)
        if (kind, value) == ('op', '('):
            self.take()
            e = self.expr()
            self.take('op', ')')
            return e
        self.fail('unexpected %r' % (value,))


def _constant(node):
    """The value of a subtree of numbers and + - * / unary minus, else None."""
    if node[0] == 'num':
        return node[1]
    if node[0] == 'neg':
        v = _constant(node[1])
        return None if v is None else -v
    if node[0] == 'bin':
        a, b = _constant(node[2]), _constant(node[3])
        if a is None or b is None or (node[1] == '/' and b == 0.0):
            return None
        return {'+': a + b, '-': a - b, '*': a * b, '/': a / b if b else None}[node[1]]
    return None


def split_definitions(energy, where='expression'):
    """'expr; a = ...; b = ...' -> (expr, {name: text})."""
    parts = [p.strip() for p in str(energy).split(';')]
    parts = [p for p in parts if p]
    if not parts:
        raise NotImplementedError('%s: empty energy expression' % where)
    definitions = {}
    for p in parts[1:]:
        name, eq, body = p.partition('=')
        if not eq or not re.fullmatch(r'[A-Za-z_][A-Za-z_0-9]*', name.strip()):
            raise NotImplementedError('%s: %r is not a definition name = expression' % (where, p))
        definitions[name.strip()] = body.strip()
    return parts[0], definitions


def compile_expression(energy, variables, parameters, global_columns, where='expression', tabulated=(), periodic_distance=False,
                       n_particles=0, particle_prefix='p'):
    """The postfix program of ``energy``.

    variables: the force's own variable names in operand order; parameters: the per-term parameter names in order; global_columns:
    {global parameter name: column of the handle's table}; tabulated: names of tabulated functions (refused); periodic_distance:
    whether periodicdistance(...) is allowed (an external force that uses periodic boundary conditions); n_particles: the particles
    per bond of a compound-bond force (0: another force), which opens distance / angle / dihedral over p1 ... pP and pointdistance;
    particle_prefix: 'p', or 'g' for the groups g1 ... gP of a centroid-bond force (the messages then speak of groups).

    Returns dict(program int32 [n][2], consts float64 [m], stack_depth).
    """
    body, definitions = split_definitions(energy, where)
    _PARTICLE_NAME, noun = _PARTICLE_NAMES[particle_prefix]
    other = {'p': 'g', 'g': 'p'}[particle_prefix]
    trees = {}
    program, consts, const_index = [], [], {}
    depth = [0, 0]                              # current, maximum

    def tree_of(name):
        if name not in trees:
            trees[name] = _Parser(definitions[name], where).parse()
        return trees[name]

    def emit(op, arg=0):
        program.append((op, int(arg)))
        depth[0] += 1 - POPS.get(op, 1)
        depth[1] = max(depth[1], depth[0])

    def push_const(v):
        v = float(v)
        key = np.float64(v).tobytes()
        if key not in const_index:
            const_index[key] = len(consts)
            consts.append(v)
        emit(CONST, const_index[key])

    def walk(node, active):
        kind = node[0]
        folded = _constant(node)
        if folded is not None:
            return push_const(folded)
        if kind == 'name':
            name = node[1]
            if name in definitions:
                if name in active:
                    raise NotImplementedError('%s: the definition of %r refers to itself' % (where, name))
                return walk(tree_of(name), active | {name})
            if name in variables:
                return emit(VAR, variables.index(name))
            if name in parameters:
                return emit(PARAM, parameters.index(name))
            if name in global_columns:
                return emit(GLOBAL, global_columns[name])
            if n_particles and _PARTICLE_NAME.fullmatch(name):
                raise NotImplementedError('%s: %s name %r outside distance(), angle() and dihedral()' % (where, noun, name))
            if n_particles and _PARTICLE_NAMES[other][0].fullmatch(name):
                raise NotImplementedError('%s: %s name %r (the %ss of this force are %s1 ... %s%d)'
                                          % (where, _PARTICLE_NAMES[other][1], name, noun, particle_prefix, particle_prefix, n_particles))
            raise NotImplementedError('%s: unknown variable %r' % (where, name))
        if kind == 'neg':
            walk(node[1], active)
            return emit(NEG)
        if kind == 'bin':
            walk(node[2], active)
            walk(node[3], active)
            return emit(_BINARY[node[1]])
        if kind == 'pow':
            walk(node[1], active)
            n = _constant(node[2])
            if n is not None and float(n).is_integer() and abs(n) <= MAX_INTEGER_POWER:
                return emit(POWI, int(n))
            walk(node[2], active)
            return emit(POW)
        if kind == 'call':
            name, args = node[1], node[2]
            if name in tabulated:
                raise NotImplementedError('%s: tabulated function %r (tabulated functions are not supported)' % (where, name))
            if n_particles and name in PARTICLE_FUNCTIONS:
                op, n_args = PARTICLE_FUNCTIONS[name]
                if len(args) != n_args:
                    raise NotImplementedError('%s: function %r takes %d %ss, not %d' % (where, name, n_args, noun, len(args)))
                packed = 0
                for k, a in enumerate(args):
                    m = _PARTICLE_NAME.fullmatch(a[1]) if a[0] == 'name' else None
                    if m is None and a[0] == 'name' and _PARTICLE_NAMES[other][0].fullmatch(a[1]):
                        raise NotImplementedError('%s: %s name %r (the %ss of this force are %s1 ... %s%d)'
                                                  % (where, _PARTICLE_NAMES[other][1], a[1], noun, particle_prefix, particle_prefix, n_particles))
                    if m is None:
                        raise NotImplementedError('%s: the arguments of %r are %s names %s1 ... %s%d'
                                                  % (where, name, noun, particle_prefix, particle_prefix, n_particles))
                    if int(m.group(1)) > n_particles:
                        raise NotImplementedError('%s: %s %r in a bond of %d %ss' % (where, noun, a[1], n_particles, noun))
                    packed |= (int(m.group(1)) - 1) << (4 * k)
                return emit(op, packed)
            if n_particles and name in ('pointangle', 'pointdihedral'):
                raise NotImplementedError('%s: function %r (pointangle and pointdihedral are not supported)' % (where, name))
            if n_particles and name == 'pointdistance':
                if len(args) != 6:
                    raise NotImplementedError('%s: function %r takes 6 arguments, not %d' % (where, name, len(args)))
                for a in args:
                    walk(a, active)
                return emit(PERIODICDISTANCE)
            if name not in FUNCTIONS or (name == 'periodicdistance' and not periodic_distance):
                raise NotImplementedError('%s: unknown function %r' % (where, name))
            op, n_args = FUNCTIONS[name]
            if len(args) != n_args:
                raise NotImplementedError('%s: function %r takes %d arguments, not %d' % (where, name, n_args, len(args)))
            for a in args:
                walk(a, active)
            return emit(op)
        raise NotImplementedError('%s: cannot compile %r' % (where, node))

    walk(_Parser(body, where).parse(), frozenset())
    if len(program) > MAX_PROGRAM:
        raise NotImplementedError('%s: a program of %d instructions (the engine takes %d)' % (where, len(program), MAX_PROGRAM))
    if depth[1] > MAX_STACK:
        raise NotImplementedError('%s: an expression that needs %d stack slots (the engine has %d)' % (where, depth[1], MAX_STACK))
    return dict(program=np.array(program, dtype=np.int32).reshape(-1, 2), consts=np.array(consts, dtype=np.float64),
                stack_depth=int(depth[1]))


# ---- the forces of a System -------------------------------------------------------------------------------------------------------
def _per_term_names(force):
    return list(force._per_bond)


def is_custom_term_force(force):
    """Whether system_to_desc sends this force down the expression path: one of the four classes whose energy is neither the
    HarmonicOscillator string (ext_K / ext_x0 / ext_U0) nor one of the restraint forms (csrc/restraints.hip), or a
    CustomCompoundBondForce, or a system.CustomCentroidBondForce (forces.CustomCentroidBondForce, the restraints' base, is another class)."""
    from . import system as _system
    from . import forces as _forces
    if isinstance(force, (_system.CustomCompoundBondForce, _system.CustomCentroidBondForce)):
        return True
    if isinstance(force, _system.CustomExternalForce):
        return not force.is_harmonic_oscillator()
    if isinstance(force, (_system.CustomAngleForce, _system.CustomTorsionForce)):
        return True
    if isinstance(force, _system.CustomBondForce):
        return not _forces.is_restraint_form(force)
    return False


def centroid_groups(force, masses):
    """The groups of a centroid-bond force in CSR form: (group_offsets int32 [G+1], group_atoms int32, group_weights float64), the
    weights normalised to sum 1 per group in f64 -- the group's own where it gives any, else the particles' masses."""
    n_atoms = None if masses is None else len(masses)
    offsets, atoms, weights = [0], [], []
    for g in range(force.getNumGroups()):
        particles, w = force.getGroupParameters(g)
        if len(particles) == 0:
            raise ValueError('CustomCentroidBondForce: group %d is empty' % g)
        if len(w) not in (0, len(particles)):
            raise ValueError('CustomCentroidBondForce: group %d has %d particles and %d weights' % (g, len(particles), len(w)))
        if min(particles) < 0 or (n_atoms is not None and max(particles) >= n_atoms):
            raise ValueError('CustomCentroidBondForce: group %d names particle %d (the System has %s)'
                             % (g, min(particles) if min(particles) < 0 else max(particles), n_atoms))
        if len(w) == 0:
            if masses is None:
                raise ValueError('CustomCentroidBondForce: group %d has no weights and no masses were given' % g)
            w = [float(masses[p]) for p in particles]
        w = np.array(w, dtype=np.float64)
        if np.any(w < 0.0):
            raise ValueError('CustomCentroidBondForce: group %d has a negative weight' % g)
        if not w.sum() > 0.0:
            raise ValueError('CustomCentroidBondForce: the weights of group %d sum to zero' % g)
        atoms += list(particles)
        weights.append(w / w.sum())
        offsets.append(len(atoms))
    return (np.array(offsets, dtype=np.int32), np.array(atoms, dtype=np.int32),
            np.concatenate(weights) if weights else np.zeros(0, dtype=np.float64))


def custom_terms_desc(forces, masses=None):
    """The 'custom_terms' entry of system.system_to_desc for the custom forces ``forces`` (in System order): a dict keyed by position
    ('000', '001', ...), each value dict(kind, atoms [n][1..4] ([n][P] and n_particles = P of a compound-bond force; of a centroid-bond force atoms holds
    group numbers and group_offsets, group_atoms, group_weights describe the groups, centroid_groups(force, masses)), params [n][p], global_names, global_defaults, program, consts,
    stack_depth, periodic, force_group, energy).  The global names and defaults are the handle's columns, the same in every entry: a
    global two forces share is one column."""
    if len(forces) > MAX_FORCES:
        raise NotImplementedError('%d custom forces in one System (the engine takes %d)' % (len(forces), MAX_FORCES))
    names, defaults = [], []
    for f in forces:
        for i in range(f.getNumGlobalParameters()):
            name, value = f.getGlobalParameterName(i), float(f.getGlobalParameterDefaultValue(i))
            if name in names:
                if defaults[names.index(name)] != value:
                    raise ValueError('%s: global parameter %r has the default value %r here and %r in another force'
                                     % (type(f).__name__, name, value, defaults[names.index(name)]))
            else:
                names.append(name)
                defaults.append(value)
    if len(names) > MAX_GLOBALS:
        raise NotImplementedError('%d global parameters in the custom forces of one System (the engine takes %d): %s'
                                  % (len(names), MAX_GLOBALS, ', '.join(names)))
    groups = sorted({int(f.getForceGroup()) for f in forces})
    if len(groups) > 1:
        raise NotImplementedError('custom forces in several force groups (%s): every custom force of a System must sit in one (%s)'
                                  % (', '.join(str(g) for g in groups), ', '.join('%s in %d' % (type(f).__name__, f.getForceGroup()) for f in forces)))
    columns = {n: i for i, n in enumerate(names)}
    out = {}
    for k, f in enumerate(forces):
        cls = [c for c in KIND_OF_CLASS if c in [b.__name__ for b in type(f).__mro__]][0]
        kind = KIND_OF_CLASS[cls]
        where = '%s (energy %r)' % (cls, f.getEnergyFunction())
        per_term = _per_term_names(f)
        if len(per_term) > MAX_PARAMS:
            raise NotImplementedError('%s: %d per-term parameters (the engine takes %d): %s' % (cls, len(per_term), MAX_PARAMS, ', '.join(per_term)))
        tabulated = [f.getTabulatedFunctionName(i) for i in range(f.getNumTabulatedFunctions())]
        own = {n: columns[n] for n in (f.getGlobalParameterName(i) for i in range(f.getNumGlobalParameters()))}
        periodic = bool(f.usesPeriodicBoundaryConditions())
        n_particles = 0
        if kind == KIND_COMPOUND:
            n_particles = int(f.getNumParticlesPerBond())
            if not 1 <= n_particles <= MAX_PARTICLES:
                raise NotImplementedError('%s: bonds of %d particles (the engine takes 1 ... %d)' % (cls, n_particles, MAX_PARTICLES))
        if kind == KIND_CENTROID:
            n_particles = int(f.getNumGroupsPerBond())
            if not 1 <= n_particles <= MAX_PARTICLES:
                raise NotImplementedError('%s: bonds of %d groups (the engine takes 1 ... %d)' % (cls, n_particles, MAX_PARTICLES))
        prog = compile_expression(f.getEnergyFunction(), compound_variables(n_particles) if n_particles else VARIABLES[kind], per_term, own,
                                  where=where, tabulated=tabulated, periodic_distance=(kind == KIND_EXTERNAL and periodic),
                                  n_particles=n_particles, particle_prefix='g' if kind == KIND_CENTROID else 'p')
        atoms, params = f._term_arrays()
        if len(atoms) == 0:
            continue
        if kind == KIND_CENTROID:
            groups = centroid_groups(f, masses)
            if atoms.min() < 0 or atoms.max() >= f.getNumGroups():
                raise ValueError('%s: a bond names group %d (the force has %d)'
                                 % (cls, atoms.min() if atoms.min() < 0 else atoms.max(), f.getNumGroups()))
        out['%03d' % len(out)] = dict(kind=kind, atoms=atoms, params=params, global_names=list(names),
                                      global_defaults=np.array(defaults, dtype=np.float64), program=prog['program'], consts=prog['consts'],
                                      stack_depth=prog['stack_depth'], periodic=int(periodic), force_group=int(f.getForceGroup()),
                                      energy=f.getEnergyFunction())
        if n_particles:
            out['%03d' % (len(out) - 1)]['n_particles'] = n_particles
        if kind == KIND_CENTROID:
            out['%03d' % (len(out) - 1)].update(group_offsets=groups[0], group_atoms=groups[1], group_weights=groups[2])
    return out


def custom_globals(system, names, states):
    """[K][n]: the value of each global column at every state -- the state's GlobalParameterState where it carries the name, else the
    default value the forces carry."""
    defaults = {}
    for f in system.getForces():
        if is_custom_term_force(f):
            for i in range(f.getNumGlobalParameters()):
                defaults.setdefault(f.getGlobalParameterName(i), float(f.getGlobalParameterDefaultValue(i)))
    out = np.empty((len(states), len(names)))
    for k, s in enumerate(states):
        for i, name in enumerate(names):
            v = s.global_parameter(name) if hasattr(s, 'global_parameter') else None
            out[k, i] = defaults[name] if v is None else float(v)
    return out
