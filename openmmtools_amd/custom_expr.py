"""Compiler of OpenMM energy expressions for the custom bond, angle, torsion, external, compound-bond, centroid-bond, nonbonded and
donor-acceptor forces (system.CustomBondForce, CustomAngleForce, CustomTorsionForce, CustomExternalForce, CustomCompoundBondForce,
CustomCentroidBondForce, CustomNonbondedForce, CustomHbondForce): an energy string becomes the postfix program of include/remd_hip_custom.h, which csrc/custom_terms.hip,
csrc/custom_compound.hip, csrc/custom_centroid.hip, csrc/custom_cv.hip and csrc/custom_nonbonded.hip run on a forward-mode stack machine (every stack slot a value and its partial derivatives with respect to
the force's variables).

A compound-bond force of P particles (1 ... MAX_PARTICLES) has the variables x1 y1 z1 ... xP yP zP (operand 3*(i-1)+c) and the
functions distance(pi,pj), angle(pi,pj,pk) and dihedral(pi,pj,pk,pl), whose operand packs the zero-based particle slots in 4-bit
fields, first argument lowest; the particle names p1 ... pP are legal only there.  pointdistance(x1,y1,z1,x2,y2,z2) is the
periodicdistance opcode (the engine images it only where the force is periodic); pointangle and pointdihedral are refused.

A centroid-bond force of P groups per bond is the same thing over the groups' centroids: the same variables, the same functions with
the names g1 ... gP in place of p1 ... pP, the same program.  Its descriptor carries the groups beside it (custom_terms_desc).

A nonbonded force has the one variable r; a per-particle parameter p appears as p1 and p2 (PARAM operand k for particle 1,
n_params + k for particle 2; at most MAX_PAIR_PARAMS per-particle parameters, so that MAX_PARAMS bounds the operand).  A bare
per-particle name, a suffix 3 and x / y / z are refused by name.  Its long-range correction is computed here, on the host in f64
(long_range_coefficients).

A donor-acceptor force (system.CustomHbondForce) compiles through the compound-bond path: distance, angle and dihedral over the names
d1 d2 d3 (particle slots 0 1 2) and a1 a2 a3 (slots 3 4 5), no coordinates, no pointdistance; the per-donor parameters are the first
PARAM operands, the per-acceptor ones follow; the set of particle slots the expression names is recorded as a 6-bit mask
(particle_mask): the engine runs one seeded pass per named slot (csrc/custom_hbond.hip).

A many-particle force (system.CustomManyParticleForce, three particles per set) compiles the same way over the names p1 p2 p3
(particle slots 0 1 2); per-particle parameter q is legal with the slot appended only (sigma1, sigma2, sigma3) and is PARAM operand
3 q + s for slot s; the 3-bit particle_mask is recorded likewise (csrc/custom_manyparticle.hip).

Grammar: numbers (exponent notation included), ``+ - * / ^``, unary minus, parentheses, function calls, and ``;``-separated
definitions ``name = expr`` in any order, substituted where they are used.  ``^`` binds tighter than unary minus and groups to the
right, as in OpenMM's Lepton.  A constant integer exponent up to +-64 becomes REMD_CX_POWI (multiplications: defined for a negative
base); every other power is REMD_CX_POW.

Tabulated functions: a call of a force's system.Continuous1DFunction (natural or periodic cubic spline) compiles to TABLE1D, of a
system.Discrete1DFunction to LOOKUP1D; the function's samples, and the spline's second derivatives solved here in f64
(spline_second_derivatives), travel as a block of the force's constants behind the scalars, the operand its offset (layout and
out-of-range rules: include/remd_hip_custom.h).  At most MAX_TABLE_POINTS points per function.  A system.Continuous2DFunction
compiles to TABLE2D (two arguments; the block carries f, fx, fy, fxy at every node, fitted here in f64: table2d_nodes), a
system.Discrete2DFunction to LOOKUP2D and a system.Discrete3DFunction to LOOKUP3D (three arguments); at most MAX_TABLE_CELLS values.

The limits are the engine's (include/remd_hip_custom.h); what is over them, an unknown name, an unknown function or a tabulated
function of another kind is refused with NotImplementedError naming the force and the item.
"""
import re

import numpy as np

MAX_PROGRAM, MAX_STACK, MAX_PARAMS, MAX_GLOBALS, MAX_FORCES = 256, 16, 16, 16, 8
MAX_INTEGER_POWER = 64
MAX_PARTICLES = 8                               # particles per bond of a compound-bond force
MAX_PAIR_PARAMS = MAX_PARAMS // 2               # per-particle parameters of a nonbonded force (each appears twice in a pair's program)
MAX_TABLE_POINTS = 8192                         # points of one tabulated function of one argument
MAX_TABLE_CELLS = 65536                         # values (the product of the sizes) of one tabulated function of two or three arguments

KIND_BOND, KIND_ANGLE, KIND_TORSION, KIND_EXTERNAL, KIND_COMPOUND, KIND_CENTROID, KIND_NONBONDED = 0, 1, 2, 3, 4, 5, 6
KIND_CV = 7                                     # system.CustomCVForce over RMSDForce variables (csrc/custom_cv.hip)
MAX_CVS = 3                                     # collective variables per CustomCVForce: the machine carries three partials
KIND_CMAP = 8                                   # system.CMAPTorsionForce: no expression, the energy a map of two dihedrals (csrc/cmap.hip)
MAX_MAPS = 64                                   # maps per CMAPTorsionForce
KIND_HBOND = 10                                 # system.CustomHbondForce: donor-acceptor pairs (csrc/custom_hbond.hip)
HBOND_SLOTS = dict(d1=0, d2=1, d3=2, a1=3, a2=4, a3=5)   # the particle names of a donor-acceptor expression -> particle slot
KIND_MANYPARTICLE = 11                          # system.CustomManyParticleForce: sets of three particles (csrc/custom_manyparticle.hip)
MANYPARTICLE_SLOTS = dict(p1=0, p2=1, p3=2)     # the particle names of a many-particle expression -> particle slot
MAX_SET_PARAMS = 5                              # per-particle parameters of a many-particle force: 3 x 5 of the machine's 16 columns
MP_MAX_NEIGHBORS = 128                          # REMD_CUSTOM_MP_MAX_NEIGHBORS: the capacity of one particle's neighbour row
KIND_OF_CLASS = {'CustomNonbondedForce': KIND_NONBONDED, 'CustomBondForce': KIND_BOND, 'CustomAngleForce': KIND_ANGLE, 'CustomTorsionForce': KIND_TORSION,
                 'CustomExternalForce': KIND_EXTERNAL, 'CustomCompoundBondForce': KIND_COMPOUND, 'CustomCentroidBondForce': KIND_CENTROID,
                 'CustomCVForce': KIND_CV, 'CMAPTorsionForce': KIND_CMAP, 'CustomHbondForce': KIND_HBOND,
                 'CustomManyParticleForce': KIND_MANYPARTICLE}
VARIABLES = {KIND_BOND: ('r',), KIND_ANGLE: ('theta',), KIND_TORSION: ('theta',), KIND_EXTERNAL: ('x', 'y', 'z'), KIND_NONBONDED: ('r',)}


def compound_variables(n_particles):
    """x1 y1 z1 ... xP yP zP: the variables of a compound-bond force in operand order"""
    return tuple('%s%d' % (c, i) for i in range(1, n_particles + 1) for c in 'xyz')


# opcodes (include/remd_hip_custom.h)
(CONST, VAR, PARAM, GLOBAL, ADD, SUB, MUL, DIV, NEG, POWI, POW, SQRT, EXP, LOG, SIN, COS, TAN, ASIN, ACOS, ATAN, ATAN2, SINH, COSH,
 TANH, ERF, ERFC, ABS, MIN, MAX, STEP, DELTA, SELECT, FLOOR, CEIL, PERIODICDISTANCE, DISTANCE, ANGLE, DIHEDRAL, TABLE1D,
 LOOKUP1D, TABLE2D, LOOKUP2D, LOOKUP3D) = range(43)

# name -> (opcode, number of arguments)
FUNCTIONS = dict(sqrt=(SQRT, 1), exp=(EXP, 1), log=(LOG, 1), sin=(SIN, 1), cos=(COS, 1), tan=(TAN, 1), asin=(ASIN, 1), acos=(ACOS, 1),
                 atan=(ATAN, 1), atan2=(ATAN2, 2), sinh=(SINH, 1), cosh=(COSH, 1), tanh=(TANH, 1), erf=(ERF, 1), erfc=(ERFC, 1),
                 abs=(ABS, 1), min=(MIN, 2), max=(MAX, 2), step=(STEP, 1), delta=(DELTA, 1), select=(SELECT, 3), floor=(FLOOR, 1),
                 ceil=(CEIL, 1), periodicdistance=(PERIODICDISTANCE, 6))
_BINARY = {'+': ADD, '-': SUB, '*': MUL, '/': DIV}
# slots an opcode takes from the stack (it pushes one)
POPS = {CONST: 0, VAR: 0, PARAM: 0, GLOBAL: 0, ADD: 2, SUB: 2, MUL: 2, DIV: 2, POW: 2, ATAN2: 2, MIN: 2, MAX: 2, SELECT: 3,
        PERIODICDISTANCE: 6, DISTANCE: 0, ANGLE: 0, DIHEDRAL: 0, TABLE2D: 2, LOOKUP2D: 2, LOOKUP3D: 3}
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


def spline_second_derivatives(values, lo, hi, periodic=False):
    """y'' [n] of the cubic spline through ``values`` at n uniformly spaced points over [lo, hi], in f64: the natural spline (y'' = 0 at
    both ends; the tridiagonal system y''[i-1] + 4 y''[i] + y''[i+1] = 6 (y[i+1] - 2 y[i] + y[i-1]) / h^2 by the Thomas algorithm) or the
    periodic one (the same rows cyclically over the n - 1 distinct points, by the Thomas algorithm with the Sherman-Morrison correction;
    y''[n-1] = y''[0])."""
    y = np.asarray(values, dtype=np.float64)
    n = len(y)
    h = (float(hi) - float(lo)) / (n - 1)
    out = np.zeros(n)

    def thomas(diag, rhs):                      # off-diagonals 1
        m = len(rhs)
        c, d = np.zeros(m), np.zeros(m)
        c[0], d[0] = 1.0 / diag[0], rhs[0] / diag[0]
        for i in range(1, m):
            w = diag[i] - c[i - 1]
            c[i], d[i] = 1.0 / w, (rhs[i] - d[i - 1]) / w
        x = np.zeros(m)
        x[-1] = d[-1]
        for i in range(m - 2, -1, -1):
            x[i] = d[i] - c[i] * x[i + 1]
        return x

    if not periodic:
        if n > 2:
            out[1:-1] = thomas(np.full(n - 2, 4.0), 6.0 * (y[2:] - 2.0 * y[1:-1] + y[:-2]) / (h * h))
        return out
    m = n - 1                                   # the distinct points; the neighbours of point i are i - 1 and i + 1 modulo m
    p = y[:m]
    rhs = 6.0 * (np.roll(p, -1) - 2.0 * p + np.roll(p, 1)) / (h * h)
    if m == 2:                                  # both neighbours are the other point: 4 a + 2 b = rhs0, 2 a + 4 b = rhs1
        out[0], out[1] = (4.0 * rhs[0] - 2.0 * rhs[1]) / 12.0, (4.0 * rhs[1] - 2.0 * rhs[0]) / 12.0
    else:
        gamma = -4.0
        diag = np.full(m, 4.0)
        diag[0] -= gamma
        diag[-1] -= 1.0 / gamma
        u = np.zeros(m)
        u[0], u[-1] = gamma, 1.0
        x, z = thomas(diag, rhs), thomas(diag, u)
        out[:m] = x - z * (x[0] + x[-1] / gamma) / (1.0 + z[0] + z[-1] / gamma)
    out[-1] = out[0]
    return out


def spline_node_derivatives(values, lo, hi, periodic=False):
    """s'(x_i) [..., n] of the cubic splines (natural or periodic) through the rows ``values[..., :]`` at n uniformly spaced points over
    [lo, hi]: (y[i+1] - y[i]) / h - h (2 M[i] + M[i+1]) / 6, at the last node (y[n-1] - y[n-2]) / h + h (M[n-2] + 2 M[n-1]) / 6, M the
    second derivatives of spline_second_derivatives; the last node of a periodic spline repeats the first"""
    y = np.asarray(values, dtype=np.float64)
    n = y.shape[-1]
    h = (float(hi) - float(lo)) / (n - 1)
    flat = y.reshape(-1, n)
    M = np.array([spline_second_derivatives(row, lo, hi, periodic) for row in flat])
    d = np.empty_like(flat)
    d[:, :-1] = (flat[:, 1:] - flat[:, :-1]) / h - h * (2.0 * M[:, :-1] + M[:, 1:]) / 6.0
    d[:, -1] = d[:, 0] if periodic else (flat[:, -1] - flat[:, -2]) / h + h * (M[:, -2] + 2.0 * M[:, -1]) / 6.0
    return d.reshape(y.shape)


def table2d_nodes(nx, ny, values, xmin, xmax, ymin, ymax, periodic=False):
    """node [ny][nx][4] = (f, fx, fy, fxy) of a Continuous2DFunction (include/remd_hip_custom.h): fx the node derivatives of the 1D
    splines along x for every j, fy those along y for every i, fxy those of fx along y"""
    f = np.asarray(values, dtype=np.float64).reshape(ny, nx)
    fx = spline_node_derivatives(f, xmin, xmax, periodic)
    fy = spline_node_derivatives(f.T, ymin, ymax, periodic).T
    fxy = spline_node_derivatives(fx.T, ymin, ymax, periodic).T
    return np.stack([f, fx, fy, fxy], axis=-1)


def cmap_block(size, energy):
    """The block of one map of a system.CMAPTorsionForce: the periodic Continuous2DFunction layout [nx, ny, 0, 2 pi, 0, 2 pi, 1, 0],
    node [ny][nx][4] with nx = ny = size + 1 -- energy[i + size*j] at (2 pi i / size, 2 pi j / size), the first row and column repeated
    at the end, and the node derivatives of periodic cubic splines (table2d_nodes: OpenMM's calcMapDerivatives)."""
    size = int(size)
    grid = np.asarray(energy, dtype=np.float64).reshape(size, size)
    grid = np.concatenate([grid, grid[:1]], axis=0)
    grid = np.concatenate([grid, grid[:, :1]], axis=1)
    two_pi = 2.0 * np.pi
    nodes = table2d_nodes(size + 1, size + 1, grid.reshape(-1), 0.0, two_pi, 0.0, two_pi, periodic=True)
    return np.concatenate([[size + 1.0, size + 1.0, 0.0, two_pi, 0.0, two_pi, 1.0, 0.0], nodes.reshape(-1)])


def _cmap_entry(f, names, defaults, n_atoms):
    """the entry of a CMAPTorsionForce: atoms [n][8] and n_particles = 8, map_index int32 [n], map_offsets int32 [n_maps] into consts,
    which holds the maps' blocks (cmap_block) back to back; no program, no parameters; None for a force without torsions"""
    n_maps, n = f.getNumMaps(), f.getNumTorsions()
    if n and not n_maps:
        raise ValueError('CMAPTorsionForce: %d torsions but no map' % n)
    if n_maps > MAX_MAPS:
        raise NotImplementedError('CMAPTorsionForce: %d maps in one force (the engine takes %d)' % (n_maps, MAX_MAPS))
    if not n:
        return None
    terms = np.array([f.getTorsionParameters(k) for k in range(n)], dtype=np.int64).reshape(n, 9)
    for k, row in enumerate(terms):
        if not 0 <= row[0] < n_maps:
            raise ValueError('CMAPTorsionForce: torsion %d names map %d (the force has %d)' % (k, row[0], n_maps))
        for quad in (row[1:5], row[5:9]):
            if len(set(quad.tolist())) != 4:
                raise ValueError('CMAPTorsionForce: torsion %d names particle %d twice in one dihedral'
                                 % (k, [p for p in quad.tolist() if quad.tolist().count(p) > 1][0]))
        bad = [int(p) for p in row[1:] if p < 0 or (n_atoms is not None and p >= n_atoms)]
        if bad:
            raise ValueError('CMAPTorsionForce: torsion %d names particle %d (the System has %s)' % (k, bad[0], n_atoms))
    blocks, offsets = [], []
    for m in range(n_maps):
        size, energy = f.getMapParameters(m)
        if (size + 1) ** 2 > MAX_TABLE_CELLS:
            raise NotImplementedError('CMAPTorsionForce: map %d of size %d (the engine takes 2 ... 255)' % (m, size))
        offsets.append(sum(len(b) for b in blocks))
        blocks.append(cmap_block(size, energy))
    return dict(kind=KIND_CMAP, atoms=terms[:, 1:].astype(np.int32), params=np.zeros((n, 0)), global_names=list(names),
                global_defaults=np.array(defaults, dtype=np.float64), program=np.zeros((0, 2), dtype=np.int32), consts=np.concatenate(blocks),
                stack_depth=0, periodic=int(bool(f.usesPeriodicBoundaryConditions())), force_group=int(f.getForceGroup()),
                energy=CMAP_ENERGY_TEXT, n_particles=8, map_index=terms[:, 0].astype(np.int32), map_offsets=np.array(offsets, dtype=np.int32))


def _table_block(name, function, where):
    """(opcode, the function's block of the constant table): [n, min, max, periodic], y [n], y'' [n] of a Continuous1DFunction,
    [n], values [n] of a Discrete1DFunction, [nx, ny, xmin, xmax, ymin, ymax, periodic, 0], node [ny][nx][4] of a Continuous2DFunction,
    [nx, ny], values [ny][nx] of a Discrete2DFunction, [nx, ny, nz, 0], values [nz][ny][nx] of a Discrete3DFunction
    (include/remd_hip_custom.h)"""
    from . import system as _system
    if isinstance(function, (_system.Continuous2DFunction, _system.Discrete2DFunction, _system.Discrete3DFunction)):
        parameters = function.getFunctionParameters()
        dims = 3 if isinstance(function, _system.Discrete3DFunction) else 2
        sizes = parameters[:dims]
        if int(np.prod(sizes)) > MAX_TABLE_CELLS:
            raise NotImplementedError('%s: tabulated function %r has %d values (%s; the engine takes %d)'
                                      % (where, name, int(np.prod(sizes)), ' x '.join(str(n) for n in sizes), MAX_TABLE_CELLS))
        if isinstance(function, _system.Continuous2DFunction):
            periodic = bool(function.getPeriodic())
            nodes = table2d_nodes(*parameters, periodic=periodic)
            return TABLE2D, np.concatenate([[sizes[0], sizes[1]], parameters[3:], [float(periodic), 0.0], nodes.reshape(-1)])
        return (LOOKUP3D if dims == 3 else LOOKUP2D), np.concatenate([list(sizes) + [0.0] * (dims == 3), parameters[dims]])
    if isinstance(function, _system.Continuous1DFunction):
        values, lo, hi = function.getFunctionParameters()
        periodic = bool(function.getPeriodic())
        if len(values) > MAX_TABLE_POINTS:
            raise NotImplementedError('%s: tabulated function %r has %d points (the engine takes %d)' % (where, name, len(values), MAX_TABLE_POINTS))
        return TABLE1D, np.concatenate([[len(values), lo, hi, float(periodic)], values, spline_second_derivatives(values, lo, hi, periodic)])
    if isinstance(function, _system.Discrete1DFunction):
        values = function.getFunctionParameters()
        if len(values) > MAX_TABLE_POINTS:
            raise NotImplementedError('%s: tabulated function %r has %d points (the engine takes %d)' % (where, name, len(values), MAX_TABLE_POINTS))
        return LOOKUP1D, np.concatenate([[len(values)], values])
    raise NotImplementedError('%s: tabulated function %r (a %s: only Continuous1DFunction, Discrete1DFunction, Continuous2DFunction, '
                              'Discrete2DFunction and Discrete3DFunction are supported)'
                              % (where, name, type(function).__name__))


def compile_expression(energy, variables, parameters, global_columns, where='expression', tabulated=(), periodic_distance=False,
                       n_particles=0, particle_prefix='p', pair_parameters=(), particle_slots=None, set_parameters=None):
    """The postfix program of ``energy``.

    variables: the force's own variable names in operand order; parameters: the per-term parameter names in order; global_columns:
    {global parameter name: column of the handle's table}; tabulated: the force's (name, function) pairs: a call of a
    system.Continuous1DFunction compiles to TABLE1D, of a system.Discrete1DFunction to LOOKUP1D (of the 2D and 3D classes to TABLE2D,
    LOOKUP2D, LOOKUP3D, with two and three arguments), the operand the offset of the
    function's block in the constants (behind the scalar constants, one block per function called); periodic_distance:
    whether periodicdistance(...) is allowed (an external force that uses periodic boundary conditions); n_particles: the particles
    per bond of a compound-bond force (0: another force), which opens distance / angle / dihedral over p1 ... pP and pointdistance;
    particle_prefix: 'p', or 'g' for the groups g1 ... gP of a centroid-bond force (the messages then speak of groups);
    pair_parameters: the per-particle parameter names of a nonbonded force, in order: name p is legal as p1 (PARAM operand k) and p2
    (operand len(pair_parameters) + k) only; particle_slots: {particle name: slot} of a donor-acceptor force (HBOND_SLOTS), which opens
    distance / angle / dihedral over exactly those names and nothing else of the compound-bond forces; set_parameters: the bare
    per-particle parameter names of a many-particle force (None: another force; whose suffixed forms are in ``parameters``): named bare,
    they are refused by name, and so are the raw coordinates x1 y1 z1 ...

    Returns dict(program int32 [n][2], consts float64 [m], stack_depth), and particle_mask (bit s: slot s is named) with particle_slots.
    """
    body, definitions = split_definitions(energy, where)
    _PARTICLE_NAME, noun = _PARTICLE_NAMES[particle_prefix]
    other = {'p': 'g', 'g': 'p'}[particle_prefix]
    trees = {}
    program, consts, const_index = [], [], {}
    functions = dict(tabulated)                 # name -> function
    blocks, table_calls = {}, []                # name -> (opcode, block), in the order first called; (instruction, name) of every call
    depth = [0, 0]                              # current, maximum
    named_slots = set()                         # (particle_slots) the slots the expression names

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
            if pair_parameters:
                if name[-1:] in ('1', '2') and name[:-1] in pair_parameters:
                    return emit(PARAM, pair_parameters.index(name[:-1]) + (len(pair_parameters) if name[-1] == '2' else 0))
                if name in pair_parameters:
                    raise NotImplementedError('%s: per-particle parameter %r without a particle suffix (%s1 or %s2)' % (where, name, name, name))
                if name[-1:].isdigit() and name.rstrip('0123456789') in pair_parameters:
                    raise NotImplementedError('%s: per-particle parameter %r (a pair has the particles 1 and 2: %s1, %s2)'
                                              % (where, name, name.rstrip('0123456789'), name.rstrip('0123456789')))
                if name in ('x', 'y', 'z'):
                    raise NotImplementedError('%s: variable %r (the only variable of a nonbonded force is r)' % (where, name))
            if particle_slots is not None and name in particle_slots:
                raise NotImplementedError('%s: particle name %r outside distance(), angle() and dihedral()' % (where, name))
            if set_parameters is not None and re.fullmatch(r'[xyz][0-9]+', name):
                raise NotImplementedError('%s: variable %r (raw coordinates are not variables of this force: use distance(), angle() and dihedral())' % (where, name))
            if set_parameters is not None and name in set_parameters:
                raise NotImplementedError('%s: per-particle parameter %r without a particle suffix (%s1, %s2 or %s3)' % (where, name, name, name, name))
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
            if name in functions:
                if name not in blocks:
                    blocks[name] = _table_block(name, functions[name], where)
                n_args = POPS.get(blocks[name][0], 1)
                if len(args) != n_args:
                    raise NotImplementedError('%s: tabulated function %r takes %d argument%s, not %d'
                                              % (where, name, n_args, 's' if n_args > 1 else '', len(args)))
                for a in args:
                    walk(a, active)
                table_calls.append((len(program), name))
                return emit(blocks[name][0])
            if particle_slots is not None and name in PARTICLE_FUNCTIONS:
                op, n_args = PARTICLE_FUNCTIONS[name]
                if len(args) != n_args:
                    raise NotImplementedError('%s: function %r takes %d particles, not %d' % (where, name, n_args, len(args)))
                packed = 0
                for k, a in enumerate(args):
                    if a[0] != 'name' or a[1] not in particle_slots:
                        raise NotImplementedError('%s: the arguments of %r are particle names among %s%s' % (
                            where, name, ' '.join(particle_slots), ', not %r' % (a[1],) if a[0] == 'name' else ''))
                    named_slots.add(particle_slots[a[1]])
                    packed |= particle_slots[a[1]] << (4 * k)
                return emit(op, packed)
            if particle_slots is not None and name in ('pointdistance', 'pointangle', 'pointdihedral'):
                raise NotImplementedError('%s: function %r (pointdistance, pointangle and pointdihedral are not functions of this force)' % (where, name))
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
    # the tables' blocks behind the scalar constants (which deduplicate among themselves only); a call's operand is its block's offset
    offsets = {}
    for name, (_, block) in blocks.items():
        offsets[name] = len(consts)
        consts += block.tolist()
    for pc, name in table_calls:
        program[pc] = (program[pc][0], offsets[name])
    if len(program) > MAX_PROGRAM:
        raise NotImplementedError('%s: a program of %d instructions (the engine takes %d)' % (where, len(program), MAX_PROGRAM))
    if depth[1] > MAX_STACK:
        raise NotImplementedError('%s: an expression that needs %d stack slots (the engine has %d)' % (where, depth[1], MAX_STACK))
    out = dict(program=np.array(program, dtype=np.int32).reshape(-1, 2), consts=np.array(consts, dtype=np.float64),
               stack_depth=int(depth[1]))
    if particle_slots is not None:
        out['particle_mask'] = sum(1 << s for s in named_slots)
    return out


# ---- the forces of a System -------------------------------------------------------------------------------------------------------
def _per_term_names(force):
    return list(force._per_bond)


def is_custom_term_force(force):
    """Whether system_to_desc sends this force down the expression path: one of the four classes whose energy is neither the
    HarmonicOscillator string (ext_K / ext_x0 / ext_U0) nor one of the restraint forms (csrc/restraints.hip), or a
    CustomCompoundBondForce, or a system.CustomCentroidBondForce (forces.CustomCentroidBondForce, the restraints' base, is another class)."""
    from . import system as _system
    from . import forces as _forces
    if isinstance(force, (_system.CustomCompoundBondForce, _system.CustomCentroidBondForce, _system.CustomNonbondedForce,
                          _system.CustomCVForce, _system.RMSDForce, _system.CMAPTorsionForce, _system.CustomHbondForce,
                          _system.CustomManyParticleForce)):
        return True
    if isinstance(force, _system.CustomExternalForce):
        return not force.is_harmonic_oscillator()
    if isinstance(force, (_system.CustomAngleForce, _system.CustomTorsionForce)):
        return True
    if isinstance(force, _system.CustomBondForce):
        return not _forces.is_restraint_form(force)
    return False


def energy_text(force):
    """The energy string by which a message names a custom force; a bare RMSDForce has none of its own (OpenMM gives it no
    getEnergyFunction): it is named by the expression it acts as, 'v'; a CMAPTorsionForce has no expression at all and is named
    by CMAP_ENERGY_TEXT."""
    from . import system as _system
    if isinstance(force, _system.CMAPTorsionForce):
        return CMAP_ENERGY_TEXT
    return as_cv_force(force).getEnergyFunction()


CMAP_ENERGY_TEXT = 'map(dihedral(a1,a2,a3,a4), dihedral(b1,b2,b3,b4))'


def as_cv_force(force):
    """A bare system.RMSDForce as what it acts as in a System, CustomCVForce('v') with itself as v; every other force as it is."""
    from . import system as _system
    if not isinstance(force, _system.RMSDForce):
        return force
    cv = _system.CustomCVForce('v')
    cv.addCollectiveVariable('v', force)
    cv.setForceGroup(force.getForceGroup())
    return cv


def cv_variables(force, n_atoms):
    """The collective variables of a CustomCVForce in CSR form: (names, cv_offsets int32 [n + 1], cv_atoms int32, cv_reference float64
    [sum n][3]), each variable's reference rows centred on the centroid of its own particles in f64."""
    from . import system as _system
    n_cvs = force.getNumCollectiveVariables()
    if n_cvs == 0:
        raise ValueError('CustomCVForce (energy %r) has no collective variable' % (force.getEnergyFunction(),))
    if n_cvs > MAX_CVS:
        raise NotImplementedError('CustomCVForce (energy %r): %d collective variables (the engine takes 1 ... %d): %s'
                                  % (force.getEnergyFunction(), n_cvs, MAX_CVS, ', '.join(force.getCollectiveVariableName(i) for i in range(n_cvs))))
    global_names = [force.getGlobalParameterName(i) for i in range(force.getNumGlobalParameters())]
    names, offsets, atoms, reference = [], [0], [], []
    for i in range(n_cvs):
        name, v = force.getCollectiveVariableName(i), force.getCollectiveVariable(i)
        where = 'CustomCVForce: collective variable %r' % name
        if name in names:
            raise ValueError('%s is named twice' % where)
        if name in global_names:
            raise ValueError('%s is also a global parameter of the force' % where)
        if not isinstance(v, _system.RMSDForce):
            raise NotImplementedError('%s is a %s (only RMSDForce collective variables are supported)' % (where, type(v).__name__))
        ref = v.getReferencePositions()
        if n_atoms is not None and len(ref) != n_atoms:
            raise ValueError('%s: RMSDForce has %d reference positions, the System has %d particles' % (where, len(ref), n_atoms))
        particles = v.getParticles() or list(range(len(ref)))
        if len(particles) < 3:
            raise ValueError('%s: RMSDForce over %d particles (an RMSD after superposition needs at least 3)' % (where, len(particles)))
        if min(particles) < 0 or max(particles) >= len(ref):
            raise ValueError('%s: RMSDForce names particle %d (the System has %d)'
                             % (where, min(particles) if min(particles) < 0 else max(particles), len(ref)))
        if len(set(particles)) != len(particles):
            raise ValueError('%s: RMSDForce names particle %d twice' % (where, [p for p in particles if particles.count(p) > 1][0]))
        rows = ref[particles]
        if not np.all(np.isfinite(rows)):
            raise ValueError('%s: RMSDForce has a reference position that is not finite' % where)
        names.append(name)
        atoms += particles
        reference.append(rows - rows.mean(axis=0))
        offsets.append(len(atoms))
    return names, np.array(offsets, dtype=np.int32), np.array(atoms, dtype=np.int32), np.concatenate(reference).astype(np.float64)


def barostat_molecules(desc):
    """molecule number of every particle, as the engine's barostats move them (csrc/forces.hip: the components of the NonbondedForce's
    exceptions and of the constraints, each stretched to a contiguous range of indices, interleaved ones merged).  None where the
    System has no NonbondedForce (no table from it)."""
    n = int(desc['n_atoms'])
    if int(desc.get('nb_method', 0)) == 0:
        return None
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    def unite(a, b):
        a, b = find(int(a)), find(int(b))
        if a != b:
            parent[max(a, b)] = min(a, b)
    for i, j in np.asarray(desc['exception_atoms']).reshape(-1, 2):
        unite(i, j)
    for w in np.asarray(desc['settle_atoms']).reshape(-1, 3):
        unite(w[0], w[1]); unite(w[0], w[2])
    for c in np.asarray(desc['shake_atoms']).reshape(-1, 4):
        for k in range(1, 4):
            if c[k] >= 0:
                unite(c[0], c[k])
    hi = list(range(n))
    for i in range(n):
        r = find(i)
        hi[r] = max(hi[r], i)
    molecule = np.zeros(n, dtype=np.int64)
    i = m = 0
    while i < n:
        end, k = hi[find(i)], i
        while k <= end:
            end = max(end, hi[find(k)])
            k += 1
        molecule[i:end + 1] = m
        i, m = end + 1, m + 1
    return molecule


def check_cv_molecules(desc, terms):
    """RMSDForce takes no minimum images (OpenMM's rule) while the engine's barostats wrap molecule by molecule: on a periodic System a
    collective variable whose particles span more than one molecule is refused."""
    periodic = int(desc.get('nb_method', 0)) in (1, 2) or any(int(t.get('nb_method', 0)) == 2 for t in terms.values())
    if not periodic:
        return
    molecule = barostat_molecules(desc)
    for t in terms.values():
        if t['kind'] != KIND_CV:
            continue
        for k, name in enumerate(t['cv_names']):
            atoms = t['cv_atoms'][t['cv_offsets'][k]:t['cv_offsets'][k + 1]]
            if molecule is None:
                # (periodic through a CutoffPeriodic CustomNonbondedForce alone: the barostat's molecules then come from the table the
                # library builds from the custom bonds, csrc/custom_terms.hip, which the host does not rebuild)
                raise NotImplementedError('CustomCVForce (energy %r): collective variable %r in a periodic System without a NonbondedForce: the '
                                          'molecules a barostat wraps are then known to the library only, and RMSDForce takes no minimum images '
                                          '(imaging across molecules is not supported)' % (t['energy'], name))
            spans = len(set(molecule[atoms].tolist()))
            if spans > 1:
                raise NotImplementedError('CustomCVForce (energy %r): collective variable %r spans %d molecules of a periodic System: RMSDForce '
                                          'takes no minimum images and the barostat wraps molecule by molecule (imaging across molecules is not supported)'
                                          % (t['energy'], name, spans))


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


def table_values(consts, offset, x):
    """TABLE1D at every element of x: the spline of the block at ``offset`` (the formulas of the device, csrc/custom_machine.h); 0 outside
    [min, max] of a function that is not periodic, NaN for a NaN argument"""
    consts, x = np.asarray(consts, dtype=np.float64), np.asarray(x, dtype=np.float64)
    n, lo, hi, periodic = int(consts[offset]), consts[offset + 1], consts[offset + 2], consts[offset + 3] != 0.0
    y, y2 = consts[offset + 4:offset + 4 + n], consts[offset + 4 + n:offset + 4 + 2 * n]
    h = (hi - lo) / (n - 1)
    with np.errstate(all='ignore'):
        # (the wrap's rounding may leave t an ulp outside [min, max]: clamped; np.clip keeps a NaN)
        t = np.clip(x - (hi - lo) * np.floor((x - lo) / (hi - lo)), lo, hi) if periodic else x
        inside = (t >= lo) & (t <= hi)
        s = (np.where(inside, t, lo) - lo) / h
        i = np.clip(s.astype(np.int64), 0, n - 2)
        b = s - i                               # (t - x_i) / h, and a = (x_{i+1} - t) / h taken as 1 - b: a + b is exactly 1
        a = 1.0 - b
        v = a * y[i] + b * y[i + 1] + ((a * a * a - a) * y2[i] + (b * b * b - b) * y2[i + 1]) * (h * h / 6.0)
    return np.where(inside, v, np.where(np.isnan(t), np.nan, 0.0))


def lookup_values(consts, offset, x):
    """LOOKUP1D at every element of x: values[round(x)], halves away from zero; NaN where the index is outside 0 ... n - 1"""
    consts, x = np.asarray(consts, dtype=np.float64), np.asarray(x, dtype=np.float64)
    n = int(consts[offset])
    with np.errstate(all='ignore'):
        whole = np.trunc(x)
        k = whole + np.where(np.abs(x - whole) >= 0.5, np.sign(x), 0.0)
        inside = (k >= 0.0) & (k <= n - 1.0)
        v = consts[offset + 1 + np.where(inside, k, 0.0).astype(np.int64)]
    return np.where(inside, v, np.nan)


def _round_half_away(x):
    whole = np.trunc(x)
    return whole + np.where(np.abs(x - whole) >= 0.5, np.sign(x), 0.0)


def _axis(n, lo, hi, periodic, x):
    """(inside, patch index, offset in the patch, is NaN) of one argument of TABLE2D, the device's cst_table_axis"""
    h = (hi - lo) / (n - 1)
    t = np.clip(x - (hi - lo) * np.floor((x - lo) / (hi - lo)), lo, hi) if periodic else x
    inside = (t >= lo) & (t <= hi)
    s = (np.where(inside, t, lo) - lo) / h
    i = np.clip(s.astype(np.int64), 0, n - 2)
    return inside, i, s - i, np.isnan(t)


def table2d_values(consts, offset, x, y):
    """TABLE2D at every element of x, y: the sixteen-term bicubic Hermite sum over the patch's corners (include/remd_hip_custom.h); 0
    where either argument of a function that is not periodic lies outside its range, NaN for a NaN argument"""
    consts = np.asarray(consts, dtype=np.float64)
    x, y = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
    nx, ny = int(consts[offset]), int(consts[offset + 1])
    xmin, xmax, ymin, ymax = consts[offset + 2:offset + 6]
    periodic = consts[offset + 6] != 0.0
    node = consts[offset + 8:offset + 8 + 4 * nx * ny].reshape(ny, nx, 4)
    hx, hy = (xmax - xmin) / (nx - 1), (ymax - ymin) / (ny - 1)
    with np.errstate(all='ignore'):
        inx, i, u, nanx = _axis(nx, xmin, xmax, periodic, x)
        iny, j, w, nany = _axis(ny, ymin, ymax, periodic, y)

        def basis(t):                           # [h0a][a], [h1a][a]
            return ((2.0 * t ** 3 - 3.0 * t ** 2 + 1.0, 3.0 * t ** 2 - 2.0 * t ** 3), (t ** 3 - 2.0 * t ** 2 + t, t ** 3 - t ** 2))
        bu, bw = basis(u), basis(w)
        v = np.zeros(x.shape)
        for a in (0, 1):
            for b in (0, 1):
                c = node[j + b, i + a]
                v = v + (bu[0][a] * bw[0][b] * c[..., 0] + hx * bu[1][a] * bw[0][b] * c[..., 1] + hy * bu[0][a] * bw[1][b] * c[..., 2]
                         + hx * hy * bu[1][a] * bw[1][b] * c[..., 3])
    return np.where(nanx | nany, np.nan, np.where(inx & iny, v, 0.0))


def lookup_grid_values(consts, offset, *args):
    """LOOKUP2D (two arguments) / LOOKUP3D (three) at every element: values[round(x) + nx round(y) (+ nx ny round(z))], halves away
    from zero; NaN where an index is outside its range"""
    consts = np.asarray(consts, dtype=np.float64)
    dims = len(args)
    args = np.broadcast_arrays(*[np.asarray(a, dtype=np.float64) for a in args])
    sizes = [int(consts[offset + k]) for k in range(dims)]
    with np.errstate(all='ignore'):
        inside, flat, stride = np.ones(args[0].shape, dtype=bool), np.zeros(args[0].shape, dtype=np.int64), 1
        for n, a in zip(sizes, args):
            k = _round_half_away(a)
            ok = (k >= 0.0) & (k <= n - 1.0)
            inside &= ok
            flat = flat + stride * np.where(ok, k, 0.0).astype(np.int64)
            stride *= n
        v = consts[offset + (4 if dims == 3 else 2) + flat]
    return np.where(inside, v, np.nan)


def run_values(prog, r, params, global_values):
    """The value of a compiled one-variable program at every element of the array ``r`` (f64): the Python interpreter of the machine,
    values only (no partials), numpy-vectorised over r.  params: the PARAM operands' values; global_values: the GLOBAL columns'."""
    from math import erf, erfc
    r = np.asarray(r, dtype=np.float64)
    one = np.ones_like(r)
    verf, verfc = np.vectorize(erf, otypes=[float]), np.vectorize(erfc, otypes=[float])
    unary = {NEG: np.negative, SQRT: np.sqrt, EXP: np.exp, LOG: np.log, SIN: np.sin, COS: np.cos, TAN: np.tan, ASIN: np.arcsin,
             ACOS: np.arccos, ATAN: np.arctan, SINH: np.sinh, COSH: np.cosh, TANH: np.tanh, ERF: verf, ERFC: verfc, ABS: np.abs,
             STEP: lambda x: (x >= 0.0) * 1.0, DELTA: lambda x: (x == 0.0) * 1.0, FLOOR: np.floor, CEIL: np.ceil}
    binary = {ADD: np.add, SUB: np.subtract, MUL: np.multiply, DIV: np.divide, POW: np.power, ATAN2: np.arctan2, MIN: np.minimum,
              MAX: np.maximum}
    stack = []
    with np.errstate(all='ignore'):
        for op, arg in np.asarray(prog['program']).reshape(-1, 2).tolist():
            if op == CONST:
                stack.append(prog['consts'][arg] * one)
            elif op == VAR:
                if arg != 0:
                    raise NotImplementedError('run_values: a program of one variable')
                stack.append(r.copy())
            elif op == PARAM:
                stack.append(float(params[arg]) * one)
            elif op == GLOBAL:
                stack.append(float(global_values[arg]) * one)
            elif op in binary:
                y, x = stack.pop(), stack.pop()
                stack.append(binary[op](x, y))
            elif op == SELECT:
                z, y, x = stack.pop(), stack.pop(), stack.pop()
                stack.append(np.where(x != 0.0, y, z))
            elif op == POWI:
                x = stack.pop()
                v = one.copy()
                for _ in range(abs(arg)):
                    v = v * x
                stack.append(1.0 / v if arg < 0 else v)
            elif op in unary:
                stack.append(unary[op](stack.pop()))
            elif op == TABLE1D:
                stack.append(table_values(prog['consts'], arg, stack.pop()))
            elif op == LOOKUP1D:
                stack.append(lookup_values(prog['consts'], arg, stack.pop()))
            elif op == TABLE2D:
                y, x = stack.pop(), stack.pop()
                stack.append(table2d_values(prog['consts'], arg, x, y))
            elif op == LOOKUP2D:
                y, x = stack.pop(), stack.pop()
                stack.append(lookup_grid_values(prog['consts'], arg, x, y))
            elif op == LOOKUP3D:
                z, y, x = stack.pop(), stack.pop(), stack.pop()
                stack.append(lookup_grid_values(prog['consts'], arg, x, y, z))
            else:
                raise NotImplementedError('run_values: opcode %d' % op)
    assert len(stack) == 1
    return stack[0]


def _refined_quadrature(f, a, b, what):
    """Gauss-Legendre of f over (a, b), the order doubled until two successive refinements agree to 1e-12 relative."""
    previous = None
    for n in (16, 32, 64, 128, 256, 512, 1024):
        x, w = np.polynomial.legendre.leggauss(n)
        value = 0.5 * (b - a) * float(np.dot(w, f(0.5 * (b - a) * x + 0.5 * (b + a))))
        if not np.isfinite(value):
            break
        if previous is not None and abs(value - previous) <= 1e-12 * max(abs(value), abs(previous)):
            return value
        previous = value
    raise ValueError('%s does not converge (the energy must fall off faster than 1 / r^3)' % what)


class LongRangeCorrection:
    """The long-range correction of one nonbonded force (OpenMM's CustomNonbondedForceImpl::calcLongRangeCorrection, the convention
    alchemy.alchemical_long_range_constants restates): coefficient(g) = 2 pi N^2 sum_pairs-of-classes count I / (N (N + 1) / 2), the
    energy coefficient / V.  I = int_rc^inf E r^2 dr, plus int_rs^rc (1 - S) E r^2 dr with a switch, E the compiled program under
    the class pair's parameters and the globals g; count = n_a (n_a + 1) / 2 within a class, n_a n_b across classes.  The outer
    integral is taken in x = rc / r over (0, 1], where a Lennard-Jones tail is a polynomial and Gauss-Legendre exact.  Integrals are
    cached by (class pair, globals row)."""

    def __init__(self, term):
        self.term = term
        self.n = len(term['params'])
        n_params = int(np.asarray(term['params']).size // max(self.n, 1))
        params = np.asarray(term['params'], dtype=np.float64).reshape(self.n, n_params)
        classes = {}
        for row in params:
            classes[tuple(row.tolist())] = classes.get(tuple(row.tolist()), 0) + 1
        self.classes = sorted(classes.items())
        self.rc, self.rs = float(term['cutoff']), float(term['switch_distance'])
        self._cache = {}

    def _integral(self, pa, pb, g):
        key = (pa, pb, tuple(g))
        if key in self._cache:
            return self._cache[key]
        prog, rc, rs, par = self.term, self.rc, self.rs, list(pa) + list(pb)
        where = 'CustomNonbondedForce (energy %r): the long-range correction' % (self.term.get('energy'),)

        def tail(x):                            # r = rc / x: E r^2 dr = rc^3 E(rc / x) x^-4 dx
            return rc ** 3 * run_values(prog, rc / x, par, g) / x ** 4
        value = _refined_quadrature(tail, 0.0, 1.0, where)
        if rs >= 0.0:
            def switched(r):
                t = (r - rs) / (rc - rs)
                return (10.0 * t ** 3 - 15.0 * t ** 4 + 6.0 * t ** 5) * run_values(prog, r, par, g) * r * r
            value += _refined_quadrature(switched, rs, rc, where)
        self._cache[key] = value
        return value

    def coefficient(self, g):
        """kJ/mol nm^3 under the globals row g (the handle's columns)"""
        g = [float(v) for v in g]
        total = 0.0
        for a, (pa, na) in enumerate(self.classes):
            for pb, nb in self.classes[a:]:
                total += (na * (na + 1) // 2 if pa == pb else na * nb) * self._integral(pa, pb, g)
        return 2.0 * np.pi * self.n * self.n * total / (self.n * (self.n + 1) / 2.0)


def long_range_coefficients(terms, global_values, cache=None):
    """[K][n_forces]: the long-range coefficient of every state (row of global_values [K][n_globals]) and custom force of ``terms``
    (the list of custom_terms_desc's entries); zero for a force without the correction.  cache: a dict that keeps the integrators
    between calls, keyed by position; an entry made for another term (another dict object) is replaced, not reused."""
    global_values = np.asarray(global_values, dtype=np.float64)
    if global_values.ndim != 2:
        raise ValueError('long_range_coefficients: global_values is [K][n_globals]')
    out = np.zeros((len(global_values), len(terms)))
    cache = {} if cache is None else cache
    for i, t in enumerate(terms):
        if not t.get('long_range_correction'):
            continue
        if i not in cache or cache[i].term is not t:
            cache[i] = LongRangeCorrection(t)
        lrc = cache[i]
        for k, g in enumerate(global_values):
            out[k, i] = lrc.coefficient(g)
    return out


def nonbonded_exclusions(force, n):
    """The exclusions of a nonbonded force in CSR form: (excl_offsets int32 [n + 1], excl_atoms int32), symmetric, each row sorted."""
    rows = [set() for _ in range(n)]
    for k in range(force.getNumExclusions()):
        i, j = force.getExclusionParticles(k)
        if not (0 <= i < n and 0 <= j < n):
            raise ValueError('CustomNonbondedForce: exclusion %d names particle %d (the force has %d)' % (k, i if not 0 <= i < n else j, n))
        if i == j:
            raise ValueError('CustomNonbondedForce: exclusion %d excludes particle %d from itself' % (k, i))
        if j in rows[i]:
            raise ValueError('CustomNonbondedForce: particles %d and %d are excluded twice' % (i, j))
        rows[i].add(j); rows[j].add(i)
    offsets = np.zeros(n + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([len(r) for r in rows])
    atoms = np.array([j for r in rows for j in sorted(r)], dtype=np.int32)
    return offsets, atoms


def custom_terms_desc(forces, masses=None, box_vectors=None):
    """The 'custom_terms' entry of system.system_to_desc for the custom forces ``forces`` (in System order): a dict keyed by position
    ('000', '001', ...), each value dict(kind, atoms [n][1..4] ([n][P] and n_particles = P of a compound-bond force; of a centroid-bond force atoms holds
    group numbers and group_offsets, group_atoms, group_weights describe the groups, centroid_groups(force, masses)), params [n][p], global_names, global_defaults, program, consts,
    stack_depth, periodic, force_group, energy).  The global names and defaults are the handle's columns, the same in every entry: a
    global two forces share is one column."""
    forces = [as_cv_force(f) for f in forces]
    if len(forces) > MAX_FORCES:
        raise NotImplementedError('%d custom forces in one System (the engine takes %d)' % (len(forces), MAX_FORCES))
    from . import system as _system
    names, defaults = [], []
    for f in forces:
        if isinstance(f, (_system.CMAPTorsionForce, _system.CustomGBForce)):    # (no globals of its own; a CustomGBForce's are folded into its constants)
            continue
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
    # energy parameter derivatives (addEnergyParameterDerivative): the distinct global columns in the order of their first declaration
    # over the forces, and per force the mask of those it declared (bit d: derivative_columns[d]) -- a force contributes to a
    # parameter's derivative only where it declared it, even when another force's expression names the same global (OpenMM's rule)
    derivative_names = []
    for f in forces:
        for name in getattr(f, '_derivatives', ()):
            if name not in derivative_names:
                derivative_names.append(name)
    derivative_columns = np.array([columns[n] for n in derivative_names], dtype=np.int32)

    def finish(entry, f):
        """the derivative keys of an emitted entry: the System's list (the same in every entry) and this force's mask"""
        entry.update(derivative_names=list(derivative_names), derivative_columns=derivative_columns.copy(),
                     derivative_mask=sum(1 << derivative_names.index(n) for n in getattr(f, '_derivatives', ())))
        return entry
    out = {}
    for k, f in enumerate(forces):
        if isinstance(f, _system.CustomGBForce):                            # the general path of a CustomGBForce (custom_gb.py; csrc/custom_gb.hip)
            from .custom_gb import compile_custom_gb
            out['%03d' % len(out)] = finish(compile_custom_gb(f, None if masses is None else len(masses), box_vectors, names, defaults), f)
            continue
        cls = [c for c in KIND_OF_CLASS if c in [b.__name__ for b in type(f).__mro__]][0]
        kind = KIND_OF_CLASS[cls]
        if kind == KIND_CMAP:
            entry = _cmap_entry(f, names, defaults, None if masses is None else len(masses))
            if entry is not None:
                out['%03d' % len(out)] = finish(entry, f)
            continue
        where = '%s (energy %r)' % (cls, f.getEnergyFunction())
        if kind == KIND_HBOND:
            entry = _hbond_entry(f, cls, where, names, defaults, columns, masses, box_vectors)
            if entry is not None:
                out['%03d' % len(out)] = finish(entry, f)
            continue
        if kind == KIND_MANYPARTICLE:
            out['%03d' % len(out)] = finish(_manyparticle_entry(f, cls, where, names, defaults, columns, masses, box_vectors), f)
            continue
        per_term = _per_term_names(f)
        if kind == KIND_NONBONDED and len(per_term) > MAX_PAIR_PARAMS:
            raise NotImplementedError('%s: %d per-particle parameters (the engine takes %d): %s' % (cls, len(per_term), MAX_PAIR_PARAMS, ', '.join(per_term)))
        if len(per_term) > MAX_PARAMS:
            raise NotImplementedError('%s: %d per-term parameters (the engine takes %d): %s' % (cls, len(per_term), MAX_PARAMS, ', '.join(per_term)))
        tabulated = [(f.getTabulatedFunctionName(i), f.getTabulatedFunction(i)) for i in range(f.getNumTabulatedFunctions())]
        own = {n: columns[n] for n in (f.getGlobalParameterName(i) for i in range(f.getNumGlobalParameters()))}
        periodic = bool(f.usesPeriodicBoundaryConditions())
        n_particles = 0
        if kind == KIND_CV:
            cv = cv_variables(f, None if masses is None else len(masses))
            if per_term:
                raise ValueError('%s: a CustomCVForce has no per-term parameters (%s)' % (cls, ', '.join(per_term)))
        if kind == KIND_COMPOUND:
            n_particles = int(f.getNumParticlesPerBond())
            if not 1 <= n_particles <= MAX_PARTICLES:
                raise NotImplementedError('%s: bonds of %d particles (the engine takes 1 ... %d)' % (cls, n_particles, MAX_PARTICLES))
        if kind == KIND_CENTROID:
            n_particles = int(f.getNumGroupsPerBond())
            if not 1 <= n_particles <= MAX_PARTICLES:
                raise NotImplementedError('%s: bonds of %d groups (the engine takes 1 ... %d)' % (cls, n_particles, MAX_PARTICLES))
        prog = compile_expression(f.getEnergyFunction(), compound_variables(n_particles) if n_particles else tuple(cv[0]) if kind == KIND_CV else VARIABLES[kind],
                                  () if kind == KIND_NONBONDED else per_term, own,
                                  where=where, tabulated=tabulated, periodic_distance=(kind == KIND_EXTERNAL and periodic),
                                  n_particles=n_particles, particle_prefix='g' if kind == KIND_CENTROID else 'p',
                                  pair_parameters=tuple(per_term) if kind == KIND_NONBONDED else ())
        if kind == KIND_NONBONDED and f.getUseLongRangeCorrection() and np.isin(prog['program'][:, 0], (TABLE1D, LOOKUP1D, TABLE2D, LOOKUP2D, LOOKUP3D)).any():
            # (the tail quadrature assumes a smooth integrand; a spline that ends inside the tail is not one)
            raise NotImplementedError('%s: the long-range correction of an expression that calls a tabulated function (%s)'
                                      % (where, ', '.join(repr(n) for n, _ in tabulated)))
        if kind == KIND_NONBONDED:
            out['%03d' % len(out)] = finish(_nonbonded_entry(f, cls, prog, names, defaults, per_term, masses, box_vectors), f)
            continue
        if kind == KIND_CV:
            # one term without atoms or parameters of its own: the variables are the RMSDs (VAR 0 ... 2, CustomExternalForce's operands)
            out['%03d' % len(out)] = finish(dict(kind=kind, atoms=np.zeros((1, 0), dtype=np.int32), params=np.zeros((1, 0)), global_names=list(names),
                                                 global_defaults=np.array(defaults, dtype=np.float64), program=prog['program'], consts=prog['consts'],
                                                 stack_depth=prog['stack_depth'], periodic=0, force_group=int(f.getForceGroup()),
                                                 energy=f.getEnergyFunction(), cv_names=list(cv[0]), cv_offsets=cv[1], cv_atoms=cv[2], cv_reference=cv[3]), f)
            continue
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
        finish(out['%03d' % (len(out) - 1)], f)
    return out


def _nonbonded_entry(f, cls, prog, names, defaults, per_term, masses, box_vectors):
    """the entry of a nonbonded force: atoms is empty ([0][0]; the terms are the particles, n_terms = N), params [N][n_params],
    nb_method, cutoff, switch_distance (< 0: none), excl_offsets / excl_atoms and long_range_correction beside the common keys"""
    n = f.getNumParticles()
    if masses is not None and n != len(masses):
        raise ValueError('%s has %d particles, the System has %d' % (cls, n, len(masses)))
    if n == 0:
        raise ValueError('%s has no particles' % cls)
    for k in range(n):
        if len(f.getParticleParameters(k)) != len(per_term):
            raise ValueError('%s: particle %d carries %d parameters, the force declares %d' % (cls, k, len(f.getParticleParameters(k)), len(per_term)))
    method = int(f.getNonbondedMethod())
    cutoff = float(f.getCutoffDistance()) if method else 0.0
    switch = float(f.getSwitchingDistance()) if (method and f.getUseSwitchingFunction()) else -1.0
    if method and not cutoff > 0.0:
        raise ValueError('%s: cutoff distance %r' % (cls, cutoff))
    if switch >= 0.0 and not 0.0 < switch < cutoff:
        raise ValueError('%s: the switching distance %r must lie between 0 and the cutoff %r' % (cls, switch, cutoff))
    if method == 2:
        if box_vectors is None:
            raise ValueError('%s: CutoffPeriodic needs the periodic box vectors of the System' % cls)
        box = np.asarray(box_vectors, dtype=np.float64).reshape(3, 3)
        if np.any(box != np.diag(np.diag(box))):
            raise NotImplementedError('%s: triclinic boxes are not supported (CutoffPeriodic takes a rectangular box)' % cls)
        if cutoff > 0.5 * np.diag(box).min():
            raise ValueError('%s: the cutoff %r nm exceeds half the smallest box edge (%r nm)' % (cls, cutoff, np.diag(box).min()))
    offsets, atoms = nonbonded_exclusions(f, n)
    params = np.array([f.getParticleParameters(k) for k in range(n)], dtype=np.float64).reshape(n, len(per_term))
    return dict(kind=KIND_NONBONDED, atoms=np.zeros((0, 0), dtype=np.int32), params=params, global_names=list(names),
                global_defaults=np.array(defaults, dtype=np.float64), program=prog['program'], consts=prog['consts'],
                stack_depth=prog['stack_depth'], periodic=int(method == 2), force_group=int(f.getForceGroup()),
                energy=f.getEnergyFunction(), nb_method=method, cutoff=cutoff, switch_distance=switch, excl_offsets=offsets,
                excl_atoms=atoms, long_range_correction=int(bool(f.getUseLongRangeCorrection()) and method == 2))


def hbond_exclusions(force, n_donors, n_acceptors):
    """The exclusions of a donor-acceptor force in CSR form: (offsets int32 [n_donors + 1], acceptors int32), each row sorted."""
    rows = [set() for _ in range(n_donors)]
    for k in range(force.getNumExclusions()):
        i, j = force.getExclusionParticles(k)
        if not 0 <= i < n_donors:
            raise ValueError('CustomHbondForce: exclusion %d names donor %d (the force has %d)' % (k, i, n_donors))
        if not 0 <= j < n_acceptors:
            raise ValueError('CustomHbondForce: exclusion %d names acceptor %d (the force has %d)' % (k, j, n_acceptors))
        if j in rows[i]:
            raise ValueError('CustomHbondForce: donor %d and acceptor %d are excluded twice' % (i, j))
        rows[i].add(j)
    offsets = np.zeros(n_donors + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([len(r) for r in rows])
    return offsets, np.array([j for r in rows for j in sorted(r)], dtype=np.int32), rows


def _hbond_entry(f, cls, where, names, defaults, columns, masses, box_vectors):
    """the entry of a donor-acceptor force, or None for an empty one: atoms is empty, params [0][0]; donor_atoms [nD][3] and
    acceptor_atoms [nA][3] (-1: unused), donor_params, acceptor_params, hb_excl_offsets / hb_excl_acceptors, nb_method, cutoff and
    particle_mask beside the common keys"""
    per_donor = [f.getPerDonorParameterName(i) for i in range(f.getNumPerDonorParameters())]
    per_acceptor = [f.getPerAcceptorParameterName(i) for i in range(f.getNumPerAcceptorParameters())]
    if len(per_donor) + len(per_acceptor) > MAX_PARAMS:
        raise NotImplementedError('%s: %d per-donor and %d per-acceptor parameters (the engine takes %d together): %s'
                                  % (cls, len(per_donor), len(per_acceptor), MAX_PARAMS, ', '.join(per_donor + per_acceptor)))
    twice = [n for n in per_acceptor if n in per_donor]
    if twice:
        raise ValueError('%s: %r is both a per-donor and a per-acceptor parameter' % (cls, twice[0]))
    tabulated = [(f.getTabulatedFunctionName(i), f.getTabulatedFunction(i)) for i in range(f.getNumTabulatedFunctions())]
    own = {n: columns[n] for n in (f.getGlobalParameterName(i) for i in range(f.getNumGlobalParameters()))}
    prog = compile_expression(f.getEnergyFunction(), (), per_donor + per_acceptor, own, where=where, tabulated=tabulated, particle_slots=HBOND_SLOTS)
    mask = prog['particle_mask']
    n_atoms = None if masses is None else len(masses)
    nD, nA = f.getNumDonors(), f.getNumAcceptors()
    if nD == 0 and nA == 0:
        return None
    if nD == 0 or nA == 0:
        trivial = len(prog['program']) == 1 and prog['program'][0, 0] == CONST and prog['consts'][prog['program'][0, 1]] == 0.0
        if trivial:
            return None
        raise ValueError('%s has %d donors and %d acceptors: a force with %s has no pair to act on'
                         % (where, nD, nA, 'donors but no acceptors' if nA == 0 else 'acceptors but no donors'))
    sides = []
    for side, count, get, n_par, first_slot in (('donor', nD, f.getDonorParameters, len(per_donor), 0), ('acceptor', nA, f.getAcceptorParameters, len(per_acceptor), 3)):
        atoms, params = np.empty((count, 3), dtype=np.int32), np.empty((count, n_par), dtype=np.float64)
        for k in range(count):
            row = get(k)
            p, values = [int(a) for a in row[:3]], list(row[3])
            if len(values) != n_par:
                raise ValueError('%s: %s %d carries %d parameters, the force declares %d' % (cls, side, k, len(values), n_par))
            if p[0] == -1:
                raise ValueError('%s: %s %d has no first particle (%s1 = -1)' % (cls, side, k, side[0]))
            for q, a in enumerate(p):
                if a < -1 or (n_atoms is not None and a >= n_atoms):
                    raise ValueError('%s: %s %d names particle %d (the System has %s)' % (cls, side, k, a, n_atoms))
                if a >= 0 and a in p[:q]:
                    raise ValueError('%s: %s %d names particle %d twice' % (cls, side, k, a))
                if a == -1 and (mask >> (first_slot + q)) & 1:
                    raise ValueError('%s: the expression names %s%d, which %s %d does not have (-1)' % (where, side[0], q + 1, side, k))
            atoms[k], params[k] = p, values
        sides.append((atoms, params))
    (d_atoms, d_params), (a_atoms, a_params) = sides
    offsets, excluded, rows = hbond_exclusions(f, nD, nA)
    # a pair that shares a particle has no geometry of its own: OpenMM leaves it to the user to exclude it
    of_atom = {}
    for j in range(nA):
        for a in a_atoms[j]:
            if a >= 0:
                of_atom.setdefault(int(a), []).append(j)
    for i in range(nD):
        for a in d_atoms[i]:
            for j in of_atom.get(int(a), ()) if a >= 0 else ():
                if j not in rows[i]:
                    raise ValueError('%s: donor %d and acceptor %d share particle %d and are not excluded: add the exclusion (addExclusion(%d, %d))'
                                     % (cls, i, j, a, i, j))
    method = int(f.getNonbondedMethod())
    cutoff = float(f.getCutoffDistance()) if method else 0.0
    if method and not cutoff > 0.0:
        raise ValueError('%s: cutoff distance %r' % (cls, cutoff))
    if method == 2:
        if box_vectors is None:
            raise ValueError('%s: CutoffPeriodic needs the periodic box vectors of the System' % cls)
        box = np.asarray(box_vectors, dtype=np.float64).reshape(3, 3)
        if np.any(box != np.diag(np.diag(box))):
            raise NotImplementedError('%s: triclinic boxes are not supported (CutoffPeriodic takes a rectangular box)' % cls)
        if cutoff > 0.5 * np.diag(box).min():
            raise ValueError('%s: the cutoff %r nm exceeds half the smallest box edge (%r nm)' % (cls, cutoff, float(np.diag(box).min())))
    return dict(kind=KIND_HBOND, atoms=np.zeros((0, 0), dtype=np.int32), params=np.zeros((0, 0)), global_names=list(names),
                global_defaults=np.array(defaults, dtype=np.float64), program=prog['program'], consts=prog['consts'],
                stack_depth=prog['stack_depth'], periodic=int(method == 2), force_group=int(f.getForceGroup()),
                energy=f.getEnergyFunction(), nb_method=method, cutoff=cutoff, donor_atoms=d_atoms, acceptor_atoms=a_atoms,
                donor_params=d_params, acceptor_params=a_params, hb_excl_offsets=offsets, hb_excl_acceptors=excluded,
                particle_mask=int(mask))


def manyparticle_exclusions(force, n):
    """The exclusions of a many-particle force in CSR form: (excl_offsets int32 [n + 1], excl_atoms int32), symmetric, each row sorted."""
    rows = [set() for _ in range(n)]
    for k in range(force.getNumExclusions()):
        i, j = force.getExclusionParticles(k)
        if not (0 <= i < n and 0 <= j < n):
            raise ValueError('CustomManyParticleForce: exclusion %d names particle %d (the force has %d)' % (k, i if not 0 <= i < n else j, n))
        if i == j:
            raise ValueError('CustomManyParticleForce: exclusion %d excludes particle %d from itself' % (k, i))
        if j in rows[i]:
            raise ValueError('CustomManyParticleForce: particles %d and %d are excluded twice' % (i, j))
        rows[i].add(j); rows[j].add(i)
    offsets = np.zeros(n + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([len(r) for r in rows])
    return offsets, np.array([j for r in rows for j in sorted(r)], dtype=np.int32)


def _manyparticle_entry(f, cls, where, names, defaults, columns, masses, box_vectors):
    """the entry of a many-particle force: atoms is empty ([0][0]; the terms are the particles, n_terms = N), params [N][n_params],
    nb_method, cutoff, excl_offsets / excl_atoms, permutation_mode, types [N], filters [3] (bit t: type t may fill the slot; all
    ones: no filter) and particle_mask beside the common keys"""
    if int(f.getNumParticlesPerSet()) != 3:
        raise NotImplementedError('%s: sets of %d particles (sets of 3 particles are supported)' % (cls, int(f.getNumParticlesPerSet())))
    per_particle = [f.getPerParticleParameterName(i) for i in range(f.getNumPerParticleParameters())]
    if len(per_particle) > MAX_SET_PARAMS:
        raise NotImplementedError('%s: %d per-particle parameters (the engine takes %d: three columns each of its %d): %s'
                                  % (cls, len(per_particle), MAX_SET_PARAMS, MAX_PARAMS, ', '.join(per_particle)))
    n = f.getNumParticles()
    if masses is not None and n != len(masses):
        raise ValueError('%s has %d particles, the System has %d' % (cls, n, len(masses)))
    if n == 0:
        raise ValueError('%s has no particles' % cls)
    tabulated = [(f.getTabulatedFunctionName(i), f.getTabulatedFunction(i)) for i in range(f.getNumTabulatedFunctions())]
    own = {g: columns[g] for g in (f.getGlobalParameterName(i) for i in range(f.getNumGlobalParameters()))}
    operands = ['%s%d' % (q, s + 1) for q in per_particle for s in range(3)]          # operand 3 q + s: parameter q of slot s
    prog = compile_expression(f.getEnergyFunction(), (), operands, own, where=where, tabulated=tabulated, particle_slots=MANYPARTICLE_SLOTS,
                              set_parameters=tuple(per_particle))
    params, types = np.empty((n, len(per_particle)), dtype=np.float64), np.empty(n, dtype=np.int32)
    for k in range(n):
        values, t = f.getParticleParameters(k)
        if len(values) != len(per_particle):
            raise ValueError('%s: particle %d carries %d parameters, the force declares %d' % (cls, k, len(values), len(per_particle)))
        if not 0 <= int(t) <= 31:
            raise ValueError('%s: particle %d has type %d (the types are 0 ... 31)' % (cls, k, int(t)))
        params[k], types[k] = values, int(t)
    filters = np.full(3, 0xFFFFFFFF, dtype=np.uint32)
    for s in range(3):
        allowed = list(f.getTypeFilter(s))
        for t in allowed:
            if not 0 <= int(t) <= 31:
                raise ValueError('%s: type filter %d names type %d (the types are 0 ... 31)' % (cls, s, int(t)))
        if allowed:
            filters[s] = sum(1 << int(t) for t in set(allowed))
    method = int(f.getNonbondedMethod())
    cutoff = float(f.getCutoffDistance()) if method else 0.0
    if method and not cutoff > 0.0:
        raise ValueError('%s: cutoff distance %r' % (cls, cutoff))
    if method == 0 and n > MP_MAX_NEIGHBORS + 1:
        raise NotImplementedError('%s: NoCutoff with %d particles (a neighbour row holds %d particles, so NoCutoff takes at most %d: use a cutoff)'
                                  % (cls, n, MP_MAX_NEIGHBORS, MP_MAX_NEIGHBORS + 1))
    if method == 2:
        if box_vectors is None:
            raise ValueError('%s: CutoffPeriodic needs the periodic box vectors of the System' % cls)
        box = np.asarray(box_vectors, dtype=np.float64).reshape(3, 3)
        if np.any(box != np.diag(np.diag(box))):
            raise NotImplementedError('%s: triclinic boxes are not supported (CutoffPeriodic takes a rectangular box)' % cls)
        if cutoff > 0.5 * np.diag(box).min():
            raise ValueError('%s: the cutoff %r nm exceeds half the smallest box edge (%r nm)' % (cls, cutoff, float(np.diag(box).min())))
    offsets, atoms = manyparticle_exclusions(f, n)
    return dict(kind=KIND_MANYPARTICLE, atoms=np.zeros((0, 0), dtype=np.int32), params=params, global_names=list(names),
                global_defaults=np.array(defaults, dtype=np.float64), program=prog['program'], consts=prog['consts'],
                stack_depth=prog['stack_depth'], periodic=int(method == 2), force_group=int(f.getForceGroup()),
                energy=f.getEnergyFunction(), nb_method=method, cutoff=cutoff, switch_distance=-1.0, excl_offsets=offsets, excl_atoms=atoms,
                long_range_correction=0, permutation_mode=int(f.getPermutationMode()), types=types, filters=filters,
                particle_mask=int(prog['particle_mask']))


def check_hbond_molecules(desc, terms):
    """The engine's barostats move and wrap molecule by molecule: under CutoffPeriodic the particles of one donor, and of one
    acceptor, must lie in one molecule (their differences are minimum images, so a wrapped molecule is fine, a split donor is not)."""
    molecule = None
    for t in terms.values():
        if t['kind'] != KIND_HBOND or int(t['nb_method']) != 2:
            continue
        if molecule is None:
            molecule = barostat_molecules(desc)
            if molecule is None:            # (no NonbondedForce: the library joins every donor's and acceptor's particles itself)
                return
        for side, key in (('donor', 'donor_atoms'), ('acceptor', 'acceptor_atoms')):
            for k, row in enumerate(np.asarray(t[key])):
                mols = {int(molecule[a]) for a in row if a >= 0}
                if len(mols) > 1:
                    raise NotImplementedError('CustomHbondForce (energy %r): %s %d (particles %s) spans %d molecules under CutoffPeriodic '
                                              '(the barostat moves molecules as wholes)' % (t['energy'], side, k, [int(a) for a in row if a >= 0], len(mols)))


def custom_globals(system, names, states):
    """[K][n]: the value of each global column at every state -- the state's GlobalParameterState where it carries the name, else the
    default value the forces carry."""
    defaults = {}
    for f in system.getForces():
        if is_custom_term_force(f) and hasattr(as_cv_force(f), 'getNumGlobalParameters'):   # (a CustomGBForce is none: its globals are constants)
            f = as_cv_force(f)
            for i in range(f.getNumGlobalParameters()):
                defaults.setdefault(f.getGlobalParameterName(i), float(f.getGlobalParameterDefaultValue(i)))
    out = np.empty((len(states), len(names)))
    for k, s in enumerate(states):
        for i, name in enumerate(names):
            v = s.global_parameter(name) if hasattr(s, 'global_parameter') else None
            out[k, i] = defaults[name] if v is None else float(v)
    return out
