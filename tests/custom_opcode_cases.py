"""Shared by tests/test_custom_dual_oracle_cpu.py and tests/test_custom_opcodes_gpu.py: the case table that runs every opcode of the
custom-force stack machine, and the Python interpreter of a compiled program (moved here from tests/test_custom_expr_cpu.py and
tests/test_custom_compound_cpu.py, which import it).

A row is one force of N_TERMS = 70 terms (a full wavefront, six lanes of a second one, 58 padding lanes).  ``u`` rows put the operand
``u = a*x + b*y*z + c`` (compound: ``a*x1 + b*y2*z3 + c``) of every lane at a different point of the row's interval, at BOTH replicas
(positions x and 0.9 x + 0.05, rounded to f32), and keep it 2e-3 away from the row's kinks; a, b differ per lane and from each other.
"""
import math

import numpy as np

import custom_expr_oracle as fd_oracle
from openmmtools_amd import custom_expr as cx

N_TERMS, N_ATOMS = 70, 200


# ---- the interpreter of a compiled program ----------------------------------------------------------------------------------------------
def _unary_table():
    return {cx.NEG: lambda a: (-a, -1.0), cx.SQRT: lambda a: (math.sqrt(a), 0.5 / math.sqrt(a)), cx.EXP: lambda a: (math.exp(a), math.exp(a)),
            cx.LOG: lambda a: (math.log(a), 1.0 / a), cx.SIN: lambda a: (math.sin(a), math.cos(a)), cx.COS: lambda a: (math.cos(a), -math.sin(a)),
            cx.TAN: lambda a: (math.tan(a), 1.0 + math.tan(a) ** 2), cx.ASIN: lambda a: (math.asin(a), 1.0 / math.sqrt(1.0 - a * a)),
            cx.ACOS: lambda a: (math.acos(a), -1.0 / math.sqrt(1.0 - a * a)), cx.ATAN: lambda a: (math.atan(a), 1.0 / (1.0 + a * a)),
            cx.SINH: lambda a: (math.sinh(a), math.cosh(a)), cx.COSH: lambda a: (math.cosh(a), math.sinh(a)),
            cx.TANH: lambda a: (math.tanh(a), 1.0 - math.tanh(a) ** 2),
            cx.ERF: lambda a: (math.erf(a), 2.0 / math.sqrt(math.pi) * math.exp(-a * a)),
            cx.ERFC: lambda a: (math.erfc(a), -2.0 / math.sqrt(math.pi) * math.exp(-a * a)),
            cx.ABS: lambda a: (abs(a), -1.0 if a < 0 else 1.0), cx.STEP: lambda a: (1.0 if a >= 0 else 0.0, 0.0),
            cx.DELTA: lambda a: (1.0 if a == 0 else 0.0, 0.0), cx.FLOOR: lambda a: (float(math.floor(a)), 0.0),
            cx.CEIL: lambda a: (float(math.ceil(a)), 0.0)}


def particles_op(op, arg, x, seed):
    """value and gradient with respect to particle `seed` of distance / angle / dihedral over the slots packed in `arg` (the formulas
    of the bonded kernels: bond, angle, dihedral in the sign convention of PeriodicTorsionForce)"""
    s = [(arg >> (4 * k)) & 15 for k in range(op - cx.DISTANCE + 2)]
    g = np.zeros((len(s), 3))
    if op == cx.DISTANCE:
        d = x[s[1]] - x[s[0]]
        v = np.linalg.norm(d)
        g[1], g[0] = d / v, -d / v
    elif op == cx.ANGLE:
        v0, v1 = x[s[0]] - x[s[1]], x[s[2]] - x[s[1]]
        cp = np.cross(v0, v1)
        rp = max(np.linalg.norm(cp), 1e-6)
        v = math.acos(max(-1.0, min(1.0, np.dot(v0, v1) / math.sqrt(np.dot(v0, v0) * np.dot(v1, v1)))))
        g[0], g[2] = np.cross(v0, cp) / (np.dot(v0, v0) * rp), np.cross(cp, v1) / (np.dot(v1, v1) * rp)
        g[1] = -(g[0] + g[2])
    else:
        b1, b2, b3 = x[s[1]] - x[s[0]], x[s[2]] - x[s[1]], x[s[3]] - x[s[2]]
        m, n = np.cross(b1, b2), np.cross(b2, b3)
        lb2 = np.linalg.norm(b2)
        v = math.atan2(lb2 * np.dot(b1, n), np.dot(m, n))
        g[0], g[3] = -lb2 / np.dot(m, m) * m, lb2 / np.dot(n, n) * n
        s12, s32 = np.dot(b1, b2) / lb2 ** 2, np.dot(b3, b2) / lb2 ** 2
        g[1], g[2] = -(1.0 + s12) * g[0] + s32 * g[3], -(1.0 + s32) * g[3] + s12 * g[0]
    return np.concatenate([[v], sum((g[k] for k in range(len(s)) if s[k] == seed), np.zeros(3))])


def _run(prog, push_var, params, global_values, box, push_particles):
    """-> (value, partials [3], the deepest the stack got)"""
    consts, stack, deepest = prog['consts'], [], 0
    unary = _unary_table()

    def chain(x, v, k):
        return np.concatenate([[v], k * x[1:]])

    for op, arg in prog['program']:
        if op == cx.CONST:
            stack.append(np.array([consts[arg], 0.0, 0.0, 0.0]))
        elif op == cx.VAR:
            stack.append(push_var(arg))
        elif op == cx.PARAM:
            stack.append(np.array([params[arg], 0.0, 0.0, 0.0]))
        elif op == cx.GLOBAL:
            stack.append(np.array([global_values[arg], 0.0, 0.0, 0.0]))
        elif op in (cx.DISTANCE, cx.ANGLE, cx.DIHEDRAL):
            stack.append(push_particles(op, arg))
        elif op in (cx.ADD, cx.SUB, cx.MUL, cx.DIV, cx.POW, cx.ATAN2, cx.MIN, cx.MAX):
            y, x = stack.pop(), stack.pop()
            if op == cx.ADD: z = x + y
            elif op == cx.SUB: z = x - y
            elif op == cx.MUL: z = np.concatenate([[x[0] * y[0]], x[1:] * y[0] + x[0] * y[1:]])
            elif op == cx.DIV: z = np.concatenate([[x[0] / y[0]], (x[1:] - x[0] / y[0] * y[1:]) / y[0]])
            elif op == cx.POW:
                p = x[0] ** y[0]
                z = np.concatenate([[p], y[0] * x[0] ** (y[0] - 1.0) * x[1:] + (p * math.log(x[0]) * y[1:] if np.any(y[1:] != 0.0) else 0.0)])
            elif op == cx.ATAN2: z = np.concatenate([[math.atan2(x[0], y[0])], (y[0] * x[1:] - x[0] * y[1:]) / (x[0] ** 2 + y[0] ** 2)])
            elif op == cx.MIN: z = x if x[0] < y[0] else y
            else: z = x if x[0] > y[0] else y
            stack.append(z)
        elif op == cx.SELECT:
            z, y, x = stack.pop(), stack.pop(), stack.pop()
            stack.append(y if x[0] != 0.0 else z)
        elif op == cx.PERIODICDISTANCE:
            a = [stack.pop() for _ in range(6)][::-1]
            d = np.array([a[3][0] - a[0][0], a[4][0] - a[1][0], a[5][0] - a[2][0]])
            if box is not None:
                d = fd_oracle.minimum_image(d, box)
            n = np.linalg.norm(d)
            stack.append(np.concatenate([[n], sum(d[k] / n * (a[3 + k][1:] - a[k][1:]) for k in range(3))]))
        elif op == cx.POWI:
            x = stack.pop()
            v = 1.0
            for _ in range(abs(arg)):
                v *= x[0]                                    # multiplications only: defined for a negative base
            if arg < 0:
                v = 1.0 / v
            stack.append(chain(x, v, arg * v / x[0] if arg else 0.0))
        else:
            x = stack.pop()
            v, k = unary[op](x[0])
            stack.append(chain(x, v, k))
        deepest = max(deepest, len(stack))
    assert len(stack) == 1
    return stack[0][0], stack[0][1:], deepest


def run_program(prog, variables, params, global_values, box=None):
    """a program of a one-variable kind or an external force: every slot a value and its partials with respect to the three variables"""
    def push_var(arg):
        e = np.zeros(4); e[0] = variables[arg]; e[1 + arg] = 1.0
        return e
    return _run(prog, push_var, params, global_values, box, None)


def run_pass(prog, x, params, global_values, seed, box=None):
    """one pass of a compound program over the bond's particles x [P][3] -> (value, dE/d(x, y, z) of particle seed, the deepest stack)"""
    def push_var(arg):
        e = np.zeros(4); e[0] = x[arg // 3][arg % 3]
        if arg // 3 == seed:
            e[1 + arg % 3] = 1.0
        return e
    return _run(prog, push_var, params, global_values, box, lambda op, arg: particles_op(op, arg, x, seed))


# ---- positions ------------------------------------------------------------------------------------------------------------------------
def _f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def positions():
    """[2][N_ATOMS][3]: x and 0.9 x + 0.05, each rounded to f32; every coordinate of x has a magnitude in [0.3, 1.4] and either sign"""
    rng = np.random.default_rng(20261)
    x = rng.uniform(0.3, 1.4, (N_ATOMS, 3)) * rng.choice([-1.0, 1.0], (N_ATOMS, 3))
    return np.array([_f32(x), _f32(0.9 * x + 0.05)])


XS = positions()
BOXES = np.array([[2.5, 2.75, 3.0], [2.25, 3.0, 2.5]])                  # (f32 numbers: the engine keeps a box in f32)
GLOBAL_G = 1.75

# the three placements of a row: an external force, a compound force of one particle, one of three (each pass a different particle)
PLACES = {'ext': dict(x='x', y='y', z='z', W=1), 'c1': dict(x='x1', y='y1', z='z1', W=1), 'c3': dict(x='x1', y='y2', z='z3', W=3)}


def place_atoms(place, block=0):
    """ext / c1: 70 atoms of their own (block 0 or 1: two forces of a handle share no atom); c3: bonds (3t, 3t+1, 3t+2), the last four
    on atoms 0 .. 11 again (70 x 3 = 210 > 200: twelve atoms carry two terms)"""
    if PLACES[place]['W'] == 1:
        return np.arange(N_TERMS)[:, None] + N_TERMS * block
    return (3 * np.arange(N_TERMS)[:, None] + np.arange(3)[None, :]) % 198


def _xyz(place, atoms, r):
    """the values of the placement's x, y, z at replica r, [n]"""
    cols = atoms[:, [0, 0, 0]] if atoms.shape[1] == 1 else atoms
    return XS[r][cols[:, 0], 0], XS[r][cols[:, 1], 1], XS[r][cols[:, 2], 2]


def u_values(row, r):
    x, y, z = _xyz(row['place'], row['atoms'], r)
    p = row['params']
    return p[:, 0] * x + p[:, 1] * y * z + p[:, 2]


def _u_row(name, place, body, lo, hi, kink=None, extra=(), extra_values=None, global_values=None, scale=None, block=0):
    """E = body(u), u = a*x + b*y*z + c spread over [lo, hi] at both replicas, never within 2e-3 of a kink (kink(u): the distance)"""
    P = PLACES[place]
    atoms = place_atoms(place, block)
    a = (0.1 + 0.1 * ((np.arange(N_TERMS) * 0.377) % 1.0)) * np.where(np.arange(N_TERMS) % 2, -1.0, 1.0)
    b = (0.2 - 0.1 * ((np.arange(N_TERMS) * 0.593) % 1.0) + 0.013) * np.where(np.arange(N_TERMS) % 3, 1.0, -1.0)
    (x0, y0, z0), (x1, y1, z1) = _xyz(place, atoms, 0), _xyz(place, atoms, 1)
    c = np.zeros(N_TERMS)
    for t in range(N_TERMS):
        for j in range(1000):
            target = lo + (hi - lo) * ((t * 0.6180339887 + j * 0.1371) % 1.0)
            ct = target - (a[t] * x0[t] + b[t] * y0[t] * z0[t])
            us = [a[t] * x[t] + b[t] * y[t] * z[t] + ct for x, y, z in ((x0, y0, z0), (x1, y1, z1))]
            if all(lo <= u <= hi and (kink is None or kink(u) >= 2e-3) for u in us):
                break
        else:
            raise AssertionError('no operand for lane %d of %s' % (t, name))
        c[t] = ct
    k = 5.0 + 0.1 * np.arange(N_TERMS)
    params = np.column_stack([a, b, c, k])
    names = ['a', 'b', 'c', 'k'] + list(extra)
    row = dict(name='%s/%s' % (place, name), place=place, P=P['W'] if place != 'ext' else 0, energy=None, names=names, atoms=atoms,
               params=params, globals=dict(global_values or {}), periodic=False, interval=(lo, hi), kink=kink)
    if extra_values is not None:
        row['params'] = np.column_stack([params, extra_values(row)])
    if scale is not None:                                   # k of a lane from its own operand: the bound becomes relative to the value
        row['params'][:, 3] = scale(u_values(row, 0))
    row['energy'] = '%s; u = a*%s + b*%s*%s + c' % (body, P['x'], P['y'], P['z'])
    return row


def _xyz_row(name, place, body, names=(), values=None, periodic=False, atoms=None, block=0):
    P = PLACES[place]
    atoms = place_atoms(place, block) if atoms is None else atoms
    k = 5.0 + 0.1 * np.arange(N_TERMS)
    row = dict(name='%s/%s' % (place, name), place=place, P=P['W'] if place != 'ext' else 0, energy=body.format(**P), names=['k'] + list(names),
               atoms=atoms, params=k[:, None], globals={}, periodic=periodic, interval=None, kink=None)
    if values is not None:
        row['params'] = np.column_stack([k, values(row)])
    return row


def _near(f):
    return lambda u: abs(f(u) - round(f(u))) / 3.0


UNARY = [('log', 0.2, 5.0), ('tan', -1.2, 1.2), ('asin', -0.9, 0.9), ('acos', -0.9, 0.9), ('atan', -4.0, 4.0), ('sinh', -3.0, 3.0),
         ('cosh', -3.0, 3.0), ('tanh', -3.0, 3.0), ('erf', -2.5, 2.5), ('erfc', -2.5, 2.5), ('sqrt', 0.2, 4.0), ('exp', -2.0, 2.0),
         ('sin', -3.0, 3.0), ('cos', -3.0, 3.0)]
POWERS = (0, 1, 2, 3, 7, 12, 64, -1, -2, -6, -12, -64)


def _p_two_or_three(row):
    return np.where(np.arange(N_TERMS) % 2, 3.0, 2.0)


def _select_x0(row):
    """x0 of select(x - x0, ...): the lane's own x at replica 0 (lanes 0 .. 9) or at replica 1 (10 .. 19): the condition is exactly
    zero there; above and below x in the other lanes"""
    x = [_xyz(row['place'], row['atoms'], r)[0] for r in (0, 1)]
    t = np.arange(N_TERMS)
    return np.where(t < 10, x[0], np.where(t < 20, x[1], x[0] + np.where(t % 2, 0.25, -0.25)))


def _reference_points(row):
    """x0 y0 z0 of the periodicdistance row: drawn again while a difference lies within 2e-3 box lengths of a face at either replica"""
    rng = np.random.default_rng(7)
    out = np.zeros((N_TERMS, 3))
    xyz = [np.column_stack(_xyz(row['place'], row['atoms'], r)) for r in (0, 1)]
    for t in range(N_TERMS):
        while True:
            p = rng.uniform(-2.0, 2.0, 3)
            d = [np.array([p[0] - x * y, p[1] + z - y, p[2] - (z + x)]) / BOXES[r] for r, (x, y, z) in enumerate((xyz[0][t], xyz[1][t]))]
            if all(np.abs(np.abs(q - np.rint(q)) - 0.5).min() >= 2e-3 for q in d):
                break
        out[t] = p
    return out


def rows_of(place):
    """the rows of one placement, in the order of the issue's table; ext / c1 rows alternate between the two blocks of 70 atoms, so that
    two consecutive rows make a handle in which no atom carries two terms"""
    U, X = _u_row, _xyz_row
    spec = [(U, (op, place, 'k*%s(u)' % op, lo, hi), {}) for op, lo, hi in UNARY]
    spec.append((U, ('erfc tail', place, 'k*erfc(u)', 4.0, 9.0), dict(scale=lambda u: 1.0 / np.array([math.erfc(v) for v in u]))))
    spec.append((U, ('neg', place, 'k*(-u)', -2.0, 2.0), {}))
    spec.append((U, ('abs', place, 'k*abs(u)', -2.0, 2.0), dict(kink=abs)))
    # (k of u^64 and u^-64 is 5 / u^n of the lane: 1.4^64 = 2e9 times 64 k a would leave the range of the fixed-point force, 2^31)
    spec += [(U, ('u^%d' % n, place, 'k*u^%d' % n, 0.7, 1.4), dict(scale=(lambda u, n=n: 5.0 * u ** -n) if abs(n) == 64 else None))
             for n in POWERS]
    spec += [(U, ('(-u)^%d' % n, place, 'k*u^%d' % n, -1.4, -0.7), {}) for n in (2, 3, -3)]
    spec.append((U, ('u^2.5', place, 'k*u^2.5', 0.5, 3.0), {}))
    spec.append((U, ('u^-0.5', place, 'k*u^-0.5', 0.5, 3.0), {}))
    spec.append((U, ('u^p, u < 0', place, 'k*u^p', -1.4, -0.7), dict(extra=('p',), extra_values=_p_two_or_three)))
    spec.append((U, ('g^u', place, 'k*g^u', -2.0, 2.0), dict(global_values=dict(g=GLOBAL_G))))
    spec.append((X, ('(x*y)/(z+2)', place, 'k*({x}*{y})/({z}+2)'), {}))
    spec.append((X, ('atan2', place, 'k*atan2({x}*{y}, {z}-1)'), {}))
    spec.append((X, ('min', place, 'k*min({x}*{y}, {z})'), {}))
    spec.append((X, ('max', place, 'k*max({x}*{y}, {z})'), {}))
    spec.append((X, ('select(x-x0)', place, 'k*select({x}-x0, {y}*{z}, {x}+{z})'), dict(names=('x0',), values=_select_x0)))
    spec.append((U, ('select(step)', place, 'k*select(step(u), u^2, -u^3)', -1.5, 1.5), dict(kink=abs)))
    spec.append((U, ('u*step(u)', place, 'k*u*step(u)', -2.0, 2.0), dict(kink=abs)))
    spec.append((U, ('u*floor(3u)', place, 'k*u*floor(3*u)', -2.0, 2.0), dict(kink=_near(lambda u: 3.0 * u))))
    spec.append((U, ('u*ceil(3u)', place, 'k*u*ceil(3*u)', -2.0, 2.0), dict(kink=_near(lambda u: 3.0 * u))))
    spec.append((U, ('delta', place, 'k*(u*delta(x0-x0) + delta(u))', -2.0, 2.0),
                 dict(kink=abs, extra=('x0',), extra_values=lambda row: 0.1 + 0.01 * np.arange(N_TERMS))))
    if place == 'ext':
        spec.append((X, ('periodicdistance', place, 'k*periodicdistance({x}*{y}, {y}, {z}+{x}, x0, y0+{z}, z0)'),
                     dict(names=('x0', 'y0', 'z0'), values=_reference_points, periodic=True)))
    single = PLACES[place]['W'] == 1
    out = [make(*args, block=i % 2 if single else 0, **kw) for i, (make, args, kw) in enumerate(spec)]
    # (x+1)^(y*z): the 70 atoms (bonds) whose x exceeds 0.3 at both replicas: the base lies in [1.3, 2.4]; a handle of its own
    first = np.flatnonzero(XS[0][:, 0] > 0.3)[:N_TERMS]
    assert len(first) == N_TERMS
    pick = first[:, None] if single else np.column_stack([first, (first + 67) % N_ATOMS, (first + 131) % N_ATOMS])
    out.append(_xyz_row('(x+1)^(y*z)', place, 'k*({x}+1)^({y}*{z})', atoms=pick))
    return out


def _chain_atoms(width, stride):
    """70 terms of `width` atoms over the 200: term t on atoms t, t + stride, t + 2 stride ... (an atom carries up to `width` terms)"""
    return (np.arange(N_TERMS)[:, None] + stride * np.arange(width)[None, :]) % N_ATOMS


def particle_rows():
    """particle functions fed into the new opcodes, and the one-variable kinds (six new opcodes of r or theta each)"""
    k = (5.0 + 0.1 * np.arange(N_TERMS))[:, None]
    c = (0.8 + 0.02 * np.arange(N_TERMS))[:, None]

    def row(name, kind, P, energy, names, atoms, params):
        return dict(name=name, place=kind, P=P, energy=energy, names=list(names), atoms=atoms, params=params, globals={}, periodic=False,
                    interval=None, kink=None)
    three = place_atoms('c3')
    return [row('tanh(distance)*erfc(angle)', 'compound', 3, 'k*tanh(distance(p1,p2)) * erfc(angle(p1,p2,p3))', 'k', three, k),
            row('min(distance, distance)^-2', 'compound', 3, 'k*min(distance(p1,p2), distance(p2,p3))^-2', 'k', three, k),
            row('atan2(sin(dihedral), x4-x1)', 'compound', 4, 'k*atan2(sin(dihedral(p1,p2,p3,p4)), x4-x1)', 'k', _chain_atoms(4, 50), k),
            row('pointdistance', 'compound', 3, 'k*pointdistance(x1*y2, y1, z1, x3, y3+z2, z3)', 'k', three, k),
            row('bond', 'bond', 0, 'k*(log(r) + tanh(2*r) + erfc(r) + atan2(r, c) + min(r, c)^-2 + cosh(r))', 'kc', _chain_atoms(2, 100),
                np.column_stack([k, c])),
            row('angle', 'angle', 0, 'k*(tan(theta/4) + asin(theta/4) + acos(theta/4) + sinh(theta) + erf(theta) + abs(theta-c) + max(theta, c))',
                'kc', _chain_atoms(3, 67), np.column_stack([k, c + 0.5])),
            row('torsion', 'torsion', 0, 'k*(atan(theta) + (theta+4)^-3 + abs(theta) + theta*step(theta) + theta*ceil(theta) + cosh(theta) + erfc(theta))',
                'k', _chain_atoms(4, 50), k)]


def all_rows():
    return rows_of('ext') + rows_of('c1') + rows_of('c3') + particle_rows()
