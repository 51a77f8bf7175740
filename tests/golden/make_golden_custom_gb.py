"""Golden values of OBC-family CustomGBForce energies with periodic cutoffs, from the reference's own strings.

/root/reference/openmmtools/testsystems.py:4279-4389 (CustomGBForceSystem) builds a CustomGBForce from string literals, and
/root/reference/openmmtools/alchemy/alchemy.py:2223-2345 (_alchemically_modify_CustomGBForce) rewrites such strings with fixed prefixes,
substitutions and suffixes.  openmm is absent here; this script takes the literals and the rewrite rules out of the two functions' syntax
trees UNCHANGED and evaluates them with the interpreter of the CustomGBForce semantics of make_golden_gbsa.py (imported, not edited),
extended with the minimum image and the cutoff of CutoffPeriodic (a pair computed value or pair energy term sees the pairs with r < cutoff).
Cases: small periodic configurations with pairs across the box boundary and pairs straddling the cutoff, at lambda_electrostatics 0, 0.5
and 1, one NoCutoff case and one case with OBC1's constants (0.8, 0, 2.909125).  Output: tests/golden/reference_custom_gb.json.
/root/reference does not exist on the GPU box: the tests read only the JSON.     usage: python tests/golden/make_golden_custom_gb.py
"""
import ast
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_gbsa import evaluate          # noqa: E402  (the interpreter of the CustomGBForce semantics)

TESTSYSTEMS = '/root/reference/openmmtools/testsystems.py'
ALCHEMY = '/root/reference/openmmtools/alchemy/alchemy.py'
OUT = os.path.join(HERE, 'reference_custom_gb.json')


def _method(tree, cls_name, fn_name):
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls_name)
    return next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == fn_name)


def testsystem_strings():
    """computed values and energy terms of CustomGBForceSystem.__init__, executing its string assignments in order"""
    fn = _method(ast.parse(open(TESTSYSTEMS).read()), 'CustomGBForceSystem', '__init__')
    var, computed, energy, globals_, per, consts = {}, [], [], {}, [], {}
    for node in sorted([n for n in ast.walk(fn) if isinstance(n, (ast.Assign, ast.AugAssign, ast.Expr))], key=lambda n: n.lineno):
        if isinstance(node, ast.Assign) and isinstance(node.value, ast.Constant) and isinstance(node.value.value, str):
            var[node.targets[0].id] = node.value.value
        elif isinstance(node, ast.AugAssign) and isinstance(node.value, ast.Constant):
            var[node.target.id] += node.value.value
        elif isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Name) and isinstance(node.value, (ast.BinOp, ast.Constant)):
            consts[node.targets[0].id] = ast.unparse(node.value)
        elif isinstance(node, ast.Expr) and isinstance(node.value, ast.Call) and isinstance(node.value.func, ast.Attribute):
            c = node.value
            kind = lambda a: a.attr if isinstance(a, ast.Attribute) else None
            text = lambda a: a.value if isinstance(a, ast.Constant) else var[a.id]
            if c.func.attr == 'addComputedValue':
                computed.append((c.args[0].value, text(c.args[1]), kind(c.args[2])))
            elif c.func.attr == 'addEnergyTerm':
                energy.append((text(c.args[0]), kind(c.args[1])))
            elif c.func.attr == 'addGlobalParameter':
                globals_[c.args[0].value] = float(c.args[1].value)
            elif c.func.attr == 'addPerParticleParameter':
                per.append(c.args[0].value)
    return computed, energy, globals_, per, consts, (fn.lineno, fn.end_lineno)


def rewrite_rules():
    """the prefixes, replacements and suffixes of _alchemically_modify_CustomGBForce"""
    fn = _method(ast.parse(open(ALCHEMY).read()), 'AbsoluteAlchemicalFactory', '_alchemically_modify_CustomGBForce')
    prepends, replaces, suffixes = [], [], []
    for node in ast.walk(fn):
        if isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Name) and node.targets[0].id == 'prepend':
            prepends.append((node.lineno, node.value.value))
        elif isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == 'replace':
            replaces.append((node.lineno, node.args[0].value, node.args[1].value))
        elif isinstance(node, ast.AugAssign) and isinstance(node.value, ast.Constant):
            suffixes.append((node.lineno, node.value.value))
    prepends.sort(); replaces.sort(); suffixes.sort()
    return dict(pair_value_prefix=prepends[0][1], single_term_prefix=prepends[1][1], replaces=[r[1:] for r in replaces],
                pair_term_suffix=''.join(s[1] for s in suffixes), source='alchemy.py:%d-%d' % (fn.lineno, fn.end_lineno))


def rewrite(computed, energy, rules):
    c2 = [(n, e if k == 'SingleParticle' else rules['pair_value_prefix'] + e, k) for n, e, k in computed]
    e2 = []
    for e, k in energy:
        if k == 'SingleParticle':
            e2.append((rules['single_term_prefix'] + e, k))
        else:
            for a, b in rules['replaces']:
                e = e.replace(a, b)
            e2.append((e + rules['pair_term_suffix'], k))
    return c2, e2


def custom_gb_energy(computed, energy, globals_, x, per_particle, box=None, cutoff=None):
    """make_golden_gbsa.custom_gb_energy with the minimum image under ``box`` and the pair cutoff of CutoffPeriodic"""
    n = len(x)
    values = {}

    def of(i, suffix=''):
        d = {k + suffix: float(v[i]) for k, v in per_particle.items()}
        d.update({k + suffix: float(v[i]) for k, v in values.items()})
        return d

    def dist(i, j):
        d = x[i] - x[j]
        if box is not None:
            d = d - box * np.round(d / box)
        return float(np.linalg.norm(d))

    def in_range(r):
        return cutoff is None or r < cutoff
    for name, expr, kind in computed:
        out = np.zeros(n)
        for i in range(n):
            if kind == 'SingleParticle':
                out[i] = evaluate(expr, dict(globals_, **of(i)))
            else:
                for j in range(n):
                    if j != i and in_range(dist(i, j)):
                        out[i] += evaluate(expr, dict(globals_, r=dist(i, j), **of(i, '1'), **of(j, '2')))
        values[name] = out
    e = 0.0
    for expr, kind in energy:
        if kind == 'SingleParticle':
            e += sum(evaluate(expr, dict(globals_, **of(i))) for i in range(n))
        else:
            e += sum(evaluate(expr, dict(globals_, r=dist(i, j), **of(i, '1'), **of(j, '2'))) for i in range(n) for j in range(i + 1, n)
                     if in_range(dist(i, j)))
    return e, {k: v.tolist() for k, v in values.items()}


def _configuration(rng, n, box_edge, cutoff):
    """positions in [0, box): the first two particles across the boundary of x, the next pair straddling the cutoff"""
    while True:
        x = rng.uniform(0.0, box_edge, size=(n, 3))
        x[0] = [0.05, 0.6 * box_edge, 0.5 * box_edge]
        x[1] = [box_edge - 0.3, 0.6 * box_edge + 0.1, 0.5 * box_edge]             # 0.35 nm apart through the boundary
        x[3] = x[2] + np.array([cutoff - 0.02, 0.0, 0.0])                          # just inside
        x[4] = x[2] + np.array([0.0, cutoff + 0.02, 0.0])                          # just outside
        x %= box_edge
        d = x[:, None] - x[None]
        d -= box_edge * np.round(d / box_edge)
        r = np.linalg.norm(d, axis=-1) + np.eye(n) * 10
        if r.min() > 0.3:
            return x


def main():
    computed, energy, ts_globals, per, consts, lines = testsystem_strings()
    rules = rewrite_rules()
    acomputed, aenergy = rewrite(computed, energy, rules)
    obc1 = [(n, e.replace('tanh(1*psi-0.8*psi^2+4.85*psi^3)', 'tanh(0.8*psi-0*psi^2+2.909125*psi^3)'), k) for n, e, k in computed]
    assert obc1 != computed
    out = dict(source_testsystem='testsystems.py:%d-%d' % lines, source_rewrite=rules['source'], computed_values=computed, energy_terms=energy,
               globals=ts_globals, per_particle=per, constants=consts, rewrite_rules=rules, alchemical_computed_values=acomputed,
               alchemical_energy_terms=aenergy, cases=[])
    rng = np.random.default_rng(20261016)
    for case, (n, box_edge, cutoff, model, lams) in enumerate([(9, 3.0, 1.2, 'OBC2', (0.0, 0.5, 1.0)), (12, 2.6, 1.1, 'OBC2', (0.0, 0.5, 1.0)),
                                                                 (9, 3.0, None, 'OBC2', (1.0,)), (10, 2.8, 1.2, 'OBC1', (0.5, 1.0))]):
        x = _configuration(rng, n, box_edge, cutoff or 1.2)
        pp = dict(charge=np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * rng.uniform(0.3, 1.0, n), radius=rng.uniform(0.1, 0.2, n),
                  scale=rng.uniform(0.5, 0.8, n), alchemical=(np.arange(n) < 3).astype(float))
        box = np.full(3, box_edge) if cutoff is not None else None
        for lam in lams:
            g = dict(ts_globals, lambda_electrostatics=lam)
            cv, et = (acomputed, aenergy) if model == 'OBC2' else rewrite(obc1, energy, rules)
            e, vals = custom_gb_energy(cv, et, g, x, pp, box, cutoff)
            out['cases'].append(dict(model=model, x=x.tolist(), box=None if box is None else box.tolist(), cutoff=cutoff,
                                     charge=pp['charge'].tolist(), radius=pp['radius'].tolist(), scale=pp['scale'].tolist(),
                                     alchemical=pp['alchemical'].tolist(), lambda_electrostatics=lam, energy=e, I=vals['I'], B=vals['B']))
    with open(OUT, 'w') as fh:
        json.dump(out, fh, separators=(',', ':'))
    print([(c['model'], c['cutoff'], c['lambda_electrostatics'], round(c['energy'], 6)) for c in out['cases']])


if __name__ == '__main__':
    main()
