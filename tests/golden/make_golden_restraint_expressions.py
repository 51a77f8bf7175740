"""Golden vectors for the restraint energy EXPRESSIONS, produced from the reference's own string literals.

The reference builds the energy of its four radially symmetric restraints (openmmtools/forces.py:711-1107) from two literals,

    HarmonicRestraintForceMixIn.__init__     energy_function = '(K/2)*distance(g1,g2)^2'                               (:810)
    FlatBottomRestraintForceMixIn.__init__   energy_function = 'step(distance(g1,g2)-r0) * (K/2)*(distance(g1,g2)-r0)^2' (:943)

and two rules: the centroid variants prepend the controlling parameter, ``name + ' * (' + energy_function + ')'`` (:715), the bond
variants first replace 'distance(g1,g2)' by 'r' (:763-764).  openmm is absent here, so this script takes the two literals out of the
module's syntax tree, applies the two rules as the reference's constructors do, and evaluates each expression (OpenMM's syntax:
^ = power, step(x) = 1 for x >= 0) on a grid of (r, K, r0, lambda).  The class-hash rule float(zlib.adler32(class name)) is that of
openmmtools/utils/utils.py:1023-1037.  Strings, inputs and values go to tests/golden/reference_restraint_expressions.json.

The reference tree does not exist on the GPU box: the tests read only the JSON.   usage: python tests/golden/make_golden_restraint_expressions.py
"""
import ast
import itertools
import json
import os
import zlib

REF = '/root/reference/openmmtools/forces.py'
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'reference_restraint_expressions.json')


def literals():
    tree = ast.parse(open(REF).read())
    out = {}
    for node in tree.body:
        if isinstance(node, ast.ClassDef) and node.name in ('HarmonicRestraintForceMixIn', 'FlatBottomRestraintForceMixIn'):
            for stmt in ast.walk(node):
                if isinstance(stmt, ast.Assign) and getattr(stmt.targets[0], 'id', None) == 'energy_function':
                    out[node.name] = stmt.value.value
    return out


def evaluate(expression, r, K, r0, lam):
    expr = expression.replace('^', '**').replace('distance(g1,g2)', 'r')
    return float(eval(expr, {'step': lambda x: 1.0 if x >= 0 else 0.0}, dict(r=r, K=K, r0=r0, lambda_restraints=lam)))


def main():
    lit = literals()
    bodies = {'harmonic': lit['HarmonicRestraintForceMixIn'], 'flat_bottom': lit['FlatBottomRestraintForceMixIn']}
    classes = {'HarmonicRestraintForce': ('harmonic', False), 'HarmonicRestraintBondForce': ('harmonic', True),
               'FlatBottomRestraintForce': ('flat_bottom', False), 'FlatBottomRestraintBondForce': ('flat_bottom', True)}
    grid = list(itertools.product([0.0, 0.05, 0.2, 0.35, 0.8, 1.7], [10.0, 418.4, 2000.0], [0.0, 0.3, 1.0], [0.0, 0.25, 1.0]))
    out = {'bodies': bodies, 'classes': {}, 'grid': [list(g) for g in grid]}
    for name, (kind, bond) in classes.items():
        body = bodies[kind].replace('distance(g1,g2)', 'r') if bond else bodies[kind]
        energy = 'lambda_restraints' + ' * (' + body + ')'
        out['classes'][name] = {'energy': energy, 'class_hash': float(zlib.adler32(name.encode())),
                                'values': [evaluate(energy, *g) for g in grid]}
    json.dump(out, open(OUT, 'w'), indent=1)


if __name__ == '__main__':
    main()
