"""CPU: the general path of a CustomGBForce (openmmtools_amd/custom_gb.py compile_custom_gb; REMD_CUSTOM_GB of include/remd_hip_custom.h).
The compiler's pass splitting, staged columns, folded globals and refusals; the dispatch beside the template path; the compiled
programs interpreted here in Python, stage by stage in the order of the five launches of csrc/custom_gb.hip, against
tests/custom_gb_expr_oracle.py; the oracle's forces against central differences of its energies; and the host plan
(csrc/custom_gb_plan.h) through tools/custom_gb_plan_check.cpp, a program with its own main built with -fsanitize=address,undefined."""
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import custom_gb_expr_cases as cases
import custom_gb_expr_oracle as oracle
from openmmtools_amd import alchemy, custom_expr as cx, custom_gb, states, system as sysmod, testsystems as ts, unit
from openmmtools_amd.system import System, NonbondedForce, CustomGBForce, Discrete2DFunction, system_to_desc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SINGLE, PAIR, PAIR_NX = cases.SINGLE, cases.PAIR, cases.PAIR_NX


def _system(n, force, box=None, nonbonded=None):
    s = System()
    for _ in range(n):
        s.addParticle(12.0)
    if box is not None:
        s.setDefaultPeriodicBoxVectors([box[0], 0, 0], [0, box[1], 0], [0, 0, box[2]])
    if nonbonded is not None:
        nb = NonbondedForce()
        nb.setNonbondedMethod(nonbonded)
        for _ in range(n):
            nb.addParticle(0.0, 0.3, 0.0)
        s.addForce(nb)
    s.addForce(force)
    return s


def _entry(spec, box=None):
    return system_to_desc(_system(len(spec['params']), cases.build(spec), box))['custom_terms']['000']


def _simple(computed, terms, per=('q',), n=4, **kw):
    return dict(per_particle=list(per), params=np.full((n, len(per)), 0.5), globals=kw.pop('globals', {}), computed=computed, terms=terms,
                method=kw.pop('method', 0), cutoff=kw.pop('cutoff', 0.0), **kw)


# ---- the compiler ---------------------------------------------------------------------------------------------------------------------------
def test_passes_one_two_and_three():
    values = [('a', 'q1*q2/r', PAIR_NX), ('b', 'a+q', SINGLE), ('c', 'a*b', SINGLE), ('d', 'c+b', SINGLE)]
    for named, want in ((['a'], 1), (['a', 'b'], 2), (['a', 'b', 'c', 'd'], 3)):
        text = '+'.join('%s1*%s2' % (v, v) for v in named) + '+r'
        e = _entry(_simple(values, [(text, PAIR_NX)]))
        rows = [s for s in e['stages'] if s[0] == 3]
        assert [int(s[3]) for s in rows] == list(range(want)) == list(range(math.ceil((1 + 2 * len(named)) / 3)))
        # r is variable 0 of the first pass and a staged column of the others; every value is a variable in exactly one pass
        assert rows[0][7] == 0 and all(0 in s[11:11 + s[10]] for s in rows[1:])
        variables = [int(c) for s in rows for c in s[7:10] if c >= 0]
        assert sorted(variables) == [0] + sorted(1 + 2 * k + p for k in range(len(named)) for p in (0, 1))
    single = [s for s in _entry(_simple(values, [('a*b*c*d', SINGLE)]))['stages'] if s[0] == 2]
    assert [int(s[3]) for s in single] == [0, 1] and [int(c) for c in single[0][7:10]] == [1, 3, 5] and single[1][7] == 7


def test_only_named_columns_are_staged_and_globals_are_folded():
    e = _entry(cases.born(5, cases.HCT_B))
    pair = [s for s in e['stages'] if s[0] == 3][0]
    assert [int(c) for c in pair[7:10]] == [0, 3, 4] and [int(c) for c in pair[11:11 + pair[10]]] == [16, 17]      # r, B1, B2; charge1, charge2
    value = e['stages'][0]
    assert [int(c) for c in value[7:10]] == [0, -1, -1] and [int(c) for c in value[11:11 + value[10]]] == [18, 19, 21]   # radius1, radius2, scale2
    assert not np.any(e['program'][:, 0] == cx.GLOBAL) and len(e['global_names']) == 0
    # solventDielectric, a global, is a constant of the self term's and of the pair term's program
    assert np.count_nonzero(e['consts'] == 78.5) == 2
    assert e['kind'] == 12 and e['n_values'] == 2 and e['stages'].shape == (4, 28)


REFUSALS = [
    (NotImplementedError, r"variable 'x'", lambda: _simple([('a', 'r', PAIR_NX)], [('q*x', SINGLE)])),
    (NotImplementedError, r"computed value 'b' of type ParticlePair behind the first", lambda: _simple([('a', 'r', PAIR_NX), ('b', 'r', PAIR)], [('a', SINGLE)])),
    (NotImplementedError, r"first computed value 'a' is of type SingleParticle", lambda: _simple([('a', 'q', SINGLE)], [('a', SINGLE)])),
    (NotImplementedError, r'5 computed values \(the engine takes 4\)',
     lambda: _simple([('a', 'r', PAIR_NX)] + [('v%d' % k, 'a', SINGLE) for k in range(4)], [('a', SINGLE)])),
    (NotImplementedError, r'9 energy terms \(the engine takes 8\)', lambda: _simple([('a', 'r', PAIR_NX)], [('a', SINGLE)] * 9)),
    (NotImplementedError, r'a program of \d+ instructions \(the engine takes 256\)', lambda: _simple([('a', '+'.join(['sin(r)'] * 140), PAIR_NX)], [('a', SINGLE)])),
    (NotImplementedError, r'needs \d+ stack slots \(the engine has 16\)',
     lambda: _simple([('a', 'r' + ''.join('+(r*%d' % k for k in range(2, 20)) + ')' * 18, PAIR_NX)],
                     [('a', SINGLE)])),
    (NotImplementedError, r'names 17 staged columns \(the engine takes 16\)',
     lambda: _simple([('a', '+'.join(['p%d1' % k for k in range(9)] + ['p%d2' % k for k in range(8)]) + '+r', PAIR_NX)], [('a', SINGLE)],
                     per=['p%d' % k for k in range(9)])),
    (ValueError, r'exclusion 0 names particle 9', lambda: _simple([('a', 'r', PAIR)], [('a', SINGLE)], exclusions=[(0, 9)])),
    (ValueError, r'particles 1 and 0 are excluded twice', lambda: _simple([('a', 'r', PAIR)], [('a', SINGLE)], exclusions=[(0, 1), (1, 0)])),
    (NotImplementedError, r"per-particle name 'q' without a particle suffix", lambda: _simple([('a', 'q*r', PAIR_NX)], [('a', SINGLE)])),
    (NotImplementedError, r"unknown variable 'zeta'", lambda: _simple([('a', 'r', PAIR_NX)], [('a*zeta', SINGLE)])),
]


@pytest.mark.parametrize('k', range(len(REFUSALS)))
def test_refusals_by_their_message(k):
    error, message, make = REFUSALS[k]
    with pytest.raises(error, match=message):
        _entry(make())


def test_refusals_of_the_system_around_the_force():
    spec = _simple([('a', 'q1*q2/r', PAIR_NX)], [('a', SINGLE)])
    with pytest.raises(ValueError, match='CustomGBForce has 4 particles, system has 5'):
        system_to_desc(_system(5, cases.build(spec)))
    periodic = dict(spec, method=2, cutoff=1.2)
    with pytest.raises(ValueError, match='exceeds half the smallest box edge'):
        system_to_desc(_system(4, cases.build(periodic), box=[2.0, 3.0, 3.0]))
    s = _system(4, cases.build(periodic), box=[3.0, 3.0, 3.0])
    s.setDefaultPeriodicBoxVectors([3.0, 0, 0], [0.5, 3.0, 0], [0, 0, 3.0])
    with pytest.raises(NotImplementedError, match='triclinic'):
        system_to_desc(s)
    assert system_to_desc(_system(4, cases.build(dict(spec, method=1, cutoff=1.0))))['custom_terms']['000']['nb_method'] == 1
    # the alchemical factory
    t = ts.AlanineDipeptideImplicit(implicitSolvent='HCT')
    with pytest.raises(NotImplementedError, match='general expression path'):
        alchemy.AbsoluteAlchemicalFactory().create_alchemical_system(t.system, alchemy.AlchemicalRegion(alchemical_atoms=range(6)))


def test_a_global_parameter_state_may_not_set_a_global_of_a_general_force():
    class DielectricState(states.GlobalParameterState):
        solventDielectric = states.GlobalParameterState.GlobalParameter('solventDielectric', standard_value=78.5)
    t = ts.AlanineDipeptideImplicit(implicitSolvent='HCT')
    with pytest.raises(states.GlobalParameterError, match='solventDielectric of a CustomGBForce cannot be controlled'):
        DielectricState(solventDielectric=40.0).apply_to_system(t.system)


def test_the_engine_pool_system_xml_the_netcdf4_layout_the_cpu_port_and_a_later_change_refuse_it():
    import types
    from openmmtools_amd import _engine, system_xml
    from openmmtools_amd.multistate import _engine_pool
    from openmmtools_amd.multistate._reference_store import ReferenceStoreWriter
    t = ts.AlanineDipeptideImplicit(implicitSolvent='HCT')
    s = t.system
    # System XML stays as it was: the document of such a force is refused where it is read, by the recognizer's sentence
    with pytest.raises(NotImplementedError, match=r"CustomGBForce: computed value 'B' does not match"):
        system_xml.from_xml(system_xml.to_xml(s))
    with_table = _system(5, cases.build(cases.gbn2_shaped(5)))
    with pytest.raises(NotImplementedError, match='CustomGBForce with tabulated functions'):
        system_xml.to_xml(with_table)
    # the netCDF4 layout: layout='auto' then keeps the record container
    why = ReferenceStoreWriter.can_store([states.ThermodynamicState(s, 300.0 * unit.kelvin)], [], [])
    assert why is not None and 'CustomGBForce' in why and 'general expression path' in why and "'I', 'B'" in why
    assert ReferenceStoreWriter.can_store([states.ThermodynamicState(ts.AlanineDipeptideImplicit().system, 300.0 * unit.kelvin)], [], []) is None
    # several compatibility groups
    pool = _engine_pool.EnginePool.__new__(_engine_pool.EnginePool)
    pool.G = 2
    with pytest.raises(NotImplementedError, match='Generalized-Born expressions.*more than one compatibility group'):
        pool.set_system([system_to_desc(s), system_to_desc(s)])
    # the CPU port of the ABI exports none of include/remd_hip_custom.h
    d = system_to_desc(s)
    eng = object.__new__(_engine.HipEngine)
    eng.lib, eng.h = types.SimpleNamespace(), None
    for call in (lambda: eng.set_custom_terms([d['custom_terms']['000']]), lambda: eng.set_custom_globals(np.zeros((1, 0))),
                 lambda: eng.custom_energies()):
        with pytest.raises(NotImplementedError, match='Generalized-Born expressions.*remd_hip_custom.h is GPU-only'):
            call()
    # a change after set_system
    with pytest.raises(NotImplementedError, match='CustomGBForce: changing particles, exclusions or functions after set_system'):
        s.forces[-1].updateParametersInContext()


class _StandIn:
    """what gb_force_from_openmm asks of an openmm.CustomGBForce"""
    class _Table:
        def getFunctionParameters(self): return (2, 2, [0.1, 0.2, 0.3, 0.4])
    _Table.__name__ = 'Discrete2DFunction'
    def getNumPerParticleParameters(self): return 2
    def getPerParticleParameterName(self, i): return ['q', 'radindex'][i]
    def getNumGlobalParameters(self): return 1
    def getGlobalParameterName(self, i): return 'k'
    def getGlobalParameterDefaultValue(self, i): return 2.5
    def getNumTabulatedFunctions(self): return 1
    def getTabulatedFunctionName(self, i): return 'm0'
    def getTabulatedFunction(self, i): return self._Table()
    def getNumComputedValues(self): return 2
    def getComputedValueParameters(self, i): return [('a', 'q2*m0(radindex1,radindex2)/r', 1), ('b', 'k*a', 0)][i]
    def getNumEnergyTerms(self): return 1
    def getEnergyTermParameters(self, i): return ('q*b', 0)
    def getNumParticles(self): return 3
    def getParticleParameters(self, i): return (0.5 + i, float(i % 2))
    def getNumExclusions(self): return 1
    def getExclusionParticles(self, i): return (2, 0)
    def getNonbondedMethod(self): return 1
    def getCutoffDistance(self): return 8.0 * unit.angstroms
    def getForceGroup(self): return 4


def test_from_openmm_by_a_stand_in_carries_the_tabulated_functions():
    g = sysmod.gb_force_from_openmm(_StandIn())
    assert isinstance(g, CustomGBForce) and g.computed == [('a', 'q2*m0(radindex1,radindex2)/r', 1), ('b', 'k*a', 0)] and g.energy_terms == [('q*b', 0)]
    assert (g.getNumParticles(), g.getParticleParameters(2), g.getExclusionParticles(0)) == (3, [2.5, 0.0], [2, 0])
    assert (g.getNonbondedMethod(), g.getForceGroup()) == (1, 4) and g.getCutoffDistance() == pytest.approx(0.8, rel=1e-14)
    assert g.getGlobalParameterDefaultValue(0) == 2.5 and g.per_particle == ['q', 'radindex']
    assert g.getTabulatedFunctionName(0) == 'm0' and isinstance(g.getTabulatedFunction(0), Discrete2DFunction)
    e = system_to_desc(_system(3, g))['custom_terms']['000']
    assert e['kind'] == 12 and np.any(e['program'][:, 0] == cx.LOOKUP2D) and e['stages'][0][1] == 1
    import inspect
    assert "'CustomGBForce'" in inspect.getsource(sysmod.from_openmm)


def test_dispatch_keeps_the_template_path_and_its_errors():
    s = ts.CustomGBForceSystem()
    d = system_to_desc(s.system)
    assert d['gbsa']['method'] == 2 and 'custom_terms' not in d
    general = system_to_desc(_system(5, cases.build(cases.born(5, cases.OBC2_B))))
    assert 'gbsa' not in general and general['custom_terms']['000']['kind'] == 12
    with pytest.raises(NotImplementedError):
        custom_gb.recognize_custom_gb(cases.build(cases.born(5, cases.OBC2_B)))
    # the errors behind a successful recognition are raised as before
    force = [f for f in s.system.forces if isinstance(f, CustomGBForce)][0]
    with pytest.raises(NotImplementedError, match='larger than half the shortest box edge'):
        custom_gb.custom_gb_to_desc(force, 140, 1, np.full(3, 3.0))
    with pytest.raises(NotImplementedError, match='NonbondedForce is not periodic'):
        custom_gb.custom_gb_to_desc(force, 140, 3, np.full(3, 10.0))
    small = cases.build(dict(cases.born(3, 'x'), computed=ts.CustomGBForceSystem().system.forces[-1].computed, globals={}))
    small.energy_terms = list(force.energy_terms); small.globals = [list(g) for g in force.globals]
    small.particles[0] = (1.0, 0.005, 0.8)
    with pytest.raises(ValueError, match='radii must exceed the offset'):
        custom_gb.custom_gb_to_desc(small, 3, 3, np.zeros(3))


def test_hct_test_system_and_what_stays_refused():
    t = ts.AlanineDipeptideImplicit(implicitSolvent='HCT')
    d = system_to_desc(t.system)
    e = d['custom_terms']['000']
    assert 'gbsa' not in d and e['kind'] == 12 and e['params'].shape == (22, 3) and e['nb_method'] == 0
    assert d['custom_globals']['names'] == []
    with pytest.raises(NotImplementedError, match="'OBC2'"):
        ts.AlanineDipeptideImplicit(implicitSolvent='GBn')


# ---- the programs, interpreted --------------------------------------------------------------------------------------------------------------
def _run(entry, row, x, columns):
    """the forward-mode machine on one stage: (value, partial 0, partial 1, partial 2)"""
    consts, stack = entry['consts'], []
    unary = {cx.NEG: (lambda a: -a, lambda a: -1.0), cx.SQRT: (math.sqrt, lambda a: 0.5 / math.sqrt(a) if a > 0.0 else 0.0),
             cx.EXP: (math.exp, math.exp), cx.LOG: (math.log, lambda a: 1.0 / a), cx.TANH: (math.tanh, lambda a: 1.0 - math.tanh(a) ** 2),
             cx.ABS: (abs, lambda a: -1.0 if a < 0.0 else 1.0), cx.STEP: (lambda a: 1.0 if a >= 0.0 else 0.0, lambda a: 0.0)}
    for op, arg in entry['program'][row[4]:row[4] + row[5]].tolist():
        if op == cx.CONST:
            stack.append(np.array([consts[arg], 0.0, 0.0, 0.0]))
        elif op == cx.VAR:
            v = np.zeros(4); v[0] = x[arg]; v[1 + arg] = 1.0
            stack.append(v)
        elif op == cx.PARAM:
            stack.append(np.array([columns[arg], 0.0, 0.0, 0.0]))
        elif op in (cx.ADD, cx.SUB, cx.MUL, cx.DIV, cx.MIN, cx.MAX, cx.LOOKUP2D):
            b, a = stack.pop(), stack.pop()
            if op == cx.ADD: stack.append(a + b)
            elif op == cx.SUB: stack.append(a - b)
            elif op == cx.MUL: stack.append(np.concatenate([[a[0] * b[0]], a[1:] * b[0] + a[0] * b[1:]]))
            elif op == cx.DIV: stack.append(np.concatenate([[a[0] / b[0]], (a[1:] - a[0] / b[0] * b[1:]) / b[0]]))
            elif op == cx.MIN: stack.append(a if a[0] < b[0] else b)
            elif op == cx.MAX: stack.append(a if a[0] > b[0] else b)
            else: stack.append(np.array([float(cx.lookup_grid_values(consts, arg, a[0], b[0])), 0.0, 0.0, 0.0]))
        elif op == cx.POWI:
            a = stack.pop()
            stack.append(np.concatenate([[a[0] ** arg], arg * a[0] ** (arg - 1) * a[1:]]))
        elif op in unary:
            a = stack.pop()
            f, df = unary[op]
            stack.append(np.concatenate([[f(a[0])], df(a[0]) * a[1:]]))
        else:
            raise AssertionError('opcode %d' % op)
    assert len(stack) == 1
    return stack[0]


def _interpret(entry, x, excluded=()):
    """energy and forces of a compiled entry (NoCutoff), the five launches of csrc/custom_gb.hip one after the other"""
    N, nv, stages, par = len(x), entry['n_values'], entry['stages'], entry['params']
    ex = set(excluded) | {(j, i) for i, j in excluded}
    V = np.zeros((nv, N))

    def quantity(code, p1, p2, r):
        if code == 0:
            return r
        k, s = divmod(code - (1 if code < 16 else 16), 2)
        return (V if code < 16 else par.T)[k][p2 if s else p1]

    def run(row, p1, p2, r):
        return _run(entry, row, [quantity(c, p1, p2, r) if c >= 0 else 0.0 for c in row[7:10]], [quantity(c, p1, p2, r) for c in row[11:11 + row[10]]])

    d = x[None] - x[:, None]                                  # d[i][j] = x_j - x_i
    R = np.sqrt((d ** 2).sum(axis=2))
    on = lambda row, i, j: i != j and not (row[1] and (i, j) in ex)
    for i in range(N):                                        # 1
        V[0, i] = sum(run(stages[0], i, j, R[i, j])[0] for j in range(N) if on(stages[0], i, j))
    E, G, F = 0.0, np.zeros((nv, N)), np.zeros((N, 3))
    for i in range(N):                                        # 2
        for row in stages[1:]:
            if row[0] == 1:
                V[row[2], i] = run(row, i, i, 0.0)[0]
            elif row[0] == 2:
                e = run(row, i, i, 0.0)
                E += e[0] if row[3] == 0 else 0.0
                for v in range(3):
                    if row[7 + v] >= 1:
                        G[(row[7 + v] - 1) // 2, i] += e[1 + v]
    for i in range(N):                                        # 3
        for j in range(N):
            for row in stages:
                if row[0] != 3 or not on(row, i, j):
                    continue
                p1, p2, own = (i, j, 0) if i < j else (j, i, 1)
                e = run(row, p1, p2, R[i, j])
                E += 0.5 * e[0] if row[3] == 0 else 0.0
                for v in range(3):
                    code = row[7 + v]
                    if code == 0:
                        F[i] += e[1 + v] * d[i, j] / R[i, j]
                    elif code > 0 and (code - 1) % 2 == own:
                        G[(code - 1) // 2, i] += e[1 + v]
    for i in range(N):                                        # 4
        for q in range(nv - 1, 0, -1):
            e = run(stages[q], i, i, 0.0)
            for v in range(3):
                if stages[q][7 + v] >= 1:
                    G[(stages[q][7 + v] - 1) // 2, i] += G[q, i] * e[1 + v]
    for i in range(N):                                        # 5
        for j in range(N):
            if on(stages[0], i, j):
                k = G[0, i] * run(stages[0], i, j, R[i, j])[1] + G[0, j] * run(stages[0], j, i, R[i, j])[1]
                F[i] += k * d[i, j] / R[i, j]
    return E, F


CASES = {'obc2 in parentheses': lambda: cases.born(9, cases.OBC2_B), 'hct': lambda: cases.born(9, cases.HCT_B), 'gbn2-shaped': lambda: cases.gbn2_shaped(9),
         'exclusions': lambda: cases.excluded(9, [(0, 1), (2, 7)]), 'three values': lambda: cases.three_values(9), 'single only': lambda: cases.single_only(9)}


@pytest.mark.parametrize('name', sorted(CASES))
def test_interpreted_programs_match_the_oracle(name):
    spec = CASES[name]()
    x = cases.positions(9, 23)[0]
    ref = oracle.evaluate(spec, x)
    E, F = _interpret(_entry(spec), x, spec.get('exclusions', ()))
    assert abs(E - ref['E']) <= 1e-12 * ref['abs_energy']
    assert np.abs(F - ref['F']).max() <= 1e-11 * max(np.abs(ref['F']).max(), ref['peak'].max())
    if name == 'gbn2-shaped':
        assert len(spec['per_particle']) == 7 and np.any(_entry(spec)['program'][:, 0] == cx.LOOKUP2D)


@pytest.mark.parametrize('name', sorted(CASES))
def test_oracle_forces_are_the_central_differences_of_its_energies(name):
    spec = CASES[name]()
    x = cases.positions(9, 23)[0]
    ref = oracle.evaluate(spec, x)
    h = 1e-5
    for a, c in ((0, 0), (4, 1), (8, 2)):
        xp, xm = x.copy(), x.copy()
        xp[a, c] += h; xm[a, c] -= h
        fd = -(oracle.evaluate(spec, xp)['E'] - oracle.evaluate(spec, xm)['E']) / (2.0 * h)
        assert abs(fd - ref['F'][a, c]) <= 1e-6 * max(np.abs(ref['F']).max(), 1.0)


# ---- the host plan under the sanitizers --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def planner(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    tmp = tmp_path_factory.mktemp('custom_gb_plan')
    exe = str(tmp / 'custom_gb_plan_check')
    subprocess.check_call([cxx, '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           os.path.join(ROOT, 'tools', 'custom_gb_plan_check.cpp'), '-o', exe])

    def arr(f, a, fmt):
        if a is None:
            f.write(struct.pack('<i', -1)); return
        a = np.asarray(a).reshape(-1)
        f.write(struct.pack('<i', len(a)) + struct.pack('<%d%s' % (len(a), fmt), *a.tolist()))

    def run(descs):
        path = tmp / 'cases.bin'
        with open(path, 'wb') as f:
            f.write(struct.pack('<i', len(descs)))
            for facts, e in descs:
                f.write(struct.pack('<4i', facts['N'], facts['Npad'], 1, len(facts.get('boxes', ()))))
                f.write(struct.pack('<%dd' % len(facts.get('boxes', ())), *facts.get('boxes', ())))
                f.write(struct.pack('<10i', len(e['params']), e['params'].shape[1], len(e['program']), len(e['consts']), e['stack_depth'], e['periodic'],
                                    0, e['nb_method'], e['n_values'], len(e['stages'])))
                f.write(struct.pack('<d', e['cutoff']))
                arr(f, e['params'], 'd'); arr(f, e['program'], 'i'); arr(f, e['consts'], 'd')
                arr(f, e['excl_offsets'], 'i'); arr(f, e['excl_atoms'] if len(e['excl_atoms']) else None, 'i'); arr(f, e['stages'], 'i')
        done = subprocess.run([exe, str(path)], capture_output=True, text=True)
        assert done.returncode == 0 and 'ERROR' not in done.stderr and 'runtime error' not in done.stderr, done.stderr[-3000:]
        slices = {int(l.split()[1]): [int(v) for v in l.split()[2:]] for l in done.stdout.splitlines() if l.startswith('SLICES')}
        out, plan = [], None
        for line in done.stdout.splitlines():
            if line.startswith('REFUSED '):
                out.append(line[8:])
            elif line == 'PLAN':
                plan = {}
            elif line == 'END':
                out.append(plan)
            elif plan is not None and not line.startswith('SLICES'):
                name, count, *v = line.split()
                plan[name] = [int(t) for t in v]
        return slices, out
    return run


def test_slices_put_a_wavefront_on_every_compute_unit(planner):
    slices, _ = planner([])
    for N, (nb, s, *borders) in slices.items():
        assert nb == (N + 63) // 64 and 1 <= s <= nb and s == min(nb, -(-64 // nb))
        assert borders[0] == 0 and borders[-1] == nb and all(b > a for a, b in zip(borders, borders[1:]))      # every slice has a column block
    nb, s = slices[2000][:2]
    assert 8 * nb * s >= 256                                   # 8 replicas x 2000 particles on the 256 compute units of an MI355X
    assert slices[130][1] == 3 and slices[65][1] == 2 and slices[22][1] == 1


def test_plan_layout_and_refusals(planner):
    spec = cases.excluded(130, [(0, 1), (63, 64), (5, 129)])
    e = _entry(spec)
    facts = dict(N=130, Npad=192)
    bad_stage = dict(e, stages=e['stages'].copy()); bad_stage['stages'][1, 7] = 5            # a value names a value it cannot know
    bad_column = dict(e, stages=e['stages'].copy()); bad_column['stages'][0, 11] = 16 + 2 * 2  # parameter 2 of a force with two
    bad_program = dict(e, stages=e['stages'].copy()); bad_program['stages'][-1, 5] += 1        # a program past the force's
    bad_excl = dict(e, excl_atoms=np.where(e['excl_atoms'] == 129, 130, e['excl_atoms']))
    periodic = _entry(dict(spec, method=2, cutoff=1.0), box=[2.5, 2.5, 2.5])
    _, out = planner([(facts, e), (dict(N=131, Npad=192), e), (facts, bad_stage), (facts, bad_column), (facts, bad_program), (facts, bad_excl),
                      (dict(facts, boxes=[2.5, 2.5, 1.9]), periodic), (dict(facts, boxes=[2.5, 2.5, 2.0]), periodic), (facts, e)])
    plan = out[0]
    nb, s, nv = 3, 3, 2
    assert plan['force'] == [12, 130, 64 * nb * (s + 1), nv, len(e['stages']), 0, s, 0, 0]
    assert plan['layout'] == [0, s * 192, (s + nv) * 192, (s + 2 * nv) * 192, (s + 2 * nv + s * nv) * 192]
    assert plan['scalars'] == [1, 64 * nb * (s + 1), plan['layout'][-1], nb * (s + 1)] and plan['par'] == [2 * 192]
    assert plan['gb_stages'] == e['stages'].reshape(-1).tolist()
    assert plan['excl_off'] == e['excl_offsets'].tolist() and plan['excl_atoms'] == e['excl_atoms'].tolist()
    assert out[1] == 'force 0: a Generalized-Born force has 130 particles, the system has 131'
    assert out[2] == 'force 0: stage 1: a variable that is not r or a value known to the stage'
    assert out[3] == 'force 0: stage 0: a staged column that is no quantity of the stage'
    assert out[4] == "force 0: stage %d: a program outside the force's" % (len(e['stages']) - 1)
    assert out[5] == 'force 0: exclusion index out of range'
    assert out[6] == 'force 0: box smaller than twice the cutoff'
    assert isinstance(out[7], dict) and out[8] == plan                                          # a refusal leaves nothing behind
