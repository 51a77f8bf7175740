"""CPU: CustomManyParticleForce -- the f64 helper tests/custom_manyparticle_oracle.py held to hand-written closed forms and to
compound_expr_oracle on the explicit list of sets; the class, its descriptor arrays and getters, from_openmm by a duck-typed stand-in,
and every refusal by name."""
import itertools
import math

import numpy as np
import pytest

import custom_manyparticle_oracle as oracle
import compound_expr_oracle
from openmmtools_amd import custom_expr as cx, system as sysmod, testsystems, unit
from openmmtools_amd.system import System, system_to_desc, CustomManyParticleForce, Discrete1DFunction

SP, UCP = CustomManyParticleForce.SinglePermutation, CustomManyParticleForce.UniqueCentralParticle
SW = 'lam*eps*(cos(angle(p2,p1,p3))+1/3)^2*exp(g*s/(distance(p1,p2)-a*s))*exp(g*s/(distance(p1,p3)-a*s)); lam=23.15; eps=25.9; g=1.2; s=0.24; a=1.8'
AT = 'nu*(1+3*cos(angle(p2,p1,p3))*cos(angle(p1,p2,p3))*cos(angle(p1,p3,p2)))/(distance(p1,p2)*distance(p2,p3)*distance(p1,p3))^3'


def _force(energy, n, mode=SP, params=(), values=None, types=None, method=0, cutoff=1.0):
    f = CustomManyParticleForce(3, energy)
    for name in params:
        f.addPerParticleParameter(name)
    for k in range(n):
        f.addParticle([] if values is None else values[k], 0 if types is None else int(types[k]))
    f.setPermutationMode(mode)
    f.setNonbondedMethod(method)
    f.setCutoffDistance(cutoff)
    return f


def _system(n, forces, box=None):
    s = System()
    for _ in range(n):
        s.addParticle(12.0)
    if box is not None:
        s.setDefaultPeriodicBoxVectors([box[0], 0, 0], [0, box[1], 0], [0, 0, box[2]])
    for f in forces:
        s.addForce(f)
    return s


# ---- the oracle against closed forms -------------------------------------------------------------------------------------------------------------
def sw_closed(x, i, j, k, lam=23.15, eps=25.9, g=1.2, s=0.24, a=1.8):
    """Stillinger-Weber's three-body term with central particle i, written out by hand"""
    u, v = x[j] - x[i], x[k] - x[i]
    ru, rv = np.linalg.norm(u), np.linalg.norm(v)
    if ru >= a * s or rv >= a * s:
        return 0.0
    c = u @ v / (ru * rv)
    return lam * eps * (c + 1.0 / 3.0) ** 2 * math.exp(g * s / (ru - a * s)) * math.exp(g * s / (rv - a * s))


def at_closed(x, i, j, k, nu):
    """Axilrod-Teller: nu (1 + 3 cos a cos b cos c) / (r_ij r_jk r_ik)^3"""
    rij, rik, rjk = x[j] - x[i], x[k] - x[i], x[k] - x[j]
    dij, dik, djk = np.linalg.norm(rij), np.linalg.norm(rik), np.linalg.norm(rjk)
    ci, cj, ck = rij @ rik / (dij * dik), -rij @ rjk / (dij * djk), rik @ rjk / (dik * djk)
    return nu * (1.0 + 3.0 * ci * cj * ck) / (dij * dik * djk) ** 3


def _central_gradient(fun, x, h=1e-6):
    g = np.zeros_like(x)
    for a in range(x.shape[0]):
        for c in range(3):
            p, m = x.copy(), x.copy()
            p[a, c] += h; m[a, c] -= h
            g[a, c] = (fun(p) - fun(m)) / (2.0 * h)
    return g


def test_the_oracle_is_stillinger_weber_s_closed_form_with_its_gradient():
    rng = np.random.default_rng(41)
    x = np.array([[a, b, c] for a in range(2) for b in range(2) for c in range(2)], dtype=np.float64) * 0.3 + rng.uniform(-0.04, 0.04, (8, 3))
    cutoff = 1.8 * 0.24
    ref = oracle.evaluate(SW, [], np.zeros((8, 0)), np.zeros(8, int), None, {}, x, None, oracle.CUTOFF_NON_PERIODIC, cutoff, (), UCP)
    assert oracle.clear_of_cutoff(ref, cutoff, 1e-6)

    def total(y):
        return sum(sw_closed(y, i, j, k) for i in range(8) for j, k in itertools.combinations([q for q in range(8) if q != i], 2))
    assert len(ref['E']) > 20
    assert ref['E'].sum() == pytest.approx(total(x), rel=1e-13)
    assert np.allclose(ref['F'], -_central_gradient(total, x), rtol=1e-6, atol=1e-6 * np.abs(ref['F']).max())


def test_the_oracle_is_axilrod_teller_s_closed_form_with_its_gradient():
    rng = np.random.default_rng(42)
    x = rng.uniform(0.0, 0.8, (6, 3))
    ref = oracle.evaluate(AT, [], np.zeros((6, 0)), np.zeros(6, int), None, dict(nu=0.003), x, None, oracle.NO_CUTOFF, 0.0, (), SP)

    def total(y):
        return sum(at_closed(y, i, j, k, 0.003) for i, j, k in itertools.combinations(range(6), 3))
    assert len(ref['E']) == 20
    assert ref['E'].sum() == pytest.approx(total(x), rel=1e-13)
    assert np.allclose(ref['F'], -_central_gradient(total, x), rtol=1e-6, atol=1e-6 * np.abs(ref['F']).max())


def test_the_oracle_is_the_compound_bond_oracle_on_the_explicit_list_of_sets():
    rng = np.random.default_rng(43)
    N = 7
    x = rng.uniform(0.0, 0.9, (N, 3))
    q = rng.uniform(0.5, 1.5, (N, 1))
    energy = 'k*q1*q2*q3*(distance(p1,p2)-0.3)^2*(1+cos(angle(p2,p1,p3)))+0.1*q1*distance(p2,p3)'
    for mode in (SP, UCP):
        ref = oracle.evaluate(energy, ['q'], q, np.zeros(N, int), None, dict(k=3.0), x, None, oracle.NO_CUTOFF, 0.0, ((0, 4),), mode)
        if mode == SP:
            sets = [s for s in itertools.combinations(range(N), 3) if not {0, 4} <= set(s)]
        else:
            sets = [(i, j, k) for i in range(N) for j, k in itertools.combinations([a for a in range(N) if a != i], 2) if not {0, 4} <= {i, j, k}]
        assert sorted(map(tuple, ref['sets'].tolist())) == sorted(sets)
        params = np.array([[q[a, 0] for a in s] for s in ref['sets']])
        E, F = compound_expr_oracle.evaluate(3, energy, ref['sets'], ['q1', 'q2', 'q3'], params, dict(k=3.0), x)
        assert np.allclose(ref['E'], E, rtol=1e-12, atol=1e-14) and np.allclose(ref['F'], F, rtol=1e-10, atol=1e-12)


def test_set_counts_without_a_cutoff():
    x = np.random.default_rng(44).uniform(0.0, 1.0, (9, 3))
    for mode, count in ((SP, math.comb(9, 3)), (UCP, 3 * math.comb(9, 3))):
        sets, _ = oracle.enumerate_sets(x, np.zeros(9, int), None, mode=mode)
        assert len(sets) == count and len({tuple(s) for s in sets.tolist()}) == count


def test_the_filter_assignment_rule_on_a_two_type_example_by_hand():
    """particles 0 1 2 3 of types A B A B (0 1 0 1), filters (A, B, any).  SinglePermutation: {0,1,2}: (0,1,2) passes first.  {0,1,3}:
    (0,1,3).  {0,2,3}: (0,2,3) fails (p2 = 2 is A), (0,3,2) passes.  {1,2,3}: (1,..) fails (p1 is B), (2,1,3) passes.
    UniqueCentralParticle: only 0 and 2 may be central; for central 0: {1,2}: (0,1,2); {1,3}: (0,1,3); {2,3}: (0,3,2); for central 2: {0,1}:
    (2,0,1) fails, (2,1,0) passes; {0,3}: (2,3,0); {1,3}: (2,1,3)."""
    x = np.random.default_rng(45).uniform(0.0, 1.0, (4, 3))
    filters = ([0], [1], [])
    sets, _ = oracle.enumerate_sets(x, [0, 1, 0, 1], filters, mode=SP)
    assert sets.tolist() == [[0, 1, 2], [0, 1, 3], [0, 3, 2], [2, 1, 3]]
    sets, _ = oracle.enumerate_sets(x, [0, 1, 0, 1], filters, mode=UCP)
    assert sets.tolist() == [[0, 1, 2], [0, 1, 3], [0, 3, 2], [2, 1, 0], [2, 1, 3], [2, 3, 0]]


def test_the_cutoff_rule_of_the_two_modes_and_the_decisive_distances():
    x = np.array([[0.0, 0.0, 0.0], [0.4, 0.0, 0.0], [-0.4, 0.0, 0.0], [5.0, 0.0, 0.0]])
    sets, r_all = oracle.enumerate_sets(x, np.zeros(4, int), None, None, oracle.CUTOFF_NON_PERIODIC, 0.5, (), SP)
    assert len(sets) == 0 and len(r_all) == 6
    sets, _ = oracle.enumerate_sets(x, np.zeros(4, int), None, None, oracle.CUTOFF_NON_PERIODIC, 0.5, (), UCP)
    assert sets.tolist() == [[0, 1, 2]]
    assert not oracle.clear_of_cutoff(dict(r_all=np.array([0.3, 0.5 + 5e-7])), 0.5, 1e-6)
    y = x + [0.9, 0, 0]
    y[1, 0] -= 1.6                                                         # particle 1 has left through the x face
    y[3] = [0.9, 4.5, 0.0]
    sets, _ = oracle.enumerate_sets(y, np.zeros(4, int), None, [1.6, 9.0, 9.0], oracle.CUTOFF_PERIODIC, 0.5, (), UCP)
    assert sets.tolist() == [[0, 1, 2]] and abs(y[1, 0] - y[0, 0]) > 1.0


# ---- the class and its descriptor ----------------------------------------------------------------------------------------------------------------
def test_getters_defaults_and_descriptor_arrays():
    f = CustomManyParticleForce(3, 'c*sig1*sig2*eps3*distance(p1,p2)*tab(ty3)+0*angle(p1,p2,p3)')
    assert (f.getNumParticlesPerSet(), f.getNonbondedMethod(), f.getCutoffDistance(), f.getPermutationMode()) == (3, 0, 1.0, SP)
    assert f.addPerParticleParameter('sig') == 0 and f.addPerParticleParameter('eps') == 1 and f.addPerParticleParameter('ty') == 2
    assert f.addGlobalParameter('c', 2.0) == 0
    f.addTabulatedFunction('tab', Discrete1DFunction([1.0, 2.0]))
    for k in range(5):
        assert f.addParticle([0.1 * k, 1.0 + k, k % 2], k % 2) == k
    f.setParticleParameters(4, [9.0, 8.0, 1.0], 3)
    assert f.getParticleParameters(4) == ([9.0, 8.0, 1.0], 3) and f.getNumParticles() == 5
    f.addExclusion(3, 1); f.addExclusion(0, 4)
    assert f.getNumExclusions() == 2 and f.getExclusionParticles(0) == (3, 1)
    f.setNonbondedMethod(CustomManyParticleForce.CutoffPeriodic); f.setCutoffDistance(0.7); f.setPermutationMode(UCP)
    f.setTypeFilter(0, [3, 0]); f.setTypeFilter(2, [1])
    assert f.getTypeFilter(0) == [0, 3] and f.getTypeFilter(1) == [] and f.usesPeriodicBoundaryConditions()
    f.setForceGroup(5)
    assert (f.getNumPerParticleParameters(), f.getPerParticleParameterName(1), f.getNumGlobalParameters(), f.getNumTabulatedFunctions()) == (3, 'eps', 1, 1)
    t = system_to_desc(_system(5, [f], [2.0, 2.0, 2.0]))['custom_terms']['000']
    assert t['kind'] == cx.KIND_MANYPARTICLE == 11 and t['nb_method'] == 2 and t['periodic'] == 1 and t['cutoff'] == 0.7 and t['force_group'] == 5
    assert t['permutation_mode'] == 1 and t['types'].tolist() == [0, 1, 0, 1, 3] and t['particle_mask'] == 0b111
    assert t['filters'].tolist() == [0b1001, 0xFFFFFFFF, 0b10]
    assert t['params'].shape == (5, 3) and t['params'][4].tolist() == [9.0, 8.0, 1.0]
    assert t['excl_offsets'].tolist() == [0, 1, 2, 2, 3, 4] and t['excl_atoms'].tolist() == [4, 3, 1, 0]
    # operand 3 q + s: sig1 -> 0, sig2 -> 1, eps3 -> 5, ty3 -> 8
    assert [a for op, a in t['program'].tolist() if op == cx.PARAM] == [0, 1, 5, 8]
    only = CustomManyParticleForce(3, 'distance(p1,p3)')
    for _ in range(3):
        only.addParticle()
    assert system_to_desc(_system(3, [only]))['custom_terms']['000']['particle_mask'] == 0b101


def test_create_exclusions_from_bonds():
    f = _force('distance(p1,p2)+distance(p2,p3)', 5)
    f.createExclusionsFromBonds([(0, 1), (1, 2), (3, 4)], 2)
    assert sorted(f.getExclusionParticles(k) for k in range(f.getNumExclusions())) == [(0, 1), (0, 2), (1, 2), (3, 4)]


class _StandIn:
    """what manyparticle_force_from_openmm asks of an openmm.CustomManyParticleForce"""
    def getNumParticlesPerSet(self): return 3
    def getEnergyFunction(self): return 'k*s1*distance(p1,p2)*angle(p1,p2,p3)'
    def getNumPerParticleParameters(self): return 1
    def getPerParticleParameterName(self, i): return 's'
    def getNumGlobalParameters(self): return 1
    def getGlobalParameterName(self, i): return 'k'
    def getGlobalParameterDefaultValue(self, i): return 2.5
    def getNumTabulatedFunctions(self): return 0
    def getNumParticles(self): return 4
    def getParticleParameters(self, i): return ([0.5 + i], i % 2)
    def getNumExclusions(self): return 1
    def getExclusionParticles(self, i): return (2, 0)
    def getNonbondedMethod(self): return 1
    def getCutoffDistance(self): return 8.0 * unit.angstroms
    def getPermutationMode(self): return 1
    def getTypeFilter(self, i): return [[1], [], [0, 1]][i]
    def getForceGroup(self): return 4


def test_from_openmm_by_a_stand_in():
    g = sysmod.manyparticle_force_from_openmm(_StandIn())
    assert isinstance(g, CustomManyParticleForce) and g.getEnergyFunction() == 'k*s1*distance(p1,p2)*angle(p1,p2,p3)'
    assert (g.getNumParticles(), g.getParticleParameters(3), g.getExclusionParticles(0)) == (4, ([3.5], 1), (2, 0))
    assert (g.getNonbondedMethod(), g.getPermutationMode(), g.getForceGroup()) == (1, 1, 4) and g.getCutoffDistance() == pytest.approx(0.8, rel=1e-14)
    assert [g.getTypeFilter(s) for s in range(3)] == [[1], [], [0, 1]] and g.getGlobalParameterDefaultValue(0) == 2.5
    import inspect
    assert "'CustomManyParticleForce'" in inspect.getsource(sysmod.from_openmm)


def test_the_stillinger_weber_fluid():
    ts = testsystems.StillingerWeberFluid(nparticles=64)
    two, three = ts.system.getForces()
    assert type(two).__name__ == 'CustomNonbondedForce' and isinstance(three, CustomManyParticleForce)
    assert three.getPermutationMode() == UCP and three.getCutoffDistance() == pytest.approx(1.8 * 0.23925) == two.getCutoffDistance()
    assert 'not one of the reference' in testsystems.StillingerWeberFluid.__doc__.lower()
    box = np.diag(ts.system.getDefaultPeriodicBoxVectors())
    assert 64 / np.prod(box) == pytest.approx(33.4, rel=1e-6) and ts.positions.shape == (64, 3)
    terms = system_to_desc(ts.system, box=box)['custom_terms']
    assert [terms[k]['kind'] for k in sorted(terms)] == [6, 11]
    with pytest.raises(ValueError, match='cube'):
        testsystems.StillingerWeberFluid(nparticles=100)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------
def _desc(f, n, box=None):
    return system_to_desc(_system(n, [f], box))


def test_bad_input_raises_value_error():
    f = _force('distance(p1,p2)+s1', 4, params=['s'], values=[[1.0]] * 4)
    f.setParticleParameters(2, [1.0, 2.0], 0)
    with pytest.raises(ValueError, match='particle 2 carries 2 parameters, the force declares 1'):
        _desc(f, 4)
    with pytest.raises(ValueError, match=r'particle type 32 \(the types are 0 ... 31\)'):
        _force('distance(p1,p2)', 1).addParticle([], 32)
    with pytest.raises(ValueError, match='particle type -1'):
        _force('distance(p1,p2)', 1).setParticleParameters(0, [], -1)
    for index in (-1, 3):
        with pytest.raises(ValueError, match=r'type filter index %d \(the particles of a set are 0 ... 2\)' % index):
            _force('distance(p1,p2)', 3).setTypeFilter(index, [0])
    with pytest.raises(ValueError, match='type filter 1 names type 40'):
        _force('distance(p1,p2)', 3).setTypeFilter(1, [40])
    f = _force('distance(p1,p2)', 4); f.addExclusion(1, 4)
    with pytest.raises(ValueError, match=r'exclusion 0 names particle 4 \(the force has 4\)'):
        _desc(f, 4)
    f = _force('distance(p1,p2)', 4); f.addExclusion(1, 2); f.addExclusion(2, 1)
    with pytest.raises(ValueError, match='particles 2 and 1 are excluded twice'):
        _desc(f, 4)
    f = _force('distance(p1,p2)', 4); f.addExclusion(3, 3)
    with pytest.raises(ValueError, match='exclusion 0 excludes particle 3 from itself'):
        _desc(f, 4)
    with pytest.raises(ValueError, match='has 4 particles, the System has 5'):
        _desc(_force('distance(p1,p2)', 4), 5)
    f = _force('distance(p1,p2)', 4, method=2, cutoff=1.01)
    with pytest.raises(ValueError, match='the cutoff 1.01 nm exceeds half the smallest box edge'):
        _desc(f, 4, [3.0, 2.0, 3.0])
    with pytest.raises(ValueError, match='permutation mode 2'):
        _force('distance(p1,p2)', 1).setPermutationMode(2)
    with pytest.raises(ValueError, match='nonbonded method 3'):
        _force('distance(p1,p2)', 1).setNonbondedMethod(3)


@pytest.mark.parametrize('energy, sentence', [
    ('x1+distance(p1,p2)', "variable 'x1' (raw coordinates are not variables of this force"),
    ('z3*distance(p1,p2)', "variable 'z3' (raw coordinates"),
    ('distance(p1,p4)', "the arguments of 'distance' are particle names among p1 p2 p3, not 'p4'"),
    ('distance(p1,p2)*s', "per-particle parameter 's' without a particle suffix (s1, s2 or s3)"),
    ('distance(p1,p2)*s4', "unknown variable 's4'"),
    ('distance(p1,p2)*q', "unknown variable 'q'"),
    ('p1*distance(p1,p2)', "particle name 'p1' outside distance(), angle() and dihedral()"),
    ('pointdistance(0,0,0,1,1,1)', "function 'pointdistance' (pointdistance, pointangle and pointdihedral are not functions of this force)"),
    ('pointangle(0,0,0,1,1,1,2,2,2)', "function 'pointangle'"),
    ('pointdihedral(0,0,0,1,1,1,2,2,2,3,3,3)', "function 'pointdihedral'"),
    ('nosuch(distance(p1,p2))', "unknown function 'nosuch'"),
])
def test_names_the_expression_may_not_use(energy, sentence):
    f = _force(energy, 3, params=['s'], values=[[1.0]] * 3)
    with pytest.raises(NotImplementedError) as e:
        _desc(f, 3)
    assert sentence in str(e.value)


def test_unbuilt_ground_raises_not_implemented():
    for per_set in (2, 4):
        with pytest.raises(NotImplementedError, match=r'sets of %d particles \(sets of 3 particles are supported\)' % per_set):
            CustomManyParticleForce(per_set, 'distance(p1,p2)')
    names = ['a', 'b', 'c', 'd', 'e', 'f']
    f = _force('distance(p1,p2)', 3, params=names, values=[[0.0] * 6] * 3)
    with pytest.raises(NotImplementedError, match=r'6 per-particle parameters \(the engine takes 5'):
        _desc(f, 3)
    with pytest.raises(NotImplementedError, match=r'NoCutoff with 130 particles \(a neighbour row holds 128 particles, so NoCutoff takes at most 129'):
        _desc(_force('distance(p1,p2)', 130), 130)
    _desc(_force('distance(p1,p2)', 129), 129)
    f = _force('distance(p1,p2)', 4, method=2, cutoff=0.5)
    s = _system(4, [f])
    s.setDefaultPeriodicBoxVectors([2.0, 0, 0], [0.5, 2.0, 0], [0, 0, 2.0])
    with pytest.raises(NotImplementedError, match='triclinic boxes are not supported'):
        system_to_desc(s)
    with pytest.raises(NotImplementedError, match='changing particles, exclusions or filters after set_system'):
        _force('distance(p1,p2)', 3).updateParametersInContext()


def test_the_alchemical_factory_refuses_such_a_system():
    from openmmtools_amd import alchemy
    system = _system(4, [_force('distance(p1,p2)*angle(p1,p2,p3)', 4)])
    with pytest.raises(NotImplementedError, match='the alchemical modification of a CustomManyParticleForce is not supported'):
        alchemy.AbsoluteAlchemicalFactory().create_alchemical_system(system, alchemy.AlchemicalRegion(alchemical_atoms=[0]))


def test_the_engine_pool_the_xml_writer_the_netcdf4_layout_and_the_cpu_port_refuse_it():
    import types
    from openmmtools_amd import _engine, states, system_xml
    from openmmtools_amd.multistate import _engine_pool
    from openmmtools_amd.multistate._reference_store import ReferenceStoreWriter
    s = _system(4, [_force('distance(p1,p2)*angle(p1,p2,p3)', 4)])
    with pytest.raises(NotImplementedError, match='CustomManyParticleForce'):
        system_xml.to_xml(s)
    why = ReferenceStoreWriter.can_store([states.ThermodynamicState(s, 300.0 * unit.kelvin)], [], [])
    assert why is not None and 'CustomManyParticleForce' in why and 'distance(p1,p2)*angle(p1,p2,p3)' in why     # layout='auto' then keeps records
    pool = _engine_pool.EnginePool.__new__(_engine_pool.EnginePool)
    pool.G = 2
    with pytest.raises(NotImplementedError, match='many-particle forces.*more than one compatibility group'):
        pool.set_system([system_to_desc(s), system_to_desc(s)])
    # the CPU port of the ABI exports none of include/remd_hip_custom.h: an engine on such a library names the header and the kind
    d = system_to_desc(s)
    eng = object.__new__(_engine.HipEngine)
    eng.lib, eng.h = types.SimpleNamespace(), None
    for call in (lambda: eng.set_custom_terms([d['custom_terms']['000']]), lambda: eng.set_custom_globals(np.zeros((1, 0))),
                 lambda: eng.custom_energies()):
        with pytest.raises(NotImplementedError, match='many-particle forces.*remd_hip_custom.h is GPU-only'):
            call()


def test_what_decides_these_refusals_names_the_class():
    """the XML writer and the netCDF4 layout ask custom_expr.is_custom_term_force; the pool and the engine ask for the 'custom_terms' of
    the description: both must keep answering for this class"""
    f = _force('distance(p1,p2)', 3)
    assert cx.is_custom_term_force(f) and cx.KIND_OF_CLASS['CustomManyParticleForce'] == cx.KIND_MANYPARTICLE
    assert list(system_to_desc(_system(3, [f]))['custom_terms']) == ['000']
