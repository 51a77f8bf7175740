"""CPU: system.CustomHbondForce -- the API, the compiler (custom_expr.py kind 10), system_to_desc, every refusal by its message, the
alchemical factory, the store layouts, the openmm converter on a stand-in object, and the oracle of the GPU tests
(tests/custom_hbond_oracle.py) held to finite differences of its own energy and to a closed form in plain numpy."""
import math

import numpy as np
import pytest

import custom_hbond_oracle as oracle
from openmmtools_amd import alchemy, custom_expr as cx, states, unit
from openmmtools_amd.system import (System, system_to_desc, CustomHbondForce, NonbondedForce, Discrete1DFunction, hbond_force_from_openmm)

REFERENCE = 'k*(distance(d1,a1)-r0)^2*(1+cos(angle(d2,d1,a1)))^2*step(rc-distance(d1,a1))'


def _system(n, forces, box=None):
    s = System()
    for _ in range(n):
        s.addParticle(12.0)
    if box is not None:
        s.setDefaultPeriodicBoxVectors([box[0], 0, 0], [0, box[1], 0], [0, 0, box[2]])
    for f in forces:
        s.addForce(f)
    return s


def _reference_force():
    f = CustomHbondForce(REFERENCE)
    f.addPerDonorParameter('k')
    f.addPerAcceptorParameter('r0')
    f.addGlobalParameter('rc', 0.5)
    f.addDonor(0, 1, -1, [2.0]); f.addDonor(2, 3, -1, [3.0])
    f.addAcceptor(4, -1, -1, [0.3]); f.addAcceptor(5, 6, 7, [0.31]); f.addAcceptor(1, -1, -1, [0.32])
    f.addExclusion(1, 1); f.addExclusion(0, 2)
    return f


# ---- the API ------------------------------------------------------------------------------------------------------------------------------------
def test_the_api_round_trips():
    f = _reference_force()
    assert (f.getNumDonors(), f.getNumAcceptors(), f.getNumExclusions()) == (2, 3, 2)
    assert (f.getNumPerDonorParameters(), f.getPerDonorParameterName(0)) == (1, 'k')
    assert (f.getNumPerAcceptorParameters(), f.getPerAcceptorParameterName(0)) == (1, 'r0')
    assert (f.getNumGlobalParameters(), f.getGlobalParameterName(0), f.getGlobalParameterDefaultValue(0)) == (1, 'rc', 0.5)
    f.setGlobalParameterDefaultValue(0, 0.6)
    assert f.getGlobalParameterDefaultValue(0) == 0.6
    assert f.getDonorParameters(1) == (2, 3, -1, [3.0]) and f.getAcceptorParameters(1) == (5, 6, 7, [0.31])
    f.setDonorParameters(1, 3, 2, -1, [4.0]); f.setAcceptorParameters(0, 4, 6, -1, [0.2])
    assert f.getDonorParameters(1) == (3, 2, -1, [4.0]) and f.getAcceptorParameters(0) == (4, 6, -1, [0.2])
    assert f.getExclusionParticles(0) == (1, 1)
    f.setExclusionParticles(0, 1, 0)
    assert f.getExclusionParticles(0) == (1, 0)
    assert (f.getNonbondedMethod(), f.getCutoffDistance(), f.usesPeriodicBoundaryConditions()) == (0, 1.0, False)
    assert (CustomHbondForce.NoCutoff, CustomHbondForce.CutoffNonPeriodic, CustomHbondForce.CutoffPeriodic) == (0, 1, 2)
    f.setNonbondedMethod(CustomHbondForce.CutoffPeriodic); f.setCutoffDistance(0.8)
    assert (f.getNonbondedMethod(), f.getCutoffDistance(), f.usesPeriodicBoundaryConditions()) == (2, 0.8, True)
    with pytest.raises(ValueError, match='CustomHbondForce: nonbonded method 3'):
        f.setNonbondedMethod(3)
    f.setEnergyFunction('distance(d1,a1)')
    assert f.getEnergyFunction() == 'distance(d1,a1)'
    assert f.addTabulatedFunction('t', Discrete1DFunction([1.0, 2.0])) == 0 and f.getNumTabulatedFunctions() == 1 and f.getTabulatedFunctionName(0) == 't'
    assert f.addDonor(6, -1, -1, [1.0]) == 2 and f.addAcceptor(7, -1, -1, [1.0]) == 3 and f.addExclusion(2, 3) == 2


# ---- the compiler and the descriptor ------------------------------------------------------------------------------------------------------------
def test_the_compiled_program_of_the_reference_expression():
    p = cx.compile_expression(REFERENCE, (), ['k', 'r0'], {'rc': 0}, particle_slots=cx.HBOND_SLOTS)
    D, A = cx.DISTANCE, cx.ANGLE
    assert p['program'].tolist() == [[cx.PARAM, 0], [D, 0 | 3 << 4], [cx.PARAM, 1], [cx.SUB, 0], [cx.POWI, 2], [cx.MUL, 0], [cx.CONST, 0],
                                     [A, 1 | 0 << 4 | 3 << 8], [cx.COS, 0], [cx.ADD, 0], [cx.POWI, 2], [cx.MUL, 0], [cx.GLOBAL, 0], [D, 0 | 3 << 4],
                                     [cx.SUB, 0], [cx.STEP, 0], [cx.MUL, 0]]
    assert p['consts'].tolist() == [1.0] and p['stack_depth'] == 3
    assert p['particle_mask'] == 0b001011                                 # d1, d2, a1: three seeded passes
    q = cx.compile_expression('dihedral(d3,d2,a2,a3) + s; s = 2*qa + 3*pd', (), ['pd', 'qa'], {}, particle_slots=cx.HBOND_SLOTS)
    assert q['particle_mask'] == 0b110110 and [cx.DIHEDRAL, 2 | 1 << 4 | 4 << 8 | 5 << 12] in q['program'].tolist()
    assert [cx.PARAM, 1] in q['program'].tolist() and [cx.PARAM, 0] in q['program'].tolist()
    assert cx.compile_expression('2*pd', (), ['pd'], {}, particle_slots=cx.HBOND_SLOTS)['particle_mask'] == 0


def test_system_to_desc_emits_the_force_as_kind_10():
    f = _reference_force()
    f.setNonbondedMethod(CustomHbondForce.CutoffNonPeriodic); f.setCutoffDistance(0.7); f.setForceGroup(4)
    d = system_to_desc(_system(8, [f]))
    t = d['custom_terms']['000']
    assert t['kind'] == cx.KIND_HBOND == 10 and t['atoms'].shape == (0, 0) and (t['nb_method'], t['cutoff'], t['periodic'], t['force_group']) == (1, 0.7, 0, 4)
    assert t['donor_atoms'].tolist() == [[0, 1, -1], [2, 3, -1]] and t['acceptor_atoms'].tolist() == [[4, -1, -1], [5, 6, 7], [1, -1, -1]]
    assert t['donor_params'].tolist() == [[2.0], [3.0]] and t['acceptor_params'].tolist() == [[0.3], [0.31], [0.32]]
    assert t['hb_excl_offsets'].tolist() == [0, 1, 2] and t['hb_excl_acceptors'].tolist() == [2, 1]
    assert t['particle_mask'] == 0b001011 and t['global_names'] == ['rc'] and d['custom_globals']['names'] == ['rc']
    f.setNonbondedMethod(0)
    assert system_to_desc(_system(8, [f]))['custom_terms']['000']['cutoff'] == 0.0
    # an empty force is legal and emits nothing; it counts among the 8 custom forces and the 16 global columns otherwise
    assert 'custom_terms' not in system_to_desc(_system(8, [CustomHbondForce('distance(d1,a1)')]))
    with pytest.raises(NotImplementedError, match='9 custom forces'):
        system_to_desc(_system(8, [_reference_force() for _ in range(9)]))
    g = _reference_force()
    g.setForceGroup(1)
    with pytest.raises(NotImplementedError, match='several force groups'):
        system_to_desc(_system(8, [_reference_force(), g]))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def _refused(kind, match, build, n=8, box=None):
    f = _reference_force()
    build(f)
    with pytest.raises(kind, match=match):
        system_to_desc(_system(n, [f], box))


def test_refusals_of_expressions():
    for text, match in (('distance(d1,a3)', r"names a3, which acceptor 0 does not have"),
                        ('angle(d3,d1,a1)', r"names d3, which donor 0 does not have"),
                        ('x1 + distance(d1,a1)', r"CustomHbondForce \(energy .*unknown variable 'x1'"),
                        ('distance(p1,a1)', r"CustomHbondForce.*particle names among d1 d2 d3 a1 a2 a3, not 'p1'"),
                        ('distance(d1,g1)', r"not 'g1'"),
                        ('r + distance(d1,a1)', r"unknown variable 'r'"),
                        ('d1 + distance(d1,a1)', r"particle name 'd1' outside distance\(\), angle\(\) and dihedral\(\)"),
                        ('pointdistance(0,0,0,1,1,1)', r"CustomHbondForce.*function 'pointdistance'"),
                        ('pointangle(0,0,0,1,1,1,2,2,2)', r"function 'pointangle'"),
                        ('pointdihedral(0,0,0,1,1,1,2,2,2,3,3,3)', r"function 'pointdihedral'"),
                        ('distance(d1)', r"function 'distance' takes 2 particles, not 1")):
        kind = ValueError if 'does not have' in match else NotImplementedError
        _refused(kind, match, lambda f, text=text: f.setEnergyFunction(text))


def test_refusals_of_donors_acceptors_and_exclusions():
    _refused(ValueError, r'CustomHbondForce: donor 2 has no first particle \(d1 = -1\)', lambda f: f.addDonor(-1, 6, -1, [1.0]))
    _refused(ValueError, r'CustomHbondForce: acceptor 3 has no first particle \(a1 = -1\)', lambda f: f.addAcceptor(-1, 6, -1, [1.0]))
    _refused(ValueError, r'CustomHbondForce: donor 2 names particle 8 \(the System has 8\)', lambda f: f.addDonor(6, 8, -1, [1.0]))
    _refused(ValueError, r'CustomHbondForce: acceptor 3 names particle -2', lambda f: f.addAcceptor(6, -2, -1, [1.0]))
    _refused(ValueError, r'CustomHbondForce: donor 2 names particle 6 twice', lambda f: f.addDonor(6, 6, -1, [1.0]))
    _refused(ValueError, r'CustomHbondForce: donor 2 carries 0 parameters, the force declares 1', lambda f: f.addDonor(6, 7, -1))
    _refused(ValueError, r'donor 2 and acceptor 0 share particle 4 and are not excluded: add the exclusion \(addExclusion\(2, 0\)\)',
             lambda f: f.addDonor(8, 4, -1, [1.0]), n=10)
    _refused(ValueError, r'CustomHbondForce: exclusion 2 names donor 2 \(the force has 2\)', lambda f: f.addExclusion(2, 0))
    _refused(ValueError, r'CustomHbondForce: exclusion 2 names acceptor 3 \(the force has 3\)', lambda f: f.addExclusion(0, 3))
    _refused(ValueError, r'CustomHbondForce: donor 1 and acceptor 1 are excluded twice', lambda f: f.addExclusion(1, 1))

    def many(f):
        for k in range(8):
            f.addPerDonorParameter('pd%d' % k); f.addPerAcceptorParameter('pa%d' % k)
    _refused(NotImplementedError, r'CustomHbondForce: 9 per-donor and 9 per-acceptor parameters \(the engine takes 16 together\)', many)
    only_donors = CustomHbondForce('distance(d1,a1)')
    only_donors.addDonor(0, -1, -1)
    with pytest.raises(ValueError, match=r'1 donors and 0 acceptors: a force with donors but no acceptors'):
        system_to_desc(_system(8, [only_donors]))
    only_acceptors = CustomHbondForce('distance(d1,a1)')
    only_acceptors.addAcceptor(0, -1, -1)
    with pytest.raises(ValueError, match=r'0 donors and 1 acceptors: a force with acceptors but no donors'):
        system_to_desc(_system(8, [only_acceptors]))
    with pytest.raises(NotImplementedError, match='CustomHbondForce: changing donors, acceptors or exclusions after set_system'):
        _reference_force().updateParametersInContext()
    with pytest.raises(ValueError, match='CustomHbondForce: periodic boundary conditions follow the nonbonded method'):
        _reference_force().setUsesPeriodicBoundaryConditions(True)


def test_refusals_of_the_periodic_method():
    def periodic(cutoff):
        def build(f):
            f.setNonbondedMethod(CustomHbondForce.CutoffPeriodic); f.setCutoffDistance(cutoff)
        return build
    _refused(ValueError, r'CustomHbondForce: the cutoff 1.6 nm exceeds half the smallest box edge \(3.0 nm\)', periodic(1.6), box=(3.0, 3.5, 4.0))
    f = _reference_force()
    periodic(1.0)(f)
    s = _system(8, [f], (3.0, 3.0, 3.0))
    s.setDefaultPeriodicBoxVectors([3.0, 0, 0], [0.5, 3.0, 0], [0, 0, 3.0])
    with pytest.raises(NotImplementedError, match='CustomHbondForce: triclinic boxes are not supported'):
        system_to_desc(s)
    # a donor whose atoms lie in different molecules of a System with a NonbondedForce: the barostat would tear it
    nb = NonbondedForce()
    for _ in range(8):
        nb.addParticle(0.0, 0.3, 0.1)
    nb.setNonbondedMethod(NonbondedForce.CutoffPeriodic); nb.setCutoffDistance(1.0)
    nb.addException(2, 3, 0.0, 0.3, 0.0); nb.addException(5, 6, 0.0, 0.3, 0.0); nb.addException(6, 7, 0.0, 0.3, 0.0)
    with pytest.raises(NotImplementedError, match=r'CustomHbondForce \(energy .*donor 0 \(particles \[0, 1\]\) spans 2 molecules under CutoffPeriodic'):
        system_to_desc(_system(8, [f, nb], (3.0, 3.0, 3.0)))
    nb.addException(0, 1, 0.0, 0.3, 0.0)
    assert system_to_desc(_system(8, [f, nb], (3.0, 3.0, 3.0)))['custom_terms']['000']['periodic'] == 1


def test_the_engine_pool_the_xml_writer_and_the_netcdf4_layout_refuse_it():
    from openmmtools_amd import system_xml
    from openmmtools_amd.multistate import _engine_pool
    from openmmtools_amd.multistate._reference_store import ReferenceStoreWriter
    s = _system(8, [_reference_force()])
    with pytest.raises(NotImplementedError, match='CustomHbondForce'):
        system_xml.to_xml(s)
    why = ReferenceStoreWriter.can_store([states.ThermodynamicState(s, 300.0 * unit.kelvin)], [], [])
    assert why is not None and 'CustomHbondForce' in why and 'distance(d1,a1)' in why          # layout='auto' then keeps records
    pool = _engine_pool.EnginePool.__new__(_engine_pool.EnginePool)
    pool.G = 2
    with pytest.raises(NotImplementedError, match='more than one compatibility group'):
        pool.set_system([system_to_desc(s), system_to_desc(s)])


# ---- the alchemical factory ---------------------------------------------------------------------------------------------------------------------
def _alchemical_reference():
    nb = NonbondedForce()
    for k in range(10):
        nb.addParticle(0.0, 0.3, 0.2)
    nb.setNonbondedMethod(NonbondedForce.CutoffPeriodic); nb.setCutoffDistance(1.0)
    return _system(10, [nb, _reference_force()], (3.0, 3.0, 3.0))


def test_the_alchemical_factory_passes_it_through_or_refuses_by_name():
    factory = alchemy.AbsoluteAlchemicalFactory()
    reference = _alchemical_reference()
    out = factory.create_alchemical_system(reference, alchemy.AlchemicalRegion(alchemical_atoms=[8, 9]))     # no donor or acceptor holds them
    kept = [f for f in out.getForces() if isinstance(f, CustomHbondForce)]
    assert len(kept) == 1 and kept[0] is not reference.getForces()[1]
    a, b = system_to_desc(out)['custom_terms']['000'], system_to_desc(reference)['custom_terms']['000']
    for key, value in b.items():
        assert np.array_equal(value, a[key]), key
    with pytest.raises(NotImplementedError, match=r'CustomHbondForce \(energy .*acceptor 1 holds the alchemical particle 7'):
        factory.create_alchemical_system(reference, alchemy.AlchemicalRegion(alchemical_atoms=[7, 9]))
    with pytest.raises(NotImplementedError, match=r'CustomHbondForce \(energy .*donor 1 holds the alchemical particle 2'):
        factory.create_alchemical_system(reference, alchemy.AlchemicalRegion(alchemical_atoms=[2]))


# ---- the openmm converter on a stand-in ---------------------------------------------------------------------------------------------------------
class _Quantity:
    def __init__(self, nm):
        self.nm = nm

    def value_in_unit_system(self, system):
        return self.nm


md_unit_system = object()                                                 # (unit.to_md looks the unit system up beside the Quantity's class)


def test_the_converter_reads_a_stand_in_openmm_force():
    src = _reference_force()
    src.setNonbondedMethod(2); src.setCutoffDistance(0.9); src.setForceGroup(3)
    src.addTabulatedFunction('t', Discrete1DFunction([1.0, 2.0]))
    stand_in = type('CustomHbondForce', (), {name: getattr(src, name) for name in dir(src) if name.startswith(('get', 'uses'))})()
    stand_in.getCutoffDistance = lambda: _Quantity(0.9)
    out = hbond_force_from_openmm(stand_in)
    assert isinstance(out, CustomHbondForce) and out is not src
    a, b = system_to_desc(_system(8, [src], (3.0, 3.0, 3.0))), system_to_desc(_system(8, [out], (3.0, 3.0, 3.0)))
    for key, value in a['custom_terms']['000'].items():
        assert np.array_equal(value, b['custom_terms']['000'][key]), key


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------------------
def _oracle_case(method, box):
    rng = np.random.default_rng(77)
    x = rng.uniform(0.0, 1.5, (14, 3))
    donors = [[0, 1, 2], [3, 4, 5], [6, 7, 8]]
    acceptors = [[9, 10, -1], [11, 12, -1], [13, 0, -1]]
    energy = 'k*exp(-distance(d1,a1)/w)*(1+cos(angle(d2,d1,a1)))*(2+sin(dihedral(d3,d2,d1,a1)-dihedral(d2,d1,a1,a2)))'
    args = (energy, ['k'], ['w'], donors, acceptors, [[1.0], [2.0], [0.5]], [[0.3], [0.4], [0.5]], {})
    kw = dict(box=box, method=method, cutoff=0.9, exclusions=[(0, 2)])
    return args, kw, x


@pytest.mark.parametrize('method,box', [(0, None), (1, None), (2, np.array([1.9, 2.0, 2.1]))])
def test_the_oracle_against_central_differences_of_its_own_energy(method, box):
    args, kw, x = _oracle_case(method, box)
    ref = oracle.evaluate(*args, x, **kw)
    assert oracle.clear_of_cutoff(ref, 0.9, 1e-4) and 2 <= len(ref['E']) <= 8
    assert (0, 2) not in set(zip(ref['i'].tolist(), ref['j'].tolist()))
    h = 1e-5
    for a in range(14):
        for c in range(3):
            xp, xm = x.copy(), x.copy()
            xp[a, c] += h; xm[a, c] -= h
            fd = -(oracle.evaluate(*args, xp, **kw)['E'].sum() - oracle.evaluate(*args, xm, **kw)['E'].sum()) / (2.0 * h)
            assert abs(fd - ref['F'][a, c]) <= 1e-6 * max(1.0, np.abs(ref['F']).max()), (a, c, fd, ref['F'][a, c])
    assert ref['count'].sum() == 5 * len(ref['E'])                        # d1 d2 d3 a1 a2: five contributions per pair


def test_the_oracle_against_a_closed_form_in_numpy():
    """E = k (r - r0)^2 (1 + cos theta): r = |a1 - d1|, theta the angle at d1 between d2 and a1; the gradient written out by hand"""
    rng = np.random.default_rng(78)
    x = rng.uniform(0.0, 1.0, (5, 3))
    donors, acceptors = [[0, 1, -1]], [[2, -1, -1], [3, -1, -1], [4, -1, -1]]
    k, r0 = 3.0, [0.2, 0.3, 0.4]
    ref = oracle.evaluate('k*(distance(d1,a1)-r0)^2*(1+cos(angle(d2,d1,a1)))', [], ['r0'], donors, acceptors, [[]], [[v] for v in r0], {'k': k}, x)
    E, F = 0.0, np.zeros((5, 3))
    for j in range(3):
        u, v = x[1] - x[0], x[2 + j] - x[0]
        r, lu = np.linalg.norm(v), np.linalg.norm(u)
        c = np.dot(u, v) / (lu * r)
        E += k * (r - r0[j]) ** 2 * (1.0 + c)
        dc_du = v / (lu * r) - c * u / lu ** 2
        dc_dv = u / (lu * r) - c * v / r ** 2
        dE_dv = 2.0 * k * (r - r0[j]) * (1.0 + c) * v / r + k * (r - r0[j]) ** 2 * dc_dv
        dE_du = k * (r - r0[j]) ** 2 * dc_du
        F[2 + j] -= dE_dv; F[1] -= dE_du; F[0] += dE_dv + dE_du
    assert abs(ref['E'].sum() - E) <= 1e-13 * abs(E) and np.allclose(ref['F'], F, rtol=1e-11, atol=1e-12)
    assert ref['count'].tolist() == [3, 3, 1, 1, 1]
