"""CustomGBForce of the OBC family: the one recognizer that system_to_desc, system_xml and _alchemical_xml share, and the reference's
alchemical rewrite of a CustomGBForce.

Two paths.  The template path (csrc/gbsa.hip) evaluates no expression language: it takes a CustomGBForce whose strings are one of two
template shapes with numbers in named slots, every other literal fixed (below).  Every other CustomGBForce goes the general path at the
end of this module: compile_custom_gb turns every computed value and energy term into programs of the custom forces' stack machine
(REMD_CUSTOM_GB of include/remd_hip_custom.h, csrc/custom_gb.hip).  The templates:

  A  the strings of testsystems.CustomGBForceSystem (the reference's testsystems.py:4332-4351): computed values I (ParticlePairNoExclusions)
     and B (SingleParticle), one SingleParticle energy term (surface term + self term) and one ParticlePairNoExclusions pair term, the
     dielectrics numbers or bound to globals by ``soluteDielectric = <global>`` / ``solventDielectric = <global>`` lines;
  B  the GBSA strings of the alchemical factory (alchemy.py:2172-2225; _alchemical_xml.py writes them): the same model with the self,
     surface and pair terms apart, ``offset`` and the dielectrics as globals, the lambda_electrostatics factors in the strings or not;

either one also after the rewrite of _alchemically_modify_CustomGBForce (alchemy.py:2223-2345): the ``alchemical_scaling*unscaled``
prefixes, the ``alchemically_scaled_charge1/2`` substitutions, the ``alchemical`` per-particle parameter and the lambda_electrostatics
global.  The free slots are the offset (one value in I and in B), alpha, beta, gamma of tanh(alpha psi - beta psi^2 + gamma psi^3),
the Coulomb constant k_e and the surface coefficient and probe radius.  NoCutoff and CutoffPeriodic; global parameters take their
default values.  The model goes to the engine through remd_set_gb_model (include/remd_hip_gb.h).
"""
import re

import numpy as np

# the model of GBSAOBCForce (OBC2 + ACE) in the units of remd_gb_model_desc: the constants csrc/gbsa.hip had as literals
OBC2_MODEL = dict(offset=0.009, alpha=1.0, beta=0.8, gamma=4.85, ke=138.935485, surface=28.3919551, probe=0.14, method=0, cutoff=0.0)
MODEL_KEYS = ('offset', 'alpha', 'beta', 'gamma', 'ke', 'surface', 'probe', 'method', 'cutoff')

SINGLE, PAIR, PAIR_NO_EXCLUSIONS = 0, 1, 2
DIELECTRICS = ('soluteDielectric', 'solventDielectric')

# ---- the reference's rewrite (alchemy.py:2284-2310), verbatim ----------------------------------------------------------------------
_PAIR_VALUE_PREFIX = ('alchemical_scaling*unscaled; '
                      'alchemical_scaling = (lambda_electrostatics*alchemical2 + (1-alchemical2)); '
                      'unscaled = ')
_SINGLE_TERM_PREFIX = ('alchemical_scaling*unscaled; '
                       'alchemical_scaling = (lambda_electrostatics*alchemical + (1-alchemical)); '
                       'unscaled = ')
_PAIR_TERM_SUFFIX = (' ; alchemically_scaled_charge1 = (lambda_electrostatics*alchemical1+(1-alchemical1)) * charge1;'
                     ' ; alchemically_scaled_charge2 = (lambda_electrostatics*alchemical2+(1-alchemical2)) * charge2;')


def alchemically_modify_custom_gb(reference_force, alchemical_atoms):
    """_alchemically_modify_CustomGBForce (alchemy.py:2223-2345) for one region: a new CustomGBForce with the rewritten strings."""
    from .system import CustomGBForce
    f = CustomGBForce()
    for k in range(reference_force.getNumGlobalParameters()):
        f.addGlobalParameter(reference_force.getGlobalParameterName(k), reference_force.getGlobalParameterDefaultValue(k))
    f.addGlobalParameter('lambda_electrostatics', 1.0)
    for k in range(reference_force.getNumPerParticleParameters()):
        f.addPerParticleParameter(reference_force.getPerParticleParameterName(k))
    f.addPerParticleParameter('alchemical')
    f.setNonbondedMethod(reference_force.getNonbondedMethod())
    f.setCutoffDistance(reference_force.getCutoffDistance())
    for k in range(reference_force.getNumComputedValues()):
        name, expression, kind = reference_force.getComputedValueParameters(k)
        if kind != CustomGBForce.SingleParticle:
            expression = _PAIR_VALUE_PREFIX + expression
        f.addComputedValue(name, expression, kind)
    for k in range(reference_force.getNumEnergyTerms()):
        expression, kind = reference_force.getEnergyTermParameters(k)
        if kind == CustomGBForce.SingleParticle:
            expression = _SINGLE_TERM_PREFIX + expression
        else:
            expression = expression.replace('charge1', 'alchemically_scaled_charge1')
            expression = expression.replace('charge2', 'alchemically_scaled_charge2')
            expression += ' ; alchemically_scaled_charge1 = (lambda_electrostatics*alchemical1+(1-alchemical1)) * charge1;'
            expression += ' ; alchemically_scaled_charge2 = (lambda_electrostatics*alchemical2+(1-alchemical2)) * charge2;'
        f.addEnergyTerm(expression, kind)
    A = set(int(a) for a in alchemical_atoms)
    for k in range(reference_force.getNumParticles()):
        f.addParticle(list(reference_force.getParticleParameters(k)) + [1.0 if k in A else 0.0])
    for k in range(reference_force.getNumTabulatedFunctions()):
        f.addTabulatedFunction(reference_force.getTabulatedFunctionName(k), reference_force.getTabulatedFunction(k))
    for k in range(reference_force.getNumExclusions()):
        f.addExclusion(*reference_force.getExclusionParticles(k))
    f.setForceGroup(reference_force.getForceGroup())
    return f


def _compact(s):
    return re.sub(r'\s+', '', s)


def is_alchemically_modified(force):
    """True for a CustomGBForce that _alchemically_modify_CustomGBForce wrote (its prefixes and substitutions, the extra parameters)"""
    if not force.per_particle or force.per_particle[-1] != 'alchemical' or not force.globals or force.globals[-1][0] != 'lambda_electrostatics':
        return False
    for name, expr, kind in force.computed:
        if kind != SINGLE and not _compact(expr).startswith(_compact(_PAIR_VALUE_PREFIX)):
            return False
    for expr, kind in force.energy_terms:
        c = _compact(expr)
        if kind == SINGLE and not c.startswith(_compact(_SINGLE_TERM_PREFIX)):
            return False
        if kind != SINGLE and not c.endswith(_compact(_PAIR_TERM_SUFFIX)):
            return False
    return True


def _strip(expr, prefix=None, suffix=None):
    c = _compact(expr)
    if prefix is not None:
        c = c[len(_compact(prefix)):]
    if suffix is not None:
        c = c[:-len(_compact(suffix))].replace('alchemically_scaled_charge', 'charge')
    return c


def unmodify_custom_gb(force):
    """The CustomGBForce _alchemically_modify_CustomGBForce was given (expressions in compact form) + its alchemical atoms."""
    from .system import CustomGBForce
    if not is_alchemically_modified(force):
        raise NotImplementedError('CustomGBForce: not the alchemical factory\'s rewrite of a CustomGBForce')
    f = CustomGBForce()
    for name, v in force.globals[:-1]:
        f.addGlobalParameter(name, v)
    for name in force.per_particle[:-1]:
        f.addPerParticleParameter(name)
    f.setNonbondedMethod(force.getNonbondedMethod()); f.setCutoffDistance(force.getCutoffDistance())
    for name, expr, kind in force.computed:
        f.addComputedValue(name, expr if kind == SINGLE else _strip(expr, prefix=_PAIR_VALUE_PREFIX), kind)
    for expr, kind in force.energy_terms:
        f.addEnergyTerm(_strip(expr, prefix=_SINGLE_TERM_PREFIX) if kind == SINGLE else _strip(expr, suffix=_PAIR_TERM_SUFFIX), kind)
    atoms = []
    for k, p in enumerate(force.particles):
        f.addParticle(p[:-1])
        if p[-1] != 0.0:
            atoms.append(k)
    for name, fn in force.functions:
        f.addTabulatedFunction(name, fn)
    for i, j in force.exclusions:
        f.addExclusion(i, j)
    f.setForceGroup(force.getForceGroup())
    return f, atoms


# ---- the templates ---------------------------------------------------------------------------------------------------------------
_NUM = r'(?:\d+(?:\.\d*)?(?:[eE][-+]?\d+)?|\.\d+(?:[eE][-+]?\d+)?)'
_S = {'S': '(lambda_electrostatics*alchemical+(1-alchemical))*', 'S1': '(lambda_electrostatics*alchemical1+(1-alchemical1))*',
      'S2': '(lambda_electrostatics*alchemical2+(1-alchemical2))*'}


def _regex(template):
    """'{slot}' -> a number in a named group ('{offset}' may also be the global 'offset'); '{S}', '{S1}', '{S2}' -> the factory's
    optional lambda_electrostatics factor"""
    out, pos = [], 0
    for m in re.finditer(r'\{(\w+)\}', template):
        out.append(re.escape(template[pos:m.start()]))
        name = m.group(1)
        if name in _S:
            out.append('(?P<%s>%s)?' % (name, re.escape(_S[name])))
        elif name == 'offset':
            out.append('(?P<offset>%s|offset)' % _NUM)
        else:
            out.append('(?P<%s>%s)' % (name, _NUM))
        pos = m.end()
    out.append(re.escape(template[pos:]))
    return re.compile(''.join(out) + r'\Z')


_I_DEFS = [('U', 'r+sr2'), ('C', '2*(1/or1-1/L)*step(sr2-r-or1)'), ('L', 'max(or1,D)'), ('D', 'abs(r-sr2)'), ('sr2', 'scale2*or2'),
           ('or1', 'radius1-{offset}'), ('or2', 'radius2-{offset}')]
_F_DEFS = [('f', 'sqrt(r^2+B1*B2*exp(-r^2/(4*B1*B2)))')]
_SHAPES = {
    'A': dict(values=[('I', PAIR_NO_EXCLUSIONS, 'step(r+sr2-or1)*0.5*(1/L-1/U+0.25*(1/U^2-1/L^2)*(r-sr2*sr2/r)+0.5*log(L/U)/r+C)', _I_DEFS),
                      ('B', SINGLE, '1/(1/or-tanh({alpha}*psi-{beta}*psi^2+{gamma}*psi^3)/radius)', [('psi', 'I*or'), ('or', 'radius-{offset}')])],
              terms=[('surface+self', SINGLE, '{surface}*(radius+{probe})^2*(radius/B)^6-0.5*{ke}*(1/soluteDielectric-1/solventDielectric)*charge^2/B', []),
                     ('pair', PAIR_NO_EXCLUSIONS, '-{ke}*(1/soluteDielectric-1/solventDielectric)*charge1*charge2/f', _F_DEFS)],
              optional=()),
    'B': dict(values=[('I', PAIR_NO_EXCLUSIONS, '{S2}step(r+sr2-or1)*0.5*(1/L-1/U+0.25*(r-sr2^2/r)*(1/(U^2)-1/(L^2))+0.5*log(L/U)/r+C)', _I_DEFS),
                      ('B', SINGLE, '1/(1/or-tanh(psi-{beta}*psi^2+{gamma}*psi^3)/radius)', [('psi', 'I*or'), ('or', 'radius-{offset}')])],
              terms=[('self', SINGLE, '-0.5*{ke}*(1/soluteDielectric-1/solventDielectric)*{S}charge^2/B', []),
                     ('surface', SINGLE, '{S}{surface}*(radius+{probe})^2*(radius/B)^6', []),
                     ('pair', PAIR_NO_EXCLUSIONS, '-{ke}*(1/soluteDielectric-1/solventDielectric)*{S1}charge1*{S2}charge2/f', _F_DEFS)],
              optional=('surface',)),
}
_COMPILED = {k: dict(values=[(n, t, _regex(h), [(dn, _regex(dv)) for dn, dv in defs]) for n, t, h, defs in v['values']],
                     terms=[(n, t, _regex(h), [(dn, _regex(dv)) for dn, dv in defs]) for n, t, h, defs in v['terms']],
                     optional=v['optional']) for k, v in _SHAPES.items()}


def _parts(expression):
    """split at ';', strip whitespace: (head, [(name, definition)])"""
    parts = [_compact(p) for p in expression.split(';')]
    parts = [p for p in parts if p]
    if not parts:
        return '', []
    defs = []
    for p in parts[1:]:
        if '=' not in p:
            return parts[0], None
        name, rhs = p.split('=', 1)
        defs.append((name, rhs))
    return parts[0], defs


def _match(expression, head_re, def_res, dielectric_defs):
    """slot values of one expression, or None; the dielectric definition lines go to dielectric_defs"""
    head, defs = _parts(expression)
    if defs is None:
        return None
    own = []
    for name, rhs in defs:
        if name in DIELECTRICS:
            if name in dielectric_defs and dielectric_defs[name] != rhs:
                return None
            dielectric_defs[name] = rhs
        else:
            own.append((name, rhs))
    if [n for n, _ in own] != [n for n, _ in def_res]:
        return None
    slots = {}
    for text, rx in [(head, head_re)] + [(rhs, rx) for (_, rhs), (_, rx) in zip(own, def_res)]:
        m = rx.match(text)
        if m is None:
            return None
        for k, v in m.groupdict().items():
            if k in _S:
                v = v is not None
                if slots.setdefault('factor', v) != v:
                    return None
                continue
            if slots.setdefault(k, v) != v:
                return None
    return slots


def recognize_custom_gb(force):
    """The model of an OBC-family CustomGBForce: dict(shape, alchemical, offset, alpha, beta, gamma, ke, surface, probe, surface_area,
    solute_dielectric, solvent_dielectric, method, cutoff).  NotImplementedError naming CustomGBForce and the first term that does not
    match, for anything else."""
    def refuse(what):
        raise NotImplementedError('CustomGBForce: %s (only the OBC-family strings of testsystems.CustomGBForceSystem and of the alchemical '
                                  'factory\'s GBSA are evaluated, see openmmtools_amd/custom_gb.py)' % what)
    if force.getNumTabulatedFunctions():
        refuse('tabulated function %r' % force.getTabulatedFunctionName(0))
    method = force.getNonbondedMethod()
    if method not in (0, 2):
        refuse('nonbonded method %d (CutoffNonPeriodic): only NoCutoff and CutoffPeriodic' % method)
    for name, expr, kind in force.computed:
        if kind == PAIR:
            refuse('computed value %r of type ParticlePair (with exclusions)' % name)
    for expr, kind in force.energy_terms:
        if kind == PAIR:
            refuse('energy term of type ParticlePair (with exclusions): %r' % expr[:60])
    rewritten = is_alchemically_modified(force)
    plain, _ = unmodify_custom_gb(force) if rewritten else (force, None)
    per = list(plain.per_particle)
    if not force.computed:
        refuse('no computed values')
    # the shape: the first whose I matches
    dd = {}                                  # the dielectric definition lines of all terms
    first = plain.computed[0]
    shape = next((k for k, c in _COMPILED.items() if first[0] == 'I' and first[2] == PAIR_NO_EXCLUSIONS and
                  _match(first[1], c['values'][0][2], c['values'][0][3], {}) is not None), None)
    if shape is None:
        refuse('computed value %r does not match: %r' % (first[0], first[1][:80]))
    c = _COMPILED[shape]
    slots = {}

    def take(new, what):
        for k, v in new.items():
            if slots.setdefault(k, v) != v:
                refuse('%s: %s %s differs from %s in an earlier term' % (what, k, v, slots[k]))
    if len(plain.computed) != len(c['values']):
        refuse('computed values %s (expected %s)' % (', '.join(repr(v[0]) for v in plain.computed), ', '.join(repr(v[0]) for v in c['values'])))
    for (name, expr, kind), (want, wkind, hr, drs) in zip(plain.computed, c['values']):
        s = _match(expr, hr, drs, dd) if (name == want and kind == wkind) else None
        if s is None:
            refuse('computed value %r does not match: %r' % (name, expr[:80]))
        take(s, 'computed value %r' % name)
    terms = list(plain.energy_terms)
    wanted = list(c['terms'])
    surface_present = True
    if c['optional'] and len(terms) == len(wanted) - len(c['optional']):
        wanted = [w for w in wanted if w[0] not in c['optional']]
        surface_present = False
    for k, (expr, kind) in enumerate(terms):
        if k >= len(wanted):
            refuse('energy term %d does not match: %r' % (k, expr[:80]))
        wname, wkind, hr, drs = wanted[k]
        s = _match(expr, hr, drs, dd) if kind == wkind else None
        if s is None:
            refuse('energy term %d (%s) does not match: %r' % (k, wname, expr[:80]))
        take(s, 'energy term %d' % k)
    if len(terms) < len(wanted):
        refuse('energy term %r is missing' % wanted[len(terms)][0])
    factor = slots.pop('factor', False)
    alchemical = rewritten or factor
    if rewritten and factor:
        refuse('both the factory\'s lambda_electrostatics factors and the rewrite of _alchemically_modify_CustomGBForce')
    # parameters and globals
    want_per = ['charge', 'radius', 'scale'] + (['alchemical'] if factor else [])
    if per != want_per:
        refuse('per-particle parameters %r (expected %r)' % (per, want_per))
    g = dict((n, v) for n, v in force.globals)
    used = set(['lambda_electrostatics']) if alchemical else set()
    vals = {}
    for name in DIELECTRICS:
        rhs = dd.get(name, name)
        if re.fullmatch(_NUM, rhs):
            vals[name] = float(rhs)
        elif rhs in g:
            vals[name] = g[rhs]; used.add(rhs)
        else:
            refuse('%s = %r is neither a number nor a global parameter' % (name, rhs))
    if slots['offset'] == 'offset':
        if 'offset' not in g:
            refuse('the offset names a global parameter the force does not have')
        used.add('offset')
        slots['offset'] = g['offset']
    for n in g:
        if n not in used:
            refuse('global parameter %r' % n)
    model = dict(shape=shape, alchemical=bool(alchemical), method=int(method), cutoff=float(force.getCutoffDistance()) if method == 2 else 0.0,
                 solute_dielectric=vals['soluteDielectric'], solvent_dielectric=vals['solventDielectric'],
                 offset=float(slots['offset']), alpha=float(slots.get('alpha', 1.0)), beta=float(slots['beta']), gamma=float(slots['gamma']),
                 ke=float(slots['ke']), surface=float(slots['surface']) if surface_present else OBC2_MODEL['surface'],
                 probe=float(slots['probe']) if surface_present else OBC2_MODEL['probe'],
                 surface_area=int(surface_present and float(slots['surface']) != 0.0))
    return model


def custom_gb_to_desc(force, n, nb_method, box):
    """d['gbsa'] of system_to_desc for a CustomGBForce: the particle tables and the model (remd_set_gbsa + remd_set_gb_model); None for
    a force the recognizer refuses: system_to_desc then compiles it for the general path (compile_custom_gb)"""
    try:
        m = recognize_custom_gb(force)
    except NotImplementedError:
        if not force.computed and not force.energy_terms:      # nothing to compile: the recognizer's sentence stands
            raise
        return None
    if force.getNumParticles() != n:
        raise ValueError('CustomGBForce has %d particles, system has %d' % (force.getNumParticles(), n))
    if m['method'] == 2:
        if nb_method not in (1, 2):
            raise NotImplementedError('CustomGBForce: CutoffPeriodic in a system whose NonbondedForce is not periodic')
        if not 0.0 < m['cutoff'] <= 0.5 * float(np.min(box)):
            raise NotImplementedError('CustomGBForce: cutoff %g nm is larger than half the shortest box edge (%g nm)' % (m['cutoff'], 0.5 * float(np.min(box))))
    elif nb_method != 3:
        raise NotImplementedError('CustomGBForce: NoCutoff needs a NoCutoff NonbondedForce')
    p = np.array(force.particles, dtype=np.float64).reshape(n, -1)
    alch = (p[:, 3] != 0.0).astype(np.int32) if m['alchemical'] else np.zeros(n, dtype=np.int32)
    if np.any(p[:, 1] <= m['offset']):
        raise ValueError('CustomGBForce: radii must exceed the offset %g nm' % m['offset'])
    d = dict(charge=p[:, 0].copy(), radius=p[:, 1].copy(), scale=p[:, 2].copy(), alchemical=alch,
             solute_dielectric=m['solute_dielectric'], solvent_dielectric=m['solvent_dielectric'], surface_area=m['surface_area'])
    d.update({k: m[k] for k in MODEL_KEYS})
    return d


def is_default_model(gb):
    """True when d['gbsa'] is OBC2 without a cutoff: remd_set_gbsa alone evaluates it (no remd_set_gb_model call)"""
    for k in MODEL_KEYS:
        if k == 'surface' and not gb.get('surface_area', 1):
            continue
        if float(gb.get(k, OBC2_MODEL[k])) != float(OBC2_MODEL[k]):
            return False
    return True


# ---- the general path: every other CustomGBForce, compiled for the stack machine (csrc/custom_gb.hip) ---------------------------------
KIND_GB = 12                                    # REMD_CUSTOM_GB of include/remd_hip_custom.h
MAX_VALUES, MAX_TERMS, MAX_STAGES, STAGE_INTS = 4, 8, 32, 28
STAGE_PAIR_VALUE, STAGE_SINGLE_VALUE, STAGE_SINGLE_ENERGY, STAGE_PAIR_ENERGY = 0, 1, 2, 3
_TYPE_NAMES = {SINGLE: 'SingleParticle', PAIR: 'ParticlePair', PAIR_NO_EXCLUSIONS: 'ParticlePairNoExclusions'}


def quantity_code(kind, index=0, particle=0):
    """the stage table's code of a quantity: 'r'; ('value', k, s) = value k of particle s; ('param', q, s) = parameter q of particle s
    (s = 0: particle 1, or the particle itself in a single-particle expression; 1: particle 2)"""
    return 0 if kind == 'r' else (1 if kind == 'value' else 16) + 2 * index + particle


def _names_of(expression, where):
    """every name an expression and its definitions use (function names included)"""
    from .custom_expr import split_definitions, _TOKEN
    body, definitions = split_definitions(expression, where)
    names = set()
    for text in [body] + list(definitions.values()):
        for m in _TOKEN.finditer(text):
            if m.group(2) is not None:
                names.add(m.group(2))
    return names, definitions


def compile_gb_expression(expression, pair, values_known, per_particle, global_values, tabulated, where):
    """The programs of one expression of a CustomGBForce, one per pass: [dict(program, consts, stack_depth, variables, columns)],
    variables and columns being quantity codes.  The quantities to be differentiated -- r and name1 / name2 of every value the
    expression names (pair), the values it names (single particle) -- are the machine's three variables, pass by pass; everything
    else the expression names is a staged column.  Globals are folded into the constants: each becomes a definition
    ``name = value`` unless the expression defines the name itself."""
    from .custom_expr import compile_expression, MAX_PARAMS
    used, definitions = _names_of(expression, where)
    if not pair:
        for bad in ('x', 'y', 'z'):
            if bad in used and bad not in definitions and bad not in per_particle and bad not in values_known:
                raise NotImplementedError('%s: variable %r (a single-particle expression of a CustomGBForce that depends on the position is not supported)' % (where, bad))
    text = str(expression).rstrip().rstrip(';')
    for name, value in global_values:
        if name in used and name not in definitions:
            text += '; %s = %r' % (name, float(value))
    # what a name means here: name -> quantity code
    meaning = {}
    for s in ((0, 1) if pair else (0,)):
        suffix = str(s + 1) if pair else ''
        for k, v in enumerate(values_known):
            meaning[v + suffix] = quantity_code('value', k, s)
        for q, p in enumerate(per_particle):
            meaning[p + suffix] = quantity_code('param', q, s)
    if pair:
        meaning['r'] = 0
        for name in sorted(used):
            if name not in definitions and name not in meaning and (name in per_particle or name in values_known):
                raise NotImplementedError('%s: per-particle name %r without a particle suffix (%s1 or %s2)' % (where, name, name, name))
    named = [n for n in sorted(used, key=lambda n: meaning.get(n, -1)) if n in meaning and n not in definitions]
    if pair:
        values_named = sorted({(meaning[n] - 1) // 2 for n in named if 1 <= meaning[n] < 16})
        differentiated = ['r'] + [values_known[k] + s for k in values_named for s in ('1', '2')]
    else:
        differentiated = [n for n in named if 1 <= meaning[n] < 16]
    passes = [differentiated[k:k + 3] for k in range(0, len(differentiated), 3)] or [[]]
    out = []
    for variables in passes:
        columns = [n for n in named if n not in variables]
        if len(columns) > MAX_PARAMS:
            raise NotImplementedError('%s: a program that names %d staged columns (the engine takes %d): %s' % (where, len(columns), MAX_PARAMS, ', '.join(columns)))
        prog = compile_expression(text, tuple(variables), columns, {}, where=where, tabulated=tabulated)
        out.append(dict(program=prog['program'], consts=prog['consts'], stack_depth=prog['stack_depth'],
                        variables=[meaning[n] for n in variables], columns=[meaning[n] for n in columns]))
    return out


def gb_exclusions(force, n):
    """The exclusions of a CustomGBForce in CSR form: (excl_offsets int32 [n + 1], excl_atoms int32), symmetric, each row sorted."""
    rows = [set() for _ in range(n)]
    for k in range(force.getNumExclusions()):
        i, j = force.getExclusionParticles(k)
        if not (0 <= i < n and 0 <= j < n):
            raise ValueError('CustomGBForce: exclusion %d names particle %d (the force has %d)' % (k, i if not 0 <= i < n else j, n))
        if i == j:
            raise ValueError('CustomGBForce: exclusion %d excludes particle %d from itself' % (k, i))
        if j in rows[i]:
            raise ValueError('CustomGBForce: particles %d and %d are excluded twice' % (i, j))
        rows[i].add(j); rows[j].add(i)
    offsets = np.zeros(n + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([len(r) for r in rows])
    return offsets, np.array([j for r in rows for j in sorted(r)], dtype=np.int32)


_TABLE_OPS = (38, 39, 40, 41, 42)               # TABLE1D ... LOOKUP3D: their operand is an offset into the constants, like CONST's (0)


def compile_custom_gb(force, n_atoms=None, box_vectors=None, global_names=(), global_defaults=()):
    """The custom_terms entry of a CustomGBForce on the general path (REMD_CUSTOM_GB): the common keys, with program and consts the
    stages' back to back, params [N][n_params], nb_method, cutoff, excl_offsets / excl_atoms, n_values and stages int32
    [n][STAGE_INTS] (include/remd_hip_custom.h).  global_names / global_defaults are the handle's columns (the other custom forces');
    the force's own globals are folded into its constants at their default values.  ValueError for bad input, NotImplementedError for
    what the engine does not evaluate."""
    cls = 'CustomGBForce'
    n = force.getNumParticles()
    if n_atoms is not None and n != n_atoms:
        raise ValueError('%s has %d particles, system has %d' % (cls, n, n_atoms))
    if n == 0:
        raise ValueError('%s has no particles' % cls)
    per_particle = list(force.per_particle)
    for k in range(n):
        if len(force.particles[k]) != len(per_particle):
            raise ValueError('%s: particle %d carries %d parameters, the force declares %d' % (cls, k, len(force.particles[k]), len(per_particle)))
    from .custom_expr import MAX_PARAMS, CONST
    if len(per_particle) > MAX_PARAMS:
        raise NotImplementedError('%s: %d per-particle parameters (the engine takes %d): %s' % (cls, len(per_particle), MAX_PARAMS, ', '.join(per_particle)))
    if not force.computed and not force.energy_terms:
        raise ValueError('%s has neither computed values nor energy terms' % cls)
    if len(force.computed) > MAX_VALUES:
        raise NotImplementedError('%s: %d computed values (the engine takes %d): %s' % (cls, len(force.computed), MAX_VALUES, ', '.join(v[0] for v in force.computed)))
    if len(force.energy_terms) > MAX_TERMS:
        raise NotImplementedError('%s: %d energy terms (the engine takes %d)' % (cls, len(force.energy_terms), MAX_TERMS))
    computed = list(force.computed)
    if not computed:                            # (energy terms alone: a pair value that is zero keeps the stage table's shape)
        computed = [('__none', '0', PAIR_NO_EXCLUSIONS)]
    for k, (name, expr, kind) in enumerate(computed):
        if kind not in _TYPE_NAMES:
            raise ValueError('%s: computed value %r has the unknown type %r' % (cls, name, kind))
        if k == 0 and kind == SINGLE:
            raise NotImplementedError('%s: the first computed value %r is of type SingleParticle (it must be ParticlePair or ParticlePairNoExclusions)' % (cls, name))
        if k > 0 and kind != SINGLE:
            raise NotImplementedError('%s: computed value %r of type %s behind the first (every value after the first must be SingleParticle)'
                                      % (cls, name, _TYPE_NAMES[kind]))
        if name in [v[0] for v in computed[:k]] or name in per_particle:
            raise ValueError('%s: computed value %r is named twice' % (cls, name))
    for expr, kind in force.energy_terms:
        if kind not in _TYPE_NAMES:
            raise ValueError('%s: energy term %r has the unknown type %r' % (cls, expr[:60], kind))
    method = int(force.getNonbondedMethod())
    if method not in (0, 1, 2):
        raise NotImplementedError('%s: nonbonded method %d (NoCutoff, CutoffNonPeriodic and CutoffPeriodic are supported)' % (cls, method))
    cutoff = float(force.getCutoffDistance()) if method else 0.0
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
    offsets, excluded = gb_exclusions(force, n)
    tabulated = list(force.functions)
    global_values = [(g[0], g[1]) for g in force.globals]
    value_names = [v[0] for v in computed]
    program, consts, stages = [], [], []

    def add_stages(kind_code, excl, target, passes):
        for p, s in enumerate(passes):
            base = len(consts)
            prog = np.array(s['program'], dtype=np.int64).reshape(-1, 2)
            shift = np.isin(prog[:, 0], (CONST,) + _TABLE_OPS)
            prog[shift, 1] += base
            row = np.zeros(STAGE_INTS, dtype=np.int32)
            row[:7] = (kind_code, excl, target, p, len(program), len(prog), s['stack_depth'])
            row[7:10] = (list(s['variables']) + [-1, -1, -1])[:3]
            row[10] = len(s['columns'])
            row[11:11 + len(s['columns'])] = s['columns']
            stages.append(row)
            program.extend(prog.tolist())
            consts.extend(np.asarray(s['consts'], dtype=np.float64).tolist())

    for k, (name, expr, kind) in enumerate(computed):
        where = '%s (computed value %r = %r)' % (cls, name, expr)
        passes = compile_gb_expression(expr, k == 0, value_names[:k], per_particle, global_values, tabulated, where)
        if k == 0:
            passes[0]['variables'] = [0]        # (one pass with r: an expression without r still has the variable)
            if len(passes) > 1:
                raise AssertionError('the first value names no value')
            if 0 in passes[0]['columns']:
                raise AssertionError('r is a variable')
        add_stages(STAGE_PAIR_VALUE if k == 0 else STAGE_SINGLE_VALUE, int(kind == PAIR), k, passes)
    for t, (expr, kind) in enumerate(force.energy_terms):
        where = '%s (energy term %d = %r)' % (cls, t, expr)
        passes = compile_gb_expression(expr, kind != SINGLE, value_names, per_particle, global_values, tabulated, where)
        add_stages(STAGE_SINGLE_ENERGY if kind == SINGLE else STAGE_PAIR_ENERGY, int(kind == PAIR), t, passes)
    if len(stages) > MAX_STAGES:
        raise NotImplementedError('%s: %d stages (values, and one per energy term and pass; the engine takes %d)' % (cls, len(stages), MAX_STAGES))
    params = np.array(force.particles, dtype=np.float64).reshape(n, len(per_particle))
    return dict(kind=KIND_GB, atoms=np.zeros((0, 0), dtype=np.int32), params=params, global_names=list(global_names),
                global_defaults=np.array(global_defaults, dtype=np.float64), program=np.array(program, dtype=np.int32).reshape(-1, 2),
                consts=np.array(consts, dtype=np.float64), stack_depth=int(max(s[6] for s in stages)), periodic=int(method == 2),
                force_group=int(force.getForceGroup()), energy='CustomGBForce(%s)' % '; '.join(v[0] for v in force.computed),
                nb_method=method, cutoff=cutoff, switch_distance=-1.0, excl_offsets=offsets, excl_atoms=excluded, long_range_correction=0,
                n_values=len(computed), stages=np.array(stages, dtype=np.int32).reshape(-1, STAGE_INTS), value_names=value_names)


def takes_general_path(force):
    """True for a CustomGBForce that recognize_custom_gb refuses: system_to_desc then compiles it (compile_custom_gb)"""
    try:
        recognize_custom_gb(force)
    except NotImplementedError:
        return True
    return False
