"""CustomGBForce of the OBC family: the one recognizer that system_to_desc, system_xml and _alchemical_xml share, and the reference's
alchemical rewrite of a CustomGBForce.

The engine evaluates no expression language.  A CustomGBForce is accepted when its strings are one of two template shapes with numbers
in named slots, every other literal fixed:

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
    """d['gbsa'] of system_to_desc for a CustomGBForce: the particle tables and the model (remd_set_gbsa + remd_set_gb_model)"""
    m = recognize_custom_gb(force)
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
