"""The CustomGBForce models the general-path tests share (tests/test_custom_gb_expr_cpu.py, tests/test_custom_gb_expr_gpu.py): each as
a system.CustomGBForce and as the plain dict tests/custom_gb_expr_oracle.py takes, built from the same strings and numbers."""
import numpy as np

import tabulated2d_oracle
from openmmtools_amd.system import CustomGBForce, Discrete2DFunction

SINGLE, PAIR, PAIR_NX = CustomGBForce.SingleParticle, CustomGBForce.ParticlePair, CustomGBForce.ParticlePairNoExclusions

I_TEXT = ('step(r+sr2-or1)*0.5*(1/L-1/U+0.25*(1/U^2-1/L^2)*(r-sr2*sr2/r)+0.5*log(L/U)/r+C); U=r+sr2; C=2*(1/or1-1/L)*step(sr2-r-or1);'
          'L=max(or1,D); D=abs(r-sr2); sr2=scale2*or2; or1=radius1-0.009; or2=radius2-0.009')
SELF_TEXT = '28.3919551*(radius+0.14)^2*(radius/B)^6-0.5*138.935485*(1/soluteDielectric-1/solventDielectric)*charge^2/B'
PAIR_TEXT = '-138.935485*(1/soluteDielectric-1/solventDielectric)*charge1*charge2/f; f=sqrt(r^2+B1*B2*exp(-r^2/(4*B1*B2)))'
GLOBALS = dict(solventDielectric=78.5, soluteDielectric=1.0)
# OBC2's B with one pair of parentheses the template does not know: recognize_custom_gb refuses it, the model is the same
OBC2_B = '1/(1/or-tanh((1*psi-0.8*psi^2+4.85*psi^3))/radius); psi=I*or; or=radius-0.009'
HCT_B = '1/(1/or-I); or=radius-0.009'


def born_parameters(n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-0.8, 0.8, n), rng.uniform(0.12, 0.2, n), rng.uniform(0.7, 0.9, n)], axis=1)


def positions(n, seed, spacing=0.32, jitter=0.04, replicas=2):
    """[replicas][n][3], f32-representable: a jittered cubic lattice, so that r > 0.2 nm for every pair"""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(n ** (1.0 / 3.0)))
    grid = np.array([[a, b, c] for a in range(side) for b in range(side) for c in range(side)], dtype=np.float64)[:n] * spacing
    return np.asarray([grid + rng.uniform(-jitter, jitter, grid.shape) for _ in range(replicas)], dtype=np.float32).astype(np.float64)


def build(spec):
    """the system.CustomGBForce of an oracle dict (functions: spec['tables'] = {name: Discrete2DFunction})"""
    f = CustomGBForce()
    for name in spec['per_particle']:
        f.addPerParticleParameter(name)
    for name, value in spec.get('globals', {}).items():
        f.addGlobalParameter(name, value)
    for name, text, kind in spec['computed']:
        f.addComputedValue(name, text, kind)
    for text, kind in spec['terms']:
        f.addEnergyTerm(text, kind)
    for row in np.asarray(spec['params']).reshape(len(spec['params']), -1):
        f.addParticle(row)
    for i, j in spec.get('exclusions', ()):
        f.addExclusion(i, j)
    for name, fn in spec.get('tables', {}).items():
        f.addTabulatedFunction(name, fn)
    f.setNonbondedMethod(spec['method'])
    f.setCutoffDistance(spec['cutoff'] if spec['method'] else 1.0)
    return f


def born(n, b_text, method=0, cutoff=0.0, seed=7):
    return dict(per_particle=['charge', 'radius', 'scale'], params=born_parameters(n, seed), globals=dict(GLOBALS),
                computed=[('I', I_TEXT, PAIR_NX), ('B', b_text, SINGLE)], terms=[(SELF_TEXT, SINGLE), (PAIR_TEXT, PAIR_NX)],
                method=method, cutoff=cutoff)


def gbn2_shaped(n, seed=11):
    """the shape of GBn2: 7 per-particle parameters, a neck correction from two Discrete2DFunctions of the particles' radius indices
    (smooth synthetic values, not Amber's tables), per-particle alpha, beta, gamma in the tanh"""
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(-0.8, 0.8, n), rng.uniform(0.12, 0.2, n), rng.uniform(0.7, 0.9, n), rng.uniform(0.7, 1.0, n),
                  rng.uniform(0.6, 0.9, n), rng.uniform(2.0, 3.0, n), rng.integers(0, 5, n).astype(np.float64)], axis=1)
    a, b = np.meshgrid(np.arange(5.0), np.arange(5.0))           # values[i + 5 j]
    m0 = (0.02 + 0.004 * a + 0.003 * b).reshape(-1)
    d0 = (0.25 + 0.01 * a + 0.015 * b).reshape(-1)
    i_text = ('Ivdw+neckScale*Ineck; Ineck=step(radius1+radius2+neckCut-r)*m0(radindex1,radindex2)/(1+100*(r-d0(radindex1,radindex2))^2+'
              '0.3*1000000*(r-d0(radindex1,radindex2))^6);' + 'Ivdw=' + I_TEXT)
    b_text = '1/(1/or-tanh(alpha*psi-beta*psi^2+gamma*psi^3)/radius); psi=I*or; or=radius-0.009'
    return dict(per_particle=['charge', 'radius', 'scale', 'alpha', 'beta', 'gamma', 'radindex'], params=p,
                globals=dict(GLOBALS, neckScale=0.826836, neckCut=0.68),
                computed=[('I', i_text, PAIR_NX), ('B', b_text, SINGLE)], terms=[(SELF_TEXT, SINGLE), (PAIR_TEXT, PAIR_NX)], method=0, cutoff=0.0,
                tables=dict(m0=Discrete2DFunction(5, 5, m0), d0=Discrete2DFunction(5, 5, d0)),
                functions=tabulated2d_oracle_functions(m0, d0))


def tabulated2d_oracle_functions(m0, d0):
    return dict(m0=tabulated2d_oracle.Lookup2D(5, 5, m0), d0=tabulated2d_oracle.Lookup2D(5, 5, d0))


def excluded(n, pairs, seed=13):
    """a ParticlePair value and a ParticlePair energy term with exclusions, beside a term without"""
    rng = np.random.default_rng(seed)
    return dict(per_particle=['q', 's'], params=np.stack([rng.uniform(0.5, 1.0, n), rng.uniform(0.2, 0.3, n)], axis=1), globals=dict(k=3.0),
                computed=[('n', 'q2*exp(-r/s1)', PAIR), ('w', '1/(1+n)', SINGLE)],
                terms=[('k*q1*q2*w1*w2/(r+0.1)', PAIR), ('0.5*(n1+n2)*exp(-r*r)', PAIR_NX), ('q*w^2', SINGLE)],
                method=0, cutoff=0.0, exclusions=list(pairs))


def three_values(n, seed=17):
    """3 computed values and a pair term that names two of them: r, a1, a2, c1, c2 -- two passes"""
    rng = np.random.default_rng(seed)
    return dict(per_particle=['q'], params=rng.uniform(0.5, 1.0, (n, 1)), globals={},
                computed=[('a', 'q1*q2/(1+r^2)', PAIR_NX), ('b', 'sqrt(1+a)', SINGLE), ('c', 'a*b+q', SINGLE)],
                terms=[('a1*c2+c1*a2*exp(-r)', PAIR_NX), ('b*c', SINGLE)], method=0, cutoff=0.0)


def single_only(n, seed=19):
    """no pair energy term: the pair launches of the terms have nothing to walk"""
    rng = np.random.default_rng(seed)
    return dict(per_particle=['q'], params=rng.uniform(0.5, 1.0, (n, 1)), globals=dict(c=2.0),
                computed=[('v', 'q2*exp(-c*r)', PAIR_NX)], terms=[('q*log(1+v)', SINGLE)], method=0, cutoff=0.0)
