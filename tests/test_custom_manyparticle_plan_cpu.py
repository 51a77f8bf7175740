"""CPU: the host set-up of the many-particle forces (csrc/custom_manyparticle_plan.h inside csrc/custom_plan.h) through
tools/custom_manyparticle_plan_check.cpp, a program with its own main built with -fsanitize=address,undefined and run as a child
process, as tests/test_custom_hbond_plan_cpu.py does for its kind.  The layout is computed HERE with numpy from what
include/remd_hip_custom.h and DESIGN.md section 24 document (one wavefront per central particle, parameters and types one column per atom
padded to Npad, the rebased exclusion rows, Npad neighbour rows per force), never from a dump; the refusals are held to their exact
sentences."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MANYPARTICLE = 11
CONST, PARAM, GLOBAL, ADD, MUL, DISTANCE, ANGLE = 0, 2, 3, 4, 6, 35, 36
INTS = ['n_terms', 'n_params', 'n_program', 'n_consts', 'stack_depth', 'n_globals', 'periodic', 'force_group', 'nb_method',
        'mp_permutation_mode', 'mp_particle_mask', 'filter0', 'filter1', 'filter2']
ARRAYS = [('params', 'd'), ('program', 'i'), ('consts', 'd'), ('global_defaults', 'd'), ('mp_types', 'i'), ('excl_offsets', 'i'), ('excl_atoms', 'i')]
N, NPAD = 70, 128
FACTS = dict(N=N, Npad=NPAD, K=2, bare=0, boxes=[], states_version=3)
WHO = 'force 0: '
RNG = np.random.default_rng(24)
ALL = -1                                                                 # (all ones as an int32)


def many(n=N, n_params=2, excl=(), method=1, cutoff=0.5, mode=1, filters=(ALL, ALL, ALL), **kw):
    """n particles; the program is distance(p1, p2) * angle(p2, p1, p3) * PARAM[3 * 1 + 2] (mask 0b111)"""
    rows = [sorted({b for a, b in excl if a == i} | {a for a, b in excl if b == i}) for i in range(n)]
    d = dict.fromkeys(INTS, 0)
    d.update(n_terms=n, n_params=n_params, mp_particle_mask=0b111, mp_permutation_mode=mode, filter0=filters[0], filter1=filters[1], filter2=filters[2],
             program=[DISTANCE, 0 | 1 << 4, ANGLE, 1 | 0 << 4 | 2 << 8, MUL, 0] + ([PARAM, 5, MUL, 0] if n_params >= 2 else []), stack_depth=2,
             consts=None, n_globals=1, global_defaults=[0.5], force_group=2, nb_method=method, periodic=int(method == 2), cutoff=cutoff,
             params=RNG.normal(size=(n, n_params)) if n_params else None, mp_types=(np.arange(n) % 3).tolist(),
             excl_offsets=[0] + np.cumsum([len(r) for r in rows]).tolist(), excl_atoms=[j for r in rows for j in r])
    d.update(kw)
    if 'n_program' not in kw:
        d['n_program'] = 0 if d['program'] is None else len(d['program']) // 2
    if 'n_consts' not in kw:
        d['n_consts'] = 0 if d['consts'] is None else len(d['consts'])
    return d


def _but(d, **kw):
    return dict(d, **kw)


def write_case(f, facts, descs):
    f.write(struct.pack('<5iq', facts['N'], facts['Npad'], facts['K'], facts['bare'], len(facts['boxes']), facts['states_version']))
    np.asarray(facts['boxes'], dtype='<f8').tofile(f)
    f.write(struct.pack('<i', len(descs)))
    for d in descs:
        f.write(struct.pack('<14id', *[d[k] for k in INTS], d['cutoff']))
        for name, t in ARRAYS:
            a = d[name]
            f.write(struct.pack('<i', -1 if a is None else len(np.ravel(a))))
            if a is not None:
                np.ravel(np.asarray(a, dtype='<i4' if t == 'i' else '<f8')).tofile(f)


@pytest.fixture(scope='module')
def planner(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    tmp = tmp_path_factory.mktemp('custom_manyparticle_plan')
    exe = str(tmp / 'custom_manyparticle_plan_check')
    subprocess.check_call([cxx, '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           os.path.join(ROOT, 'tools', 'custom_manyparticle_plan_check.cpp'), '-o', exe])
    count = [0]

    def run(cases):
        count[0] += 1
        path = tmp / ('case%d.bin' % count[0])
        with open(path, 'wb') as f:
            f.write(struct.pack('<i', len(cases)))
            for facts, descs in cases:
                write_case(f, facts, descs)
        done = subprocess.run([exe, str(path)], capture_output=True, text=True)
        assert done.returncode == 0 and 'ERROR' not in done.stderr and 'runtime error' not in done.stderr, done.stderr[-3000:]
        out, plan = [], None
        for line in done.stdout.splitlines():
            if line.startswith('REFUSED '):
                out.append(line[len('REFUSED '):])
            elif line == 'PLAN':
                plan = {'force': []}
            elif line == 'END':
                out.append(plan)
            else:
                w = line.split()
                vals = [float.fromhex(v) if 'x' in v or v in ('inf', '-inf', 'nan') else int(v) for v in w[2:]]
                assert len(vals) == int(w[1])
                if w[0] == 'force':
                    plan['force'].append(vals)
                else:
                    plan[w[0]] = vals
        assert len(out) == len(cases)
        return out
    return run


def expected(descs, facts=FACTS):
    """what the documented layout gives for many-particle forces alone: every other part of the term space is empty"""
    F, types, par, excl_off, excl_atoms, wave_force, total, rows, cutoff = [], [], [], [], [], [], 0, 0, 0.0
    npad_atoms = facts['Npad']
    for k, d in enumerate(descs):
        n = d['n_terms']
        column = np.minimum(np.arange(npad_atoms), n - 1)
        F.append([MANYPARTICLE, d['periodic'], n, d['n_params'], total, 64 * n, len(par), d['nb_method'], len(excl_off), d['mp_permutation_mode'],
                  len(types), rows, d['mp_particle_mask']] + [d['filter%d' % s] & 0xFFFFFFFF for s in range(3)] + [d['cutoff'] if d['nb_method'] else 0.0])
        types += np.asarray(d['mp_types'])[column].tolist()
        if d['params'] is not None:
            par += np.asarray(d['params'], dtype=float).reshape(n, -1)[column].T.ravel().tolist()
        excl_off += [len(excl_atoms) + o for o in d['excl_offsets']]
        excl_atoms += list(d['excl_atoms'])
        wave_force += [k] * n
        total += 64 * n
        rows += npad_atoms
        if d['nb_method'] == 2:
            cutoff = max(cutoff, d['cutoff'])
    return dict(force=F, mp_types=types, par=par, excl_off=excl_off, excl_atoms=excl_atoms, wave_force=wave_force,
                part_end=[0] * 7 + [total // 64], scalars=[len(descs), 1, facts['K'], total, rows], periodic_cutoff=[cutoff])


def check(got, want):
    assert isinstance(got, dict), got
    for name, w in want.items():
        assert got[name] == w, name


def test_one_wavefront_per_particle_padded_columns_and_rebased_rows_of_two_forces(planner):
    descs = [many(excl=[(0, 3), (0, 69), (5, 64)], filters=(1, 6, ALL)),
             many(n_params=0, method=2, cutoff=0.9, mode=0, excl=[(1, 2)])]
    (got,) = planner([(FACTS, descs)])
    check(got, expected(descs))
    assert [f[5] for f in got['force']] == [64 * N, 64 * N] and got['part_end'][-1] == 2 * N
    assert len(got['mp_types']) == 2 * NPAD and len(got['par']) == 2 * NPAD and got['scalars'][4] == 2 * NPAD


def test_nocutoff_takes_129_particles(planner):
    d = many(n=129, method=0, cutoff=0.0)
    (got,) = planner([(dict(FACTS, N=129, Npad=192), [d])])
    check(got, expected([d], dict(FACTS, N=129, Npad=192)))


M = many(n=6, excl=[(0, 1)])
SMALL = dict(FACTS, N=6, Npad=64)
REFUSALS = [
    (WHO + 'a many-particle force has 5 particles, the system has 6', _but(M, n_terms=5)),
    (WHO + 'a many-particle force takes at most REMD_CUSTOM_MAX_PARAMS / 3 per-particle parameters', _but(M, n_params=6, params=np.zeros((6, 6)))),
    (WHO + 'unknown permutation mode (0 SinglePermutation, 1 UniqueCentralParticle)', _but(M, mp_permutation_mode=2)),
    (WHO + 'mp_particle_mask names the particle slots 0 ... 2', _but(M, mp_particle_mask=8)),
    (WHO + 'mp_particle_mask is not the set of particle slots the program names', _but(M, mp_particle_mask=0b011)),
    (WHO + 'unknown nonbonded method (0 NoCutoff, 1 CutoffNonPeriodic, 2 CutoffPeriodic)', _but(M, nb_method=3)),
    (WHO + 'a many-particle force is periodic exactly where its method is CutoffPeriodic', _but(M, periodic=1)),
    (WHO + 'a cutoff that is not positive', _but(M, cutoff=0.0)),
    (WHO + 'a many-particle force without a cutoff takes at most REMD_CUSTOM_MP_MAX_NEIGHBORS + 1 particles', many(n=130, method=0),
     dict(FACTS, N=130, Npad=192)),
    (WHO + 'a many-particle force needs mp_types', _but(M, mp_types=None)),
    (WHO + 'particle 4: a type outside 0 ... 31', _but(M, mp_types=[0, 1, 2, 0, 32, 2])),
    (WHO + 'excl_offsets [N + 1] must start at 0', _but(M, excl_offsets=None)),
    (WHO + 'excl_offsets must not decrease', _but(M, excl_offsets=[0, 1, 0, 0, 0, 0, 0], excl_atoms=[1])),
    (WHO + 'exclusion index out of range', _but(M, excl_offsets=[0, 1, 1, 1, 1, 1, 1], excl_atoms=[6])),
    (WHO + 'a particle excluded from itself', _but(M, excl_offsets=[0, 1, 1, 1, 1, 1, 1], excl_atoms=[0])),
    (WHO + 'an exclusion row that is not sorted, or names a particle twice', _but(M, excl_offsets=[0, 2, 3, 4, 4, 4, 4], excl_atoms=[2, 1, 0, 0])),
    (WHO + 'an exclusion row that is not sorted, or names a particle twice', _but(M, excl_offsets=[0, 2, 3, 3, 3, 3, 3], excl_atoms=[1, 1, 0])),
    (WHO + 'particle 0 excludes 1, which does not exclude it', _but(M, excl_offsets=[0, 1, 1, 1, 1, 1, 1], excl_atoms=[1])),
    (WHO + 'box smaller than twice the cutoff', many(n=6, method=2, cutoff=1.0), dict(SMALL, boxes=[3.0, 3.0, 3.0, 3.0, 1.99, 3.0])),
    (WHO + 'a particle slot out of range', _but(M, program=[DISTANCE, 0 | 3 << 4], n_program=1, stack_depth=1, mp_particle_mask=1)),
    (WHO + 'a variable index out of range', _but(M, program=[1, 0], n_program=1, stack_depth=1, mp_particle_mask=0)),
    (WHO + 'a parameter index out of range', _but(M, program=[PARAM, 6], n_program=1, stack_depth=1, mp_particle_mask=0)),
]
REFUSALS = [(r[0], [r[1]], r[2] if len(r) > 2 else SMALL) for r in REFUSALS]


def test_every_refusal_has_its_exact_sentence_and_leaves_nothing_behind(planner):
    valid = [many(excl=[(64, 2)])]
    cases = []
    for sentence, descs, facts in REFUSALS:
        cases += [(facts, descs), (FACTS, valid)]
    got = planner(cases)
    (fresh,) = planner([(FACTS, valid)])
    check(fresh, expected(valid))
    for k, (sentence, descs, facts) in enumerate(REFUSALS):
        assert got[2 * k] == sentence, (k, sentence, got[2 * k])
        assert got[2 * k + 1] == fresh, (k, sentence)


def test_the_list_of_refusals_is_the_header_s():
    """every sentence csrc/custom_manyparticle_plan.h can return is part of a listed refusal"""
    text = open(os.path.join(ROOT, 'openmmtools_amd', 'csrc', 'custom_manyparticle_plan.h')).read()
    literals = set()
    for line in text.splitlines():
        if 'return' in line and not line.lstrip().startswith('//'):
            literals.update(s for s in re.findall(r'"((?:[^"\\]|\\.)*)"', line.split('return', 1)[1]) if s.strip())
    assert len(literals) > 15
    listed = [r[0] for r in REFUSALS]
    missing = [s for s in literals if not any(s.strip() in t for t in listed)]
    assert not missing, missing
