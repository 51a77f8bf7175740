"""CPU: the host set-up of the custom forces (csrc/custom_plan.h) through tools/custom_plan_check.cpp, a program with its own main built
with -fsanitize=address,undefined and run as a child process.  The test writes descriptors, the program runs cst_build_plan and dumps
the plan or the refusal, and the test compares: the layouts with ones computed HERE, with numpy, from the layout that
include/remd_hip_custom.h and DESIGN.md sections 12-21 document (never from a dump), the refusals with their exact sentences."""
import math
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOND, ANGLE, TORSION, EXTERNAL, COMPOUND, CENTROID, NONBONDED, CV, CMAP = range(9)
CONST, VAR, PARAM, GLOBAL, ADD, MUL, POWI, DISTANCE, TABLE1D, LOOKUP1D, TABLE2D, LOOKUP2D, LOOKUP3D = 0, 1, 2, 3, 4, 6, 9, 35, 38, 39, 40, 41, 42
INTS = ['kind', 'n_terms', 'n_params', 'n_program', 'n_consts', 'stack_depth', 'n_globals', 'periodic', 'force_group', 'n_particles',
        'n_groups', 'nb_method', 'long_range_correction', 'n_cvs', 'n_maps']
ARRAYS = [('atoms', 'i'), ('params', 'd'), ('program', 'i'), ('consts', 'd'), ('global_defaults', 'd'), ('group_offsets', 'i'),
          ('group_atoms', 'i'), ('group_weights', 'd'), ('excl_offsets', 'i'), ('excl_atoms', 'i'), ('cv_offsets', 'i'), ('cv_atoms', 'i'),
          ('cv_reference', 'd'), ('map_index', 'i'), ('map_offsets', 'i')]
N, NPAD = 65, 128
FACTS = dict(N=N, Npad=NPAD, K=3, bare=0, boxes=[], states_version=7)
WHO = 'force 0: '


def desc(kind, n_terms, **kw):
    """a descriptor; n_program and n_consts follow the arrays unless given; the default program is `VAR 0` (depth 1)"""
    d = dict.fromkeys(INTS, 0)
    d.update({name: None for name, _ in ARRAYS})
    d.update(kind=kind, n_terms=n_terms, cutoff=0.0, switch_distance=-1.0, program=None if kind == CMAP else [VAR, 0], stack_depth=0 if kind == CMAP else 1)
    d.update(kw)
    d.setdefault('n_program', 0)
    if 'n_program' not in kw:
        d['n_program'] = 0 if d['program'] is None else len(d['program']) // 2
    if 'n_consts' not in kw:
        d['n_consts'] = 0 if d['consts'] is None else len(d['consts'])
    return d


def write_case(f, facts, descs):
    f.write(struct.pack('<5iq', facts['N'], facts['Npad'], facts['K'], facts['bare'], len(facts['boxes']), facts['states_version']))
    np.asarray(facts['boxes'], dtype='<f8').tofile(f)
    f.write(struct.pack('<i', len(descs)))
    for d in descs:
        f.write(struct.pack('<15i2d', *[d[k] for k in INTS], d['cutoff'], d['switch_distance']))
        for name, t in ARRAYS:
            a = d[name]
            f.write(struct.pack('<i', -1 if a is None else len(np.ravel(a))))
            if a is not None:
                np.ravel(np.asarray(a, dtype='<i4' if t == 'i' else '<f8')).tofile(f)


@pytest.fixture(scope='module')
def planner(tmp_path_factory):
    """tools/custom_plan_check.cpp built with the sanitizers; returns run(cases) -> one result per case: the refusal's sentence, or the dump
    as {name: list of values}"""
    cxx = shutil.which('g++') or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    tmp = tmp_path_factory.mktemp('custom_plan')
    exe = str(tmp / 'custom_plan_check')
    subprocess.check_call([cxx, '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           os.path.join(ROOT, 'tools', 'custom_plan_check.cpp'), '-o', exe])
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


# ---- the layout, computed here -------------------------------------------------------------------------------------------------------------
PART_OF_KIND = {BOND: 0, ANGLE: 0, TORSION: 0, EXTERNAL: 0, COMPOUND: 1, NONBONDED: 2, CENTROID: 3, CV: 4, CMAP: 5}   # the term-space order
WIDTH = {BOND: 2, ANGLE: 3, TORSION: 4, EXTERNAL: 1, NONBONDED: 0, CV: 0, CMAP: 8}
FORCE_FIELDS = ['kind', 'periodic', 'n_terms', 'n_params', 'n_particles', 'slot0', 'npad', 'par0', 'prog0', 'n_prog', 'const0', 'nb_method', 'excl0',
                'lrc', 'cv0', 'n_cvs', 'map0', 'n_maps', 'cutoff', 'switch_dist']


def expected(facts, descs):
    n, Npad, K = len(descs), facts['Npad'], facts['K']
    F, par, prog, consts, excl_off, excl_atoms, cv_off, cv_atoms, cv_ref, map_off = [], [], [], [], [], [], [], [], [], []
    for d in descs:
        kind, nt, npar = d['kind'], d['n_terms'], d['n_params']
        f = dict.fromkeys(FORCE_FIELDS, 0)
        f.update(kind=kind, periodic=int(d['periodic'] != 0), n_terms=nt, n_params=npar, n_particles=d['n_particles'] if kind in (COMPOUND, CENTROID) else WIDTH[kind],
                 npad=-(-nt // 64) * 64, par0=len(par), prog0=len(prog) // 2, n_prog=d['n_program'], const0=len(consts), cutoff=0.0, switch_dist=-1.0)
        stride = f['npad']
        if kind == NONBONDED:
            tiles = -(-nt // 64)
            f.update(npad=64 * tiles * (tiles + 1) // 2, nb_method=d['nb_method'], cutoff=d['cutoff'] if d['nb_method'] else 0.0,
                     switch_dist=d['switch_distance'] if d['switch_distance'] >= 0 else -1.0, lrc=int(d['long_range_correction'] != 0), excl0=len(excl_off))
            stride = Npad
            excl_off += [len(excl_atoms) + o for o in d['excl_offsets']]      # rebased: rows of this force start where the atoms of the ones before end
            excl_atoms += list(d['excl_atoms'] or [])[:d['excl_offsets'][-1]]
        if npar:
            P = np.asarray(d['params'], dtype=float).reshape(nt, npar)
            par += P[np.minimum(np.arange(stride), nt - 1)].T.ravel().tolist()           # [n_params][stride], padding repeats the last term
        prog += list(d['program'] or [])
        consts += list(d['consts'] or [])
        if kind == CV:
            f.update(cv0=len(cv_off) - 1 if cv_off else 0, n_cvs=d['n_cvs'])
            if not cv_off:
                cv_off.append(0)
            cv_off += [len(cv_atoms) + o for o in d['cv_offsets'][1:]]
            cv_atoms += list(d['cv_atoms'])
            cv_ref += np.ravel(d['cv_reference']).tolist()
        if kind == CMAP:
            f.update(map0=len(map_off), n_maps=d['n_maps'])
            map_off += [f['const0'] + o for o in d['map_offsets']]
        F.append(f)
    # the term space: part by part, descriptors' order within a part
    total, part_end, wave_force = 0, [], []
    for part in range(6):
        for i, f in enumerate(F):
            if PART_OF_KIND[f['kind']] == part:
                f['slot0'] = total
                total += f['npad']
                wave_force += [i] * (f['npad'] // 64)
        part_end.append(total // 64)
    rows = max([4] + [f['n_particles'] for f in F])
    atoms = np.zeros((rows, total), dtype=int)
    grp_off, grp_atoms, grp_w, grp_periodic, n_groups = [], [], [], [], 0
    named = []
    for f, d in zip(F, descs):
        wd, nt, group0 = f['n_particles'], f['n_terms'], n_groups
        if f['kind'] == CENTROID:
            if not grp_off:
                grp_off.append(0)
            grp_off += [len(grp_atoms) + o for o in d['group_offsets'][1:]]
            grp_atoms += list(d['group_atoms']); grp_w += list(d['group_weights'])
            grp_periodic += [f['periodic']] * d['n_groups']
            n_groups += d['n_groups']
            named += [[] for _ in range(d['n_groups'])]
        if wd:
            A = np.asarray(d['atoms']).reshape(nt, wd) + (group0 if f['kind'] == CENTROID else 0)
            atoms[:wd, f['slot0']:f['slot0'] + f['npad']] = A[np.minimum(np.arange(f['npad']), nt - 1)].T
        if f['kind'] == CENTROID:
            for b in range(nt):
                for a in range(wd):
                    named[A[b, a]].append((f['slot0'] + b - 64 * part_end[2]) * 8 + a)
    ref_off = ([0] + np.cumsum([len(v) for v in named]).tolist()) if n_groups else []
    map_index = np.zeros(total - 64 * part_end[4], dtype=int)
    for f, d in zip(F, descs):
        if f['kind'] == CMAP:
            m = np.asarray(d['map_index'])[np.minimum(np.arange(f['npad']), f['n_terms'] - 1)]
            map_index[f['slot0'] - 64 * part_end[4]:][:f['npad']] = m
    periodic_cutoff = max([0.0] + [d['cutoff'] for d in descs if d['kind'] == NONBONDED and d['nb_method'] == 2])
    mol_first, mol_size = [], []
    if periodic_cutoff > 0 and facts['bare']:
        label = np.arange(facts['N'])
        edges = [(t[0], a) for f, d in zip(F, descs) if f['kind'] in (BOND, ANGLE, TORSION, COMPOUND, CMAP)
                 for t in np.asarray(d['atoms']).reshape(f['n_terms'], f['n_particles']) for a in t[1:]]
        for _ in range(facts['N']):
            for p, q in edges:
                label[p] = label[q] = min(label[p], label[q])
        mols = [np.flatnonzero(label == r) for r in np.unique(label)]
        if all(np.array_equal(m, np.arange(m[0], m[0] + len(m))) for m in mols):
            mol_first, mol_size = [int(m[0]) for m in mols], [len(m) for m in mols]
    defaults = list(descs[0]['global_defaults'] or [])
    return dict(force=[[f[k] for k in FORCE_FIELDS] for f in F], part_end=part_end, part_begin=[0] + part_end[:-1], wave_force=wave_force,
                atoms=atoms.ravel().tolist(), par=par, prog=prog, consts=consts, glob=(defaults * K) or [0.0], defaults=defaults,
                grp_off=grp_off, grp_atoms=grp_atoms, grp_w=grp_w, grp_periodic=grp_periodic, ref_off=ref_off, refs=[x for v in named for x in v],
                cv_off=cv_off, cv_atoms=cv_atoms, cv_ref=cv_ref, map_off=map_off, map_index=map_index.tolist(), excl_off=excl_off,
                excl_atoms=excl_atoms, lrc=[0.0] * (max(K, 1) * n), mol_first=mol_first, mol_size=mol_size, periodic_cutoff=[periodic_cutoff],
                scalars=[n, len(defaults), K, total, n_groups, len(cv_atoms) and len(cv_off) - 1, 1, int(any(f['lrc'] for f in F)), 0, facts['states_version']])


# ---- descriptors ----------------------------------------------------------------------------------------------------------------------------
G = dict(n_globals=2, global_defaults=[0.25, 4.0], force_group=3)
RNG = np.random.default_rng(12)


def listed(kind, n_terms, stride=1, **kw):
    """n_terms terms of a one-variable kind with two parameters each: term t names atoms stride t, stride t + 1, ..."""
    wd = WIDTH[kind]
    atoms = [[(stride * t + a) % N for a in range(wd)] for t in range(n_terms)]
    return desc(kind, n_terms, atoms=atoms, n_params=2, params=RNG.normal(size=(n_terms, 2)), program=[PARAM, 1, VAR, 0, MUL, 0, CONST, 0, ADD, 0], stack_depth=2,
                consts=[1.5], **G, **kw)


def compound(n_terms, n_particles):
    atoms = [[(t + 7 * a) % N for a in range(n_particles)] for t in range(n_terms)]
    return desc(COMPOUND, n_terms, atoms=atoms, n_particles=n_particles, n_params=1, params=RNG.normal(size=(n_terms, 1)),
                program=[DISTANCE, 0 | (n_particles - 1) << 4, PARAM, 0, MUL, 0], stack_depth=2, **G)


def nonbonded(method=0, cutoff=0.0, lrc=0, excl=()):
    rows = [[] for _ in range(N)]
    for a, b in excl:
        rows[a].append(b); rows[b].append(a)
    off = [0] + np.cumsum([len(r) for r in rows]).tolist()
    return desc(NONBONDED, N, n_params=2, params=RNG.normal(size=(N, 2)), program=[PARAM, 0, PARAM, 3, MUL, 0, VAR, 0, MUL, 0], stack_depth=2,
                nb_method=method, cutoff=cutoff, periodic=int(method == 2), long_range_correction=lrc, excl_offsets=off,
                excl_atoms=[b for r in rows for b in sorted(r)], **G)


def centroid(groups, bonds, periodic=0):
    off = [0] + np.cumsum([len(g) for g in groups]).tolist()
    w = [1.0 / len(g) if len(g) in (1, 2, 4) else (0.5 if k == 0 else 0.5 / (len(g) - 1)) for g in groups for k in range(len(g))]
    return desc(CENTROID, len(bonds), atoms=bonds, n_particles=len(bonds[0]), n_groups=len(groups), group_offsets=off, group_atoms=[a for g in groups for a in g],
                group_weights=w, program=[DISTANCE, 0 | 1 << 4], stack_depth=1, periodic=periodic, **G)


def cv(sets):
    off = [0] + np.cumsum([len(s) for s in sets]).tolist()
    ref = []
    for s in sets:
        x = RNG.normal(size=(len(s), 3))
        x[-1] = -np.sum(x[:-1], axis=0)              # centred (the sum is tested against 1e-9 n)
        ref.append(x)
    return desc(CV, 1, n_cvs=len(sets), cv_offsets=off, cv_atoms=[a for s in sets for a in s], cv_reference=np.concatenate(ref),
                program=[VAR, len(sets) - 1], stack_depth=1, **G)


def cmap_block(nx, seed):
    return [nx, nx, 0.0, 2.0 * math.pi, 0.0, 2.0 * math.pi, 1.0, 0.0] + np.random.default_rng(seed).normal(size=4 * nx * nx).tolist()


def cmap(n_terms, sizes=(3, 4), **kw):
    blocks = [cmap_block(nx, nx) for nx in sizes]
    off = [0] + np.cumsum([len(b) for b in blocks]).tolist()[:-1]
    atoms = [[(t + a) % N for a in range(4)] + [(t + 1 + a) % N for a in range(4)] for t in range(n_terms)]
    d = dict(atoms=atoms, n_particles=8, n_maps=len(sizes), map_offsets=off, map_index=[(t + 1) % len(sizes) for t in range(n_terms)],
             consts=[x for b in blocks for x in b], **G)
    d.update(kw)
    return desc(CMAP, n_terms, **d)


def check(got, want):
    assert isinstance(got, dict), got
    for name, w in want.items():
        assert got[name] == w, name


def test_every_kind_in_one_handle_given_against_the_part_order(planner):
    """CMAP first and a bond force last: slot0 follows the parts, the energy columns (the records' order) the descriptors; 1, 64 and 65
    terms; six particles per compound bond, so the atom table has eight rows (the CMAP forces') and more than four are filled by two kinds;
    a nonbonded force of 65 particles has 3 tiles; two CMAP forces of 2 maps each, so map0 and const0 both matter; two CV forces"""
    descs = [cmap(65), cmap(1, sizes=(4, 3)), cv([[3, 9, 27, 64], [0, 1, 2], [5, 4, 3, 2, 1]]), cv([[10, 20, 30]]),
             centroid([[0, 1], [2], [3, 4, 5]], [[0, 1], [1, 2]]), nonbonded(excl=[(0, 1), (0, 64), (63, 64)]), compound(64, 6), listed(BOND, 65)]
    (got,) = planner([(FACTS, descs)])
    want = expected(FACTS, descs)
    check(got, want)
    # the figures themselves, by hand: bond 128 slots, compound 64, nonbonded 3 tiles, centroid 64, the CV forces 64 each, the CMAP forces 128 and 64
    assert got['part_end'] == [2, 3, 6, 7, 9, 12] and [f[5] for f in got['force']] == [576, 704, 448, 512, 384, 192, 128, 0]
    assert len(got['atoms']) == 8 * 768 and got['scalars'][3] == 768


def test_two_of_a_kind_share_the_tables_and_custom_bonds_give_contiguous_molecules(planner):
    """two centroid forces that share no groups (one group named by two bonds, and by both positions of one), two nonbonded forces
    (excl0 and the rebased rows; the periodic one's cutoff and correction), angles, torsions, external terms; no built-in force, so the
    bonds 0-1, 2-3, ... and the angles and torsions over 0 ... 8 make the molecule table"""
    facts = dict(FACTS, bare=1, boxes=[3.0, 3.5, 4.0] * 2)
    descs = [centroid([[8, 9, 10, 11], [1, 0]], [[1, 0], [1, 1], [0, 1]], periodic=1), nonbonded(2, 1.2, lrc=1, excl=[(1, 2), (2, 3)]),
             listed(TORSION, 1), centroid([[20], [30, 31], [40, 41, 42]], [[2, 0, 1]]), nonbonded(1, 0.9, excl=[(5, 6)]), listed(ANGLE, 3, stride=3),
             listed(EXTERNAL, 64), desc(BOND, 28, atoms=[[2 * t + 9, 2 * t + 10] for t in range(28)], **G)]
    (got,) = planner([(facts, descs)])
    want = expected(facts, descs)
    check(got, want)
    # (the torsion 0-1-2-3 and the angles 0-1-2, 3-4-5 make one molecule, the angle 6-7-8 another)
    assert got['mol_first'] == [0, 6] + list(range(9, 65, 2)) and got['mol_size'] == [6, 3] + [2] * 28 and got['periodic_cutoff'] == [1.2]
    assert got['ref_off'] == [0, 2, 6, 7, 8, 9] and got['scalars'][7] == 1


def test_custom_bonds_that_do_not_give_contiguous_molecules_leave_the_table_empty(planner):
    facts = dict(FACTS, bare=1)
    descs = [nonbonded(2, 1.0), desc(BOND, 1, atoms=[[0, 2]], **G)]
    built_in = dict(facts, bare=0)               # the same set beside a built-in force: no table either (the molecules are that force's)
    got = planner([(facts, descs), (built_in, descs), (facts, [nonbonded(2, 1.0), desc(BOND, 1, atoms=[[0, 1]], **G)])])
    check(got[0], expected(facts, descs))
    assert got[0]['mol_first'] == [] and got[1]['mol_first'] == [] and got[2]['mol_first'] == [0] + list(range(2, 65)) and got[2]['mol_size'] == [2] + [1] * 63


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def _prog(program, depth, kind=BOND, **kw):
    d = listed(kind, 2)
    d.update(program=program, n_program=len(program) // 2, stack_depth=depth)
    d.update(kw)
    d['n_consts'] = kw.get('n_consts', len(d['consts']))
    return [d]


def _but(d, **kw):
    d = dict(d); d.update(kw)
    return [d]


T1 = [3.0, 0.0, 1.0, 0.0] + [0.0] * 6                          # a spline block of 3 points
T2 = [2.0, 2.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0] + [0.0] * 16     # a patch block of 2 x 2 nodes
CV1 = cv([[0, 1, 2]])
CEN = centroid([[0, 1], [2]], [[0, 1]])
TWO = [VAR, 0, VAR, 0]
BLOCK = cmap_block(3, 1)
REFUSALS = [
    ('more than REMD_CUSTOM_MAX_FORCES custom forces', [listed(BOND, 1)] * 9),
    ('more than REMD_CUSTOM_MAX_GLOBALS global parameters', _but(listed(BOND, 1), n_globals=17, global_defaults=[0.0] * 17)),
    ('global_defaults missing', _but(listed(BOND, 1), global_defaults=None)),
    (WHO + 'unknown kind', _but(listed(BOND, 1), kind=9)),
    (WHO + 'n_particles is 8 for a CMAP force (two dihedrals of four particles)', _but(cmap(2), n_particles=4)),
    (WHO + 'n_particles is 1 ... REMD_CUSTOM_MAX_PARTICLES for a compound-bond or centroid-bond force and 0 for every other kind', _but(compound(2, 2), n_particles=9)),
    (WHO + 'n_particles is 1 ... REMD_CUSTOM_MAX_PARTICLES for a compound-bond or centroid-bond force and 0 for every other kind', _but(listed(BOND, 1), n_particles=2)),
    (WHO + 'no terms', _but(listed(BOND, 1), n_terms=0)),
    (WHO + 'no terms', _but(listed(BOND, 1), atoms=None)),
    (WHO + '0 ... REMD_CUSTOM_MAX_PARAMS parameters per term are supported', _but(listed(BOND, 1), n_params=17, params=[0.0] * 17)),
    (WHO + '0 ... REMD_CUSTOM_MAX_PARAMS parameters per term are supported', _but(listed(BOND, 1), params=None)),
    (WHO + 'a nonbonded force has 64 particles, the system has 65', _but(nonbonded(), n_terms=64)),
    (WHO + 'a nonbonded force takes at most REMD_CUSTOM_MAX_PARAMS / 2 per-particle parameters', _but(nonbonded(), n_params=9, params=np.zeros((N, 9)))),
    (WHO + 'unknown nonbonded method (0 NoCutoff, 1 CutoffNonPeriodic, 2 CutoffPeriodic)', _but(nonbonded(), nb_method=3)),
    (WHO + 'a nonbonded force is periodic exactly where its method is CutoffPeriodic', _but(nonbonded(), periodic=1)),
    (WHO + 'a cutoff that is not positive', _but(nonbonded(1, 1.0), cutoff=0.0)),
    (WHO + 'the switching distance must lie in (0, cutoff) and needs a cutoff', _but(nonbonded(1, 1.0), switch_distance=1.0)),
    (WHO + 'the switching distance must lie in (0, cutoff) and needs a cutoff', _but(nonbonded(), switch_distance=0.5)),
    (WHO + 'a long-range correction needs CutoffPeriodic', _but(nonbonded(1, 1.0), long_range_correction=1)),
    (WHO + 'excl_offsets [N + 1] must start at 0', _but(nonbonded(), excl_offsets=[1] * (N + 1), excl_atoms=[0])),
    (WHO + 'excl_offsets [N + 1] must start at 0', _but(nonbonded(), excl_offsets=None)),
    (WHO + 'excl_offsets must not decrease', _but(nonbonded(), excl_offsets=[0, 1] + [0] * (N - 1), excl_atoms=[5])),
    (WHO + 'exclusion index out of range', _but(nonbonded(), excl_offsets=[0] + [1] * N, excl_atoms=[N])),
    (WHO + 'a particle excluded from itself', _but(nonbonded(), excl_offsets=[0] + [1] * N, excl_atoms=[0])),
    (WHO + 'box smaller than twice the cutoff', nonbonded(2, 1.0), dict(FACTS, boxes=[3.0, 3.0, 3.0, 3.0, 1.99, 3.0])),
    (WHO + 'a collective-variable force has n_terms = 1, no per-term parameters and is not periodic', _but(CV1, n_terms=2)),
    (WHO + 'a collective-variable force has 1 ... REMD_CUSTOM_MAX_CVS collective variables', _but(CV1, n_cvs=4)),
    (WHO + 'a collective-variable force needs cv_offsets, cv_atoms and cv_reference', _but(CV1, cv_reference=None)),
    (WHO + 'cv_offsets must start at 0', _but(CV1, cv_offsets=[1, 3])),
    (WHO + 'collective variable 0: an RMSD needs at least 3 particles', _but(CV1, cv_offsets=[0, 2])),
    (WHO + 'collective variable 0: particle index out of range', _but(CV1, cv_atoms=[0, 1, N])),
    (WHO + 'collective variable 0: particle 1 named twice', _but(CV1, cv_atoms=[0, 1, 1])),
    (WHO + 'collective variable 0: a reference position that is not finite', _but(CV1, cv_reference=[0.0] * 8 + [math.inf])),
    (WHO + 'collective variable 0: the reference must be centred on its own centroid (within 1e-9 nm)', _but(CV1, cv_reference=[0.0] * 8 + [1e-8])),
    (WHO + 'a CMAP force has no per-term parameters and no program', _but(cmap(2), n_program=1, program=[VAR, 0])),
    (WHO + 'a CMAP force has 1 ... REMD_CUSTOM_MAX_MAPS maps', _but(cmap(2), n_maps=65)),
    (WHO + 'a CMAP force needs map_index, map_offsets and the maps\' blocks in consts', _but(cmap(2), map_index=None)),
    (WHO + 'term 1: map index out of range', _but(cmap(2), map_index=[0, 2])),
    (WHO + 'map 1: a block that runs past n_consts', _but(cmap(2, sizes=(3,)), n_maps=2, map_offsets=[0, 37])),
    (WHO + 'map 0: a block that runs past n_consts', _but(cmap(2, sizes=(3,)), consts=BLOCK[:-1], n_consts=len(BLOCK) - 1)),
    (WHO + 'map 0: a block whose sizes are not nx = ny, an integer 3 ... 256', _but(cmap(2, sizes=(3,)), consts=[2.0, 2.0] + BLOCK[2:])),
    (WHO + 'map 0: a block that is not periodic', _but(cmap(2, sizes=(3,)), consts=BLOCK[:6] + [0.0] + BLOCK[7:])),
    (WHO + 'map 0: a block whose range is not [0, 2 pi] in both angles', _but(cmap(2, sizes=(3,)), consts=BLOCK[:3] + [6.28] + BLOCK[4:])),
    (WHO + 'map 0: a node value that is not finite', _but(cmap(2, sizes=(3,)), consts=BLOCK[:-1] + [math.nan])),
    ('force 1: every descriptor must carry the handle\'s n_globals', [listed(BOND, 1)] + _but(listed(BOND, 1), n_globals=1)),
    ('force 1: global_defaults differ between the descriptors', [listed(BOND, 1)] + _but(listed(BOND, 1), global_defaults=[0.25, 4.5])),
    ('force 1: every custom force of a handle must sit in one force group (0 ... 31)', [listed(BOND, 1)] + _but(listed(BOND, 1), force_group=4)),
    (WHO + 'every custom force of a handle must sit in one force group (0 ... 31)', _but(listed(BOND, 1), force_group=32)),
    (WHO + 'an empty program', _prog([], 0)),
    (WHO + 'a program over REMD_CUSTOM_MAX_PROGRAM instructions', _prog([VAR, 0] + [VAR, 0, ADD, 0] * 128, 2)),
    (WHO + 'a constant index out of range', _prog([CONST, 1], 1)),
    (WHO + 'a variable index out of range', _prog([VAR, 1], 1)),
    (WHO + 'a variable index out of range', _but(CV1, program=[VAR, 1])),
    (WHO + 'a parameter index out of range', _prog([PARAM, 2], 1)),
    (WHO + 'a global-parameter index out of range', _prog([GLOBAL, 2], 1)),
    (WHO + 'a function of particles outside a compound-bond or centroid-bond force', _prog([DISTANCE, 16], 1)),
    (WHO + 'a particle slot out of range', _but(compound(2, 2), program=[DISTANCE, 0 | 2 << 4], n_program=1, stack_depth=1)),
    (WHO + 'a particle slot out of range', _but(compound(2, 2), program=[DISTANCE, 0 | 1 << 4 | 1 << 8], n_program=1, stack_depth=1)),
    (WHO + 'an integer power beyond +-64', _prog([VAR, 0, POWI, 65], 1)),
    (WHO + 'a table offset out of range', _prog([VAR, 0, TABLE1D, 10], 1, consts=T1)),
    (WHO + 'a table offset out of range', _prog(TWO + [TABLE2D, -1], 2, consts=T2)),
    (WHO + 'a table whose point count is not an integer 2 ... REMD_CUSTOM_MAX_TABLE_POINTS', _prog([VAR, 0, TABLE1D, 0], 1, consts=[2.5] + T1[1:])),
    (WHO + 'a lookup table whose value count is not an integer 1 ... REMD_CUSTOM_MAX_TABLE_POINTS', _prog([VAR, 0, LOOKUP1D, 0], 1, consts=[0.0, 1.0])),
    (WHO + 'a table that runs past n_consts', _prog([VAR, 0, TABLE1D, 0], 1, consts=T1[:-1])),
    (WHO + 'a table that runs past n_consts', _prog([VAR, 0, LOOKUP1D, 0], 1, consts=[2.0, 1.0])),
    (WHO + 'a table that runs past n_consts', _prog(TWO + [TABLE2D, 0], 2, consts=T2[:7])),
    (WHO + 'a table that runs past n_consts', _prog(TWO + [TABLE2D, 0], 2, consts=T2[:-1])),
    (WHO + 'a table whose bounds are not finite with min < max', _prog([VAR, 0, TABLE1D, 0], 1, consts=[3.0, 1.0, 1.0, 0.0] + [0.0] * 6)),
    (WHO + 'a table whose bounds are not finite with min < max', _prog(TWO + [TABLE2D, 0], 2, consts=T2[:5] + [math.inf] + T2[6:])),
    (WHO + 'a table whose periodic flag is neither 0 nor 1', _prog([VAR, 0, TABLE1D, 0], 1, consts=T1[:3] + [2.0] + T1[4:])),
    (WHO + 'a table whose periodic flag is neither 0 nor 1', _prog(TWO + [TABLE2D, 0], 2, consts=T2[:6] + [0.5] + T2[7:])),
    (WHO + 'a 2D table whose size is not an integer 2 ... REMD_CUSTOM_MAX_TABLE_CELLS', _prog(TWO + [TABLE2D, 0], 2, consts=[2.0, 1.0] + T2[2:])),
    (WHO + 'a lookup table whose size is not an integer 1 ... REMD_CUSTOM_MAX_TABLE_CELLS', _prog(TWO + [VAR, 0, LOOKUP3D, 0], 3, consts=[1.0, 1.0, 0.0, 0.0, 7.0])),
    (WHO + 'a table of more than REMD_CUSTOM_MAX_TABLE_CELLS cells', _prog(TWO + [LOOKUP2D, 0], 2, consts=[65536.0, 2.0])),
    (WHO + 'an unknown opcode', _prog([VAR, 0, 43, 0], 1)),
    (WHO + 'a program that pops an empty stack', _prog([VAR, 0, ADD, 0], 1)),
    (WHO + 'a program over REMD_CUSTOM_MAX_STACK stack slots', _prog([VAR, 0] * 17 + [ADD, 0] * 16, 17)),
    (WHO + 'a program that does not leave exactly one value', _prog(TWO, 2)),
    (WHO + 'a stack depth that is not the program\'s', _prog(TWO + [ADD, 0], 1)),
    (WHO + 'a centroid-bond force needs n_groups > 0, group_offsets, group_atoms and group_weights', _but(CEN, group_weights=None)),
    (WHO + 'group_offsets must start at 0', _but(CEN, group_offsets=[1, 2, 3])),
    (WHO + 'group_offsets must increase (an empty group has no centroid)', _but(CEN, group_offsets=[0, 2, 2])),
    (WHO + 'group atom index out of range', _but(CEN, group_atoms=[0, 1, N])),
    (WHO + 'negative group weight', _but(CEN, group_weights=[1.5, -0.5, 1.0])),
    (WHO + 'the weights of a group must sum to 1 (within 1e-12)', _but(CEN, group_weights=[0.5, 0.5 + 1e-11, 1.0])),
    (WHO + 'group index out of range', _but(CEN, atoms=[[0, 2]])),
    (WHO + 'atom index out of range', _but(listed(BOND, 2), atoms=[[0, 1], [1, N]])),
    (WHO + 'atom index out of range', _but(cmap(1), atoms=[[0, 1, 2, 3, 1, 2, 3, -1]])),
]
REFUSALS = [(r[0], r[1] if isinstance(r[1], list) else [r[1]], r[2] if len(r) > 2 else FACTS) for r in REFUSALS]


def test_every_refusal_has_its_exact_sentence_and_leaves_nothing_behind(planner):
    """one fault per descriptor set; behind each refusal a valid set runs in the same process on the same plan object, and its plan is the
    one a fresh process computes"""
    valid = [listed(ANGLE, 65), cmap(3)]
    cases = []
    for sentence, descs, facts in REFUSALS:
        cases += [(facts, descs), (FACTS, valid)]
    got = planner(cases)
    (fresh,) = planner([(FACTS, valid)])
    check(fresh, expected(FACTS, valid))
    for k, (sentence, descs, facts) in enumerate(REFUSALS):
        assert got[2 * k] == sentence, (k, sentence)
        assert got[2 * k + 1] == fresh, (k, sentence)


def test_the_list_of_refusals_is_the_header_s(planner):
    """every sentence the planner can return (the string literals behind `return` in csrc/custom_plan.h) is part of a listed refusal"""
    text = open(os.path.join(ROOT, 'openmmtools_amd', 'csrc', 'custom_plan.h')).read()
    literals = set()
    for line in text.splitlines():
        if 'return' in line and not line.lstrip().startswith('//'):
            literals.update(s for s in re.findall(r'"((?:[^"\\]|\\.)*)"', line.split('return', 1)[1]) if s.strip())
        elif re.match(r'\s*[:?] "', line):                    # the continuation lines of a `return a ? "..." : "..."`
            literals.update(re.findall(r'"((?:[^"\\]|\\.)*)"', line))
    assert len(literals) > 70                                 # (the parsing found them: 26 of check_program, about 50 of the validators)
    listed_sentences = [r[0] for r in REFUSALS]
    missing = [s for s in literals if not any(s in t for t in listed_sentences)]
    assert not missing, missing
