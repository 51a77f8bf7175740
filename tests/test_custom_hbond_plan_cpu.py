"""CPU: the host set-up of the donor-acceptor forces (csrc/custom_hbond_plan.h inside csrc/custom_plan.h) through
tools/custom_hbond_plan_check.cpp, a program with its own main built with -fsanitize=address,undefined and run as a child process, as
tests/test_custom_plan_cpu.py does for the other kinds.  The layout is computed HERE with numpy from what include/remd_hip_custom.h and
DESIGN.md section 23 document (tiles row by row, the padded particle and parameter columns, the rebased exclusion rows), never from a
dump; the refusals are held to their exact sentences."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBOND = 10
CONST, PARAM, GLOBAL, ADD, MUL, DISTANCE, ANGLE = 0, 2, 3, 4, 6, 35, 36
INTS = ['n_terms', 'n_params', 'n_program', 'n_consts', 'stack_depth', 'n_globals', 'periodic', 'force_group', 'nb_method', 'hb_n_donors',
        'hb_n_acceptors', 'hb_n_donor_params', 'hb_n_acceptor_params', 'hb_particle_mask']
ARRAYS = [('program', 'i'), ('consts', 'd'), ('global_defaults', 'd'), ('hb_donor_atoms', 'i'), ('hb_acceptor_atoms', 'i'), ('hb_donor_params', 'd'),
          ('hb_acceptor_params', 'd'), ('hb_excl_offsets', 'i'), ('hb_excl_acceptors', 'i')]
N, NPAD = 700, 704
FACTS = dict(N=N, Npad=NPAD, K=2, bare=0, boxes=[], states_version=3)
WHO = 'force 0: '
RNG = np.random.default_rng(23)


def hbond(nD, nA, npd=1, npa=2, excl=(), method=0, cutoff=0.0, first_atom=0, **kw):
    """nD two-particle donors (atoms first_atom + 2 i, + 2 i + 1) and nA one-particle acceptors behind them; the program is
    distance(d1, a1) * angle(d2, d1, a1) (mask 0b001011)"""
    donors = [[first_atom + 2 * i, first_atom + 2 * i + 1, -1] for i in range(nD)]
    acceptors = [[first_atom + 2 * nD + j, -1, -1] for j in range(nA)]
    rows = [sorted(j for i2, j in excl if i2 == i) for i in range(nD)]
    d = dict.fromkeys(INTS, 0)
    d.update(n_terms=nD, hb_n_donors=nD, hb_n_acceptors=nA, hb_n_donor_params=npd, hb_n_acceptor_params=npa, hb_particle_mask=0b001011,
             program=[DISTANCE, 0 | 3 << 4, ANGLE, 1 | 0 << 4 | 3 << 8, MUL, 0], stack_depth=2, consts=None, n_globals=1, global_defaults=[0.5],
             force_group=2, nb_method=method, periodic=int(method == 2), cutoff=cutoff, hb_donor_atoms=donors, hb_acceptor_atoms=acceptors,
             hb_donor_params=RNG.normal(size=(nD, npd)) if npd else None, hb_acceptor_params=RNG.normal(size=(nA, npa)) if npa else None,
             hb_excl_offsets=[0] + np.cumsum([len(r) for r in rows]).tolist(), hb_excl_acceptors=[j for r in rows for j in r])
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
    tmp = tmp_path_factory.mktemp('custom_hbond_plan')
    exe = str(tmp / 'custom_hbond_plan_check')
    subprocess.check_call([cxx, '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           os.path.join(ROOT, 'tools', 'custom_hbond_plan_check.cpp'), '-o', exe])
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


def expected(descs):
    """what the documented layout gives for donor-acceptor forces alone: every other part of the term space is empty"""
    F, hb_atoms, par, excl_off, excl_atoms, wave_force, total, cutoff = [], [], [], [], [], [], 0, 0.0
    for k, d in enumerate(descs):
        nD, nA = d['hb_n_donors'], d['hb_n_acceptors']
        ndpad, napad = -(-nD // 64) * 64, -(-nA // 64) * 64
        npad = (ndpad // 64) * napad
        F.append([HBOND, d['periodic'], nD, 0, 0, total, npad, len(par), d['nb_method'], len(excl_off), nA, len(hb_atoms),
                  100 * d['hb_n_donor_params'] + d['hb_n_acceptor_params'], d['hb_particle_mask'], d['cutoff'] if d['nb_method'] else 0.0])
        for A, n, pad in ((d['hb_donor_atoms'], nD, ndpad), (d['hb_acceptor_atoms'], nA, napad)):
            hb_atoms += np.asarray(A).reshape(n, 3)[np.minimum(np.arange(pad), n - 1)].T.ravel().tolist()
        for P, n, pad in ((d['hb_donor_params'], nD, ndpad), (d['hb_acceptor_params'], nA, napad)):
            if P is not None:
                par += np.asarray(P, dtype=float).reshape(n, -1)[np.minimum(np.arange(pad), n - 1)].T.ravel().tolist()
        excl_off += [len(excl_atoms) + o for o in d['hb_excl_offsets']]
        excl_atoms += list(d['hb_excl_acceptors'])
        wave_force += [k] * (npad // 64)
        total += npad
        if d['nb_method'] == 2:
            cutoff = max(cutoff, d['cutoff'])
    return dict(force=F, hb_atoms=hb_atoms, par=par, excl_off=excl_off, excl_atoms=excl_atoms, wave_force=wave_force,
                part_end=[0] * 6 + [total // 64], scalars=[len(descs), 1, FACTS['K'], total], periodic_cutoff=[cutoff], map_index=[])


def check(got, want):
    assert isinstance(got, dict), got
    for name, w in want.items():
        assert got[name] == w, name


def test_tiles_padding_and_exclusion_rows_of_two_forces(planner):
    """70 x 130 (2 x 3 tiles, both last blocks partial) with exclusions in every column block, then 1 x 1 with a cutoff and no
    parameters: the second force's offsets all depend on the first's tables"""
    descs = [hbond(70, 130, excl=[(0, 3), (0, 70), (1, 129), (69, 0)]),
             hbond(1, 1, npd=0, npa=0, method=2, cutoff=0.9, first_atom=300)]
    (got,) = planner([(FACTS, descs)])
    check(got, expected(descs))
    assert [f[6] for f in got['force']] == [64 * 6, 64] and got['part_end'][-1] == 7
    assert len(got['hb_atoms']) == 3 * 128 + 3 * 192 + 3 * 64 + 3 * 64


def test_a_bare_periodic_handle_gets_the_donors_and_acceptors_as_molecules(planner):
    d = hbond(3, 2, method=2, cutoff=0.9)
    (got,) = planner([(dict(FACTS, N=8, Npad=64, bare=1), [d])])
    assert got['mol_first'] == [0, 2, 4, 6, 7] and got['mol_size'] == [2, 2, 2, 1, 1]


H = hbond(3, 2)
REFUSALS = [
    (WHO + 'a donor-acceptor force has n_terms = hb_n_donors > 0 and hb_n_acceptors > 0', _but(H, hb_n_acceptors=0)),
    (WHO + 'a donor-acceptor force has n_terms = hb_n_donors > 0 and hb_n_acceptors > 0', _but(H, n_terms=2)),
    (WHO + 'a donor-acceptor force has n_params = 0 (its parameters are hb_donor_params and hb_acceptor_params)', _but(H, n_params=1)),
    (WHO + 'a donor-acceptor force needs hb_donor_atoms and hb_acceptor_atoms', _but(H, hb_acceptor_atoms=None)),
    (WHO + 'a donor-acceptor force takes at most REMD_CUSTOM_MAX_PARAMS per-donor and per-acceptor parameters together',
     _but(H, hb_n_donor_params=9, hb_n_acceptor_params=8, hb_donor_params=np.zeros((3, 9)), hb_acceptor_params=np.zeros((2, 8)))),
    (WHO + 'a parameter table is missing', _but(H, hb_acceptor_params=None)),
    (WHO + 'hb_particle_mask names the particle slots 0 ... 5', _but(H, hb_particle_mask=64)),
    (WHO + 'hb_particle_mask is not the set of particle slots the program names', _but(H, hb_particle_mask=0b001001)),
    (WHO + 'hb_particle_mask is not the set of particle slots the program names', _but(H, hb_particle_mask=0b011011)),
    (WHO + 'unknown nonbonded method (0 NoCutoff, 1 CutoffNonPeriodic, 2 CutoffPeriodic)', _but(H, nb_method=3)),
    (WHO + 'a donor-acceptor force is periodic exactly where its method is CutoffPeriodic', _but(H, periodic=1)),
    (WHO + 'a cutoff that is not positive', _but(H, nb_method=1)),
    (WHO + 'donor 1: atom index out of range', _but(H, hb_donor_atoms=[[0, 1, -1], [2, N, -1], [4, 5, -1]])),
    (WHO + 'acceptor 0: atom index out of range', _but(H, hb_acceptor_atoms=[[-2, -1, -1], [7, -1, -1]])),
    (WHO + 'acceptor 1: the first particle is missing', _but(H, hb_acceptor_atoms=[[6, -1, -1], [-1, 7, -1]])),
    (WHO + 'donor 2: the program names a particle it does not have', _but(H, hb_donor_atoms=[[0, 1, -1], [2, 3, -1], [4, -1, -1]])),
    (WHO + 'donor 0: atom 1 named twice', _but(H, hb_donor_atoms=[[0, 1, 1], [2, 3, -1], [4, 5, -1]])),
    (WHO + 'hb_excl_offsets [hb_n_donors + 1] must start at 0', _but(H, hb_excl_offsets=None)),
    (WHO + 'hb_excl_offsets must not decrease', _but(H, hb_excl_offsets=[0, 1, 0, 0], hb_excl_acceptors=[0])),
    (WHO + 'exclusion index out of range', _but(H, hb_excl_offsets=[0, 1, 1, 1], hb_excl_acceptors=[2])),
    (WHO + 'donor 0 excludes acceptor 1 twice', _but(H, hb_excl_offsets=[0, 2, 2, 2], hb_excl_acceptors=[1, 1])),
    (WHO + 'an exclusion row that is not sorted', _but(H, hb_excl_offsets=[0, 2, 2, 2], hb_excl_acceptors=[1, 0])),
    (WHO + 'donor 1 and acceptor 0 share atom 3 and are not excluded', _but(H, hb_acceptor_atoms=[[3, -1, -1], [7, -1, -1]])),
    (WHO + 'box smaller than twice the cutoff', hbond(3, 2, method=2, cutoff=1.0), dict(FACTS, boxes=[3.0, 3.0, 3.0, 3.0, 1.99, 3.0])),
    (WHO + 'a particle slot out of range', _but(H, program=[DISTANCE, 0 | 6 << 4], n_program=1, stack_depth=1, hb_particle_mask=1)),
    (WHO + 'a variable index out of range', _but(H, program=[1, 0], n_program=1, stack_depth=1, hb_particle_mask=0)),
    (WHO + 'a parameter index out of range', _but(H, program=[PARAM, 3], n_program=1, stack_depth=1, hb_particle_mask=0)),
]
REFUSALS = [(r[0], [r[1]], r[2] if len(r) > 2 else FACTS) for r in REFUSALS]


def test_every_refusal_has_its_exact_sentence_and_leaves_nothing_behind(planner):
    valid = [hbond(65, 3, excl=[(64, 2)])]
    cases = []
    for sentence, descs, facts in REFUSALS:
        cases += [(facts, descs), (FACTS, valid)]
    got = planner(cases)
    (fresh,) = planner([(FACTS, valid)])
    check(fresh, expected(valid))
    for k, (sentence, descs, facts) in enumerate(REFUSALS):
        assert got[2 * k] == sentence, (k, sentence, got[2 * k])
        assert got[2 * k + 1] == fresh, (k, sentence)


def test_a_shared_atom_is_accepted_where_the_pair_is_excluded(planner):
    d = _but(H, hb_acceptor_atoms=[[3, -1, -1], [7, -1, -1]], hb_excl_offsets=[0, 0, 1, 1], hb_excl_acceptors=[0])
    (got,) = planner([(FACTS, [d])])
    assert isinstance(got, dict) and got['excl_atoms'] == [0]


def test_the_list_of_refusals_is_the_header_s():
    """every sentence csrc/custom_hbond_plan.h can return is part of a listed refusal"""
    text = open(os.path.join(ROOT, 'openmmtools_amd', 'csrc', 'custom_hbond_plan.h')).read()
    literals = set()
    for line in text.splitlines():
        if 'return' in line and not line.lstrip().startswith('//'):
            literals.update(s for s in re.findall(r'"((?:[^"\\]|\\.)*)"', line.split('return', 1)[1]) if s.strip())
    assert len(literals) > 20
    listed = [r[0] for r in REFUSALS]
    missing = [s for s in literals if not any(s.strip() in t for t in listed)]
    assert not missing, missing
