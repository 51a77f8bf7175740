#!/usr/bin/env python
"""Records the error of the direct-space pair path against the f64 oracle on every case of tests/pair_edge_cases.py (ALL_CASES) and
prints the table kept as profiles/pair_edge_errors.txt; the bounds of tests/test_pair_edges_gpu.py are 4 x the largest value of each
family and column in that table (pair_edge_cases.family_maxima), never looser than the suite's own bars.

    python tools/record_pair_edge_errors.py > profiles/pair_edge_errors.txt           # on the MI355X
    python tools/record_pair_edge_errors.py --lib oracle/_build/libremd_cpu.so       # the f64 port: a dry run without a GPU
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import pair_edge_cases as pc
from openmmtools_amd._engine import HipEngine


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', default=None, help='another build of the ABI (default: the device library)')
    ap.add_argument('--commit', default=None, help='commit the library was built from (default: git rev-parse HEAD)')
    ap.add_argument('--only', default=None, help='only the cases whose id contains this')
    a = ap.parse_args()
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(['git', '-C', ROOT, 'rev-parse', 'HEAD'], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = 'unknown'
    print('# the direct-space pair path (force group of its own) against the f64 oracle, classes={4} (oracle/forcefield.py), tests/pair_edge_cases.py ALL_CASES')
    print('# library built from commit %s; command: python tools/record_pair_edge_errors.py%s' % (commit, ' --lib ' + a.lib if a.lib else ''))
    print('# f_max_rel: max |f - f_ref| / max |f_ref| of the group; f_rms_rel: RMS of the per-atom error vector / max |f_ref|; f_atom_rel: dimers,')
    print('# the largest |df_i| / |f_ref,i| over the atoms of pairs inside the cutoff; e_rel: |U - U_ref| of the total potential / |E(classes={4})|;')
    print('# e_tot_rel: the same / |U_ref|')
    print('# columns: row case replica N ' + ' '.join(pc.COLUMNS) + ' | family max|f_ref| E_direct E_total ms')
    rows = []
    for cid in pc.ALL_CASES:
        if a.only and a.only not in cid:
            continue
        case = pc.build_case(cid)
        eng = pc.make_engine(lambda: HipEngine(lib_path=a.lib), cid)
        try:
            pc.setup_engine(eng, case)
            t0 = time.perf_counter()
            f, U, ukl, xd = pc.evaluate(eng)
            ms = 1e3 * (time.perf_counter() - t0)
        finally:
            eng.close()
        for r, w in enumerate(pc.errors(case, f, U, *pc.oracle_reference(case, xd))):
            rows.append(dict(w, case=cid, r=r))
            print('row %-30s %d %4d ' % (cid, r, xd.shape[1]) + ' '.join('%.4e' % w[k] for k in pc.COLUMNS)
                  + ' | %-5s %.5e %.8e %.8e %.1f' % (pc.case_family(cid), w['f_ref'], w['e_direct'], w['e_total'], ms), flush=True)
    for fam, m in sorted(pc.family_maxima(rows).items()):
        for k in pc.COLUMNS:
            worst = [w['case'] for w in rows if pc.case_family(w['case']) == fam and w[k] == m[k]]
            print('# max %-6s %-11s %.4e  (%s)' % (fam, k, m[k], worst[0] if worst else '?'))


if __name__ == '__main__':
    main()
