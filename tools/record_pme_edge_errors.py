#!/usr/bin/env python
"""Records the error of the PME reciprocal-space path against the f64 oracle on every case of tests/pme_edge_cases.py
(MATRIX + PER_REPLICA) and prints the table kept as profiles/pme_edge_errors.txt; the bounds of tests/test_pme_edges_gpu.py are
4 x the largest value of each family in that table (pme_edge_cases.family_maxima).

    python tools/record_pme_edge_errors.py > profiles/pme_edge_errors.txt           # on the MI355X
    python tools/record_pme_edge_errors.py --lib oracle/_build/libremd_cpu.so       # the f64 port: a dry run without a GPU
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import numpy as np

import pme_edge_cases as pc
from openmmtools_amd._engine import HipEngine


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', default=None, help='another build of the ABI (default: the device library)')
    ap.add_argument('--commit', default=None, help='commit the library was built from (default: git rev-parse HEAD)')
    a = ap.parse_args()
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(['git', '-C', ROOT, 'rev-parse', 'HEAD'], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = 'unknown'
    print('# PME reciprocal space against the f64 oracle on the same mesh (oracle/forcefield.py), tests/pme_edge_cases.py MATRIX + PER_REPLICA')
    print('# library built from commit %s; command: python tools/record_pme_edge_errors.py%s' % (commit, ' --lib ' + a.lib if a.lib else ''))
    print('# f_max: max |f - f_ref| of the reciprocal force group [kJ/mol/nm]; f_rms: RMS of the per-atom error vector; *_rel: over max |f_ref|')
    print('# of that group; e_abs: |U - U_ref| of the total potential [kJ/mol]; e_rel: e_abs / |E(classes={5})|')
    print('# columns: row case replica N ' + ' '.join(pc.FAMILIES) + ' | max|f_ref| E_recip E_total ms')
    rows = []
    for case in pc.MATRIX + pc.PER_REPLICA:
        desc, x, box = pc.build_case(case)
        eng = HipEngine(lib_path=a.lib)
        try:
            pc.setup_engine(eng, desc, x, box)
            t0 = time.perf_counter()
            f, U, xd = pc.evaluate(eng)
            ms = 1e3 * (time.perf_counter() - t0)
        finally:
            eng.close()
        for r, w in enumerate(pc.errors(f, U, *pc.oracle_reference(desc, xd, box))):
            rows.append(dict(w, case=pc.case_id(case), r=r))
            print('row %-28s %d %4d ' % (pc.case_id(case), r, x.shape[1]) + ' '.join('%.4e' % w[k] for k in pc.FAMILIES)
                  + ' | %.5e %.8e %.8e %.1f' % (w['f_ref'], w['e_recip'], w['e_total'], ms), flush=True)
    print('# largest per family (relative force families without the %s cases, absolute ones on them alone):' % '/'.join(pc.SMALL))
    for k, v in pc.family_maxima(rows).items():
        worst = [w for w in rows if w.get(k.replace('_small', '')) == v]
        print('# max %-12s %.4e  (%s)' % (k, v, worst[0]['case'] if worst else '?'))


if __name__ == '__main__':
    main()
