"""Records the error of the device evaluator of collective variables (csrc/frame_cvs.hip through _engine.frame_cvs) against the
50-digit oracle of tests/frame_cvs_oracle.py on every case of tests/frame_cvs_cases.py, and the host evaluator's beside it.  Needs an
MI355X.  The rows of the degenerate families are what the tests take their bounds from (4 x the largest recorded device error of the
family); the rows of the other cases document the margin under the fixed bar of 1e-10.

    python tools/record_frame_cv_errors.py [OUTPUT]      (default: profiles/frame_cv_errors.txt)
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import frame_cvs_cases as fc                                # noqa: E402
from openmmtools_amd import _engine                         # noqa: E402
from openmmtools_amd.multistate import analysis as an       # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'frame_cv_errors.txt')
    try:
        commit = subprocess.check_output(['git', 'rev-parse', 'HEAD'], cwd=ROOT, stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = 'a working tree'
    lines = ['# collective variables of stored frames: max |value - oracle| over frames and variables (nm, rad), the oracle at 50 digits',
             '# (tests/frame_cvs_oracle.py), cases of tests/frame_cvs_cases.py; dihedral-cut modulo 2 pi',
             '# library built from %s; command: python tools/record_frame_cv_errors.py' % commit,
             '# columns: row case family device_error | numpy_error frames variables']
    for case in fc.all_cases():
        cvs = case.descriptors(an)
        dev = _engine.frame_cvs(cvs, case.pos, case.box, case.masses)
        host = an.frame_cvs_numpy(cvs, case.pos, case.box, case.masses)
        e_dev, e_host = fc.errors(case.name, dev), fc.errors(case.name, host)
        lines.append('row %-16s %-14s %.4e | %.4e %d %d' % (case.name, case.family or 'general', e_dev.max(), e_host.max(),
                                                          len(case.pos), len(case.variables)))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
