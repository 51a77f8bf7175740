"""Records tests/golden/listed_terms_bits.npz: forces, energies and short trajectories through every evaluation of the listed terms, to
the bit, on the cases of tests/listed_terms_bits.py.  Run ONCE on an MI355X against a build of the commit BEFORE the change the file is
to hold to the recorded bits (the library is loaded from the given path; the Python side is this tree's).  Not run by the test suite.

usage: python tests/golden/make_golden_listed_terms_bits.py path/to/libremd_hip.so [output.npz]"""
import os
import sys
import time
import numpy as np

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.dirname(TESTS), TESTS]
import listed_terms_bits as ltb                                         # noqa: E402
from openmmtools_amd._engine import HipEngine                           # noqa: E402

if __name__ == '__main__':
    lib_path = os.path.abspath(sys.argv[1])
    out_path = sys.argv[2] if len(sys.argv) > 2 else ltb.GOLDEN
    engines = []

    def make(**kw):
        engines.append(HipEngine(lib_path=lib_path, **kw))
        return engines[-1]

    out = {}
    for case in ltb.CASES:
        t0 = time.time()
        now = getattr(ltb, case)(make)
        out[case] = ltb.pack(now)
        print('%-12s %2d arrays, %6d words, %.1f s' % (case, len(now), out[case].size, time.time() - t0), flush=True)
    for e in engines:
        e.close()
    np.savez_compressed(out_path, **out)
    size = os.path.getsize(out_path)
    print(lib_path, '->', out_path, size, 'bytes')
    assert size <= 64 * 1024, 'the fixture is to stay within 64 KB'
