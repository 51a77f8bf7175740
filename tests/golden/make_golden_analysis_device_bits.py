"""Records tests/golden/analysis_device_bits.npz: what the device analysis passes return, to the bit, on the cases of
tests/analysis_device_bits.py.  Run ONCE on an MI355X from a build of the commit BEFORE the several-series pass moved into
csrc/timeseries.hip (the tests then hold every later commit to these bits); it also prints whether, at that commit, one series through
series_inefficiency_multiple already equals DeviceTimeseries at origin 0 to the bit.  Not run by the test suite.

usage: python tests/golden/make_golden_analysis_device_bits.py [output.npz]"""
import os
import sys
import numpy as np

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.dirname(TESTS), TESTS]
import analysis_device_bits as adb                                      # noqa: E402
import timeseries_cases as tc                                           # noqa: E402
from openmmtools_amd._engine import DeviceTimeseries, series_inefficiency_multiple      # noqa: E402

if __name__ == '__main__':
    out_path = sys.argv[1] if len(sys.argv) > 1 else adb.GOLDEN
    ts = DeviceTimeseries([0.0, 1.0])
    chunk = ts.chunk()
    assert chunk == tc.CHUNK
    now = adb.mbar_and_energy_store()
    out = {'single': adb.pack(adb.single_series(chunk)), 'several': adb.pack(adb.several_series(chunk)),
           'mbar': adb.pack({k: v for k, v in now.items() if k.startswith('mbar/')}),
           'energy_store': adb.pack({k: v for k, v in now.items() if k.startswith('energy_store/')})}
    np.savez_compressed(out_path, **out)
    print({k: v.size for k, v in out.items()}, '->', out_path, os.path.getsize(out_path), 'bytes')
    same = True
    for N in (2, 100, chunk + 1, 3 * chunk + 7):
        A = tc.series('ar05', N)
        one = DeviceTimeseries(A)
        for fast, mintime in adb.SETTINGS:
            g, status, last = one.inefficiency([0], fast=fast, mintime=mintime)
            g2, status2, last2 = series_inefficiency_multiple(A[None, :], fast=fast, mintime=mintime)[:3]
            ok = np.float64(g2).view(np.uint64) == g.view(np.uint64)[0] and (status2, last2) == (status[0], last[0])
            same = same and bool(ok)
            print('K = 1 against origin 0: N %d fast %d mintime %d: %s' % (N, fast, mintime, 'same bits' if ok else 'DIFFERENT'))
    print('K = 1 equals the single series at origin 0 everywhere:', same)
