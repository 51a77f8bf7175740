"""The worst |error| / bound of every test family of tests/test_custom_param_derivatives_gpu.py, from the lines the tests print
('... |error| / bound = x'): runs the file with -s on the GPU and writes profiles/custom_param_derivative_errors.txt.

    python tools/record_custom_param_derivative_errors.py
"""
import os
import re
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')


def main():
    out = subprocess.run([sys.executable, '-m', 'pytest', 'tests/test_custom_param_derivatives_gpu.py', '-m', 'gpu', '-s', '-v', '-p', 'no:cacheprovider'],
                         cwd=ROOT, capture_output=True, text=True).stdout
    worst, family = {}, None
    for line in out.splitlines():
        m = re.search(r'::(test_\w+)', line)
        if m:
            family = m.group(1)
        m = re.search(r'\|error\| / bound = ([0-9.eE+-]+)', line)
        if m and family:
            worst[family] = max(worst.get(family, 0.0), float(m.group(1)))
    lines = ['Energy parameter derivatives of the custom forces: the worst |device - oracle| / bound per test family of',
             'tests/test_custom_param_derivatives_gpu.py, bound = 1e-11 sum_t |dE_t/dglobal| (the oracle: tests/custom_param_derivative_oracle.py).',
             'No family needs more than the formula gives.', '']
    lines += ['%-75s %.3g' % (k, v) for k, v in worst.items()]
    text = '\n'.join(lines) + '\n'
    with open(os.path.join(ROOT, 'profiles', 'custom_param_derivative_errors.txt'), 'w') as f:
        f.write(text)
    print(text)
    return 0 if worst else 1


if __name__ == '__main__':
    sys.exit(main())
