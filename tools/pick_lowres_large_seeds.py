#!/usr/bin/env python
"""Choose the seeds of the joint fits of tests/test_gpu_lowres_large.py on the CPU: for every case walk the seeds upwards
from the one the test file holds and keep the first whose S scenes are all DECIDED in the reference alone -- Case.
seed_is_decided of tests/test_gpu_lowres_limits.py: the float32 and the float64 restatement (lowres_common.fit) agree
on the support of every morphology after every iteration and differ by at most 1e-6.  Prints the table the test file
holds.  No device is used, but importing scarlet_amd needs the built library and the oracle its C part: run
`python -c "import __graft_entry__ as g; g.build()"` first.

    python tools/pick_lowres_large_seeds.py [case ...]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_gpu_lowres_large as t          # noqa: E402

BUILDERS = dict(t.CASES, inactive=t._inactive)


def pick(name):
    seed = t.SEEDS[name]
    while not BUILDERS[name](seed).seed_is_decided():
        seed += 1
    return seed


if __name__ == "__main__":
    for name in (sys.argv[1:] or sorted(BUILDERS)):
        print('    "%s": %d,' % (name, pick(name)), flush=True)
