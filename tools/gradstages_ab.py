"""Build-against-build comparison of the gradient step's launch stages, in the manner of tools/dump_fit.py: the cases
of tests/gradient_stage_cases.py with two builds of the library (SCARLET_LIB_PATH, tools/ab_variants.sh).  In front of
the command, `--cases MODULE` takes another table with that module's interface (tests/launch_form_cases.py).

    python tools/gradstages_ab.py dump DIR            # 3 iterations of every case: DIR/<case>/<array>.npy
    python tools/gradstages_ab.py compare DIR_A DIR_B # every array byte for byte; lists them; exit status 1 if one differs
    python tools/gradstages_ab.py run                 # 1 iteration of every case, for `rocprofv3 --kernel-trace -- python ...`
    python tools/gradstages_ab.py launches A.csv B.csv  # the two kernel traces case by case

With SCARLET_PSF_HIPFFT=1 in the environment `dump` and `run` take the cases that reach the hipFFT chain (the switch
freezes with the first PSF workspace, so they need a process of their own).  In a trace the cases are told apart by a
one-element torch.lgamma launched in front of each; `launches` compares per case the multiset of (kernel, grid,
workgroup, LDS bytes) and, except for the cases that launch on two streams, their order."""
import collections
import csv
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import importlib                         # noqa: E402

if sys.argv[1:2] == ["--cases"]:
    gs = importlib.import_module(sys.argv[2])
    del sys.argv[1:3]
else:
    import gradient_stage_cases as gs    # noqa: E402

HIPFFT = os.environ.get("SCARLET_PSF_HIPFFT") == "1"
MARK = "lgamma"


def case_names():
    return (gs.HIPFFT_CASES if HIPFFT else list(gs.CASES)) + (["convolve_same"] if hasattr(gs, "convolve_inputs") else [])


def run_cases(iters, out=None):
    import torch
    import scarlet_amd
    from scarlet_amd.psfconv import convolve_same
    mark = torch.full((1,), 0.5, device="cuda")
    for name in case_names():
        torch.lgamma(mark)
        arrays = {}
        if name == "convolve_same":
            img, kers = gs.convolve_inputs()
            for nk, ker in kers.items():
                arrays["out_nk%d" % nk] = convolve_same(img, ker).cpu().numpy()
        else:
            c = gs.CASES[name]
            with gs.options(scarlet_amd, c):
                b = gs.make_batch(scarlet_amd, c, *gs.scenes(c))
                torch.cuda.synchronize()
                torch.lgamma(mark)                      # (the constructors' launches lie between two marks: not compared)
                n = getattr(c, "iters", None) or iters  # (a case may fix its own number)
                assert b.fit(n, e_rel=0, approximate_L=c.approximate_L) == n
                arrays = gs.state(b)
        torch.cuda.synchronize()
        if out:
            os.makedirs(os.path.join(out, name), exist_ok=True)
            for key, a in arrays.items():
                np.save(os.path.join(out, name, key + ".npy"), a)
    torch.lgamma(mark)
    torch.cuda.synchronize()
    print("%d cases, %d iteration(s)%s" % (len(case_names()), iters, ", dumped to " + out if out else ""))


def compare(da, db):
    cases = sorted(os.listdir(da))
    assert cases and cases == sorted(os.listdir(db)), "different sets of cases"
    n, bad = 0, []
    for case in cases:
        names = sorted(os.listdir(os.path.join(da, case)))
        assert names and names == sorted(os.listdir(os.path.join(db, case))), "different sets of arrays: " + case
        same = [np.array_equal(np.load(os.path.join(da, case, f)), np.load(os.path.join(db, case, f)), equal_nan=True)
                for f in names]
        bad += [case + "/" + f for f, ok in zip(names, same) if not ok]
        n += len(names)
        print("%-28s %s  %s" % (case, "identical" if all(same) else "DIFFERENT",
                                " ".join(f[:-4] for f in names)))
    print("%d arrays of %d cases compared, %d differ %s" % (n, len(cases), len(bad), bad))
    return 1 if bad else 0


def read_trace(path):
    """per case (in the order of case_names()): the fit's launches [(kernel, grid, workgroup, LDS bytes)] in dispatch order"""
    with open(path) as f:
        rows = list(csv.DictReader(f))
    col = lambda *parts: next(k for k in rows[0] if all(p in k.lower() for p in parts))
    name, disp, lds = col("kernel", "name"), col("dispatch"), col("lds")
    grid = [col("grid", a) for a in "xyz"]
    wg = [col("workgroup", a) for a in "xyz"]
    rows.sort(key=lambda r: int(r[disp]))
    groups = [[]]
    for r in rows:
        if MARK in r[name]:
            groups.append([])
        else:
            groups[-1].append((r[name], tuple(int(r[g]) for g in grid), tuple(int(r[w]) for w in wg), int(r[lds])))
    groups = groups[1:-1]                               # (before the first mark: start-up; after the last: nothing)
    out, i = collections.OrderedDict(), 0
    for case in case_names():
        if case == "convolve_same":
            out[case] = groups[i]; i += 1
        else:
            out[case] = groups[i + 1]; i += 2           # (groups[i]: the constructors)
    assert i == len(groups), (i, len(groups))
    return out


def launches(pa, pb):
    a, b = read_trace(pa), read_trace(pb)
    bad = []
    for case in a:
        ordered = case not in gs.SIDE_STREAM_CASES
        same = collections.Counter(a[case]) == collections.Counter(b[case]) and (not ordered or a[case] == b[case])
        print("%-28s %3d launches  %s" % (case, len(a[case]), ("same multiset, same order" if ordered else
                                                               "same multiset (two streams)") if same else "DIFFERENT"))
        if not same:
            bad.append(case)
    print("%d cases compared, %d differ %s" % (len(a), len(bad), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    cmd = sys.argv[1]
    if cmd == "dump":
        run_cases(gs.ITERS, sys.argv[2])
    elif cmd == "run":
        run_cases(1)
    elif cmd == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(launches(sys.argv[2], sys.argv[3]))
