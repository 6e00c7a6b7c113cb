"""A converging fit for build-against-build comparisons: fit(60, e_rel=1e-3) on 1 600 scenes of 5 x 64 x 64 with K = 4
(160 distinct ones, tiled), every output written as .npy into DIR.  Run it with two builds of the library
(SCARLET_LIB_PATH, tools/ab_variants.sh) and compare the directories:

    python tools/dump_fit.py DIR            # dump
    python tools/dump_fit.py DIR_A DIR_B    # compare: every array equal (NaN == NaN), or exit status 1
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def dump(out):
    import torch
    from scarlet_amd import synth
    from scarlet_amd.batch import BlendBatch
    U, S = 160, 1600
    d = synth.make_batch(3100, U)
    b = BlendBatch(np.tile(d["images"], (S // U, 1, 1, 1)), np.tile(d["centers"], (S // U, 1, 1)))
    b.init_extended(np.ones(5) * 0.1)
    b.fit(60, e_rel=1e-3)
    torch.cuda.synchronize()
    os.makedirs(out, exist_ok=True)
    for name, t in dict(sed=b.sed_current, morph=b.morph_current, sed0=b.sed[0], sed1=b.sed[1], morph0=b.morph[0],
                        morph1=b.morph[1], flags=b.flags, it=b.it, lipschitz=b.lipschitz, centers=b.centers,
                        shifts=b.shifts, mse=b.mse_buf, status=b.status).items():
        np.save(os.path.join(out, name + ".npy"), t.cpu().numpy())
    it = b.it.cpu().numpy()
    print("dumped to %s: iterations min %d  median %d  max %d" % (out, it.min(), np.median(it), it.max()))


def compare(da, db):
    names = sorted(f for f in os.listdir(da) if f.endswith(".npy"))
    assert names and names == sorted(f for f in os.listdir(db) if f.endswith(".npy")), "different sets of arrays"
    bad = [f for f in names if not np.array_equal(np.load(os.path.join(da, f)), np.load(os.path.join(db, f)), equal_nan=True)]
    print("%d arrays compared, %d differ %s" % (len(names), len(bad), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 2:
        dump(sys.argv[1])
    else:
        sys.exit(compare(sys.argv[1], sys.argv[2]))
