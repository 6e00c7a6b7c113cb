#!/usr/bin/env python
"""Choose the synth seeds of tests/gradient_stage_cases.py on the CPU, by the rule of tools/pick_constraint_seeds.py:
for every distinct (kind, K, B, H, W, PSF, constants) of the table walk the seeds upwards from a base and keep the first
two whose scene is DECIDED in the reference alone -- from the oracle's own starts, the float32 and the float64 oracle
agree on the support of every morphology after each of the 3 iterations and differ by at most 1e-6.  Prints the SEEDS
table the module holds.  No device is used, but importing scarlet_amd (for synth, the scene generator) needs the built
library and the oracle its C part: run `python -c "import __graft_entry__ as g; g.build()"` first.

    python tools/pick_gradient_stage_seeds.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import constraints_common as cc          # noqa: E402
import gradient_stage_cases as gs        # noqa: E402
from conftest import rel_err              # noqa: E402
from oracle import pgm                    # noqa: E402

BASE = 9000


def trace(c, img, cen, dt):
    """the morphologies after every iteration of the oracle's fit from its own starts"""
    on = np.ones(c.K, np.uint8)
    off = np.full(c.K, -1.0, np.float32)
    if c.kind == "obs":
        n = gs.OBS_BANDS[0]
        starts = [pgm.init_combined_extended_source(tuple(int(v) for v in p), [img[:n], img[n:]],
                                                    [np.ones(m) * gs.BG for m in gs.OBS_BANDS]) for p in cen]
        sc = pgm.scene_from_state(np.zeros(img.shape, dt), np.array([a for a, _ in starts]).astype(dt),
                                  np.array([m for _, m in starts]).astype(dt), cen, None)
        sc.observations = [dict(images=img[:n].astype(dt), band_slice=slice(0, n), weights=1,
                                diff_kernel=gs.diff_kernel(n).astype(dt)),
                           dict(images=img[n:].astype(dt), band_slice=slice(n, c.B), weights=1, diff_kernel=None)]
    else:
        sed0, morph0, cen0, sh0 = cc.oracle_start(img, cen, on, on, off, off)
        okw = dict(diff_kernel=gs.diff_kernel(c.B)) if c.psf else {}
        sc = cc.build_scene(cc.spec_of(img, sed0, morph0, cen0, sh0, on, on, off, off, okw=okw), dt)
    post = []
    pgm.fit(sc, gs.ITERS, e_rel=0, approximate_L=c.approximate_L,
            callback=lambda scn: post.append(np.array([s.morph.copy() for s in scn.sources])))
    return post


def decided(c, seed):
    from scarlet_amd import synth
    scn = synth.make_scene(seed, B=c.B, H=c.H, W=c.W, K=c.K, min_sep=c.min_sep)
    try:
        o32, o64 = (trace(c, scn["images"], scn["centers"], dt) for dt in (np.float32, np.float64))
    except pgm.SourceInitError:
        return False
    for a, b in zip(o32, o64):
        if ((a == 0) != (b == 0)).any() or not np.isfinite(a).all() or rel_err(a, b) > cc.SEED_TOL:
            return False
    return len(o32) == gs.ITERS


if __name__ == "__main__":
    seed, done = BASE, {}
    for c in gs.CASES.values():
        key = gs.seed_key(c)
        if key in done:
            continue
        picks = []
        while len(picks) < gs.S:
            if decided(c, seed):
                picks.append(seed)
            seed += 1
        done[key] = picks
        print("    %r: %r," % (key, picks), flush=True)
