#!/usr/bin/env python
"""Choose the synth seeds of tests/test_gpu_constraints.py on the CPU: for every case, walk the seeds upwards
from the case's base and keep, for batch position s, the first seed whose scene is DECIDED in the reference alone --
tests/constraints_common.seed_is_decided: from the oracle's own starts, the float32 and the float64 oracle agree on the
support of every morphology after every iteration and differ by at most 1e-6.  Prints the table the test file holds.
No device is used, but importing scarlet_amd (for synth, the scene generator) needs the built library
scarlet_amd/csrc/libscarlet_hip.so, and the oracle its C part: run `python -c "import __graft_entry__ as g; g.build()"`
first.

    python tools/pick_constraint_seeds.py [case ...]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import constraints_common as cc          # noqa: E402
from oracle import pgm                    # noqa: E402
from scarlet_amd import synth             # noqa: E402

# name: (S, K, B, H, W, iterations, base seed, kind, also with approximate_L)
CASES = {
    "fused_k4_b3": (4, 4, 3, 24, 32, 10, 5000, "extended", True),
    "fused_k3_b3": (4, 3, 3, 24, 32, 10, 5100, "extended", True),
    "fused_k4_b6": (4, 4, 6, 24, 32, 10, 5200, "extended", True),
    "fused_k4_b8": (4, 4, 8, 24, 32, 10, 6300, "extended", False),
    "box_72x80": (2, 3, 2, 72, 80, 10, 5300, "extended", False),
    "tile_128": (2, 3, 2, 128, 128, 5, 5400, "extended", False),
    "plane_160x144": (1, 3, 2, 160, 144, 5, 5500, "extended", False),
    "streamed_272x48": (1, 3, 2, 272, 48, 5, 5600, "extended", False),
    "k9_32": (2, 9, 3, 32, 32, 10, 5700, "extended", False),
    "ragged": (3, 4, 3, 24, 32, 6, 5800, "ragged", False),
    "group": (2, 3, 3, 24, 32, 6, 5900, "group", False),
    "prior": (2, 4, 3, 24, 32, 6, 6000, "prior", False),
    "two_obs": (2, 4, 3, 24, 32, 6, 6100, "two_obs", False),
    "blend_32": (1, 2, 3, 32, 32, 10, 6200, "blend", False),
    "blend_obs_32": (1, 2, 3, 32, 32, 10, 6400, "blend_obs", False),
}
RAGGED_COUNTS = (2, 4, 3)
PRIOR_WEIGHTS = (0.3, 2.0)               # sed / morph weight of the quadratic prior on component 0 (which has l0 set)


def scene_spec(kind, s, S, K, B, H, W, seed, approximate_L):
    sym, mono, l0, l1 = cc.pattern(S, K)
    n = K
    extra = dict(approximate_L=approximate_L)
    if kind == "ragged":
        n = RAGGED_COUNTS[s]
    if kind in ("blend", "blend_obs"):
        sym[0, :2], mono[0, :2] = (0, 1), (1, 0)
        l0[:] = -1; l1[:] = -1
    if kind == "group":
        sym[s, :2], mono[s, :2] = 1, 1                         # the two layers share (1, 1) ...
        sym[s, 2], mono[s, 2] = 0, 1                           # ... beside a (0, 1) source
        l0[:] = -1; l1[:] = -1
    scn = synth.make_scene(seed, B=B, H=H, W=W, K=(n - 1 if kind == "group" else n), min_sep=3 if K > 4 else 4)
    img, cen = scn["images"], scn["centers"]
    sy, mo, a0, a1 = sym[s, :n], mono[s, :n], l0[s, :n], l1[s, :n]
    if kind == "group":
        seds, morphs = pgm.init_multicomponent_source(tuple(int(v) for v in cen[0]), img, np.ones(B) * cc.BG)
        comps = [pgm.Source(seds[j], morphs[j], cen[0], np.float32) for j in range(2)]
        ms = pgm.MultiSource(comps, cen[0])
        pgm.multi_source_update(ms, 0)
        s1, m1, c1, h1 = cc.oracle_start(img, cen[1:], sy[2:], mo[2:], a0[2:], a1[2:])
        sed0 = np.concatenate([np.array([c.sed for c in comps]), s1])
        morph0 = np.concatenate([np.array([c.morph for c in comps]), m1])
        cen0 = np.concatenate([np.array([ms.center, ms.center]), c1])
        sh0 = np.concatenate([np.full((2, 2), np.nan), h1])
        extra["group"] = np.array([0, 0, -1])
    elif kind == "two_obs":
        starts = [pgm.init_combined_extended_source(tuple(int(v) for v in c), [img[:2], img[2:]], [np.ones(2) * cc.BG, np.ones(1) * cc.BG])
                  for c in cen]
        sed0, morph0 = np.array([a for a, _ in starts]), np.array([m for _, m in starts])
        cen0, sh0 = cen, np.full((n, 2), np.nan)
        extra["observations"] = [dict(images=img[:2], band_slice=slice(0, 2)), dict(images=img[2:], band_slice=slice(2, 3))]
    else:
        sed0, morph0, cen0, sh0 = cc.oracle_start(img, cen, sy, mo, a0, a1)
    if kind == "blend_obs":            # sources started on the full observation, fitted against its two band slices
        extra["observations"] = [dict(images=img[:2], band_slice=slice(0, 2)), dict(images=img[2:], band_slice=slice(2, 3))]
    if kind == "prior":
        ws, wm = np.zeros(n), np.zeros(n)
        ws[0], wm[0] = PRIOR_WEIGHTS
        extra.update(ws=ws, wm=wm)
    return cc.spec_of(img, sed0, morph0, cen0, sh0, sy, mo, a0, a1, **extra)


def pick(name):
    S, K, B, H, W, iters, base, kind, approx = CASES[name]
    seeds, seed = [], base
    for s in range(S):
        while True:
            try:
                ok = all(cc.seed_is_decided(scene_spec(kind, s, S, K, B, H, W, seed, ap), iters)
                         for ap in ((False, True) if approx else (False,)))
            except pgm.SourceInitError:
                ok = False
            seed += 1
            if ok:
                seeds.append(seed - 1)
                break
    return seeds


if __name__ == "__main__":
    for name in (sys.argv[1:] or CASES):
        print('    "%s": %s,' % (name, pick(name)), flush=True)
