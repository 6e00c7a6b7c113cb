"""Fits of batches whose components carry their own constraint switches: scene-iterations per second of the headline
shape (10 000 scenes x 5 x 64 x 64, K = 4, 50 iterations at e_rel = 0) on three paths, alternated in one process and
repeated (`--repeats`), each timed with device events:

  a  the mixed pattern -- component k of scene s takes the (symmetric, monotonic) pair ((1,1), (0,1), (1,0), (0,0))[(k + s) % 4],
     one l0_thresh in scene 0 and one l1_thresh in scene 1 -- through scarlet_fit_constrained: the four-wave kernel's
     per-component instance, one launch per iteration
  b  the same batch with NO_FUSED: the general path, four launches per iteration
  c  a uniform batch (every component (1,1), scalars) through FUSED_V1: the same four-wave kernel with the batch's scalars

a / b is what keeping the one-launch iteration is worth; a against c shows what the imbalance between the waves costs
(a (0,0) component's wave is done early while a (1,1) wave runs the symmetry GEMMs and the sweep) -- with the caveat
that the mixed batch also does less work in total.  The launch counts per kernel class (scarlet_profile_end) go with
every leg.  One JSON line; `--out` also writes it to a file."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAIRS = ((1, 1), (0, 1), (1, 0), (0, 0))
NAMES = ["k_grad", "k_step", "k_source_update", "k_converge", "k_iterate", "psf_convolution", "k_prior_step"]


def mixed_pattern(S, K):
    k, s = np.meshgrid(np.arange(K), np.arange(S))
    pair = np.array(PAIRS, np.uint8)[(k + s) % 4]
    l0 = np.full((S, K), -1.0, np.float32)
    l1 = np.full((S, K), -1.0, np.float32)
    l0[0, 0] = 0.3
    l1[min(1, S - 1), 1] = 0.2
    return np.ascontiguousarray(pair[..., 0]), np.ascontiguousarray(pair[..., 1]), l0, l1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=10000)
    ap.add_argument("--bands", type=int, default=5)
    ap.add_argument("--side", type=int, default=64)
    ap.add_argument("--sources", type=int, default=4)
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--distinct", type=int, default=256, help="distinct synthetic scenes, tiled to --scenes")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import scarlet_amd as scarlet
    from scarlet_amd import _lib, synth
    S, B, side, K, iters = a.scenes, a.bands, a.side, a.sources, a.iterations
    d = synth.make_batch(4000, min(a.distinct, S), B=B, H=side, W=side, K=K)
    reps = (S + len(d["images"]) - 1) // len(d["images"])
    images = torch.as_tensor(np.tile(d["images"], (reps, 1, 1, 1))[:S]).cuda()
    centers = np.tile(d["centers"], (reps, 1, 1))[:S]
    sym, mono, l0, l1 = mixed_pattern(S, K)
    bg = np.ones(B) * 0.1
    mixed = scarlet.BlendBatch(images, centers, symmetric=sym, monotonic=mono, l0_thresh=l0, l1_thresh=l1,
                               mse_capacity=iters + 1).init_extended(bg)
    uniform = scarlet.BlendBatch(images, centers, mse_capacity=iters + 1).init_extended(bg)
    assert mixed.constrained and not uniform.constrained
    start = {id(b): (b.sed_current.clone(), b.morph_current.clone(), b.centers.clone(), b.shifts.clone())
             for b in (mixed, uniform)}
    legs = dict(a=(mixed, ()), b=(mixed, ("NO_FUSED",)), c=(uniform, ("FUSED_V1",)))

    def fit(leg, profile=False):
        b, opts = legs[leg]
        sed0, morph0, cen0, sh0 = start[id(b)]
        b.set_state(sed0, morph0)
        b.centers.copy_(cen0); b.shifts.copy_(sh0)
        b.it.zero_()
        prev = [_lib.set_option(o, 1) for o in opts]
        try:
            if profile:
                _lib.check(_lib.lib.scarlet_profile_begin(iters + 1))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            n = b.fit(iters, e_rel=0, check_every=0)
            e1.record()
            torch.cuda.synchronize()
            assert n == iters and int(b.it.min().item()) == iters
            if profile:
                tot, cnt = (ctypes.c_double * 8)(), (ctypes.c_int64 * 8)()
                _lib.check(_lib.lib.scarlet_profile_end(tot, cnt))
                return {NAMES[i]: int(cnt[i]) for i in range(len(NAMES)) if cnt[i]}
            return e0.elapsed_time(e1)
        finally:
            for o, p in zip(opts, prev):
                _lib.set_option(o, p)

    use = [x for x in a.legs.split(",") if x in legs]
    out = dict(bench="constraints", scenes=S, bands=B, side=side, sources=K, iterations=iters, repeats=a.repeats)
    for leg in use:
        out["launches_" + leg] = fit(leg, profile=True)           # (also the warm-up)
    ms = {leg: [] for leg in use}
    for _ in range(a.repeats):
        for leg in use:
            ms[leg].append(fit(leg))
    for leg in use:
        out["ms_" + leg] = [round(v, 3) for v in ms[leg]]
        out["scene_iterations_per_s_" + leg] = round(S * iters / (float(np.median(ms[leg])) * 1e-3), 1)
    if "a" in use and "b" in use:
        out["a_over_b"] = round(out["scene_iterations_per_s_a"] / out["scene_iterations_per_s_b"], 3)
    if "a" in use and "c" in use:
        out["a_over_c"] = round(out["scene_iterations_per_s_a"] / out["scene_iterations_per_s_c"], 3)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
