"""Timing of ragged-frame batches: scenes of different frame sizes in one BlendBatch (frame_shapes).  bench.py measures
the BASELINE configs and is left alone.

A seeded population of S = 4096 scenes, B = 5, K = 4, heights and widths drawn independently and uniformly from 24..64
(survey cut-outs: every blend has its own footprint).  `--steps` iterations at e_rel = 0 are timed four ways:
  (a) ragged   one ragged-frame batch, every scene padded to 64 x 64: the one-launch iteration of the four-wave
               kernel's ragged-frames instance (profile class 4);
  (b) buckets  the same scenes grouped into one uniform batch per distinct shape, fitted one after the other -- the only
               way to get the same results without frame_shapes.  Every bucket is built, initialised and warmed up
               before the clock starts; the time is that of the fit calls alone;
  (c) ceiling  a uniform 64 x 64 batch of S scenes on the general path (the NO_FUSED switch), the cost ceiling of (d);
  (d) general  the batch of (a) under the NO_FUSED switch: the general path, which every ragged-frame batch took before
               the one-launch instance existed and which larger ones still take -- in the same process as (a).
Each figure: `--warmup` iterations, then `--steps` iterations between two CUDA events, `--repeats` repeats on fresh
batches, the median.  One more run of (a) and of (d) under scarlet_profile_begin / _end gives the time per kernel class
(0 k_grad, 1 k_step, 2 the constraint update, 3 k_converge, 4 the one-launch kernels) and, for (d), the share of the
gradient kernels, which stream the padded planes: the padding's share of their pixels is 1 - mean(h w) / (H W).

    python tools/bench_ragged_frames.py --out ragged_frames_fused_run.json

(profiles/ragged_frames_bench.json is the record of the general path alone, made before leg (d) existed.)
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, B, K, LO, HI = 4096, 5, 4, 24, 64


def population(n_scenes, seed=0):
    """[(images (B, h, w), centres (K, 2))] with sides uniform in LO..HI"""
    from scarlet_amd import synth
    sides = np.random.default_rng(seed).integers(LO, HI + 1, size=(n_scenes, 2))
    out = []
    for i, (h, w) in enumerate(sides):
        sc = synth.make_scene(52000 + i, B=B, H=int(h), W=int(w), K=K, min_sep=2)
        out.append((sc["images"], sc["centers"]))
    return out, sides.astype(np.int32)


def timed(batches, steps, warmup):
    """ms of `steps` iterations of every batch, one after the other"""
    import torch
    for b in batches:
        b.fit(warmup, e_rel=0, check_every=0)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for b in batches:
        b.fit(steps, e_rel=0, check_every=0)
    e1.record()
    torch.cuda.synchronize()
    for b in batches:
        assert int(b.status.abs().sum().item()) == 0
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--scenes", type=int, default=S)
    ap.add_argument("--out", default="ragged_frames_fused_run.json")
    args = ap.parse_args()
    import torch
    from scarlet_amd import _lib
    from scarlet_amd.batch import BlendBatch, default_centroid_weight, pad_frames
    n_scenes = args.scenes
    scenes, sides = population(n_scenes)
    cw = default_centroid_weight()
    bg = np.ones(B) * 0.1
    cap = args.steps + args.warmup + 1
    centers = np.stack([c for _, c in scenes])
    block, shapes = pad_frames([im for im, _ in scenes])
    H, W = block.shape[2:]

    def make(images, cen, **kw):
        return BlendBatch(images, cen, mse_capacity=cap, centroid_weight=cw, **kw).init_extended(bg)

    def median_of(build):
        times = []
        for _ in range(args.repeats):
            batches = build()
            times.append(timed(batches, args.steps, args.warmup))
            del batches
        return float(np.median(times)), times

    res = dict(scenes=n_scenes, B=B, K=K, sides=[LO, HI], padded=[int(H), int(W)], steps=args.steps, warmup=args.warmup,
               repeats=args.repeats, device=torch.cuda.get_device_name(),
               mean_frame_pixels=float((sides[:, 0] * sides[:, 1]).mean()),
               padding_share_of_gradient_pixels=float(1 - (sides[:, 0] * sides[:, 1]).mean() / (H * W)))
    # (a) one ragged-frame batch
    ms, rep = median_of(lambda: [make(block, centers, frame_shapes=shapes)])
    res["ragged"] = dict(ms=ms, repeats=rep, scene_iterations_per_s=n_scenes * args.steps / ms * 1e3)
    # (b) one uniform batch per distinct shape
    groups = {}
    for i, (h, w) in enumerate(sides):
        groups.setdefault((int(h), int(w)), []).append(i)

    def buckets():
        return [make(np.stack([scenes[i][0] for i in idx]), centers[idx]) for idx in groups.values()]
    ms, rep = median_of(buckets)
    res["buckets"] = dict(ms=ms, repeats=rep, scene_iterations_per_s=n_scenes * args.steps / ms * 1e3, batches=len(groups),
                          largest_batch=max(len(v) for v in groups.values()))
    # (c) a uniform batch of the padded frame on the general path
    from scarlet_amd import synth
    full = [synth.make_scene(52000 + i, B=B, H=int(H), W=int(W), K=K, min_sep=2) for i in range(16)]
    reps = (n_scenes + 15) // 16
    fi = np.tile(np.stack([s["images"] for s in full]), (reps, 1, 1, 1))[:n_scenes]
    fc_ = np.tile(np.stack([s["centers"] for s in full]), (reps, 1, 1))[:n_scenes]
    prev = _lib.set_option("NO_FUSED", 1)
    try:
        ms, rep = median_of(lambda: [make(fi, fc_)])
    finally:
        _lib.set_option("NO_FUSED", prev)
    res["ceiling"] = dict(ms=ms, repeats=rep, scene_iterations_per_s=n_scenes * args.steps / ms * 1e3)
    # (d) the ragged-frame batch on the general path
    prev = _lib.set_option("NO_FUSED", 1)
    try:
        ms, rep = median_of(lambda: [make(block, centers, frame_shapes=shapes)])
    finally:
        _lib.set_option("NO_FUSED", prev)
    res["general"] = dict(ms=ms, repeats=rep, scene_iterations_per_s=n_scenes * args.steps / ms * 1e3)
    res["general_ms_over_ragged_ms"] = res["general"]["ms"] / res["ragged"]["ms"]
    res["buckets_ms_over_ragged_ms"] = res["buckets"]["ms"] / res["ragged"]["ms"]
    res["ceiling_ms_over_ragged_ms"] = res["ceiling"]["ms"] / res["ragged"]["ms"]
    # the kernel classes of (a) and (d): 0 k_grad, 1 k_step, 2 the constraint update, 3 k_converge, 4 the one-launch kernels
    def classes(no_fused):
        prev = _lib.set_option("NO_FUSED", no_fused)
        try:
            b = make(block, centers, frame_shapes=shapes)
            b.fit(args.warmup, e_rel=0, check_every=0)
            torch.cuda.synchronize()
            _lib.check(_lib.lib.scarlet_profile_begin(args.steps))
            b.fit(args.steps, e_rel=0, check_every=0)
            tot, cnt = (ctypes.c_double * 8)(), (ctypes.c_int64 * 8)()
            _lib.check(_lib.lib.scarlet_profile_end(tot, cnt))
        finally:
            _lib.set_option("NO_FUSED", prev)
        return dict(k_grad=tot[0], k_step=tot[1], update=tot[2], k_converge=tot[3], fused=tot[4]), [int(v) for v in cnt][:5]
    cls, cnt = classes(0)
    res["ragged_kernel_ms"], res["ragged_launches"] = cls, cnt
    res["fused_share_of_ragged"] = cls["fused"] / max(sum(cls.values()), 1e-30)
    cls, cnt = classes(1)
    res["general_kernel_ms"], res["general_launches"] = cls, cnt
    share = (cls["k_grad"] + cls["k_step"]) / max(sum(cls.values()), 1e-30)
    res["gradient_share_of_general"] = share
    res["padding_share_of_general"] = share * res["padding_share_of_gradient_pixels"]
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
