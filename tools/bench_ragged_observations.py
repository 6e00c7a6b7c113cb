"""Timing of joint fits of ragged-frame batches: scenes of different frame sizes fitted against two observations
(ObservationBatch(frame_shapes=...) -> BlendBatch.from_observations, scarlet_fit_observations_frames).  bench.py measures
the BASELINE configs and is left alone.  A record, not a pass/fail: no speed is claimed for this path.

Per padded frame (64 x 64 with 4096 scenes, 128 x 128 with 1024): a seeded population of scenes with B = 5 bands seen as
two observations (bands 0-2 and 3-4), K = 4, heights and widths drawn independently and uniformly from 3/8 .. 1 of the
padded side.  `--steps` iterations at e_rel = 0 are timed two ways, in the same process, alternating:
  (a) ragged   the joint fit with frame shapes: the constraint update runs on each scene's own frame (no box stage); the
               observations' passes stream the padded planes;
  (b) uniform  the uniform joint fit of the SAME padded block (no frame shapes).  That is a DIFFERENT computation -- the
               constraints see the padded frame, and beyond 64 pixels the box stage runs -- and is here as the yardstick of
               what the padded block costs, not as an alternative that gives the same results.
Each figure: `--warmup` iterations, then `--steps` iterations between two device events, `--repeats` repeats on fresh
batches, the median.  One more run of each under scarlet_profile_begin / _end gives the time per kernel class (0 the
observations' planes, 1 contraction / Lipschitz / step, 2 the constraint update, 3 k_converge).

    python tools/bench_ragged_observations.py --out profiles/ragged_observations_bench.json
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, SPLIT, K = 5, 3, 4
FRAMES = ((64, 4096), (128, 1024))          # (padded side, scenes)


def population(side, n_scenes, seed=0):
    """[(images (B, h, w), centres (K, 2))] with sides uniform in 3/8 side .. side"""
    from scarlet_amd import synth
    sides = np.random.default_rng(seed + side).integers(3 * side // 8, side + 1, size=(n_scenes, 2))
    out = []
    for i, (h, w) in enumerate(sides):
        sc = synth.make_scene(61000 + 1000 * side + i, B=B, H=int(h), W=int(w), K=K, min_sep=2)
        out.append((sc["images"], sc["centers"]))
    return out, sides.astype(np.int32)


def timed(b, steps, warmup):
    """ms of `steps` iterations"""
    import torch
    b.fit(warmup, e_rel=0, check_every=0)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    b.fit(steps, e_rel=0, check_every=0)
    e1.record()
    torch.cuda.synchronize()
    assert int(b.status.abs().sum().item()) == 0
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the scene counts (a rehearsal uses a small one)")
    ap.add_argument("--out", default="ragged_observations_run.json")
    args = ap.parse_args()
    import torch
    from scarlet_amd import _lib
    from scarlet_amd.batch import BlendBatch, ObservationBatch, default_centroid_weight, pad_frames
    cw = default_centroid_weight()
    bg = [np.ones(SPLIT) * 0.1, np.ones(B - SPLIT) * 0.1]
    cap = args.steps + args.warmup + 1
    res = dict(B=B, bands=[[0, SPLIT], [SPLIT, B - SPLIT]], K=K, steps=args.steps, warmup=args.warmup, repeats=args.repeats,
               device=torch.cuda.get_device_name(), frames=[])
    for side, n_scenes in FRAMES:
        n_scenes = max(2, int(n_scenes * args.scale))
        scenes, sides = population(side, n_scenes)
        centers = np.stack([c for _, c in scenes])
        block, shapes = pad_frames([im for im, _ in scenes])
        H, W = block.shape[2:]

        def make(ragged):
            fs = shapes if ragged else None
            obs = [ObservationBatch(block[:, :SPLIT], band0=0, frame_shapes=fs),
                   ObservationBatch(block[:, SPLIT:], band0=SPLIT, frame_shapes=fs)]
            return BlendBatch.from_observations(obs, centers, mse_capacity=cap, centroid_weight=cw).init_combined(bg)

        times = dict(ragged=[], uniform=[])
        for _ in range(args.repeats):                   # alternating, on fresh batches
            for leg in ("ragged", "uniform"):
                b = make(leg == "ragged")
                times[leg].append(timed(b, args.steps, args.warmup))
                del b
        row = dict(padded=[int(H), int(W)], scenes=n_scenes, mean_frame_pixels=float((sides[:, 0] * sides[:, 1]).mean()),
                   padding_share_of_pixels=float(1 - (sides[:, 0] * sides[:, 1]).mean() / (H * W)))
        for leg, t in times.items():
            ms = float(np.median(t))
            row[leg] = dict(ms=ms, repeats=t, scene_iterations_per_s=n_scenes * args.steps / ms * 1e3)
        row["ragged_ms_over_uniform_ms"] = row["ragged"]["ms"] / row["uniform"]["ms"]
        for leg in ("ragged", "uniform"):
            b = make(leg == "ragged")
            b.fit(args.warmup, e_rel=0, check_every=0)
            torch.cuda.synchronize()
            _lib.check(_lib.lib.scarlet_profile_begin(args.steps))
            b.fit(args.steps, e_rel=0, check_every=0)
            tot, cnt = (ctypes.c_double * 8)(), (ctypes.c_int64 * 8)()
            _lib.check(_lib.lib.scarlet_profile_end(tot, cnt))
            row[leg]["kernel_ms"] = dict(planes=tot[0], contract_step=tot[1], update=tot[2], k_converge=tot[3])
            row[leg]["launches"] = [int(v) for v in cnt][:4]
            del b
        res["frames"].append(row)
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
