"""Timing of crowded scenes, more than 32 components per scene (bench.py measures the BASELINE configs and is left
alone).

Workloads: 16 scenes of 6 x 256 x 256 with 64 sources, 4 scenes of 6 x 512 x 512 with 128 sources and 1 scene of
6 x 1024 x 1024 with 256 sources (a 256 x 256 scene of 16 sources tiled 4 x 4).  A few distinct synthetic scenes are
tiled to the batch size (scenes are independent).  Each workload: init_extended, `--warmup` iterations, then `--steps`
iterations at e_rel = 0 timed with CUDA events, three repeats; the median is reported as ms per iteration and as ns per
pixel x component (comparable with tools/bench_large.py).  The same is timed with approximate_L = True, which skips
the exact lambda_max(S S^T) (the Gram matrix is still formed): the difference is the share of the eigenvalue pass.
Prints one JSON line per workload and, with --out, writes them all to a JSON file.

    python tools/bench_crowded.py --steps 10 --warmup 3 --out profiles/crowded_bench.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {
    "256": dict(S=16, B=6, H=256, W=256, K=64, distinct=4, tile=1),
    "512": dict(S=4, B=6, H=512, W=512, K=128, distinct=2, tile=1),
    "1024": dict(S=1, B=6, H=1024, W=1024, K=256, distinct=1, tile=4),
}


def scenes(w):
    from scarlet_amd import synth
    n = w["tile"]
    H, W, K = w["H"] // n, w["W"] // n, w["K"] // (n * n)
    out = []
    for i in range(w["distinct"]):
        sc = synth.make_scene(9500 + i, B=w["B"], H=H, W=W, K=K, min_sep=4 if n == 1 else 12)
        images = np.tile(sc["images"], (1, n, n))
        centers = np.concatenate([sc["centers"] + np.array([H * (j // n), W * (j % n)], np.int32) for j in range(n * n)])
        out.append((images, centers))
    return out


def time_fit(images, centers, B, steps, warmup, repeats, approx):
    import torch
    from scarlet_amd.batch import BlendBatch
    times = []
    for _ in range(repeats):
        b = BlendBatch(images, centers, mse_capacity=warmup + steps + 1)
        b.init_extended(np.ones(B) * 0.1)
        b.fit(warmup, e_rel=0, approximate_L=approx, check_every=0)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.fit(steps, e_rel=0, approximate_L=approx, check_every=0)
        e1.record()
        torch.cuda.synchronize()
        assert int(b.status.abs().sum().item()) == 0
        times.append(e0.elapsed_time(e1) / steps)
        del b
    return float(np.median(times)), times


def run(name, w, steps, warmup, repeats):
    import torch
    sc = scenes(w)
    reps = w["S"] // w["distinct"]
    images = torch.as_tensor(np.stack([s[0] for s in sc])).cuda().repeat(reps, 1, 1, 1)
    centers = torch.as_tensor(np.stack([s[1] for s in sc])).cuda().repeat(reps, 1, 1)
    ms, times = time_fit(images, centers, w["B"], steps, warmup, repeats, False)
    ms_a, times_a = time_fit(images, centers, w["B"], steps, warmup, repeats, True)
    pix_comp = w["S"] * w["K"] * w["H"] * w["W"]
    return dict(workload="%d x %d x %d x %d, K=%d" % (w["S"], w["B"], w["H"], w["W"], w["K"]), name=name,
                ms_per_iteration=ms, ms_per_iteration_repeats=times,
                scene_iterations_per_s=w["S"] * 1e3 / ms, ns_per_pixel_component=ms * 1e6 / pix_comp,
                ms_per_iteration_approximate_L=ms_a, ms_per_iteration_approximate_L_repeats=times_a,
                lambda_max_share=(ms - ms_a) / ms,
                steps=steps, warmup=warmup, device=torch.cuda.get_device_name())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--workloads", default="256,512,1024")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = []
    for name in args.workloads.split(","):
        r = run(name, WORKLOADS[name], args.steps, args.warmup, args.repeats)
        print(json.dumps(r), flush=True)
        res.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
