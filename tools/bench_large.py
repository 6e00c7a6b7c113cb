"""Timing of frames beyond 256 x 256 (bench.py measures the BASELINE configs and is left alone).

Workloads: 32 scenes of 6 x 512 x 512 with 30 sources and L0, and 8 scenes of 6 x 1024 x 1024 with 30 sources and L0.
A few distinct synthetic scenes are tiled to the batch size (scenes are independent).  Each workload: init_extended,
`--warmup` iterations, then `--steps` iterations at e_rel = 0 timed with CUDA events, three repeats; the median is
reported as ms per iteration and scene-iterations per second, plus the time per pixel x component for comparison with
other shapes.  Prints one JSON line per workload and, with --out, writes them all to a JSON file.

    python tools/bench_large.py --steps 10 --warmup 3 --out profiles/large_frames_bench.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {
    "512": dict(S=32, B=6, H=512, W=512, K=30, l0=0.05, distinct=4),
    "1024": dict(S=8, B=6, H=1024, W=1024, K=30, l0=0.05, distinct=2),
}


def run(name, w, steps, warmup, repeats):
    import torch
    from scarlet_amd import synth
    from scarlet_amd.batch import BlendBatch
    scenes = [synth.make_scene(9000 + i, B=w["B"], H=w["H"], W=w["W"], K=w["K"]) for i in range(w["distinct"])]
    reps = w["S"] // w["distinct"]
    images = torch.as_tensor(np.stack([s["images"] for s in scenes])).cuda().repeat(reps, 1, 1, 1)
    centers = torch.as_tensor(np.stack([s["centers"] for s in scenes])).cuda().repeat(reps, 1, 1)
    times = []
    for _ in range(repeats):
        b = BlendBatch(images, centers, l0_thresh=w["l0"], mse_capacity=warmup + steps + 1)
        b.init_extended(np.ones(w["B"]) * 0.1)
        b.fit(warmup, e_rel=0, check_every=0)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.fit(steps, e_rel=0, check_every=0)
        e1.record()
        torch.cuda.synchronize()
        assert int(b.status.abs().sum().item()) == 0
        times.append(e0.elapsed_time(e1) / steps)
        del b
    ms = float(np.median(times))
    pix_comp = w["S"] * w["K"] * w["H"] * w["W"]
    return dict(workload="%d x %d x %d x %d, K=%d, L0" % (w["S"], w["B"], w["H"], w["W"], w["K"]), name=name,
                ms_per_iteration=ms, ms_per_iteration_repeats=times,
                scene_iterations_per_s=w["S"] * 1e3 / ms, ns_per_pixel_component=ms * 1e6 / pix_comp,
                steps=steps, warmup=warmup, device=torch.cuda.get_device_name())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--workloads", default="512,1024")
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
