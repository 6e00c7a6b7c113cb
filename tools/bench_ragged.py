"""Timing of ragged batches: scenes with different numbers of sources in one BlendBatch (n_components).  bench.py
measures the BASELINE configs and is left alone.

Workloads (the counts n_s are drawn per scene with a fixed seed; scene s is one of a few synthetic templates with n_s
sources, the uniform batch the same templates with K sources):
  R1  10 000 scenes 5 x 64^2, K = 4, n_s uniform in 1..4   vs the same templates with n_s = 4, and vs the four
                                                            K = n buckets of the ragged scenes fitted one after
                                                            another (what a caller without n_components has to do)
  R2  64 scenes 6 x 256^2, K = 30, n_s uniform in 1..30    vs every n_s = 30
  R3  16 scenes 6 x 256^2, K = 64, n_s uniform in 33..64   vs every n_s = 64
  R4  64 scenes 6 x 256^2, K = 40, n_s uniform in 1..40    vs every n_s = 40 (the K > 32 path with most scenes of at
                                                            most 32 components: one 32-block of the Gram instead of two)
Each run: init_extended, `--warmup` iterations, then `--steps` iterations at e_rel = 0 timed with CUDA events, three
repeats; the median is reported in ms per iteration.  Prints one JSON line per workload and, with --out, writes them
all to a JSON file.  --only ragged / uniform times one of the two batches (for a kernel trace of each).

    python tools/bench_ragged.py --steps 10 --warmup 3 --out profiles/ragged_bench.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {
    "R1": dict(S=10000, B=5, H=64, W=64, K=4, n_lo=1, n_hi=4, distinct=16, buckets=True),
    "R2": dict(S=64, B=6, H=256, W=256, K=30, n_lo=1, n_hi=30, distinct=4, buckets=False),
    "R3": dict(S=16, B=6, H=256, W=256, K=64, n_lo=33, n_hi=64, distinct=4, buckets=False),
    "R4": dict(S=64, B=6, H=256, W=256, K=40, n_lo=1, n_hi=40, distinct=4, buckets=False),
}


def scenes(w):
    """ragged batch: scene s shows n_s sources (a catalogue's blend list); uniform batch: the same templates with K"""
    from scarlet_amd import synth
    n = np.random.default_rng(0).integers(w["n_lo"], w["n_hi"] + 1, size=w["S"]).astype(np.int32)
    made = {}

    def scene(i, k):
        if (i, k) not in made:
            sc = synth.make_scene(9700 + i, B=w["B"], H=w["H"], W=w["W"], K=int(k), min_sep=4)
            cen = np.zeros((w["K"], 2), np.int32)
            cen[:k] = sc["centers"]
            made[(i, k)] = (sc["images"], cen)
        return made[(i, k)]
    t = np.arange(w["S"]) % w["distinct"]
    ragged = [scene(i, k) for i, k in zip(t, n)]
    uniform = [scene(i, w["K"]) for i in t]
    stack = lambda sc: (np.stack([a for a, _ in sc]), np.stack([c for _, c in sc]))
    return stack(ragged), stack(uniform), n


def time_fit(images, centers, n, B, steps, warmup, repeats):
    """median ms per iteration of one batch (n = None: every scene has K components)"""
    import torch
    from scarlet_amd.batch import BlendBatch
    times = []
    for _ in range(repeats):
        b = BlendBatch(images, centers, n_components=n, mse_capacity=warmup + steps + 1)
        b.init_extended(np.ones(B) * 0.1)
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
    return float(np.median(times)), times


def run(name, w, steps, warmup, repeats, only=None):
    import torch
    (images, centers), (images_u, centers_u), n = scenes(w)
    r = dict(workload="%s: %d x %d x %d x %d, K=%d, n_s in %d..%d" % (name, w["S"], w["B"], w["H"], w["W"], w["K"],
                                                                     w["n_lo"], w["n_hi"]),
             name=name, mean_n=float(n.mean()))
    if only != "uniform":
        ragged, ragged_r = time_fit(images, centers, n, w["B"], steps, warmup, repeats)
        r.update(ms_per_iteration_ragged=ragged, ms_per_iteration_ragged_repeats=ragged_r)
    if only != "ragged":
        uniform, uniform_r = time_fit(images_u, centers_u, None, w["B"], steps, warmup, repeats)
        r.update(ms_per_iteration_uniform=uniform, ms_per_iteration_uniform_repeats=uniform_r)
    if only is None:
        r.update(ragged_over_uniform=ragged / uniform)
    if w["buckets"] and only is None:
        per_bucket = {}
        for k in range(w["n_lo"], w["n_hi"] + 1):
            sel = n == k
            per_bucket[k] = time_fit(images[sel], np.ascontiguousarray(centers[sel, :k]), None, w["B"], steps, warmup,
                                     repeats)[0]
        r.update(ms_per_iteration_buckets=float(sum(per_bucket.values())),
                 ms_per_iteration_bucket={str(k): v for k, v in per_bucket.items()},
                 bucket_scenes={str(k): int((n == k).sum()) for k in per_bucket},
                 ragged_over_buckets=ragged / sum(per_bucket.values()))
    r.update(steps=steps, warmup=warmup, device=torch.cuda.get_device_name())
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--workloads", default="R1,R2,R3,R4")
    ap.add_argument("--only", choices=("ragged", "uniform"), default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = []
    for name in args.workloads.split(","):
        r = run(name, WORKLOADS[name], args.steps, args.warmup, args.repeats, args.only)
        print(json.dumps(r), flush=True)
        res.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
