"""Timing of BlendBatch.init_sources: 10 000 scenes of 5 x 64 x 64 with K = 4 (one two-layer MultiComponentSource, one
point source, one extended source, per-scene bg_rms), against init_extended on the same batch and against the
per-scene constructor path (scarlet_amd.MultiComponentSource / PointSource / ExtendedSource, one scene at a time),
timed on 100 scenes and scaled to the batch (labelled as scaled).

    python tools/bench_init.py [--scenes 10000] [--reps 5] [--ctor-scenes 100] [--out profiles/bench_init.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, torch, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ctor-scenes", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_init.json"))
    a = ap.parse_args()
    import torch
    import scarlet_amd as scarlet
    from scarlet_amd import synth
    base = [synth.make_scene(20000 + i, B=5, H=64, W=64, K=3, min_sep=10) for i in range(100)]
    S = a.scenes
    pick = np.arange(S) % len(base)
    images = np.stack([base[i]["images"] for i in pick])
    c = np.stack([base[i]["centers"] for i in pick])
    centers = np.concatenate([c[:, :1], c], axis=1).astype(np.int32)       # group (2 layers), point, extended
    group = np.tile(np.array([[0, 0, -1, -1]], np.int32), (S, 1))
    kind = np.tile(np.array([["extended", "extended", "point", "extended"]]), (S, 1))
    rng = np.random.default_rng(0)
    bg = (0.1 * (1 + 0.2 * rng.random((S, 5)))).astype(np.float32)
    b = scarlet.BlendBatch(images, centers, group=group)
    t_src = timed(lambda: b.init_sources(bg, kind=kind, flux_percentiles=[30]), torch, a.reps)
    t_ext = timed(lambda: b.init_extended(bg[0]), torch, a.reps)
    # the per-scene constructor path on a few scenes, scaled to S
    n = a.ctor_scenes

    def ctor():
        for s in range(n):
            im = images[s]
            frame = scarlet.Frame(im.shape)
            obs = scarlet.Observation(im).match(frame)
            p = [tuple(int(v) for v in centers[s, k]) for k in (0, 2, 3)]
            srcs = [scarlet.MultiComponentSource(frame, p[0], obs, bg[s], flux_percentiles=[30]),
                    scarlet.PointSource(frame, p[1], obs), scarlet.ExtendedSource(frame, p[2], obs, bg[s])]
            scarlet.Blend(srcs, obs)
    t0 = time.perf_counter()
    ctor()
    torch.cuda.synchronize()
    t_ctor = (time.perf_counter() - t0) * 1e3
    res = dict(scenes=S, B=5, H=64, W=64, K=4, reps=a.reps,
               init_sources_ms=float(np.median(t_src)), init_sources_all_ms=t_src,
               init_extended_ms=float(np.median(t_ext)), init_extended_all_ms=t_ext,
               constructors_scenes_timed=n, constructors_ms_timed=t_ctor,
               constructors_ms_scaled_to_batch=t_ctor * S / n,
               device=torch.cuda.get_device_name(0))
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
