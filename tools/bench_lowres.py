#!/usr/bin/env python
"""Per-iteration time of a joint fit against a low-resolution observation, beside two baselines on the same batch:

    hr_only      the batch fitted against its 5-band observation on the model's grid alone (BlendBatch.fit)
    two_grid     ... jointly against that and a second 4-band observation on the same grid (from_observations)
    lowres       ... jointly against that and a 4-band 32 x 32 observation at pixel ratio 2 (LowResObservationBatch)

Default: 4096 scenes of 5 x 64 x 64 with 4 sources.  Times are device events around `fit(steps, e_rel=0)` after a
warm-up fit, best of `--repeats`; the JSON goes to profiles/lowres_bench.json (or --out).

    python tools/bench_lowres.py [--scenes 4096] [--steps 20] [--warmup 5] [--repeats 3] [--out PATH]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=4096)
    ap.add_argument("--distinct", type=int, default=256, help="scenes generated; the batch repeats them")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lowres_bench.json"))
    args = ap.parse_args()

    import torch
    import scarlet_amd as scarlet
    from scarlet_amd import synth
    from scarlet_amd.resampling import AffineWCS

    S, B, H, W, K, h, w, Bl = args.scenes, 5, 64, 64, 4, 32, 32, 4
    d = synth.make_batch(9000, min(args.distinct, S), B=B, H=H, W=W, K=K)
    reps = -(-S // len(d["images"]))
    images = np.tile(d["images"], (reps, 1, 1, 1))[:S]
    centers = np.tile(d["centers"], (reps, 1, 1))[:S]
    # the coarse data: 2 x 2 sums of the first four bands (flux per pixel at pixel ratio 2)
    coarse = images[:, :Bl].reshape(S, Bl, h, 2, w, 2).sum(axis=(3, 5)).astype(np.float32)
    model_psf = synth.gaussian_psf((11, 11), 0.9)[None].astype(np.float32)
    lr_psfs = np.array([synth.gaussian_psf((9, 9), 0.9 + 0.1 * b) for b in range(Bl)]).astype(np.float32)
    ch = list("grizy")
    frame = scarlet.Frame((B, H, W), wcs=AffineWCS((H, W), 1.0), psfs=model_psf, channels=ch)
    geo = scarlet.LowResObservation(coarse[0], wcs=AffineWCS((h, w), 2.0), psfs=lr_psfs, channels=ch[:Bl]).match(frame)
    bg = np.ones(B, np.float32) * 0.1

    def timed(b):
        b.fit(args.warmup, e_rel=0, check_every=0)
        best = None
        for _ in range(args.repeats):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            b.fit(args.steps, e_rel=0, check_every=0)
            t1.record()
            torch.cuda.synchronize()
            ms = t0.elapsed_time(t1) / args.steps
            best = ms if best is None else min(best, ms)
        b.raise_on_status()
        return best

    res = {}
    b = scarlet.BlendBatch(images, centers).init_extended(bg)
    res["hr_only_ms_per_iteration"] = timed(b)
    sed0, morph0 = b.sed_current.clone(), b.morph_current.clone()
    del b

    def joint(second):
        b = scarlet.BlendBatch.from_observations([scarlet.ObservationBatch(images, band0=0), second], centers)
        b.set_state(sed0, morph0)
        return timed(b)
    # (both joint fits start from the single-observation fit's state: the same work per iteration for either)
    res["two_grid_ms_per_iteration"] = joint(scarlet.ObservationBatch(images[:, :Bl], band0=0))
    res["lowres_ms_per_iteration"] = joint(scarlet.LowResObservationBatch(coarse, band0=0, geometry=geo))
    res["second_observation_cost_ms"] = dict(same_grid=res["two_grid_ms_per_iteration"] - res["hr_only_ms_per_iteration"],
                                             low_resolution=res["lowres_ms_per_iteration"] - res["hr_only_ms_per_iteration"])
    f = geo.factors
    res["config"] = dict(scenes=S, bands=B, H=H, W=W, sources=K, lowres_bands=Bl, h=h, w=w, pixel_ratio=2.0,
                         padded_plane=list(f["fft_shape"]), nfy=int(f["uy"].shape[0]), nfx=int(f["ux"].shape[0]),
                         steps=args.steps, warmup=args.warmup, repeats=args.repeats, device=torch.cuda.get_device_name())
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
