"""Fits of batches with update options (BlendBatch(update=UpdateOptions(...))): scene-iterations per second on the general
path for two shapes,

  small   4096 scenes x 5 x 64 x 64, K = 4   (one wave per component)
  large   64 scenes x 6 x 256 x 256, K = 30  (the plane form: operators in place in HBM)

and per shape these legs, alternated in one process and repeated (`--repeats`), each timed with device events:

  default        update=None on the general path (NO_FUSED): the stock pipeline as the parent commit runs it -- beyond
                 64 pixels with its box stage
  default_full   the same with NO_BOX: the full-frame forms serve every component, as they do for every options batch
                 (only recorded where it differs from `default`, i.e. for the large shape)
  defaults       UpdateOptions() with every default: the options instances of the same kernels on the same work
  soft, sdss, thresh, nearest, norm_morph, norm_sed, pos_morph
                 one option for every component (tests/update_option_cases.py's sets)

With every leg go the launch counts and the summed device time per kernel class (scarlet_profile_end; class
k_source_update is the constraint stage, where the options live).  One JSON line; `--out` also writes it to a file."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = ["k_grad", "k_step", "k_source_update", "k_converge", "k_iterate", "psf_convolution", "k_prior_step"]
SHAPES = dict(small=dict(S=4096, B=5, side=64, K=4, iters=20, distinct=256),
              large=dict(S=64, B=6, side=256, K=30, iters=5, distinct=4))
OPTION_LEGS = dict(defaults=dict(), soft=dict(symmetry="soft", strength=0.5), sdss=dict(symmetry="sdss"),
                   thresh=dict(monotonic_thresh=0.1), nearest=dict(use_nearest=True), norm_morph=dict(normalization="morph"),
                   norm_sed=dict(normalization="sed"), pos_morph=dict(positive="morph"))


def run_shape(name, cfg, repeats, legs_wanted):
    import torch
    import scarlet_amd as scarlet
    from scarlet_amd import _lib, synth
    S, B, side, K, iters = cfg["S"], cfg["B"], cfg["side"], cfg["K"], cfg["iters"]
    d = synth.make_batch(4000, min(cfg["distinct"], S), B=B, H=side, W=side, K=K)
    reps = (S + len(d["images"]) - 1) // len(d["images"])
    images = torch.as_tensor(np.tile(d["images"], (reps, 1, 1, 1))[:S]).cuda()
    centers = np.tile(d["centers"], (reps, 1, 1))[:S]
    bg = np.ones(B) * 0.1
    legs = {}          # leg -> (batch, diagnostic switches)
    plain = scarlet.BlendBatch(images, centers, mse_capacity=iters + 1).init_extended(bg)
    legs["default"] = (plain, ("NO_FUSED",))
    if side > 64:
        legs["default_full"] = (plain, ("NO_FUSED", "NO_BOX"))
    for leg, kw in OPTION_LEGS.items():
        if leg in legs_wanted:
            legs[leg] = (scarlet.BlendBatch(images, centers, mse_capacity=iters + 1, update=scarlet.UpdateOptions(**kw)).init_extended(bg), ())
    legs = {k: v for k, v in legs.items() if k in legs_wanted}
    start = {id(b): (b.sed_current.clone(), b.morph_current.clone(), b.centers.clone(), b.shifts.clone()) for b, _ in legs.values()}

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
            assert n == iters and int(b.it.min().item()) == iters, (leg, n, int(b.it.min().item()))
            if profile:
                tot, cnt = (ctypes.c_double * 8)(), (ctypes.c_int64 * 8)()
                _lib.check(_lib.lib.scarlet_profile_end(tot, cnt))
                return ({NAMES[i]: int(cnt[i]) for i in range(len(NAMES)) if cnt[i]},
                        {NAMES[i]: round(float(tot[i]), 3) for i in range(len(NAMES)) if cnt[i]})
            return e0.elapsed_time(e1)
        finally:
            for o, p in zip(opts, prev):
                _lib.set_option(o, p)

    out = dict(scenes=S, bands=B, side=side, sources=K, iterations=iters)
    for leg in legs:
        out["launches_" + leg], out["class_ms_" + leg] = fit(leg, profile=True)           # (also the warm-up)
    ms = {leg: [] for leg in legs}
    for _ in range(repeats):
        for leg in legs:
            ms[leg].append(fit(leg))
    for leg in legs:
        out["ms_" + leg] = [round(v, 3) for v in ms[leg]]
        out["scene_iterations_per_s_" + leg] = round(S * iters / (float(np.median(ms[leg])) * 1e-3), 1)
    base = "default_full" if "default_full" in legs else "default"
    if base in legs:
        for leg in legs:
            out["ratio_to_%s_%s" % (base, leg)] = round(out["scene_iterations_per_s_" + leg] / out["scene_iterations_per_s_" + base], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="small,large")
    ap.add_argument("--legs", default="default,default_full," + ",".join(OPTION_LEGS))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--scenes", type=int, default=0, help="override the scene count of every shape (rehearsals)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = dict(bench="update_options", repeats=a.repeats)
    for name in a.shapes.split(","):
        cfg = dict(SHAPES[name])
        if a.scenes:
            cfg["S"] = a.scenes
        out[name] = run_shape(name, cfg, a.repeats, set(a.legs.split(",")))
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
