"""Timing of catalogue batches: ragged-frame cut-outs that hold stars, plain galaxies and bulge+disk galaxies
(BlendBatch.from_catalog / init_catalog / fit).  bench.py measures the BASELINE configs and is left alone.

A seeded population of S = 3072 cut-outs, B = 5, heights and widths drawn independently and uniformly from 24..64 (padded
64 x 64), 3 to 5 components per scene: every third scene holds a two-layer source ([25]), a point source and 0 to 2
extended sources, the others 3 to 5 extended sources.  Two routes are timed:
  (a) catalog  one from_catalog batch: every scene started (init_catalog) and fitted on its own frame -- the general
               ragged path with k_group_centers<RAGGED> in front of the RAGGED update kernels;
  (b) padded   the same scenes zero-padded to 64 x 64 with zero weights outside, as one uniform batch with group= and
               init_sources(kind=): the route such a catalogue had before.  It computes ANOTHER result (the constraints see
               the padded frame); it is quoted as a cost comparison only.
Per route: the start (one call of init_catalog / init_sources on a fresh batch, host clock around a device synchronise;
the first repeat loads the code objects and is reported apart), and the fit (`--warmup` iterations, then `--steps`
iterations at e_rel = 0 between two device events: 400 by default, about half a second).  A scene that ends with a status
(a centre the reference's max_pixel refuses, a start the reference refuses) is counted per status value; such scenes are
part of a real catalogue and stay in the timing.  `--repeats` repeats on fresh batches, alternating the routes; the
median and every repeat are written.

    python tools/bench_catalog.py --out profiles/catalog_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, B, LO, HI = 3072, 5, 24, 64


def population(n_scenes, seed=0):
    """[(images (B, h, w), [(centre, kind, percentiles)])]: the cut-outs and their catalogues"""
    from scarlet_amd import synth
    rng = np.random.default_rng(seed)
    sides = rng.integers(LO, HI + 1, size=(n_scenes, 2))
    sides[0] = (HI, HI)                              # (the padded frame is HI x HI whatever the draw)
    extra = rng.integers(0, 3, size=n_scenes)
    out = []
    for i, (h, w) in enumerate(sides):
        kinds = ["multi", "point"] + ["extended"] * int(extra[i]) if i % 3 == 0 else ["extended"] * (3 + int(extra[i]))
        sc = synth.make_scene(61000 + i, B=B, H=int(h), W=int(w), K=len(kinds), min_sep=2)
        cat = [((int(y), int(x)), kind, [25] if kind == "multi" else None) for (y, x), kind in zip(sc["centers"], kinds)]
        out.append((sc["images"], cat))
    return out, sides.astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--scenes", type=int, default=S)
    ap.add_argument("--out", default="catalog_bench_run.json")
    args = ap.parse_args()
    from scarlet_amd import _lib
    from scarlet_amd.batch import BlendBatch, SourceSpec, catalog_arrays, default_centroid_weight, pad_frames
    scenes, sides = population(args.scenes)
    specs = [[SourceSpec(px, kind=kind, flux_percentiles=perc) for px, kind, perc in cat] for _, cat in scenes]
    cutouts = [im for im, _ in scenes]
    t = catalog_arrays(sides, specs)
    block, shapes = pad_frames(cutouts)
    mask = np.zeros(block.shape, np.float32)
    for s, (h, w) in enumerate(sides):
        mask[s, :, :h, :w] = 1
    kind = np.where(t["kind"] == _lib.INIT_POINT, "point", "extended")
    torch = _lib.require_gpu()                       # (a measurement needs the device: no fallback)
    cw = default_centroid_weight()
    bg = np.ones(B) * 0.1
    cap = args.steps + args.warmup + 1

    def catalog():
        b = BlendBatch.from_catalog(cutouts, specs, mse_capacity=cap, centroid_weight=cw)
        return b, lambda: b.init_catalog(bg)

    def padded():
        b = BlendBatch(block, t["centers"], weights=mask, group=t["group"], n_components=t["n_components"], mse_capacity=cap,
                       centroid_weight=cw)
        return b, lambda: b.init_sources(bg, kind=kind, flux_percentiles=t["percentiles"])

    def one(build):
        b, start = build()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        start()
        torch.cuda.synchronize()
        init_ms = (time.perf_counter() - t0) * 1e3
        b.fit(args.warmup, e_rel=0, check_every=0)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.fit(args.steps, e_rel=0, check_every=0)
        e1.record()
        torch.cuda.synchronize()
        st = b.status.cpu().numpy()
        bits = {int(v): int((st == v).sum()) for v in np.unique(st[st != 0])}      # status value -> scenes that carry it
        return init_ms, e0.elapsed_time(e1), bits

    runs = dict(catalog=[], padded=[])
    for r in range(args.repeats + 1):                # repeat 0 loads the code objects of both routes
        for name, build in (("catalog", catalog), ("padded", padded)):
            runs[name].append(one(build))
    comps = int(t["n_components"].sum())
    res = dict(scenes=args.scenes, B=B, sides=[LO, HI], padded_frame=[int(block.shape[2]), int(block.shape[3])], components=comps,
               components_per_scene=[int(t["n_components"].min()), int(t["n_components"].max())],
               scenes_with_a_two_layer_and_a_point_source=int((t["group"] >= 0).any(axis=1).sum()), steps=args.steps,
               warmup=args.warmup, repeats=args.repeats, device=torch.cuda.get_device_name(),
               mean_frame_pixels=float((sides[:, 0] * sides[:, 1]).mean()))
    for name, rows in runs.items():
        init = [x[0] for x in rows[1:]]
        fit = [x[1] for x in rows[1:]]
        res[name] = dict(first_init_ms=rows[0][0], init_ms=float(np.median(init)), init_repeats=init,
                         fit_ms=float(np.median(fit)), fit_repeats=fit, ms_per_iteration=float(np.median(fit)) / args.steps,
                         scene_iterations_per_s=args.scenes * args.steps / float(np.median(fit)) * 1e3,
                         status_values_and_their_scenes=rows[-1][2])
    res["catalog_fit_ms_over_padded_fit_ms"] = res["catalog"]["fit_ms"] / res["padded"]["fit_ms"]
    res["catalog_init_ms_over_padded_init_ms"] = res["catalog"]["init_ms"] / res["padded"]["init_ms"]
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
