"""What update options cost a catalogue batch: the workload of tools/bench_catalog.py (S = 3072 ragged cut-outs of 24..64
pixels a side, 3 to 5 components per scene, every third scene with a two-layer and a point source) fitted
  (a) plain    without options: scarlet_fit_frames_grouped, the RAGGED update kernels;
  (b) default  with update=UpdateOptions() -- the stock pipeline's values as device rows: scarlet_fit_frames_options, the
               RAGGED x OPTIONS instances computing the same bits;
  (c) mixed    with the "mixed" options of tests/update_option_cases.py per source (source i takes index i + 1: sdss symmetry
               with the nearest-neighbour sweep, or soft symmetry of strength 0.3 with a thresholded sweep, positive="morph"
               and normalization="morph"), another result.
on the same commit, alternating on fresh batches.  Per route: the start (init_catalog, host clock around a device
synchronise; the first repeat loads the code objects and is reported apart) and the fit (`--warmup` iterations, then `--steps`
at e_rel = 0 between two device events).  The median and every repeat are written.

The other half of the measurement needs no code of its own: tools/bench_catalog.py and tools/bench_update_options.py, run
unchanged on the parent commit (three times: the spread is the margin) and on this one; `--merge` collects their JSON
files into the output.

    python tools/bench_catalog_options.py --out profiles/catalog_options_bench.json \\
        --merge parent_catalog=p1.json,p2.json,p3.json branch_catalog=b1.json ...
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

_MIXED = (dict(symmetry="sdss", use_nearest=True),
          dict(symmetry="soft", strength=0.3, monotonic_thresh=0.05, positive="morph", normalization="morph"))


def main():
    import bench_catalog as bc
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--scenes", type=int, default=bc.S)
    ap.add_argument("--out", default="catalog_options_bench_run.json")
    ap.add_argument("--merge", nargs="*", default=[], help="name=file.json[,file.json...]: results of the other tools to carry along")
    args = ap.parse_args()
    from scarlet_amd import _lib
    from scarlet_amd.batch import BlendBatch, SourceSpec, UpdateOptions, default_centroid_weight
    scenes, sides = bc.population(args.scenes)
    cutouts = [im for im, _ in scenes]

    def specs(mixed):
        return [[SourceSpec(px, kind=kind, flux_percentiles=perc, **(_MIXED[i % 2] if mixed else {}))
                 for i, (px, kind, perc) in enumerate(cat)] for _, cat in scenes]

    plain_specs, mixed_specs = specs(False), specs(True)
    torch = _lib.require_gpu()                       # (a measurement needs the device: no fallback)
    cw = default_centroid_weight()
    bg = np.ones(bc.B) * 0.1
    cap = args.steps + args.warmup + 1
    routes = (("plain", plain_specs, None), ("default", plain_specs, UpdateOptions()), ("mixed", mixed_specs, None))

    def one(sp, update):
        b = BlendBatch.from_catalog(cutouts, sp, mse_capacity=cap, centroid_weight=cw, update=update)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        b.init_catalog(bg)
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
        return init_ms, e0.elapsed_time(e1), {int(v): int((st == v).sum()) for v in np.unique(st[st != 0])}

    runs = {name: [] for name, _, _ in routes}
    for r in range(args.repeats + 1):                # repeat 0 loads the code objects of every route
        for name, sp, update in routes:
            runs[name].append(one(sp, update))
    res = dict(scenes=args.scenes, B=bc.B, sides=[bc.LO, bc.HI], steps=args.steps, warmup=args.warmup, repeats=args.repeats,
               device=torch.cuda.get_device_name())
    for name, rows in runs.items():
        init, fit = [x[0] for x in rows[1:]], [x[1] for x in rows[1:]]
        res[name] = dict(first_init_ms=rows[0][0], init_ms=float(np.median(init)), init_repeats=init,
                         fit_ms=float(np.median(fit)), fit_repeats=fit, ms_per_iteration=float(np.median(fit)) / args.steps,
                         status_values_and_their_scenes=rows[-1][2])
    for name in ("default", "mixed"):
        res["%s_fit_ms_over_plain_fit_ms" % name] = res[name]["fit_ms"] / res["plain"]["fit_ms"]
        res["%s_init_ms_over_plain_init_ms" % name] = res[name]["init_ms"] / res["plain"]["init_ms"]
    for item in args.merge:
        name, files = item.split("=", 1)
        res[name] = [json.load(open(f)) for f in files.split(",")]
    print(json.dumps({k: v for k, v in res.items() if k not in [m.split("=", 1)[0] for m in args.merge]}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
