#!/usr/bin/env python
"""Joint fits of cut-outs with their own frame sizes against a low-resolution observation, timed against the uniform
low-resolution fit of the same number of scenes all at the padded size (which the code before this feature runs too:
it is the baseline).

    workload   --scenes cut-outs whose model sides are spread evenly over 0.5 .. 1 x --side (even sides; the
               low-resolution observation has half the side, pixel ratio 2), 3 sources each, a 3-band same-grid
               observation and a 2-band low-resolution one; every scene has its own LowResObservation.match(own frame)
    ragged     BlendBatch.from_observations([ObservationBatch.from_frames, LowResObservationBatch.from_frames(geometry=)])
               in both forms: as the shape comes (LDS-resident where the maxima fit) and under LOWRES_STREAMED=1
    uniform    the same number of scenes, all --side x --side with one geometry repeated, in both forms

    same grid  both batches again with the two low-resolution bands observed on the model's grid instead: what a ragged
               batch costs beside a uniform one WITHOUT a low-resolution operator (its constraint kernels run on each
               scene's own frame; that path is older than this tool)

The six runs alternate inside every one of --rounds rounds (same process, same device), each a fit of --steps iterations
between device events after a warm-up fit; per run the JSON keeps every round's ms per iteration, the median and the
spread (max - min) / median, and the ratios of the medians, for every batch size of --scenes.  Expectation: ragged /
uniform <= 1 beyond the spread in the LDS-resident form (strictly less work per scene), about 1 in the streamed form (it
streams the padding: the same work).

    python tools/bench_ragged_lowres.py [--scenes 64,2048] [--side 64] [--steps 20] [--rounds 7] [--out PATH] [--notes PATH]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HI_BANDS, LO_BANDS, K = 3, 2, 3


def geometry(side, cache={}):
    if side in cache:
        return cache[side]
    import scarlet_amd as scarlet
    from scarlet_amd import synth
    from scarlet_amd.resampling import AffineWCS
    C = HI_BANDS + LO_BANDS
    ch = ["c%d" % c for c in range(C)]
    model_psf = synth.gaussian_psf((11, 11), 0.9)[None].astype(np.float32)
    lr_psfs = np.array([synth.gaussian_psf((9, 9), 0.9 + 0.15 * b) for b in range(LO_BANDS)]).astype(np.float32)
    frame = scarlet.Frame((C, side, side), wcs=AffineWCS((side, side), 1.0), psfs=model_psf, channels=ch)
    wl = AffineWCS((side // 2, side // 2), 2.0, crpix=(1.0, 1.0))
    geo = scarlet.LowResObservation(np.zeros((LO_BANDS, side // 2, side // 2), np.float32), wcs=wl, psfs=lr_psfs,
                                    channels=ch[HI_BANDS:]).match(frame)
    assert geo.covers
    cache[side] = geo
    return geo


def scene(side, seed):
    """(images_hi, images_lo, sed0, morph0, centres, the low-resolution bands on the model's grid) of one cut-out"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:side, :side]
    cen = np.array([(side // 2, side // 2), (side // 3 - 1, (2 * side) // 3), ((2 * side) // 3 + 1, side // 3 - 1)], dtype=np.int32)
    morph = np.array([np.exp(-((y - c[0]) ** 2 + (x - c[1]) ** 2) / (2 * (1.6 + 0.4 * k) ** 2)) for k, c in enumerate(cen)])
    sed = 1.0 + rng.random((K, HI_BANDS + LO_BANDS))
    model = np.einsum("kc,kyx->cyx", sed, morph)
    f = geometry(side).factors
    lo = np.real(f["vy"] @ ((f["uy"] @ model[HI_BANDS:] @ f["ux"].T) * f["dhat"]) @ f["vx"].T)
    noise = lambda a: (a + 0.02 * rng.standard_normal(a.shape)).astype(np.float32)
    return noise(model[:HI_BANDS]), noise(lo), (1.1 * sed).astype(np.float32), morph.astype(np.float32), cen, noise(model[HI_BANDS:])


def build(sides, ragged, lowres=True):
    import scarlet_amd as scarlet
    data = [scene(s, 100 + i) for i, s in enumerate(sides)]
    geos = [geometry(s) for s in sides]
    cen = np.stack([d[4] for d in data])
    if ragged:
        hi = scarlet.ObservationBatch.from_frames([d[0] for d in data], band0=0)
        lo = (scarlet.LowResObservationBatch.from_frames([d[1] for d in data], band0=HI_BANDS, geometry=geos) if lowres
              else scarlet.ObservationBatch.from_frames([d[5] for d in data], band0=HI_BANDS))
    else:
        hi = scarlet.ObservationBatch(np.stack([d[0] for d in data]), band0=0)
        lo = (scarlet.LowResObservationBatch(np.stack([d[1] for d in data]), band0=HI_BANDS, geometry=geos) if lowres
              else scarlet.ObservationBatch(np.stack([d[5] for d in data]), band0=HI_BANDS))
    b = scarlet.BlendBatch.from_observations([hi, lo], cen, mse_capacity=4096)
    sed = np.stack([d[2] for d in data])
    morph = np.zeros((len(data), K, b.H, b.W), np.float32)
    for i, d in enumerate(data):
        morph[i, :, :d[3].shape[1], :d[3].shape[2]] = d[3]
    b.set_state(sed, morph)
    return b


RUNS = [("ragged", 0, "ragged_lds"), ("uniform", 0, "uniform_lds"), ("ragged", 1, "ragged_streamed"),
        ("uniform", 1, "uniform_streamed"), ("ragged_same_grid", 0, "ragged_same_grid"), ("uniform_same_grid", 0, "uniform_same_grid")]


def run_case(S, args):
    import torch
    from scarlet_amd import _lib
    side = args.side
    sides = [int(2 * round(v / 2)) for v in np.linspace(side / 2, side, S)]
    batches = {"ragged": build(sides, True), "uniform": build([side] * S, False),
               "ragged_same_grid": build(sides, True, False), "uniform_same_grid": build([side] * S, False, False)}

    def fit(which, streamed, steps):
        old = _lib.set_option("LOWRES_STREAMED", streamed)
        try:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            batches[which].fit(steps, e_rel=0, check_every=0)
            t1.record()
            torch.cuda.synchronize()
        finally:
            _lib.set_option("LOWRES_STREAMED", old)
        return t0.elapsed_time(t1) / steps

    for which, streamed, _ in RUNS:                   # warm-up of every form
        fit(which, streamed, 3)
    times = {name: [] for _, _, name in RUNS}
    for _ in range(args.rounds):
        for which, streamed, name in RUNS:
            times[name].append(fit(which, streamed, args.steps))
    for b in batches.values():
        b.raise_on_status()
    res = {}
    for k, v in times.items():
        med = float(np.median(v))
        res[k] = dict(ms_per_iteration=[round(x, 4) for x in v], median=med, spread=(max(v) - min(v)) / med)
    ratio = lambda a, b: res[a]["median"] / res[b]["median"]
    res["ratios"] = dict(ragged_lds_over_uniform_lds=ratio("ragged_lds", "uniform_lds"),
                         ragged_streamed_over_uniform_streamed=ratio("ragged_streamed", "uniform_streamed"),
                         ragged_streamed_over_ragged_lds=ratio("ragged_streamed", "ragged_lds"),
                         ragged_same_grid_over_uniform_same_grid=ratio("ragged_same_grid", "uniform_same_grid"))
    # what the low-resolution observation adds to an iteration of each kind of batch
    res["lowres_cost_ms"] = dict(ragged_lds=res["ragged_lds"]["median"] - res["ragged_same_grid"]["median"],
                                 uniform_lds=res["uniform_lds"]["median"] - res["uniform_same_grid"]["median"],
                                 ragged_streamed=res["ragged_streamed"]["median"] - res["ragged_same_grid"]["median"],
                                 uniform_streamed=res["uniform_streamed"]["median"] - res["uniform_same_grid"]["median"])
    lo = batches["ragged"]._observations[1][0]
    res["config"] = dict(scenes=S, side=side, distinct_sides=sorted(set(sides)),
                         own_pixels_over_padded=sum(s * s for s in sides) / float(S * side * side), sources=K, hi_bands=HI_BANDS,
                         lo_bands=LO_BANDS, maxima=[int(v) for v in lo.dims.max(axis=0)], steps=args.steps, rounds=args.rounds)
    return res


NOTES = """# Ragged-frame batches against a low-resolution observation: timings

Written by `tools/bench_ragged_lowres.py`; the numbers are in `ragged_lowres_bench.json` beside this file.

Workload: cut-outs with model sides spread evenly over %(lo)d .. %(side)d px (their own pixels are %(pix).0f %% of the
padded %(side)d x %(side)d blocks'), %(K)d sources each, a %(hb)d-band same-grid observation and a %(lb)d-band low-resolution
one at pixel ratio 2, every scene with its own operator.  Baseline: the uniform low-resolution fit of the same number of
scenes all at %(side)d x %(side)d, which the code before this feature runs as well.  "same grid" are the two batches with the
low-resolution bands observed on the model's grid instead: a ragged batch beside a uniform one without any
low-resolution operator.  The six runs alternate inside each of %(rounds)d rounds of %(steps)d iterations, timed with device
events after a warm-up; "spread" is (max - min) / median over the rounds.  ms per iteration of the whole batch:

%(tables)s
Reading:
- **ragged / uniform, LDS-resident** is the figure the feature is judged by.  Both batches run the same-grid planes and
  the contraction on the padded frame; they differ in the low-resolution kernel (each scene's workgroup runs over its own
  sizes) and in the constraint kernels, which run on each scene's own frame in a ragged batch.  The "same grid" pair
  shows what the latter costs by itself, and "low-resolution cost" is what the observation adds to an iteration of each
  kind of batch (median minus the same-grid median of that kind).
- With fewer scenes than the device has compute units (64 against 256) the one-workgroup-per-scene kernel takes as long
  as its largest scene, which is a full-size one: the ragged instance can at best be as fast as the uniform one there,
  and the whole iteration is slower than the uniform batch's by what the ragged constraint kernels cost.  With many
  scenes the smaller ones free their compute units early, and the low-resolution cost falls below the uniform batch's.
- **ragged / uniform, streamed**: the streamed form runs the chain on the padded extents of every scene with
  zero-padded tables.  It streams the padding -- the uniform batch's work plus per-scene reads of uy and ux -- and that
  cost is not trimmed here.

Not measured: batches whose maxima do not fit LDS (the streamed form as it comes), other pixel ratios, band counts and
frame sizes than the ones above, per-kernel times (these are whole iterations between device events), and the host cost
of matching one geometry per scene.
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="64,2048", help="batch sizes, comma-separated")
    ap.add_argument("--side", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_lowres_bench.json"))
    ap.add_argument("--notes", default=os.path.join(ROOT, "profiles", "ragged_lowres_notes.md"))
    args = ap.parse_args()
    import torch
    res = {}
    for S in [int(v) for v in args.scenes.split(",")]:
        res["S%d" % S] = run_case(S, args)
    res["device"] = torch.cuda.get_device_name()
    print(json.dumps(res))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
    tables = ""
    for key, r in res.items():
        if not key.startswith("S"):
            continue
        tables += "%d scenes\n\n| run | median | spread |\n|---|---|---|\n" % r["config"]["scenes"]
        for _, _, name in RUNS:
            tables += "| %s | %.3f | %.1f %% |\n" % (name.replace("_", " "), r[name]["median"], 100 * r[name]["spread"])
        tables += "\n| ratio of medians | |\n|---|---|\n"
        for k, v in r["ratios"].items():
            tables += "| %s | %.3f |\n" % (k.replace("_over_", " / ").replace("_", " "), v)
        tables += "\n| low-resolution cost (ms per iteration) | |\n|---|---|\n"
        for k, v in r["lowres_cost_ms"].items():
            tables += "| %s | %.3f |\n" % (k.replace("_", " "), v)
        diff = lambda x, y: r[x]["median"] - r[y]["median"]
        tables += ("\nragged - uniform: %+.3f ms LDS-resident and %+.3f ms streamed, of which %+.3f ms are the same-grid pair's "
                   "(the constraint kernels on each scene's own frame).\n\n"
                   % (diff("ragged_lds", "uniform_lds"), diff("ragged_streamed", "uniform_streamed"),
                      diff("ragged_same_grid", "uniform_same_grid")))
    c = next(r for k, r in res.items() if k.startswith("S"))["config"]
    with open(args.notes, "w") as fh:
        fh.write(NOTES % dict(lo=min(c["distinct_sides"]), side=args.side, pix=100 * c["own_pixels_over_padded"], K=K, hb=HI_BANDS,
                              lb=LO_BANDS, rounds=args.rounds, steps=args.steps, tables=tables))


if __name__ == "__main__":
    main()
