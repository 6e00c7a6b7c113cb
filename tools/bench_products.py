"""Timing of BlendBatch.products (scarlet_batch_products) on three shapes against the same quantities composed from torch
operations, and against one fit iteration of the same batch.  bench.py measures the BASELINE configs and is left alone.

Workloads (scene s is one of a few synthetic templates; the batch is initialised and fitted a few iterations first):
  headline  10 000 scenes 5 x 64^2,  K = 4, no PSF
  config3    4 096 scenes 5 x 128^2, K = 8, PSF 41^2 (the LDS-resident transform)
  config5       64 scenes 6 x 256^2, K = 30, no PSF
Per workload, timed with device events around `--inner` back-to-back calls after `--warmup` calls, `--repeats` times
(median, min and max are reported; the variants are interleaved so that they see the same machine):
  products_ms            products(model, residual, loss, flux) into reused buffers
  torch_ms               einsum over sed_current / morph_current (gathered outside the timed window), the convolution
                         through scarlet_convolve_same for config3, residual, float64 loss and flux
  torch_with_gather_ms   ... with the gather of the current buffers that a caller has to do inside the window
  fit_iteration_ms       one iteration of fit() on the batch
  hbm_fraction           algorithmic bytes -- K + B planes read, 2 B planes (model, residual) written -- over products_ms,
                         as a fraction of the 8.0 TB/s HBM peak

    python tools/bench_products.py --out profiles/products_bench.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12          # bytes / s (MI355X, HBM3E)
WORKLOADS = {
    "headline": dict(S=10000, B=5, H=64, W=64, K=4, psf=False, distinct=16),
    "config3": dict(S=4096, B=5, H=128, W=128, K=8, psf=True, distinct=8),
    "config5": dict(S=64, B=6, H=256, W=256, K=30, psf=False, distinct=4),
}


def make_batch(w):
    from oracle import pgm
    from scarlet_amd import synth
    from scarlet_amd.batch import BlendBatch
    kw, diff, scale, cw = dict(B=w["B"], H=w["H"], W=w["W"], K=w["K"], min_sep=4), None, None, None
    if w["psf"]:
        obs_psfs = np.array([synth.gaussian_psf((41, 41), 1.2 + 0.15 * b) for b in range(w["B"])])
        model_psf = synth.gaussian_psf((41, 41), 0.9)
        diff = pgm.match_psfs(obs_psfs.astype(np.float32), model_psf[None].astype(np.float32)).astype(np.float32)
        scale = (model_psf.max() / obs_psfs.max(axis=(1, 2))).astype(np.float32)
        kw["psfs"], cw = obs_psfs, model_psf.astype(np.float32)
    made = [synth.make_scene(9900 + i, **kw) for i in range(w["distinct"])]
    t = np.arange(w["S"]) % w["distinct"]
    b = BlendBatch(np.stack([made[i]["images"] for i in t]), np.stack([made[i]["centers"] for i in t]), centroid_weight=cw,
                   mse_capacity=64)
    if diff is not None:
        b.set_diff_kernel(diff)
    b.init_extended(np.ones(w["B"]) * 0.1, sed_scale=scale)
    b.fit(5, e_rel=0, check_every=0)
    return b, diff


def timed(fn, inner, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def run(name, w, inner, warmup, repeats):
    import torch
    from scarlet_amd.psfconv import convolve_same
    b, diff = make_batch(w)
    S, K, B, H, W = b.S, b.K, b.B, b.H, b.W
    kernel = None if diff is None else torch.as_tensor(diff).cuda()
    wants = dict(model=True, rendered=False, residual=True, loss=True, flux=True)
    out = b.products(**wants)

    def products():
        b.products(out=out, **wants)

    def torch_products(sed=None, morph=None):
        sed = b.sed_current if sed is None else sed
        morph = b.morph_current if morph is None else morph
        model = torch.einsum("skb,skhw->sbhw", sed, morph)
        rendered = model
        if kernel is not None:      # band by band: the S planes of a band share one kernel
            planes = model.permute(1, 0, 2, 3).contiguous()
            rendered = torch.stack([convolve_same(planes[i], kernel[i:i + 1]) for i in range(B)], dim=1)
        residual = b.images - rendered
        d = residual if b.weights is None else b.weights * residual
        loss = 0.5 * (d.double() ** 2).sum(dim=(2, 3)) * b.weight_scalar ** 2
        flux = morph.sum(dim=(2, 3), dtype=torch.float64)[:, :, None] * sed.double()
        return model, residual, loss, flux

    sed, morph = b.sed_current.contiguous(), b.morph_current.contiguous()
    ref = torch_products(sed, morph)
    agree = {n: float(((getattr(out, n) - r).abs().amax() / r.abs().amax()).item())
             for n, r in zip(("model", "residual", "loss", "flux"), ref)}

    def fit_iteration():
        b.fit(1, e_rel=0, check_every=0)

    legs = dict(products_ms=products, torch_ms=lambda: torch_products(sed, morph),
                torch_with_gather_ms=torch_products)
    times = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            times[k].append(timed(fn, inner, warmup))
    b._ensure_mse_capacity(repeats * (inner + warmup) + 1)
    times["fit_iteration_ms"] = [timed(fit_iteration, inner, warmup) for _ in range(repeats)]
    r = dict(workload="%s: %d x %d x %d x %d, K=%d%s" % (name, S, B, H, W, K, ", PSF 41^2" if w["psf"] else ""), name=name)
    for k, v in times.items():
        r[k] = float(np.median(v))
        r[k.replace("_ms", "_min_max_ms")] = [float(min(v)), float(max(v))]
    nbytes = 4.0 * S * H * W * (K + B + 2 * B)
    r.update(algorithmic_bytes=nbytes, hbm_fraction=nbytes / (r["products_ms"] * 1e-3) / HBM_PEAK,
             products_over_torch=r["products_ms"] / r["torch_ms"], products_over_fit_iteration=r["products_ms"] / r["fit_iteration_ms"],
             max_rel_difference_from_torch=agree, inner=inner, warmup=warmup, repeats=repeats,
             device=torch.cuda.get_device_name())
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--workloads", default="headline,config3,config5")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = []
    for name in args.workloads.split(","):
        r = run(name, WORKLOADS[name], args.inner, args.warmup, args.repeats)
        print(json.dumps(r), flush=True)
        res.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
