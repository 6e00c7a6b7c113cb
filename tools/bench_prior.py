"""Fits with per-component priors: ms per iteration of scarlet_fit_prior against its floor, the configs of DESIGN.md
"Priors":

  P1  10 000 scenes x 5 x 64 x 64, K = 4 (the headline shape)
  P2  4096 scenes x 5 x 128 x 128, K = 8, a 41 x 41 PSF kernel
  P3  64 scenes x 6 x 256 x 256, K = 30, L0 sparsity

Quadratic priors with targets on both factors of every component, e_rel = 0, every scene active.  Legs, alternated in
one process and repeated (`--repeats`), timed with device events around enough iterations for `--min-ms` of work:

  a  scarlet_fit_prior
  b  the floor: scarlet_fit on the same batch with NO_FUSED and NO_PIPELINE -- the same gradient pass with the step
     folded in, the same constraints, one stream
  c  scarlet_fit as shipped (context only: P1 runs the fused persistent kernel there)
  d  the same prior as a callable evaluated with torch once per iteration
  z  (on request) scarlet_fit_prior with every weight zero: the prior path on the floor's own trajectory, which
     separates the cost of the path from what the prior does to the data the constraint kernels work on

and a device-to-device copy whose bytes read plus bytes written equal the algorithmic bytes of k_prior_step
(`prior_step_bytes`), the yardstick for the kernel's own time (taken from a kernel trace of a run of leg a alone).

`--legacy` is the only way a build without this feature fits with a prior: 64 scenes of P1's shape as 64 single-scene
Blend objects with scarlet.Prior, 20 iterations each.  It uses nothing newer than Blend / ExtendedSource / Prior, so it
runs on an older tree too (SCARLET_TREE=<its root>).  One JSON line per config."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.environ.get("SCARLET_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {
    "P1": dict(S=10000, B=5, side=64, K=4, psf=False, l0=None),
    "P2": dict(S=4096, B=5, side=128, K=8, psf=True, l0=None),
    "P3": dict(S=64, B=6, side=256, K=30, psf=False, l0=0.05),
    "P1_64": dict(S=64, B=5, side=64, K=4, psf=False, l0=None),      # the scenes of the --legacy leg
}
W_SED, W_MORPH = 20.0, 2000.0


def data(cfg, torch, device):
    """synthetic scenes made on the device: K circular Gaussians per scene, noise 0.05"""
    g = torch.Generator(device=device)
    g.manual_seed(0)
    S, B, side, K = cfg["S"], cfg["B"], cfg["side"], cfg["K"]
    cen = torch.randint(8, side - 8, (S, K, 2), generator=g, device=device, dtype=torch.int32)
    sed = torch.rand((S, K, B), generator=g, device=device) * 1.5 + 0.5
    yy = torch.arange(side, device=device, dtype=torch.float32).view(1, side, 1)
    xx = torch.arange(side, device=device, dtype=torch.float32).view(1, 1, side)
    morph = torch.empty((S, K, side, side), device=device)
    img = torch.zeros((S, B, side, side), device=device)
    for k in range(K):
        cy, cx = cen[:, k, 0].float().view(S, 1, 1), cen[:, k, 1].float().view(S, 1, 1)
        morph[:, k] = torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / 8.0)
        img += sed[:, k, :, None, None] * morph[:, k, None]
    img += 0.05 * torch.randn(img.shape, generator=g, device=device)
    diff = None
    if cfg["psf"]:
        y, x = np.mgrid[:41, :41]
        k = np.exp(-((y - 20) ** 2 + (x - 20) ** 2) / 2.0).astype(np.float32)
        diff = np.stack([k / k.sum()] * B)
    return img, cen, torch.ones((S, K, B), device=device), morph, diff


def prior_step_bytes(cfg):
    """HBM bytes k_prior_step must move per iteration (float32): per component plane x, g and the target read and the
    stepped value written; the same per SED; per component two weights read and two float64 constants written; per
    scene the two float64 constants, cur and active read"""
    S, K, B, HW = cfg["S"], cfg["K"], cfg["B"], cfg["side"] ** 2
    return S * (K * (4 * HW * 4 + 4 * B * 4 + 2 * 4 + 2 * 8) + 2 * 8 + 2 * 4)


def run(name, cfg, legs, repeats, min_ms):
    import torch
    import scarlet_amd as scarlet
    from scarlet_amd import _lib
    dev = torch.device("cuda", torch.cuda.current_device())
    img, cen, sed0, morph0, diff = data(cfg, torch, dev)
    b = scarlet.BlendBatch(img, cen.cpu().numpy(), l0_thresh=cfg["l0"], mse_capacity=16)
    if diff is not None:
        b.set_diff_kernel(diff)
    quad = scarlet.QuadraticPrior(sed_weight=W_SED, sed_target=sed0, morph_weight=W_MORPH, morph_target=morph0)
    ws = torch.full((cfg["S"], cfg["K"]), W_SED, device=dev)
    wm = torch.full((cfg["S"], cfg["K"]), W_MORPH, device=dev)

    def fn(sed, morph):
        return dict(grad_sed=ws[..., None] * (sed - sed0), grad_morph=wm[..., None, None] * (morph - morph0), L_sed=ws, L_morph=wm)

    zero = scarlet.QuadraticPrior(sed_weight=0.0, sed_target=sed0, morph_weight=0.0, morph_target=morph0)

    def fit(leg, n):
        if leg == "a":
            return b.fit(n, e_rel=0, check_every=0, prior=quad)
        if leg == "z":
            return b.fit(n, e_rel=0, check_every=0, prior=zero)
        if leg == "d":
            return b.fit(n, e_rel=0, check_every=0, prior=fn)
        if leg == "b":
            prev = [_lib.set_option(o, 1) for o in ("NO_FUSED", "NO_PIPELINE")]
            try:
                return b.fit(n, e_rel=0, check_every=0)
            finally:
                _lib.set_option("NO_FUSED", prev[0]); _lib.set_option("NO_PIPELINE", prev[1])
        return b.fit(n, e_rel=0, check_every=0)

    def timed(leg, n):
        b.set_state(sed0, morph0)
        b.it.zero_()
        b._ensure_mse_capacity(n)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fit(leg, n)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    out = dict(config=name, scenes=cfg["S"], pipelines_as_shipped=int(_lib.lib.scarlet_batch_pipelines(b._c)))
    iters = {}
    for leg in legs:                                    # warm-up and calibration: enough iterations for min_ms
        per = timed(leg, 3)
        iters[leg] = int(min(2000, max(5, np.ceil(min_ms / max(per, 1e-3)))))
    ms = {leg: [] for leg in legs}
    for _ in range(repeats):
        for leg in legs:
            ms[leg].append(timed(leg, iters[leg]))
    for leg in legs:
        out["ms_per_iter_" + leg] = [round(v, 4) for v in ms[leg]]
        out["iterations_" + leg] = iters[leg]
    # the library's own event recorder around every kernel class of legs a and b (scarlet_profile_begin / _end_ex):
    # ms per iteration by class, boundaries included, timed like the copy below
    names = ["k_grad", "k_step", "k_source_update", "k_converge", "k_iterate", "psf_convolution", "k_prior_step"]
    for leg in [x for x in legs if x in ("a", "b", "z")]:
        n = min(iters[leg], 50)
        b.set_state(sed0, morph0)
        b.it.zero_()
        _lib.check(_lib.lib.scarlet_profile_begin(n + 1))
        fit(leg, n)
        tot, its = (ctypes.c_double * 8)(), (ctypes.c_int64 * 8)()
        _lib.check(_lib.lib.scarlet_profile_end_ex(tot, its, None))
        out["class_ms_per_iter_" + leg] = {names[i]: round(tot[i] / n, 4) for i in range(len(names)) if its[i]}
    # the copy that moves as many bytes as k_prior_step
    nbytes = prior_step_bytes(cfg)
    src = torch.empty((nbytes // 8,), dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    reps = max(10, int(np.ceil(0.2 * min_ms / max(nbytes / 4e9, 1e-3))))
    copies = []
    for _ in range(repeats + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        copies.append(e0.elapsed_time(e1) / reps)
    out["prior_step_bytes"] = nbytes
    out["copy_same_bytes_ms"] = [round(v, 5) for v in copies[1:]]
    out["copy_GBps"] = round(nbytes / (np.median(copies[1:]) * 1e-3) / 1e9, 1)
    return out


def legacy(iters):
    """64 single-scene Blend objects with scarlet.Prior, one after the other (the Python pipeline)"""
    import time
    import torch
    import scarlet_amd as scarlet
    cfg = CONFIGS["P1_64"]
    dev = torch.device("cuda", torch.cuda.current_device())
    img, cen, _, _, _ = data(cfg, torch, dev)
    img, cen = img.cpu().numpy(), cen.cpu().numpy()
    bg = np.ones(cfg["B"]) * 0.1
    blends = []
    for s in range(cfg["S"]):
        frame = scarlet.Frame(img[s].shape)
        obs = scarlet.Observation(img[s]).match(frame)
        srcs = []
        for p in cen[s]:
            src = scarlet.ExtendedSource(frame, tuple(int(v) for v in p), obs, bg)
            sed0, morph0 = src.sed.clone(), src.morph.clone()
            grad = lambda sed, morph, sed0=sed0, morph0=morph0: (W_SED * (sed - sed0), W_MORPH * (morph - morph0))
            src.prior = scarlet.Prior(grad, lambda sed, morph: (W_SED, W_MORPH))
            srcs.append(src)
        blends.append(scarlet.Blend(srcs, obs))
    blends[0].fit(2, e_rel=0)                           # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for bl in blends[1:]:
        bl.fit(iters, e_rel=0)
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    n = len(blends) - 1
    return dict(config="legacy", scenes=n, iterations=iters, us_per_scene_iteration=round(sec * 1e6 / (n * iters), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="P1,P2,P3")
    ap.add_argument("--legs", default="a,b,c,d")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--min-ms", type=float, default=300.0)
    ap.add_argument("--legacy", action="store_true")
    ap.add_argument("--legacy-iters", type=int, default=20)
    a = ap.parse_args()
    if a.legacy:
        print(json.dumps(legacy(a.legacy_iters)), flush=True)
        return
    for name in a.configs.split(","):
        print(json.dumps(run(name, CONFIGS[name], a.legs.split(","), a.repeats, a.min_ms)), flush=True)


if __name__ == "__main__":
    main()
