"""Joint fits against several observations: ms per iteration and algorithmic bytes per iteration of
scarlet_fit_observations, the configs of DESIGN.md "Several observations":

  O1  4096 scenes x (3 + 2 bands) x 64 x 64, K = 4
  O2  1024 scenes x (5 + 5 bands, two epochs, a 41 x 41 PSF kernel each) x 128 x 128, K = 8
  O3  64 scenes x (6 + 2 bands) x 256 x 256, K = 30, L0 sparsity, per-pixel weights

`--legacy` times scarlet_fit_multi through plain BlendBatch objects instead (what a build without
from_observations offers); `--floor` times scarlet_fit on the same scenes as ONE C-channel observation with the
NO_FUSED switch (a like-for-like floor: one gradient pass over the same data).  One JSON line per config."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.environ.get("SCARLET_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {
    "O1": dict(S=4096, bands=(3, 2), epochs=False, side=64, K=4, psf=False, l0=None, weights=False),
    "O2": dict(S=1024, bands=(5, 5), epochs=True, side=128, K=8, psf=True, l0=None, weights=False),
    "O3": dict(S=64, bands=(6, 2), epochs=False, side=256, K=30, psf=False, l0=0.02, weights=True),
}


def data(cfg):
    rng = np.random.default_rng(0)
    S, side, K = cfg["S"], cfg["side"], cfg["K"]
    B = cfg["bands"][0] if cfg["epochs"] else sum(cfg["bands"])
    yy, xx = np.mgrid[:side, :side]
    cen = rng.integers(8, side - 8, size=(S, K, 2)).astype(np.int32)
    sed = rng.uniform(0.5, 2.0, size=(S, K, B)).astype(np.float32)
    img = np.zeros((S, B, side, side), np.float32)
    for k in range(K):
        prof = np.exp(-((yy[None] - cen[:, k, 0, None, None]) ** 2 + (xx[None] - cen[:, k, 1, None, None]) ** 2) / 8.0)
        img += sed[:, k, :, None, None] * prof[:, None].astype(np.float32)
    img += 0.05 * rng.standard_normal(img.shape).astype(np.float32)
    obs, b0 = [], 0
    for i, nb in enumerate(cfg["bands"]):
        if cfg["epochs"]:
            im = img if i == 0 else (img + 0.05 * rng.standard_normal(img.shape)).astype(np.float32)
            obs.append((im, 0))
        else:
            obs.append((np.ascontiguousarray(img[:, b0:b0 + nb]), b0))
            b0 += nb
    w = [None if not cfg["weights"] else (0.5 + rng.random(o[0].shape)).astype(np.float32) for o in obs]
    diff = None
    if cfg["psf"]:
        g = np.exp(-((yy[:41, :41] - 20) ** 2 + (xx[:41, :41] - 20) ** 2) / 2.0).astype(np.float32)
        diff = np.stack([g / g.sum()] * cfg["bands"][0])
    C = max(o[1] + o[0].shape[1] for o in obs)
    morph = np.zeros((S, K, side, side), np.float32)
    for k in range(K):
        morph[:, k] = np.exp(-((yy[None] - cen[:, k, 0, None, None]) ** 2 + (xx[None] - cen[:, k, 1, None, None]) ** 2) / 8.0)
    sed0 = np.ones((S, K, C), np.float32)
    return obs, w, diff, cen, sed0, morph


def algorithmic_bytes(cfg, C, mode):
    """HBM bytes one iteration must move at least (float32): per scene the images and weights of every observation,
    the morphologies read twice and written once (the second read is the step's), the SEDs; with a PSF the model
    planes and the G planes of the convolution (written and read once each); the floor reads its C-channel cube once."""
    S, HW, K = cfg["S"], cfg["side"] ** 2, cfg["K"]
    nb = sum(cfg["bands"])
    per = (nb * (2 if cfg["weights"] else 1) + 3 * K) * HW * 4
    if cfg["psf"]:
        per += 3 * cfg["bands"][0] * HW * 4 * 2
    if mode == "floor":
        per = (C * (2 if cfg["weights"] else 1) + 3 * K) * HW * 4
    return S * per


def run(name, cfg, mode, iters, warmup):
    import torch
    from scarlet_amd import _lib
    from scarlet_amd.batch import BlendBatch
    obs, w, diff, cen, sed0, morph = data(cfg)
    C = max(o[1] + o[0].shape[1] for o in obs)
    S = cfg["S"]
    kw = dict(l0_thresh=cfg["l0"], mse_capacity=iters + warmup + 2)
    if mode == "floor":
        B = C
        img = np.zeros((S, C) + obs[0][0].shape[2:], np.float32)
        for (im, b0) in obs:
            img[:, b0:b0 + im.shape[1]] += im
        b = BlendBatch(img, cen, weights=None if w[0] is None else np.concatenate(w, axis=1)[:, :C], **kw)
        if diff is not None:
            b.set_diff_kernel(np.concatenate([diff] * (C // diff.shape[0] + 1))[:C])
        fit = lambda n: b.fit(n, e_rel=0, check_every=0)
        _lib.set_option("NO_FUSED", 1)
    elif mode == "legacy":
        state = BlendBatch(np.zeros((S, C) + obs[0][0].shape[2:], np.float32), cen, **kw)
        obs_b = []
        for (im, b0), ww in zip(obs, w):
            ob = BlendBatch(im, cen, weights=ww, symmetric=False, monotonic=False)
            if diff is not None:
                ob.set_diff_kernel(diff)
            obs_b.append((ob, b0))
        b = state
        ptrs = (ctypes.POINTER(_lib.ScarletBatch) * len(obs_b))(*[ctypes.pointer(ob._c) for ob, _ in obs_b])
        band0 = np.array([b0 for _, b0 in obs_b], np.int32)

        def fit(n):
            state._ensure_mse_capacity(n)
            return _lib.check(_lib.lib.scarlet_fit_multi(ctypes.byref(state._c), ptrs, band0.ctypes.data_as(ctypes.c_void_p),
                                                         len(obs_b), n, 0.0, 0, 0, _lib.stream_ptr()))
    else:
        from scarlet_amd.batch import ObservationBatch
        ol = []
        for (im, b0), ww in zip(obs, w):
            o = ObservationBatch(im, band0=b0, weights=ww)
            if diff is not None:
                o.set_diff_kernel(diff)
            ol.append(o)
        b = BlendBatch.from_observations(ol, cen, **kw)
        fit = lambda n: b.fit(n, e_rel=0, check_every=0)
    b.set_state(sed0, morph)
    fit(warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fit(iters)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / iters
    nbytes = algorithmic_bytes(cfg, C, mode)
    if mode == "floor":
        _lib.set_option("NO_FUSED", 0)
    return dict(config=name, mode=mode, scenes=S, ms_per_iter=round(ms, 4), algorithmic_bytes_per_iter=nbytes,
                algorithmic_GBps=round(nbytes / (ms * 1e-3) / 1e9, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="O1,O2,O3")
    ap.add_argument("--mode", default="observations", choices=["observations", "legacy", "floor"])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    for name in a.configs.split(","):
        print(json.dumps(run(name, CONFIGS[name], a.mode, a.iters, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
