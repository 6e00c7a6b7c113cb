"""Joint fits over more than 8 model channels (BlendBatch.from_observations(..., wide=True),
scarlet_fit_observations_wide): ms per iteration, ms per iteration per channel plane and algorithmic bytes per
iteration, beside the 8-channel joint fit of the same scenes (which runs the kernels of multiobs.h).

  C8    two instruments of 4 + 4 bands                 (the yardstick: k_obs_contract)
  C17   three instruments of 6 + 4 + 7 bands           (LSST ugrizy + Euclid VIS/Y/J/H + Roman)
  C32   four instruments of 8 bands each

Frames are 64 x 64, K = 4 and K = 30, the first instrument carries a PSF (a 15 x 15 difference kernel).  Every layout is
timed `--repeats` times, the layouts alternating, and the median is reported with the spread; a window is `--iters`
iterations after `--warmup`, ending in a device synchronise.  Writes profiles/wide_channels_bench.json (`--out`) and prints
one JSON line per (layout, K).  `--no-psf` leaves the PSF out: the contraction and its Gram / eigenvalue passes alone."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.environ.get("SCARLET_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAYOUTS = {"C8": (4, 4), "C17": (6, 4, 7), "C32": (8, 8, 8, 8)}
SCENES = {4: 1024, 30: 256}
SIDE = 64
HBM_GBPS = 8000.0           # MI355X peak HBM3E bandwidth, GB/s


def data(widths, S, K, psf):
    rng = np.random.default_rng(0)
    C = sum(widths)
    yy, xx = np.mgrid[:SIDE, :SIDE]
    cen = rng.integers(8, SIDE - 8, size=(S, K, 2)).astype(np.int32)
    sed = rng.uniform(0.5, 2.0, size=(S, K, C)).astype(np.float32)
    morph = np.zeros((S, K, SIDE, SIDE), np.float32)
    for k in range(K):
        morph[:, k] = np.exp(-((yy[None] - cen[:, k, 0, None, None]) ** 2 + (xx[None] - cen[:, k, 1, None, None]) ** 2) / 8.0)
    img = np.einsum("skc,skyx->scyx", sed, morph).astype(np.float32)
    img += 0.05 * rng.standard_normal(img.shape).astype(np.float32)
    obs, at = [], 0
    for w in widths:
        obs.append((np.ascontiguousarray(img[:, at:at + w]), at))
        at += w
    diff = None
    if psf:
        g = np.exp(-((yy[:15, :15] - 7) ** 2 + (xx[:15, :15] - 7) ** 2) / 2.0).astype(np.float32)
        diff = np.stack([g / g.sum()] * widths[0])
    return obs, diff, cen, np.ones((S, K, C), np.float32), morph


def algorithmic_bytes(widths, S, K, psf):
    """HBM bytes one iteration must move at least (float32): the images of every observation, the morphologies read
    twice and written once, and for the instrument with a PSF its model planes and G planes written and read once"""
    HW = SIDE * SIDE
    per = (sum(widths) + 3 * K) * HW * 4
    if psf:
        per += 3 * widths[0] * HW * 4 * 2
    return S * per


def build(widths, K, psf, iters, warmup, repeats):
    from scarlet_amd.batch import BlendBatch, ObservationBatch
    S = SCENES[K]
    obs, diff, cen, sed0, morph = data(widths, S, K, psf)
    ol = []
    for i, (im, b0) in enumerate(obs):
        o = ObservationBatch(im, band0=b0)
        if diff is not None and i == 0:
            o.set_diff_kernel(diff)
        ol.append(o)
    b = BlendBatch.from_observations(ol, cen, wide=sum(widths) > 8, mse_capacity=(iters + warmup) * (repeats + 1) + 2)
    b.set_state(sed0, morph)
    return b


def window(b, iters):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    b.fit(iters, e_rel=0, check_every=0)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layouts", default="C8,C17,C32")
    ap.add_argument("--components", default="4,30")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-psf", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_channels_bench.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_wide_channels needs a GPU"
    rows = []
    for K in (int(k) for k in a.components.split(",")):
        names = a.layouts.split(",")
        batches = {n: build(LAYOUTS[n], K, not a.no_psf, a.iters, a.warmup, a.repeats) for n in names}
        for n in names:
            batches[n].fit(a.warmup, e_rel=0, check_every=0)
        times = {n: [] for n in names}
        for _ in range(a.repeats):                       # the layouts alternate
            for n in names:
                times[n].append(window(batches[n], a.iters))
        base = None
        for n in names:
            widths, S = LAYOUTS[n], SCENES[K]
            C = sum(widths)
            ms = float(np.median(times[n]))
            nbytes = algorithmic_bytes(widths, S, K, not a.no_psf)
            row = dict(layout=n, channels=C, widths=list(widths), K=K, scenes=S, side=SIDE, psf=not a.no_psf,
                       ms_per_iter=round(ms, 4), ms_min=round(min(times[n]), 4), ms_max=round(max(times[n]), 4),
                       us_per_iter_per_plane=round(ms * 1e3 / (S * C), 4), algorithmic_bytes_per_iter=nbytes,
                       algorithmic_GBps=round(nbytes / (ms * 1e-3) / 1e9, 1),
                       share_of_hbm_peak=round(nbytes / (ms * 1e-3) / 1e9 / HBM_GBPS, 4))
            if n == "C8":
                base = row["us_per_iter_per_plane"]
            if base:
                row["per_plane_ratio_to_C8"] = round(row["us_per_iter_per_plane"] / base, 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/bench_wide_channels.py", iters=a.iters, warmup=a.warmup, repeats=a.repeats, rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
