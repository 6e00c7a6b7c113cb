#!/usr/bin/env python
"""Generate tests/golden/lowres_large.npz: what the reference's LowResObservation computes at model frames past the LDS
limit of the low-resolution kernels (tests/lowres_large_common.LARGE; the other low-resolution fixtures and their
generators stay as they are).  Runs where the reference package exists; the result is data only.

    python tools/gen_lowres_large_golden.py [--no-fit]     # rewrites tests/golden/lowres_large.npz

Per square geometry p (96 x 96), q (104 x 104), r (256 x 256), with the keys of lowres_limits.npz: the seeded inputs, the
reference's `_fft_shape` and `shifts`, `_render` of one model and `get_loss`.  p and q carry a random 2-band model, r one
band of a smooth model (the file stays below the largest fixture).  Geometry n (100 x 90 with 30 x 27) is not square:
the file records the reference's error message.  At p also the 5-iteration joint fit of tools/gen_lowres_golden.py
(`_fit_*`), whose dense adjoint takes 2 x 9216 renders of the reference: --no-fit leaves it out.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import refshim                      # noqa: E402
import lowres_common as lc                      # noqa: E402
import lowres_large_common as ll                # noqa: E402
import gen_lowres_golden as base                # noqa: E402

SEEDS = {"p": 21, "q": 22, "r": 23, "n": 24}
BANDS = {"p": 2, "q": 2, "r": 1, "n": 2}
FIT_CENTERS = ((36, 39), (60, 54))


def inputs(name, with_model):
    (H, W), (h, w), ratio, origin, psf_px, _ = ll.LARGE[name]
    B = BANDS[name]
    rng = np.random.default_rng(SEEDS[name])
    d = dict(model_shape=np.array([H, W]), lr_shape=np.array([h, w]), ratio=np.float64(ratio), origin=np.array(origin, dtype=np.float64))
    d["model_psf"], d["lr_psfs"] = lc.limit_psfs(psf_px, B)
    d["hr_psfs"] = np.array([lc.gauss(psf_px[0], 1.1 + 0.1 * b) for b in range(3)]).astype(np.float32)
    if with_model and name == "r":
        blobs = [base.blob((H, W), rng.uniform(30, H - 30), rng.uniform(30, W - 30), rng.uniform(3, 9), rng.uniform(3, 9))
                 for _ in range(12)]
        d["models"] = np.sum(blobs, axis=0)[None, None].astype(np.float32)
    elif with_model:
        d["models"] = rng.random((1, B, H, W)).astype(np.float32)
    d["images_lr"] = rng.standard_normal((B, h, w)).astype(np.float32)
    if with_model:
        d["weights_lr"] = (0.5 + rng.random((B, h, w))).astype(np.float32)
    return d


def main():
    ref = refshim.load_reference()
    out = {}
    for name in ("p", "q", "r", "n"):
        runs = name in ll.SQUARE
        d = inputs(name, runs)
        for k, v in d.items():
            out[name + "_" + k] = v
        (H, W), (h, w), ratio, origin = ll.LARGE[name][:4]
        wm, wl = lc.wcs_pair((H, W), (h, w), ratio, origin)
        ch = ["r", "i"][:BANDS[name]]
        frame = ref.Frame((len(ch), H, W), wcs=wm, psfs=d["model_psf"].copy(), channels=ch)
        obs = ref.LowResObservation(d["images_lr"].copy(), wcs=wl, psfs=d["lr_psfs"].copy(),
                                    weights=d["weights_lr"].copy() if runs else None, channels=ch)
        if not runs:
            try:
                obs.match(frame)
                raise SystemExit("the reference matched geometry %s: record its outputs instead of its error" % name)
            except ValueError as e:
                out[name + "_reference_error"] = np.array("%s: %s" % (type(e).__name__, e))
            continue
        obs.match(frame)
        out[name + "_fft_shape"] = np.array(obs._fft_shape)
        out[name + "_shifts"] = np.array(obs.shifts, dtype=np.float64)
        out[name + "_renders"] = np.array([obs._render(m) for m in d["models"]], dtype=np.float32)
        out[name + "_losses"] = np.array([obs.get_loss(m) for m in d["models"]], dtype=np.float64)
        print(name, "rendered", flush=True)
    if "--no-fit" not in sys.argv:
        # the joint fit of gen_lowres_golden.reference_run at p (it renders p's model again: the same values)
        base.GEOMETRIES["p"] = ll.LARGE["p"][:4]
        base.CENTERS = FIT_CENTERS
        d = {k[2:]: v for k, v in out.items() if k.startswith("p_")}
        base.reference_run(ref, "p", d, out)
    path = os.path.join(ROOT, "tests", "golden", "lowres_large.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    print("n", out["n_reference_error"])


if __name__ == "__main__":
    main()
