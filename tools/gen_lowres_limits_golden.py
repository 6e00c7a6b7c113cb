#!/usr/bin/env python
"""Generate tests/golden/lowres_limits.npz: what the reference's LowResObservation computes at the geometries where the
low-resolution kernels reach their LDS limits (tests/lowres_common.LIMITS; tests/golden/lowres.npz and its generator
tools/gen_lowres_golden.py stay as they are).  Runs where the reference package exists; the result is data only.

    python tools/gen_lowres_limits_golden.py     # rewrites tests/golden/lowres_limits.npz

Per geometry d, e, f: the seeded inputs (PSFs, one random 2-band model, images, weights), the reference's `_fft_shape`
and `shifts`, `_render` of the model and `get_loss`.  Geometries g and h pad to a plane that is not square (75 x 80,
45 x 48: the last axis of a real transform is made even), which the reference cannot match: the file records their
inputs and the reference's error message, as lowres.npz does for geometry c.  Geometries i and j have non-square frames,
the case c already records; they need nothing from the reference.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import refshim                      # noqa: E402
import lowres_common as lc                      # noqa: E402

SEEDS = {"d": 14, "e": 15, "f": 16, "g": 17, "h": 18}
CH2 = ["r", "i"]


def inputs(name, with_model):
    (H, W), (h, w), ratio, origin, psf_px, _ = lc.LIMITS[name]
    rng = np.random.default_rng(SEEDS[name])
    d = dict(model_shape=np.array([H, W]), lr_shape=np.array([h, w]), ratio=np.float64(ratio), origin=np.array(origin, dtype=np.float64))
    d["model_psf"], d["lr_psfs"] = lc.limit_psfs(psf_px, 2)
    if with_model:
        d["models"] = rng.random((1, 2, H, W)).astype(np.float32)
    d["images_lr"] = rng.standard_normal((2, h, w)).astype(np.float32)
    if with_model:
        d["weights_lr"] = (0.5 + rng.random((2, h, w))).astype(np.float32)
    return d


def main():
    ref = refshim.load_reference()
    out = {}
    for name in ("d", "e", "f", "g", "h"):
        runs = name in "def"
        d = inputs(name, runs)
        for k, v in d.items():
            out[name + "_" + k] = v
        (H, W), (h, w), ratio, origin = lc.LIMITS[name][:4]
        wm, wl = lc.wcs_pair((H, W), (h, w), ratio, origin)
        frame = ref.Frame((2, H, W), wcs=wm, psfs=d["model_psf"].copy(), channels=CH2)
        obs = ref.LowResObservation(d["images_lr"].copy(), wcs=wl, psfs=d["lr_psfs"].copy(),
                                    weights=d["weights_lr"].copy() if runs else None, channels=CH2)
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
    path = os.path.join(ROOT, "tests", "golden", "lowres_limits.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    for name in "gh":
        print(name, out[name + "_reference_error"])


if __name__ == "__main__":
    main()
