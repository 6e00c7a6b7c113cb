#!/usr/bin/env python
"""Times of the streamed form of the low-resolution operator (csrc/lowres_stream.h), pixel ratio 5 throughout:

    fit_256        ms per iteration of a joint fit: 5 x 256 x 256 model channels, a same-grid 3-band observation and a
                   2 x 48 x 48 low-resolution one (--scenes scenes of 4 sources)
    planes_512     render and adjoint of --planes planes of 512 x 512 (96 x 96 observation)
    planes_1024    one render and one adjoint of 4 planes of 1024 x 1024 (192 x 192 observation)
    geometry_d     64 x 64 at B = 8 (32 x 32 observation, ratio 2), 256 planes: the streamed form forced (LOWRES_STREAMED)
                   against the LDS-resident form

Every plane-operator entry carries the float32 operations of its GEMM chain and the rate they were done at, beside the
155 TFLOP/s a gfx950 device offers v_mfma_f32_16x16x4_f32.  Times are device events after a warm-up, best of
--repeats; the JSON goes to profiles/lowres_large_bench.json (or --out).

    python tools/bench_lowres_large.py [--scenes 16] [--planes 16] [--steps 10] [--repeats 3] [--only NAME] [--out PATH]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_TFLOPS = 155.0


def geometry(side, lr_side, ratio, B, C=None, band0=0):
    import scarlet_amd as scarlet
    from scarlet_amd import synth
    from scarlet_amd.resampling import AffineWCS
    ch = ["c%d" % c for c in range(band0 + B if C is None else C)]
    mine = ch[band0:band0 + B] if len(ch) != B else ch
    model_psf = synth.gaussian_psf((15, 15), 0.9)[None].astype(np.float32)
    lr_psfs = np.array([synth.gaussian_psf((9, 9), 0.9 + 0.1 * b) for b in range(B)]).astype(np.float32)
    frame = scarlet.Frame((len(ch), side, side), wcs=AffineWCS((side, side), 1.0), psfs=model_psf, channels=ch)
    org = (side - lr_side * ratio) / 2.0
    wl = AffineWCS((lr_side, lr_side), ratio, crpix=(1 - org / ratio, 1 - org / ratio))
    return scarlet.LowResObservation(np.zeros((B, lr_side, lr_side), np.float32), wcs=wl, psfs=lr_psfs, channels=mine).match(frame)


def chain_flops(H, W, h, w, nfy, nfx):
    """float32 operations (2 per multiply-add) of the four GEMMs of a render; the adjoint's four have the same sizes"""
    return 2.0 * (H * 2 * nfx * W + 2 * nfy * 2 * nfx * H + 2 * nfy * w * 2 * nfx + h * w * 2 * nfy)


def time_planes(geo, n, repeats, large=True):
    import torch
    import scarlet_amd as scarlet
    from scarlet_amd import _lib
    (H, W), (B, h, w) = geo.model_shape, geo.frame.shape
    lr, keep = scarlet.LowResObservationBatch(np.zeros((1, B, h, w), np.float32), geometry=geo).lowres_struct("cuda")
    x = torch.rand((n, H, W), device="cuda")
    y = torch.randn((n, h, w), device="cuda")
    band = (torch.arange(n, device="cuda") % B).to(torch.int32)
    Tx, Ty = torch.empty_like(y), torch.empty_like(x)
    nbytes = int(_lib.check(_lib.lib.scarlet_lowres_op_scratch_bytes(n, H, W, ctypes.byref(lr)))) if large else 0
    scratch = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device="cuda")

    def run(adjoint):
        if large:
            fn = _lib.lib.scarlet_lowres_adjoint_large if adjoint else _lib.lib.scarlet_lowres_render_large
            _lib.check(fn((y if adjoint else x).data_ptr(), n, H, W, ctypes.byref(lr), band.data_ptr(), None,
                          (Ty if adjoint else Tx).data_ptr(), scratch.data_ptr(), nbytes, _lib.stream_ptr()))
        else:
            fn = _lib.lib.scarlet_lowres_adjoint if adjoint else _lib.lib.scarlet_lowres_render
            _lib.check(fn((y if adjoint else x).data_ptr(), n, H, W, ctypes.byref(lr), band.data_ptr(), None,
                          (Ty if adjoint else Tx).data_ptr(), _lib.stream_ptr()))
    out = {}
    f = geo.factors
    flops = n * chain_flops(H, W, h, w, f["uy"].shape[0], f["ux"].shape[0])
    for adjoint, what in ((False, "render"), (True, "adjoint")):
        run(adjoint)
        best = None
        for _ in range(repeats):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            run(adjoint)
            t1.record()
            torch.cuda.synchronize()
            best = t0.elapsed_time(t1) if best is None else min(best, t0.elapsed_time(t1))
        out[what + "_ms"] = best
        out[what + "_tflops"] = flops / (best * 1e-3) / 1e12
    out.update(planes=n, H=H, W=W, h=h, w=w, nfy=int(f["uy"].shape[0]), nfx=int(f["ux"].shape[0]), gemm_gflop=flops / 1e9,
               scratch_mib=nbytes / 2.0 ** 20, peak_tflops=PEAK_TFLOPS)
    return out


def fit_256(args):
    import torch
    import scarlet_amd as scarlet
    from scarlet_amd import synth
    S, C, side, K = args.scenes, 5, 256, 4
    d = synth.make_batch(9100, min(4, S), B=C, H=side, W=side, K=K)
    reps = -(-S // len(d["images"]))
    images, centers = np.tile(d["images"], (reps, 1, 1, 1))[:S], np.tile(d["centers"], (reps, 1, 1))[:S]
    geo = geometry(side, 48, 5.0, 2, C=C, band0=3)
    model = torch.as_tensor(images[:, 3:]).cuda()
    coarse = torch.stack([geo.render(torch.nn.functional.pad(m, (0, 0, 0, 0, 3, 0))) for m in model]).cpu().numpy()
    b = scarlet.BlendBatch(images, centers).init_extended(np.ones(C, np.float32) * 0.1)
    sed0, morph0 = b.sed_current.clone(), b.morph_current.clone()
    del b
    b = scarlet.BlendBatch.from_observations([scarlet.ObservationBatch(images[:, :3], band0=0),
                                              scarlet.LowResObservationBatch(coarse, band0=3, geometry=geo)], centers)
    b.set_state(sed0, morph0)
    b.fit(2, e_rel=0, check_every=0)
    best = None
    for _ in range(args.repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        b.fit(args.steps, e_rel=0, check_every=0)
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / args.steps
        best = ms if best is None else min(best, ms)
    b.raise_on_status()
    return dict(ms_per_iteration=best, scenes=S, channels=C, H=side, W=side, sources=K, lowres_bands=2, h=48, w=48, steps=args.steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=16)
    ap.add_argument("--planes", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lowres_large_bench.json"))
    args = ap.parse_args()
    import torch
    from scarlet_amd import _lib
    res = {}
    want = lambda name: args.only in (None, name)
    if want("fit_256"):
        res["fit_256"] = fit_256(args)
    if want("planes_512"):
        res["planes_512"] = time_planes(geometry(512, 96, 5.0, 2), args.planes, args.repeats)
    if want("planes_1024"):
        res["planes_1024"] = time_planes(geometry(1024, 192, 5.0, 2), 4, 1)
    if want("geometry_d"):
        geo = geometry(64, 32, 2.0, 8)
        res["geometry_d"] = dict(lds=time_planes(geo, 256, args.repeats, large=False))
        old = _lib.set_option("LOWRES_STREAMED", 1)
        try:
            res["geometry_d"]["streamed"] = time_planes(geo, 256, args.repeats)
        finally:
            _lib.set_option("LOWRES_STREAMED", old)
    res["config"] = dict(repeats=args.repeats, device=torch.cuda.get_device_name())
    print(json.dumps(res))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
