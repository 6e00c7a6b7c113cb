"""Timing of the products of a LOW-RESOLUTION observation in one call (BlendBatch.products on a joint batch,
scarlet_observations_products_lowres) against the same quantities composed the way a caller had to compose them before:
get_model(), scarlet_lowres_render_large on the observation's channel slice, torch for residual and loss.  bench.py
measures the BASELINE configs and is left alone.

Workloads (a same-grid observation on channels 0-2, the low-resolution one on channels 3-4; scene s is one of a few
synthetic templates; the batch is fitted two iterations first):
  lds       the README's joint batch: 5 x 64 x 64 model frames, 2 x 32 x 32 images (k_lowres_products, factors in LDS)
  streamed  5 x 256 x 256 model frames, 2 x 128 x 128 images (the streamed chain of lowres_stream.h)
Per workload, timed with device events around `--inner` back-to-back calls after `--warmup` calls, `--repeats` times
(median, min and max are reported; the variants are interleaved so that they see the same machine):
  one_call_ms        products(model=False, flux=False, obs=[1]): rendered, residual and loss of the low-resolution
                     observation, into reused buffers
  one_call_model_ms  ... with model=True: the streamed form then reads the band models from the `model` output
  composed_ms        get_model(), the channel slice made contiguous, scarlet_lowres_render_large, images - rendered and
                     the float64 loss in torch
  composed_model_ms  get_model() alone (what the composed path spends before it renders)
The composed path on the same commit is the yardstick; no speed-up is fixed in advance.

    python tools/bench_lowres_products.py --out profiles/lowres_products_bench.json
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

WORKLOADS = {
    "lds": dict(S=1024, side=64, lr_side=32, ratio=2.0, K=4, distinct=4),
    "streamed": dict(S=64, side=256, lr_side=128, ratio=2.0, K=4, distinct=4),
}
C, BAND0, B = 5, 3, 2


def make_batch(w):
    import torch
    import scarlet_amd as scarlet
    from scarlet_amd import synth
    from bench_lowres_large import geometry
    S, side = w["S"], w["side"]
    d = synth.make_batch(9300, w["distinct"], B=C, H=side, W=side, K=w["K"])
    t = np.arange(S) % w["distinct"]
    images, centers = d["images"][t], d["centers"][t]
    geo = geometry(side, w["lr_side"], w["ratio"], B, C=C, band0=BAND0)
    fine = torch.as_tensor(d["images"][:, BAND0:]).cuda()
    coarse = torch.stack([geo.render(torch.nn.functional.pad(m, (0, 0, 0, 0, BAND0, 0))) for m in fine]).cpu().numpy()[t]
    weights = (0.5 + np.random.default_rng(1).random(coarse.shape)).astype(np.float32)
    b = scarlet.BlendBatch(images, centers).init_extended(np.ones(C, np.float32) * 0.1)
    sed0, morph0 = b.sed_current.clone(), b.morph_current.clone()
    del b
    b = scarlet.BlendBatch.from_observations([scarlet.ObservationBatch(images[:, :BAND0], band0=0),
                                              scarlet.LowResObservationBatch(coarse, band0=BAND0, geometry=geo, weights=weights)],
                                             centers, lowres_products=True)
    b.set_state(sed0, morph0)
    b.fit(2, e_rel=0, check_every=0)
    b.raise_on_status()
    return b, geo


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
    from scarlet_amd import _lib
    b, geo = make_batch(w)
    S, H, W = b.S, b.H, b.W
    o, ob = b._observations[1]
    lr = b._lowres[1][0]
    h, wd = o.shape[2:]
    n = S * B
    band = torch.arange(B, dtype=torch.int32, device="cuda").repeat(S)
    rendered = torch.empty((S, B, h, wd), dtype=torch.float32, device="cuda")
    op_bytes = int(_lib.check(_lib.lib.scarlet_lowres_op_scratch_bytes(n, H, W, ctypes.byref(lr))))
    op_scratch = torch.empty((max(op_bytes, 1),), dtype=torch.uint8, device="cuda")
    wants = dict(rendered=True, residual=True, loss=True, flux=False, obs=[1])
    out = b.products(model=False, **wants)
    out_m = b.products(model=True, **wants)

    def one_call():
        b.products(model=False, out=out, **wants)

    def one_call_model():
        b.products(model=True, out=out_m, **wants)

    def composed():
        planes = b.get_model()[:, BAND0:BAND0 + B].contiguous()
        _lib.check(_lib.lib.scarlet_lowres_render_large(planes.data_ptr(), n, H, W, ctypes.byref(lr), band.data_ptr(), None,
                                                        rendered.data_ptr(), op_scratch.data_ptr(), op_bytes, _lib.stream_ptr()))
        residual = ob.images - rendered
        loss = 0.5 * ((ob.weights * residual).double() ** 2).sum(dim=(2, 3))
        return rendered, residual, loss

    ref = composed()
    agree = {k: float(((getattr(out, k)[1] - r).abs().amax() / r.abs().amax()).item())
             for k, r in zip(("rendered", "residual", "loss"), ref)}
    legs = dict(one_call_ms=one_call, one_call_model_ms=one_call_model, composed_ms=composed, composed_model_ms=b.get_model)
    times = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            times[k].append(timed(fn, inner, warmup))
    f = geo.factors
    need = int(_lib.lib.scarlet_lowres_products_scratch_bytes(ctypes.byref(b._c), ctypes.byref(ob._c), ctypes.byref(lr),
                                                              ctypes.byref(_lib.ScarletProducts(rendered=1))))
    r = dict(workload="%s: %d scenes, model %d x %d x %d (K=%d), low-resolution %d x %d x %d at band0=%d, nfy, nfx = %d, %d"
             % (name, S, C, H, W, b.K, B, h, wd, BAND0, f["uy"].shape[0], f["ux"].shape[0]), name=name,
             form="streamed" if need else "lds", scratch_mib=need / 2.0 ** 20)
    for k, v in times.items():
        r[k] = float(np.median(v))
        r[k.replace("_ms", "_min_max_ms")] = [float(min(v)), float(max(v))]
    r.update(one_call_over_composed=r["one_call_ms"] / r["composed_ms"],
             one_call_model_over_composed=r["one_call_model_ms"] / r["composed_ms"],
             max_rel_difference_from_composed=agree, rendered_bits_equal=bool(torch.equal(out.rendered[1], ref[0])),
             inner=inner, warmup=warmup, repeats=repeats, device=torch.cuda.get_device_name())
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--workloads", default="lds,streamed")
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
