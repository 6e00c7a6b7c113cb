#!/usr/bin/env python
"""Generate tests/golden/lowres.npz: what the reference's LowResObservation computes for the geometries the
low-resolution tests use.  Runs where the reference package exists (oracle.refshim loads it under its stand-ins); the
result is data only.

    python tools/gen_lowres_golden.py            # rewrites tests/golden/lowres.npz

The reference needs a WCS; astropy is not required: `scarlet_amd.resampling.AffineWCS` (a flat-sky affine map with the
few methods the reference calls) stands in for it.  Geometries:

    a  ratio 2, aligned:            32 x 32 model, 16 x 16 observation
    b  ratio 2.5, sub-pixel offset: 32 x 32 model, 12 x 12 observation whose pixel (0, 0) sits at (1.3, 0.6)
    c  non-square, 32 x 24 model, 10 x 12 observation (wider than tall): the reference cannot run it -- without a rotation it multiplies per-row and
       per-column masks elementwise (resampling.py:90-92) and needs square frames; the file records its error message

Per geometry a, b: the inputs, `_render` of three random models, `get_loss`, the difference kernels, the padded shape
and the shifts, and one Blend.fit of 5 iterations of K = 2 sources (symmetric, monotonic) against
[Observation (3 bands, with PSF), LowResObservation (2 further bands)].  refshim's analytic gradient only knows
Observation; for this run the generator installs its own, with the low-resolution adjoint taken through the dense
operator built by linearity from `_render`.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import refshim                      # noqa: E402
from scarlet_amd.resampling import AffineWCS    # noqa: E402

GEOMETRIES = {
    # name: model (H, W), observation (h, w), pixel ratio, model-frame position (y, x) of observation pixel (0, 0)
    "a": ((32, 32), (16, 16), 2.0, (0.0, 0.0)),
    "b": ((32, 32), (12, 12), 2.5, (1.3, 0.6)),
    "c": ((32, 24), (10, 12), 2.0, (1.0, 0.5)),
}
P_MODEL, P_OBS = 11, 9
CENTERS = ((12, 13), (20, 18))


def gauss(n, sigma, dy=0.0, dx=0.0):
    y, x = np.mgrid[:n, :n] - (n // 2)
    g = np.exp(-((y - dy) ** 2 + (x - dx) ** 2) / (2 * sigma ** 2))
    return g / g.sum()


def blob(shape, cy, cx, sy, sx):
    y, x = np.mgrid[:shape[0], :shape[1]]
    return np.exp(-((y - cy) ** 2 / (2 * sy ** 2) + (x - cx) ** 2 / (2 * sx ** 2)))


def wcs_pair(model_shape, lr_shape, ratio, origin):
    return (AffineWCS(model_shape, 1.0),
            AffineWCS(lr_shape, ratio, crpix=(1 - origin[1] / ratio, 1 - origin[0] / ratio)))


def inputs(name):
    """The seeded inputs of a geometry."""
    (H, W), (h, w), ratio, origin = GEOMETRIES[name]
    rng = np.random.default_rng({"a": 11, "b": 12, "c": 13}[name])
    d = dict(model_shape=np.array([H, W]), lr_shape=np.array([h, w]), ratio=np.float64(ratio), origin=np.array(origin))
    d["model_psf"] = gauss(P_MODEL, 0.9)[None].astype(np.float32)
    d["hr_psfs"] = np.array([gauss(P_MODEL, 1.1 + 0.1 * b) for b in range(3)]).astype(np.float32)
    d["lr_psfs"] = np.array([gauss(P_OBS, 0.9 + 0.15 * b, 0.2, -0.1) for b in range(2)]).astype(np.float32)
    d["models"] = rng.random((3, 2, H, W)).astype(np.float32)
    d["images_lr"] = rng.standard_normal((2, h, w)).astype(np.float32)
    d["weights_lr"] = (0.5 + rng.random((2, h, w))).astype(np.float32)
    return d


def render_of(obs):
    """The observation's forward operator on a model over the model frame's channels."""
    if hasattr(obs, "_resconv_op"):
        return obs._render
    return lambda model: obs.render(model)


def dense_operator(obs, shape):
    """[B][pixels of the observation][H W]: column p = the render of the model-frame image (`shape`) that is 1 at pixel p
    of every channel (both operators act band by band on the observation's band slice)."""
    C, H, W = shape
    render = render_of(obs)
    cols = []
    unit = np.zeros(shape, dtype=np.float32)
    for p in range(H * W):
        unit[:, p // W, p % W] = 1
        r = np.asarray(render(unit), dtype=np.float64)
        cols.append(r.reshape(r.shape[0], -1))
        unit[:, p // W, p % W] = 0
    return np.stack(cols, axis=-1)


def make_grad(dense):
    """autograd.grad stand-in for a Blend with a LowResObservation: the exact adjoint of every observation through its
    dense operator (`dense` maps id(observation) to it), loss and gradients as refshim's stand-in returns them."""
    def grad(fun, argnums):
        blend = fun.__self__

        def g(*params):
            K = blend.K
            seds, morphs = params[:K], params[K:]
            model = blend.get_model(seds, morphs)
            G = np.zeros(model.shape, dtype=np.float64)
            loss = 0
            for obs in blend.observations:
                T = dense[id(obs)]
                d = obs.weights * (render_of(obs)(model) - obs.images)
                loss = loss + 0.5 * np.sum(d ** 2)
                wd = np.asarray(obs.weights * d, dtype=np.float64).reshape(T.shape[0], -1)
                G[obs._band_slice] += np.einsum("bip,bi->bp", T, wd).reshape(G[obs._band_slice].shape)
            blend.mse.append(loss)
            dt = model.dtype
            sed_grads = tuple((G * m[None]).sum(axis=(1, 2)).astype(dt) for m in morphs)
            morph_grads = tuple((G * s[:, None, None]).sum(axis=0).astype(dt) for s in seds)
            return sed_grads + morph_grads
        return g
    return grad


def reference_run(ref, name, d, out):
    (H, W), (h, w), ratio, origin = GEOMETRIES[name]
    wm, wl = wcs_pair((H, W), (h, w), ratio, origin)
    ch2 = ["r", "i"]
    frame = ref.Frame((2, H, W), wcs=wm, psfs=d["model_psf"].copy(), channels=ch2)
    obs = ref.LowResObservation(d["images_lr"].copy(), wcs=wl, psfs=d["lr_psfs"].copy(), weights=d["weights_lr"].copy(),
                                channels=ch2)
    obs.match(frame)
    out[name + "_fft_shape"] = np.array(obs._fft_shape)
    out[name + "_shifts"] = np.array(obs.shifts, dtype=np.float64)
    out[name + "_diff_psf"] = np.array(obs.build_diffkernel(frame, None).image, dtype=np.float32)
    out[name + "_renders"] = np.array([obs._render(m) for m in d["models"]], dtype=np.float32)
    out[name + "_losses"] = np.array([obs.get_loss(m) for m in d["models"]], dtype=np.float64)

    # ---- the joint fit: 5 model channels, bands 0-2 on the model's grid with a PSF, bands 3-4 at low resolution
    rng = np.random.default_rng(100 + ord(name))
    ch5 = ["g", "r", "i", "z", "y"]
    frame5 = ref.Frame((5, H, W), wcs=wm, psfs=d["model_psf"].copy(), channels=ch5)
    lo = ref.LowResObservation(np.zeros((2, h, w), np.float32), wcs=wl, psfs=d["lr_psfs"].copy(),
                               weights=d["weights_lr"].copy(), channels=ch5[3:])
    lo.match(frame5)
    truth_sed = np.array([[1.0, 0.8, 0.6, 0.5, 0.4], [0.3, 0.5, 0.7, 0.9, 1.1]], dtype=np.float32)
    truth_morph = np.array([blob((H, W), cy + 0.3, cx - 0.2, 2.2, 1.8) for cy, cx in CENTERS], dtype=np.float32)
    truth = np.einsum("kc,kyx->cyx", truth_sed, truth_morph).astype(np.float32)
    hi = ref.Observation(np.zeros((3, H, W), np.float32), psfs=d["hr_psfs"].copy(), channels=ch5[:3])
    hi.match(frame5)
    images_hr = (hi.render(truth) + 0.01 * rng.standard_normal((3, H, W))).astype(np.float32)
    images_lo = (lo._render(truth) + 0.01 * rng.standard_normal((2, h, w))).astype(np.float32)
    hi.images, lo.images = images_hr, images_lo
    sed0 = (truth_sed * (0.7 + 0.6 * rng.random(truth_sed.shape))).astype(np.float32)
    morph0 = np.array([blob((H, W), cy, cx, 2.6, 2.6) for cy, cx in CENTERS], dtype=np.float32)

    class Started(ref.PointSource):
        """A source that starts from given factors (no initialisation from data, no update at construction)."""
        def __init__(self, frame, center, sed, morph):
            self.symmetric, self.monotonic = True, True
            self.pixel_center, self.center_step, self.delay_thresh = tuple(center), 5, 0
            ref.Component.__init__(self, frame, sed.copy(), morph.copy())
            self._centroid_weight = frame.psfs[0].image

    import scarlet.blend
    scarlet.blend.grad = make_grad({id(o): dense_operator(o, (5, H, W)) for o in (hi, lo)})
    try:
        sources = [Started(frame5, c, sed0[k], morph0[k]) for k, c in enumerate(CENTERS)]
        blend = ref.Blend(sources, [hi, lo])
        blend.fit(5, e_rel=0)
    finally:
        scarlet.blend.grad = refshim._analytic_grad
    out[name + "_fit_images_hr"], out[name + "_fit_images_lr"] = images_hr, images_lo
    out[name + "_fit_sed0"], out[name + "_fit_morph0"] = sed0, morph0
    out[name + "_fit_centers0"] = np.array(CENTERS, dtype=np.int32)
    out[name + "_fit_sed"] = np.array([s.sed for s in sources], dtype=np.float32)
    out[name + "_fit_morph"] = np.array([s.morph for s in sources], dtype=np.float32)
    out[name + "_fit_mse"] = np.array(blend.mse, dtype=np.float64)
    out[name + "_fit_centers"] = np.array([s.pixel_center for s in sources], dtype=np.int32)
    out[name + "_fit_flags"] = np.array([s.flags.value for s in sources], dtype=np.int32)


def main():
    ref = refshim.load_reference()
    out = {}
    for name in ("a", "b"):
        d = inputs(name)
        for k, v in d.items():
            out[name + "_" + k] = v
        reference_run(ref, name, d, out)
    # geometry c: what the reference says to a non-square model frame
    d = inputs("c")
    for k, v in d.items():
        out["c_" + k] = v
    (H, W), (h, w), ratio, origin = GEOMETRIES["c"]
    wm, wl = wcs_pair((H, W), (h, w), ratio, origin)
    try:
        frame = ref.Frame((2, H, W), wcs=wm, psfs=d["model_psf"].copy(), channels=["r", "i"])
        ref.LowResObservation(d["images_lr"], wcs=wl, psfs=d["lr_psfs"].copy(), channels=["r", "i"]).match(frame)
        raise SystemExit("the reference matched geometry c: record its outputs instead of its error")
    except ValueError as e:
        out["c_reference_error"] = np.array("%s: %s" % (type(e).__name__, e))
    path = os.path.join(ROOT, "tests", "golden", "lowres.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
