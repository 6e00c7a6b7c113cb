"""The cases of `Blend` as a view on `BlendBatch` ("Several observations"): every way a `Blend` builds its
batch, beside `BlendBatch.from_observations` itself and the public face of a `LowResObservation`.  For
tools/gradstages_ab.py --cases blend_view_cases: build-against-build dumps and runs for a kernel trace (the interface
of tests/launch_form_cases.py: CASES, ITERS, HIPFFT_CASES, SIDE_STREAM_CASES, scenes, make_batch, options, state).

Every case has two sources and runs 3 iterations at e_rel = 0.  The same-grid cases are one 16 x 16 scene of
launch_form_cases' blobs in five channels, cut into two band-sliced observations: the first with its own PSFs (a
difference kernel) and a scalar weight other than 1, the second with the model's PSF and array weights.  The
low-resolution cases are the joint fit of geometry "a" of tests/golden/lowres.npz (32 x 32 model frame, 16 x 16
observation).  The comparison is between two checkouts, not against the oracle.  `make_batch` builds the batch as well
(`Blend._ensure_batch`), so that the compared launches are the fit's alone.
"""
import collections

import numpy as np

import launch_form_cases as lf
import lowres_common as lc

BG = lf.BG
ITERS = 3
HIPFFT_CASES = []
SIDE_STREAM_CASES = ()
CH = list("grizy")
PHASES = ((0.0, 0.0), (0.3, -0.4), (-0.2, 0.45))      # sub-pixel cuts of the three scenes of case 11, model pixels (y, x)

Case = collections.namedtuple("Case", "name kind python approximate_L opts iters")


def _c(name, kind, python=False, approximate_L=False, opts=()):
    return Case(name, kind, python, approximate_L, tuple(opts), None)


CASES = collections.OrderedDict((c.name, c) for c in [
    _c("01_one_observation", "one"),
    _c("02_one_observation_python", "one", python=True),
    _c("03_two_observations", "two"),
    _c("04_two_observations_python", "two", python=True),
    _c("05_two_observations_python_approximate_L", "two", python=True, approximate_L=True),
    _c("06_two_observations_multicomponent", "two_layered"),
    _c("07_two_observations_mixed_symmetric", "two_mixed"),
    _c("08_two_observations_fix_sed", "two_fix_sed"),
    _c("09_lowres", "lowres"),
    _c("10_lowres_streamed", "lowres", opts=["LOWRES_STREAMED"]),
    _c("11_from_observations_S3", "batch"),
    _c("12_lowres_render_and_loss", "render"),
])


def _gauss(sigma, n=11):
    y, x = np.mgrid[:n, :n] - n // 2
    p = np.exp(-(y * y + x * x) / (2 * sigma ** 2))
    return (p / p.sum()).astype(np.float32)


def scenes(c):
    """same grid: (images (5, 16, 16), centers (2, 2), weights (2, 16, 16));  low resolution: (the fixture,)"""
    if c.kind in ("lowres", "batch", "render"):
        return (lc.fixture(),)
    images, centers = lf.scenes(lf._c("blend_view", 2, 5, 16, 16))
    weights = np.random.default_rng(16).uniform(0.5, 1.5, size=images[0, 3:].shape).astype(np.float32)
    return images[0], centers[0], weights


class _Run(object):
    """a case behind a batch's face: fit() makes the compared launches, state() returns `arrays`"""

    def __init__(self, fit):
        self._fit, self.arrays = fit, {}

    def fit(self, iters, e_rel=0, approximate_L=False):
        self.arrays = self._fit(iters, e_rel, approximate_L)
        return iters


def _blend_state(blend):
    out = lf.state(blend._batch)
    nan = (np.nan, np.nan)
    out["pixel_center"] = np.array([s.pixel_center for s in blend.sources])
    out["shift"] = np.array([nan if getattr(s, "shift", None) is None else s.shift for s in blend.sources], dtype=np.float64)
    out["blend_mse"] = np.array(blend.mse)
    out["blend_L"] = np.array([blend.L_sed, blend.L_morph], dtype=np.float64)
    return out


def _run_blend(scarlet, c, sources, observations):
    blend = scarlet.Blend(sources, observations)
    blend.python_pipeline = c.python
    assert blend._builtin_pipeline() == (not c.python)
    blend._ensure_batch()

    def fit(iters, e_rel, approximate_L):
        blend.fit(iters, e_rel=e_rel, approximate_L=approximate_L)
        assert blend.it == iters
        return _blend_state(blend)
    return _Run(fit)


def same_grid_inputs(scarlet, c, images, centers, weights):
    """(sources, observations) of a same-grid case"""
    frame = scarlet.Frame(images.shape, psfs=_gauss(0.9)[None], channels=CH)
    psfs = np.array([_gauss(1.4 + 0.1 * b) for b in range(5)])
    full = scarlet.Observation(images, psfs=psfs, channels=CH).match(frame)
    bg = np.ones(5) * BG
    cen = [tuple(int(v) for v in p) for p in centers]
    if c.kind == "one":
        observations = full
    else:
        observations = [scarlet.Observation(images[:3], psfs=psfs[:3], channels=CH[:3]).match(frame),
                        scarlet.Observation(images[3:], psfs=frame.psfs, weights=weights, channels=CH[3:]).match(frame)]
        observations[0].weights = 0.5
    if c.kind == "two_layered":
        sources = [scarlet.MultiComponentSource(frame, cen[0], full, bg), scarlet.ExtendedSource(frame, cen[1], full, bg)]
    elif c.kind == "two_mixed":
        sources = [scarlet.ExtendedSource(frame, cen[0], full, bg), scarlet.ExtendedSource(frame, cen[1], full, bg, symmetric=False)]
    elif c.kind == "two_fix_sed":
        sources = [scarlet.ExtendedSource(frame, cen[0], full, bg, fix_sed=True), scarlet.ExtendedSource(frame, cen[1], full, bg)]
    else:
        sources = [scarlet.ExtendedSource(frame, p, full, bg) for p in cen]
    return sources, observations


def _lowres_blend(scarlet, c, g, name="a"):
    lo, frame = lc.geometry(g, name, model_channels=lc.CH5, channels=lc.CH5[3:], images=g[name + "_fit_images_lr"].copy())
    hi = scarlet.Observation(g[name + "_fit_images_hr"].copy(), psfs=g[name + "_hr_psfs"].copy(), channels=lc.CH5[:3]).match(frame)
    bg = [np.ones(3, np.float32) * 0.01, np.ones(2, np.float32) * 0.01]
    sources = [scarlet.CombinedExtendedSource(frame, tuple(int(v) for v in p), [hi, lo], bg, symmetric=True, monotonic=True)
               for p in g[name + "_fit_centers0"]]
    return _run_blend(scarlet, c, sources, [hi, lo])


def _batch_of_three(scarlet, g, name="a"):
    obs, (_, _, cen0), cw, _ = lc.fit_inputs(g, name)
    S, base = len(PHASES), tuple(g[name + "_origin"])
    geo = [lc.geometry(g, name, model_channels=lc.CH5, channels=lc.CH5[3:], images=g[name + "_fit_images_lr"].copy(),
                       origin=(base[0] + 0.5 + dy, base[1] + 0.5 + dx))[0] for dy, dx in PHASES]
    rng = np.random.default_rng(32)
    hr = np.stack([obs[0]["images"] + 0.02 * s * rng.standard_normal(obs[0]["images"].shape) for s in range(S)]).astype(np.float32)
    lr = np.stack([obs[1]["images"] + 0.02 * s * rng.standard_normal(obs[1]["images"].shape) for s in range(S)]).astype(np.float32)
    wl = np.stack([obs[1]["weights"] * (1 + 0.2 * s) for s in range(S)]).astype(np.float32)
    hi_b = scarlet.ObservationBatch(hr, band0=0).set_diff_kernel(obs[0]["diff_kernel"])
    lo_b = scarlet.LowResObservationBatch(lr, band0=3, geometry=geo, weights=wl)
    b = scarlet.BlendBatch.from_observations([hi_b, lo_b], np.stack([cen0] * S), centroid_weight=cw, mse_capacity=ITERS + 1)
    return b.init_combined([np.ones(3) * 0.01, None], obs_psfs=[g[name + "_hr_psfs"], g[name + "_lr_psfs"]],
                           model_psf=g[name + "_model_psf"][0])


def _render_and_loss(g, name="a"):
    lo, _ = lc.geometry(g, name)
    H, W = lo.model_shape
    model = np.random.default_rng(12).random((2, H, W)).astype(np.float32)

    def fit(iters, e_rel, approximate_L):
        return dict(render=lo.render(model).cpu().numpy(), loss=np.array(float(lo.get_loss(model))))
    return _Run(fit)


def make_batch(scarlet, c, *inputs):
    """the case's freshly built object (the same state every time): a `_Run`, or for case 11 the batch itself"""
    if c.kind == "lowres":
        return _lowres_blend(scarlet, c, *inputs)
    if c.kind == "batch":
        return _batch_of_three(scarlet, *inputs)
    if c.kind == "render":
        return _render_and_loss(*inputs)
    return _run_blend(scarlet, c, *same_grid_inputs(scarlet, c, *inputs))


def state(b):
    import torch
    torch.cuda.synchronize()
    return b.arrays if isinstance(b, _Run) else lf.state(b)


options = lf.options
