"""-m gpu: BlendBatch.fit / update_sources through scarlet_fit_with / scarlet_source_update_with against the named entry
points, which are fixed shapes of the same request: the same kernels with the same arguments in the same order, so every
output array must be byte-identical.

One family per combination of members a batch can carry, at the smallest shape that reaches it.  Each case builds the
batch twice from the same inputs (the same start both times), runs 3 iterations at e_rel = 0 once through BlendBatch.fit
and once through the named entry point called by ctypes on the batch's own structs, and compares sed, morph, centers,
shifts, flags, mse, it, lipschitz, active and status.  The single-observation families do the same for one
update_sources() against their scarlet_source_update_* function.  No oracle run: nothing here says the numbers are right
(the families' own tests do), only that the request changes none of them."""
import contextlib
import ctypes
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITERS = 3
BG = 0.1
KEYS = ("sed", "morph", "centers", "shifts", "flags", "mse", "it", "lipschitz", "active", "status")
RAGGED = ((24, 32), (16, 20), (24, 24), (9, 32))


@pytest.fixture(scope="module")
def scarlet():
    import scarlet_amd
    scarlet_amd._lib.require_gpu()
    from oracle import build as obuild
    obuild.build()
    return scarlet_amd


@pytest.fixture(scope="module")
def arg_order():
    """the named entry points' arguments in order, as tools/record_entry_refusals.py lists them"""
    spec = importlib.util.spec_from_file_location("record_entry_refusals", os.path.join(ROOT, "tools", "record_entry_refusals.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.ENTRY_POINTS


def state(b):
    torch.cuda.synchronize()
    return dict(sed=b.sed_current.cpu().numpy(), morph=b.morph_current.cpu().numpy(), centers=b.centers.cpu().numpy(),
                shifts=b.shifts.cpu().numpy(), flags=b.flags.cpu().numpy(), mse=b.mse_buf.cpu().numpy(),
                it=b.it.cpu().numpy(), lipschitz=b.lipschitz.cpu().numpy(), active=b.active.cpu().numpy(),
                status=b.status.cpu().numpy())


def assert_identical(a, b, what):
    for key in KEYS:
        assert np.array_equal(a[key], b[key], equal_nan=True), "%s: %s differs" % (what, key)


def call_named(b, name, order, ps=None, max_iter=ITERS, in_iteration=0):
    """the named entry point `name` on the batch's own structs (what BlendBatch called before there was a request)"""
    from scarlet_amd import _lib
    r, keep = b._request(ps)                    # (only for its pointer arrays: obs, band0, lowres, lowres_frames)
    values = dict(b=ctypes.byref(b._c), c=ctypes.byref(b._cons), f=ctypes.byref(b._frames),
                  o=None if b._upd is None else ctypes.byref(b._upd), p=None if ps is None else ctypes.byref(ps),
                  obs=r.obs, band0=r.band0, n_obs=r.n_obs, lowres=r.lowres, lrf=r.lowres_frames,
                  max_iter=max_iter, e_rel=0.0, approximate_L=0, check_every=0, stream=_lib.stream_ptr(),
                  in_iteration=in_iteration)
    return _lib.check(getattr(_lib.lib, name)(*[values[a] for a in order[name]]))


def prior_struct(b, prior):
    from scarlet_amd import prior as _prior
    quad, given, fns = _prior.split_priors(prior)
    ps = b._prior_struct(quad)
    b._set_given(ps, given)
    return ps


# ---- the inputs
def blob_scene(seed, B, h, w, K):
    """K Gaussian blobs on one row through the middle of an h x w frame, a SED each, a little noise"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:h, :w]
    centers = np.array([[h // 2, (k + 1) * w // (K + 1)] for k in range(K)], np.int32)
    images = 0.02 * rng.standard_normal((B, h, w))
    for cy, cx in centers:
        images += rng.uniform(0.5, 2.0, (B, 1, 1)) * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * rng.uniform(1.5, 2.5) ** 2))
    return images.astype(np.float32), centers


def uniform_scenes(B, S=4, K=3, H=24, W=32):
    sc = [blob_scene(100 + s, B, H, W, K) for s in range(S)]
    return np.stack([im for im, _ in sc]), np.stack([c for _, c in sc])


def ragged_scenes(B, K=2):
    sc = [blob_scene(200 + s, B, h, w, K) for s, (h, w) in enumerate(RAGGED)]
    return [im for im, _ in sc], [c for _, c in sc]


def single(scarlet, **kw):
    def make():
        images, centers = uniform_scenes(3)
        return scarlet.BlendBatch(images, centers, mse_capacity=ITERS + 1, **kw).init_extended(np.ones(3) * BG)
    return make


def arrays():
    rng = np.random.default_rng(5)
    return dict(symmetric=rng.integers(0, 2, (4, 3)).astype(np.uint8), monotonic=rng.integers(0, 2, (4, 3)).astype(np.uint8),
                l0_thresh=rng.uniform(0, 0.01, (4, 3)).astype(np.float32))


def options(scarlet, K=3):
    import update_option_cases as uc
    return scarlet.UpdateOptions(**uc.update_kwargs("mixed", K))


def ragged(scarlet):
    def make():
        images, centers = ragged_scenes(3)
        return scarlet.BlendBatch(images, centers, mse_capacity=ITERS + 1).init_extended(np.ones(3) * BG)
    return make


def catalogue(scarlet, optset):
    """the `wave` catalogue: ragged frames, two- and three-layer sources (group); optset: its sources' update options"""
    import catalog_cases as cc
    import catalog_option_cases as oc

    def make():
        if optset is None:
            c = cc.CASES["wave"]
            specs = [[scarlet.SourceSpec(px, kind=kind, flux_percentiles=None if perc is None else list(perc)) for px, kind, perc in cat]
                     for cat in cc.catalog(c)]
            cutouts = [np.array(im) for im, _ in cc.scenes(c)]
        else:
            c = oc.CASES["wave"]
            specs = [[scarlet.SourceSpec(px, kind=kind, flux_percentiles=None if perc is None else list(perc), **oc.spec_kwargs(optset, i))
                      for i, (px, kind, perc) in enumerate(cat)] for cat in oc.catalog(c)]
            cutouts = [np.array(im) for im, _ in oc.scenes(c)]
        b = scarlet.BlendBatch.from_catalog(cutouts, specs, mse_capacity=ITERS + 1)
        assert b.frame_shapes is not None and b.group is not None and (b._upd is not None) == (optset is not None)
        return b.init_catalog(np.ones(c.B) * cc.BG)
    return make


def observations(scarlet, widths=(3, 2), frames=False, **kw):
    """same-grid observations that tile the model channels; frames: the scenes' own frames"""
    def make():
        C = sum(widths)
        images, centers = ragged_scenes(C) if frames else uniform_scenes(C)
        obs, at = [], 0
        for n in widths:
            if frames:
                obs.append(scarlet.ObservationBatch.from_frames([im[at:at + n] for im in images], band0=at))
            else:
                obs.append(scarlet.ObservationBatch(np.ascontiguousarray(images[:, at:at + n]), band0=at))
            at += n
        b = scarlet.BlendBatch.from_observations(obs, centers, mse_capacity=ITERS + 1, **kw)
        return b.init_combined([np.ones(n) * BG for n in widths])
    return make


def lowres(scarlet):
    """the smallest geometry of the low-resolution tests (lowres_common's fixture `a`): 3 same-grid + 2 low-resolution channels"""
    import lowres_common as lc
    g = lc.fixture()

    def make():
        obs, (sed0, morph0, cen0), cw, lo = lc.fit_inputs(g, "a")
        S = 3
        stack = lambda x: np.stack([x] * S).astype(np.float32)          # noqa: E731
        hi_b = scarlet.ObservationBatch(stack(obs[0]["images"]), band0=0).set_diff_kernel(obs[0]["diff_kernel"])
        lo_b = scarlet.LowResObservationBatch(stack(obs[1]["images"]), band0=3, geometry=lo, weights=stack(obs[1]["weights"]))
        b = scarlet.BlendBatch.from_observations([hi_b, lo_b], np.stack([cen0] * S), centroid_weight=cw, mse_capacity=ITERS + 1)
        b.set_state(stack(sed0), stack(morph0))
        return b
    return make


def lowres_frames(scarlet):
    """lowres_frame_cases `small`: ragged frames, a same-grid observation and a low-resolution one with its own tables"""
    import lowres_frame_cases as fc

    def make():
        data = fc.scene_data("small")
        d0 = data[0]
        hi = scarlet.ObservationBatch.from_frames([d["images_hi"] for d in data], band0=0).set_diff_kernel(fc.diff_kernel(d0["hi_bands"]))
        lo = scarlet.LowResObservationBatch.from_frames([d["images_lo"] for d in data], band0=d0["lo_band0"],
                                                        geometry=[d["geo"] for d in data], weights=[d["weights_lo"] for d in data])
        b = scarlet.BlendBatch.from_observations([hi, lo], [d["centers"] for d in data], centroid_weight=fc.model_psf()[0],
                                                 mse_capacity=ITERS + 1)
        S, K, C = len(data), max(len(d["sed0"]) for d in data), d0["C"]
        sed, morph = np.zeros((S, K, C), np.float32), np.zeros((S, K, b.H, b.W), np.float32)
        for s, d in enumerate(data):
            n, (h, w) = len(d["sed0"]), d["morph0"].shape[1:]
            sed[s, :n], morph[s, :n, :h, :w] = d["sed0"], d["morph0"]
        b.set_state(sed, morph)
        assert b.frame_shapes is not None and any(x is not None and "frames" in x[1] for x in b._lowres)
        return b
    return make


def quadratic(scarlet):
    return scarlet.QuadraticPrior(sed_weight=0.3, morph_weight=2.0)


# family -> (make, prior or None, library option to set or None, the named fit entry points, the named update or None)
def families(scarlet):
    S = "scarlet_"
    return {
        "plain": (single(scarlet), None, None, (S + "fit", S + "fit_constrained"), S + "source_update"),
        "arrays": (single(scarlet, **arrays()), None, None, (S + "fit_constrained",), S + "source_update_constrained"),
        "prior": (single(scarlet), quadratic, None, (S + "fit_prior", S + "fit_constrained"), S + "source_update_prior"),
        "options": (single(scarlet, update=options(scarlet)), None, None, (S + "fit_options",), S + "source_update_options"),
        "frames": (ragged(scarlet), None, None, (S + "fit_frames",), S + "source_update_frames"),
        "frames_group": (catalogue(scarlet, None), None, None, (S + "fit_frames_grouped",), S + "source_update_frames_grouped"),
        "frames_options": (catalogue(scarlet, "mixed"), None, None, (S + "fit_frames_options",), S + "source_update_frames_options"),
        "two_obs": (observations(scarlet), None, None,
                    (S + "fit_observations", S + "fit_multi", S + "fit_observations_constrained"), None),
        "obs_options": (observations(scarlet, update=options(scarlet)), None, None, (S + "fit_observations_options",), None),
        "obs_lowres": (lowres(scarlet), None, None, (S + "fit_observations_lowres", S + "fit_observations_lowres_large"), None),
        "obs_lowres_streamed": (lowres(scarlet), None, "LOWRES_STREAMED", (S + "fit_observations_lowres_large",), None),
        "obs_prior": (observations(scarlet), quadratic, None, (S + "fit_observations_prior",), None),
        "wide": (observations(scarlet, widths=(8, 4), wide=True), None, None, (S + "fit_observations_wide",), None),
        "obs_frames": (observations(scarlet, frames=True), None, None, (S + "fit_observations_frames",), None),
        "obs_frames_lowres": (lowres_frames(scarlet), None, None, (S + "fit_observations_frames_lowres",), None),
    }


FAMILIES = ("plain", "arrays", "prior", "options", "frames", "frames_group", "frames_options", "two_obs", "obs_options",
            "obs_lowres", "obs_lowres_streamed", "obs_prior", "wide", "obs_frames", "obs_frames_lowres")


@contextlib.contextmanager
def library_option(scarlet, name):
    if name is None:
        yield
        return
    old = scarlet._lib.set_option(name, 1)
    try:
        yield
    finally:
        scarlet._lib.set_option(name, old)


@pytest.mark.parametrize("family", FAMILIES)
def test_fit_with_gives_the_named_entry_points_bits(scarlet, arg_order, family):
    make, prior, opt, named, _ = families(scarlet)[family]
    with library_option(scarlet, opt):
        b = make()
        start = state(b)
        assert b.fit(ITERS, e_rel=0, check_every=0, prior=None if prior is None else prior(scarlet)) == ITERS
        ref = state(b)
        assert (ref["it"][ref["status"] == 0] == ITERS).all() and (ref["status"] == 0).any(), ref["status"]
        assert not np.array_equal(start["morph"], ref["morph"]) and not np.array_equal(start["sed"], ref["sed"])
        for name in named:
            n = make()
            assert_identical(start, state(n), family + ": the same start")
            ps = None if prior is None else prior_struct(n, prior(scarlet))
            n._ensure_mse_capacity(ITERS)
            n.active.fill_(1)
            assert call_named(n, name, arg_order, ps) == ITERS
            assert_identical(ref, state(n), "%s: fit() against %s" % (family, name))


@pytest.mark.parametrize("family", [f for f in FAMILIES if not f.startswith(("obs", "two_obs", "wide"))])
def test_update_with_gives_the_named_entry_points_bits(scarlet, arg_order, family):
    make, prior, _, _, named = families(scarlet)[family]
    a, n = make(), make()
    if prior is None:
        a.update_sources()
        call_named(n, named, arg_order)
    else:                      # (the update reads the prior's L_comp alone)
        a._lib_update(prior_struct(a, prior(scarlet)), 0)
        call_named(n, named, arg_order, prior_struct(n, prior(scarlet)))
    assert_identical(state(a), state(n), "%s: update_sources() against %s" % (family, named))
