"""-m gpu: joint fits of scenes with their own frame sizes against a LOW-RESOLUTION observation --
LowResObservationBatch.from_frames(geometry=) beside same-grid observations that carry the model frames
(scarlet_fit_observations_frames_lowres, scarlet_observations_products_frames_lowres; lowres.h k_lowres_planes_frames /
k_lowres_products_frames, and the streamed form on the padded extents).

The cases are those of tests/lowres_frame_cases.py.  Every scene must come out as `lowres_common.fit` fits it alone, on its
cropped arrays with its own LowResObservation.match(own frame).factors: sed, morph and loss history to 1e-5 max-norm
relative (the tolerance of test_gpu_lowres.py and test_gpu_observations_frames.py), centres, flags and iteration counts
exactly.  Unless noted the observations are a 3-band same-grid one with a PSF and a 2-band low-resolution one.
  1. `small`, 5 iterations, also with mixed per-component symmetric / monotonic
  2. `small` with approximate_L, and one run to convergence (exact iteration counts)
  3. `small` under LOWRES_STREAMED=1, and `streamed` as it comes
  4. `lds_edge` at B = 8 (C = 11: wide): LDS planned from the maxima, which come from different scenes
  5. pixels outside: both morphology buffers, the model, rendered and residual of the low-resolution observation
  6. all scenes full size with one geometry repeated: the bits of the uniform batch, in both forms
  7. a scene gives the same bits at index 0 and at the last index
  8. a `dims` row outside the block / one that disagrees with frame_hw: STATUS_BAD_FRAME, untouched, the others' bits stay
  9. products against float64 on the scene's own factors; repeatable; read-only
 10. init_combined: every scene as the one-scene uniform batch of that scene
 11. wide=True with the low-resolution observation at band0 = 8 (C = 10)
"""
import numpy as np
import pytest

import lowres_common as lc
import lowres_frame_cases as fc
import lowres_large_common as ll
from conftest import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
TOL = 1e-5
SWITCHES = {"small": [[(1, 0), (0, 1), (1, 1)], [(0, 1)], [(1, 1), (0, 0)], [(0, 1), (1, 0)], [(1, 1), (1, 0), (0, 1)]]}


@pytest.fixture(scope="module")
def scarlet():
    import scarlet_amd
    scarlet_amd._lib.require_gpu()
    from oracle import build as obuild
    obuild.build()
    return scarlet_amd


def _observations(scarlet, data, scalar_weights=False):
    d0 = data[0]
    hi = scarlet.ObservationBatch.from_frames([d["images_hi"] for d in data], band0=0).set_diff_kernel(fc.diff_kernel(d0["hi_bands"]))
    lo = scarlet.LowResObservationBatch.from_frames(
        [d["images_lo"] for d in data], band0=d0["lo_band0"], geometry=[d["geo"] for d in data],
        weights=1.0 if scalar_weights else [d["weights_lo"] for d in data])
    return hi, lo


def _pad_state(data, H, W):
    S, K, C = len(data), max(len(d["sed0"]) for d in data), data[0]["C"]
    sed, morph = np.zeros((S, K, C), np.float32), np.zeros((S, K, H, W), np.float32)
    for s, d in enumerate(data):
        n, (h, w) = len(d["sed0"]), d["morph0"].shape[1:]
        sed[s, :n], morph[s, :n, :h, :w] = d["sed0"], d["morph0"]
    return sed, morph


def _batch(scarlet, data, switches=None, mse_capacity=64, start=True, **kw):
    hi, lo = _observations(scarlet, data)
    if switches is not None:
        kw["symmetric"] = [[sw[0] for sw in row] for row in switches]
        kw["monotonic"] = [[sw[1] for sw in row] for row in switches]
    b = scarlet.BlendBatch.from_observations([hi, lo], [d["centers"] for d in data], centroid_weight=fc.model_psf()[0],
                                             lowres_products=True, wide=data[0]["C"] > 8, mse_capacity=mse_capacity, **kw)
    if start:
        b.set_state(*_pad_state(data, b.H, b.W))
    return b


def _state(b):
    torch.cuda.synchronize()
    return dict(sed=[t.cpu().numpy() for t in b.sed], morph=[t.cpu().numpy() for t in b.morph], cur=b.cur.cpu().numpy(),
                cen=b.centers.cpu().numpy(), shifts=b.shifts.cpu().numpy(), flags=b.flags.cpu().numpy(),
                mse=b.mse_buf.cpu().numpy(), it=b.it.cpu().numpy(), status=b.status.cpu().numpy(),
                active=b.active.cpu().numpy(), lip=b.lipschitz.cpu().numpy())


def _same(a, b, what, sa=slice(None), sb=slice(None), crop=None):
    """the states a[sa] and b[sb] hold the same bits (crop: (h, w), the part of the morphology planes to compare)"""
    for key in a:
        xs, ys = (a[key], b[key]) if isinstance(a[key], list) else ([a[key]], [b[key]])
        for i, (x, y) in enumerate(zip(xs, ys)):
            x, y = x[sa], y[sb]
            if crop is not None and key == "morph":
                x, y = x[..., :crop[0], :crop[1]], y[..., :crop[0], :crop[1]]
            assert np.array_equal(x, y, equal_nan=True), "%s: %s[%d] differs" % (what, key, i)


def _outside(shapes, H, W):
    sh = np.asarray(shapes)
    return ((np.arange(H)[None, :, None] >= sh[:, 0, None, None]) | (np.arange(W)[None, None, :] >= sh[:, 1, None, None]))[:, None]


def _compare(b, data, iters, test, e_rel=0.0, approximate_L=False, switches=None):
    """every scene of the fitted batch against lowres_common.fit of that scene alone"""
    st = _state(b)
    assert not st["status"].any(), st["status"]
    errors = []
    for s, d in enumerate(data):
        sc = fc.oracle_fit(d, iters, e_rel=e_rel, approximate_L=approximate_L, switches=None if switches is None else switches[s])
        n, (h, w) = len(d["sed0"]), d["morph0"].shape[1:]
        sed, morph = b.scene(s)
        sed, morph = sed.cpu().numpy(), morph.cpu().numpy()
        assert sed.shape == (n, d["C"]) and morph.shape == (n, h, w)
        e = dict(sed=rel_err(sed, np.array([c.sed for c in sc.sources])), morph=rel_err(morph, np.array([c.morph for c in sc.sources])),
                 mse=rel_err(b.mse(s), sc.mse))
        print("%s scene %d %s: %s" % (test, s, (h, w), {k: "%.2e" % v for k, v in e.items()}))
        errors.append(e)
        assert int(st["it"][s]) == sc.it, (s, st["it"][s], sc.it)
        np.testing.assert_array_equal(st["cen"][s, :n], np.array([c.center for c in sc.sources]))
        np.testing.assert_array_equal(st["flags"][s, :n], np.array([c.flags for c in sc.sources]))
        cur = st["cur"][s]
        assert not st["sed"][cur][s, n:].any() and not st["morph"][cur][s, n:].any()
    for s, e in enumerate(errors):
        assert max(e.values()) <= TOL, "%s scene %d: %s" % (test, s, e)
    return st


# ------------------------------------------------------------------ 1 - 4, 11: every scene against its own fit
@pytest.mark.parametrize("mixed", [False, True], ids=["batch_switches", "per_component"])
def test_small(scarlet, mixed):
    data = fc.scene_data("small")
    sw = SWITCHES["small"] if mixed else None
    b = _batch(scarlet, data, switches=sw)
    assert b.fit(5, e_rel=0) == 5
    b.raise_on_status()
    st = _compare(b, data, 5, "small" + (" per component" if mixed else ""), switches=sw)
    assert (st["it"] == 5).all()


def test_small_approximate_L(scarlet):
    data = fc.scene_data("small")
    b = _batch(scarlet, data)
    assert b.fit(5, e_rel=0, approximate_L=True) == 5
    _compare(b, data, 5, "small approximate_L", approximate_L=True)


def test_small_to_convergence(scarlet):
    data = fc.scene_data("small")
    b = _batch(scarlet, data, mse_capacity=128)
    b.fit(120, e_rel=1e-3, check_every=10)
    b.raise_on_status()
    st = _compare(b, data, 120, "small converged", e_rel=1e-3)
    print("iterations:", st["it"].tolist())
    assert (st["it"] < 120).all() and len(set(st["it"].tolist())) > 1          # every scene stopped on its own


def test_small_streamed(scarlet):
    data = fc.scene_data("small")
    with ll.options(LOWRES_STREAMED=1):
        b = _batch(scarlet, data)
        assert b.fit(5, e_rel=0) == 5
        _compare(b, data, 5, "small LOWRES_STREAMED")


def test_streamed_as_it_comes(scarlet):
    data = fc.scene_data("streamed")
    b = _batch(scarlet, data)
    assert b.fit(2, e_rel=0) == 2
    _compare(b, data, 2, "streamed")


def test_lds_edge(scarlet):
    """B = 8 beside 3 same-grid bands: C = 11, the wide entry points.  The LDS layout comes from the maxima
    (64, 64, 36, 36, 19, 37), which no one scene holds."""
    data = fc.scene_data("lds_edge")
    assert data[0]["C"] == 11
    b = _batch(scarlet, data)
    assert b.fit(2, e_rel=0) == 2
    _compare(b, data, 2, "lds_edge")


def test_wide_with_the_low_resolution_observation_at_band0_8(scarlet):
    data = fc.scene_data("small", hi_bands=8)
    assert data[0]["C"] == 10 and data[0]["lo_band0"] == 8
    b = _batch(scarlet, data)
    assert b._wide and b.fit(2, e_rel=0) == 2
    _compare(b, data, 2, "small wide")


# ------------------------------------------------------------------ 5. outside pixels
@pytest.mark.parametrize("form", ["as_it_comes", "streamed"])
def test_outside_pixels_are_zero(scarlet, form):
    data = fc.scene_data("small")
    with ll.options(LOWRES_STREAMED=int(form == "streamed")):
        b = _batch(scarlet, data)
        b.fit(3, e_rel=0)
        p = b.products()
        torch.cuda.synchronize()
    frames = [d["morph0"].shape[1:] for d in data]
    out = _outside(frames, b.H, b.W)
    for i in range(2):
        m = b.morph[i].cpu().numpy()
        assert not m[np.broadcast_to(out, m.shape)].any(), "morph[%d] outside the model frames" % i
    model = p.model.cpu().numpy()
    assert not model[np.broadcast_to(out, model.shape)].any()
    lo_out = _outside([d["images_lo"].shape[1:] for d in data], *p.rendered[1].shape[2:])
    for name in ("rendered", "residual"):
        x = getattr(p, name)[1].cpu().numpy()
        assert x.shape == (5, 2, 16, 16)
        assert not x[np.broadcast_to(lo_out, x.shape)].any(), name
        assert x[~np.broadcast_to(lo_out, x.shape)].any()


# ------------------------------------------------------------------ 6. full-size scenes: the uniform batch's bits
@pytest.mark.parametrize("form", ["as_it_comes", "streamed"])
def test_full_size_scenes_give_the_uniform_batch(scarlet, form):
    d0 = fc.scene_data("small")[0]
    S = 3
    data = [dict(d0, images_hi=d0["images_hi"] * (1 + 0.1 * s), images_lo=d0["images_lo"] * (1 + 0.1 * s)) for s in range(S)]
    with ll.options(LOWRES_STREAMED=int(form == "streamed")):
        ragged = _batch(scarlet, data)
        hi = scarlet.ObservationBatch(np.stack([d["images_hi"] for d in data]), band0=0).set_diff_kernel(fc.diff_kernel())
        lo = scarlet.LowResObservationBatch(np.stack([d["images_lo"] for d in data]), band0=3, geometry=[d0["geo"]] * S,
                                            weights=np.stack([d["weights_lo"] for d in data]))
        uniform = scarlet.BlendBatch.from_observations([hi, lo], [d["centers"] for d in data], centroid_weight=fc.model_psf()[0],
                                                       mse_capacity=64)
        uniform.set_state(*_pad_state(data, 32, 32))
        assert ragged.frame_shapes is not None and uniform.frame_shapes is None
        ragged.fit(4, e_rel=0)
        uniform.fit(4, e_rel=0)
    _same(_state(uniform), _state(ragged), "full-size ragged against uniform (%s)" % form)


# ------------------------------------------------------------------ 7. position in the batch
def test_a_scene_gives_the_same_bits_wherever_it_sits(scarlet):
    d = fc.scene_data("small")
    first, last = _batch(scarlet, [d[2], d[0], d[3]]), _batch(scarlet, [d[0], d[3], d[2]])
    first.fit(4, e_rel=0)
    last.fit(4, e_rel=0)
    assert (first.H, first.W) == (last.H, last.W)
    _same(_state(first), _state(last), "scene 2 at index 0 and at the last index", sa=slice(0, 1), sb=slice(2, 3))


# ------------------------------------------------------------------ 8. bad rows of the device table
@pytest.mark.parametrize("form", ["as_it_comes", "streamed"])
@pytest.mark.parametrize("row", ["outside", "disagrees"])
def test_a_bad_dims_row_marks_its_scene_and_nothing_else(scarlet, row, form):
    """bad input to a checked path: the device check marks the scene before any kernel reads a plane, and the kernels
    test the row again before it bounds a loop"""
    from scarlet_amd import _lib
    data = fc.scene_data("small")
    with ll.options(LOWRES_STREAMED=int(form == "streamed")):
        ref, b = _batch(scarlet, data), _batch(scarlet, data)
        dims = b._lowres[1][1]["dims"]
        if row == "outside":
            dims[1, 2] = 1000                   # h_s far beyond the padded block
        else:
            dims[1, 0] -= 1                     # H_s is not frame_hw's
        before = _state(b)
        ref.fit(3, e_rel=0)
        b.fit(3, e_rel=0)
        p = b.products(model=False)
        torch.cuda.synchronize()
    st, want = _state(b), _state(ref)
    assert st["status"][1] & _lib.STATUS_BAD_FRAME and st["active"][1] == 0 and st["it"][1] == 0
    keep = np.array([0, 2, 3, 4])
    assert not st["status"][keep].any()
    for key in ("sed", "morph", "cur", "cen", "shifts", "flags", "mse", "lip"):
        xs, ys = (st[key], before[key]) if isinstance(st[key], list) else ([st[key]], [before[key]])
        for x, y in zip(xs, ys):
            assert np.array_equal(x[1], y[1], equal_nan=True), "the marked scene's %s changed" % key
    _same(want, st, "the other scenes beside a marked one", sa=keep, sb=keep)
    with pytest.raises(ValueError, match="scenes \\[1\\]"):
        b.raise_on_status()
    assert np.isfinite(p.loss[1].cpu().numpy()).all()


# ------------------------------------------------------------------ 9. products
@pytest.mark.parametrize("name,form", [("small", "as_it_comes"), ("small", "streamed"), ("streamed", "as_it_comes")])
def test_products_against_float64_on_the_scenes_own_factors(scarlet, name, form):
    data = fc.scene_data(name)
    with ll.options(LOWRES_STREAMED=int(form == "streamed")):
        b, twin = _batch(scarlet, data), _batch(scarlet, data)
        b.fit(2, e_rel=0)
        twin.fit(2, e_rel=0)
        p = b.products()
        again = b.products(model=False, flux=False)
        b.fit(2, e_rel=0)
        twin.fit(2, e_rel=0)
        torch.cuda.synchronize()
    _same(_state(twin), _state(b), "a fit continued after products()")
    assert np.array_equal(p.loss[1].cpu().numpy(), again.loss[1].cpu().numpy())
    assert np.array_equal(p.rendered[1].cpu().numpy(), again.rendered[1].cpu().numpy())
    # against the state as it was when products() ran: the twin's, two iterations earlier -- recomputed from a third batch
    with ll.options(LOWRES_STREAMED=int(form == "streamed")):
        c = _batch(scarlet, data)
        c.fit(2, e_rel=0)
        torch.cuda.synchronize()
    rendered, residual, loss = (x[1].cpu().numpy() for x in (p.rendered, p.residual, p.loss))
    for s, d in enumerate(data):
        sed, morph = (x.cpu().numpy().astype(np.float64) for x in c.scene(s))
        model = np.einsum("kc,kyx->cyx", sed, morph)
        want = lc.apply_by_matmul(d["geo"].factors, model[d["lo_band0"]:])
        h, w = d["images_lo"].shape[1:]
        e = dict(rendered=rel_err(rendered[s, :, :h, :w], want), residual=rel_err(residual[s, :, :h, :w], d["images_lo"] - want),
                 loss=rel_err(loss[s], 0.5 * ((d["weights_lo"].astype(np.float64) * (want - d["images_lo"])) ** 2).sum(axis=(1, 2))))
        print("products %s %s scene %d: %s" % (name, form, s, {k: "%.2e" % v for k, v in e.items()}))
        assert max(e.values()) <= TOL, (s, e)
    # the shortcuts run on such a batch
    total = b.get_loss().cpu().numpy()
    assert total.shape == (len(data),) and np.isfinite(total).all()
    assert tuple(b.render(1).shape) == tuple(p.rendered[1].shape) == tuple(b.residual(1).shape)


# ------------------------------------------------------------------ 10. init_combined
def test_init_combined_gives_every_scene_its_one_scene_start(scarlet):
    data = fc.scene_data("small")
    b = _batch(scarlet, data, start=False)
    bg = [np.full(3, 0.02, np.float32), np.full(2, 0.02, np.float32)]
    psfs = [fc.hi_psfs(3), lc.limit_psfs(fc.PSF_PX, 2)[1]]
    b.init_combined(bg, obs_psfs=psfs, model_psf=fc.model_psf()[0])
    b.raise_on_status()
    torch.cuda.synchronize()
    frames = [d["morph0"].shape[1:] for d in data]
    out = _outside(frames, b.H, b.W)
    for i in range(2):
        m = b.morph[i].cpu().numpy()
        assert not m[np.broadcast_to(out, m.shape)].any()
    for s, d in enumerate(data):
        hi = scarlet.ObservationBatch(d["images_hi"][None], band0=0).set_diff_kernel(fc.diff_kernel())
        lo = scarlet.LowResObservationBatch(d["images_lo"][None], band0=3, geometry=d["geo"], weights=d["weights_lo"][None])
        one = scarlet.BlendBatch.from_observations([hi, lo], d["centers"][None], centroid_weight=fc.model_psf()[0])
        one.init_combined(bg, obs_psfs=psfs, model_psf=fc.model_psf()[0])
        sed, morph = (x.cpu().numpy() for x in b.scene(s))
        want_sed, want_morph = (x.cpu().numpy() for x in one.scene(0))
        # the low-resolution channels are the observation's pixel under the centre through the scene's own geometry
        assert np.array_equal(sed[:, 3:], want_sed[:, 3:]) and want_sed[:, 3:].any(), s
        assert rel_err(sed, want_sed) <= TOL and rel_err(morph, want_morph) <= TOL, s
    assert b.fit(2, e_rel=0) == 2
    b.raise_on_status()
