"""GPU: the products of a batch that holds a LOW-RESOLUTION observation (BlendBatch.products / render / residual /
get_loss of a batch made with from_observations(..., lowres_products=True), scarlet_observations_products_lowres;
lowres.h k_lowres_products and the streamed chain of lowres_stream.h):
the rendered model on the observation's own pixel grid, the residual and the per-band loss against the reference's
outputs (tests/golden/lowres.npz) and against float64 on the state read back from the device, to the project's 1e-5
max-norm relative (losses relative to the loss); the bit identities with scarlet_lowres_render_large, the switches and
repeated calls; and that the call is read-only, evaluates scenes of every kind and keeps a scene's NaN to itself.
Every test but the one on the next step's `mse` runs in both forms: as the shape comes, and under LOWRES_STREAMED=1.
S = 3 scenes."""
import ctypes

import numpy as np
import pytest

import lowres_common as lc
import lowres_large_common as ll
import products_common as pc
from conftest import rel_err
from parity_common import TOL

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

S = 3
PHASES = ((0.0, 0.0), (0.3, -0.4), (-0.2, 0.45))      # sub-pixel cuts of the three scenes, model pixels (y, x)
OBSERVED = ("rendered", "residual", "loss")


@pytest.fixture(scope="module")
def scarlet():
    import scarlet_amd
    scarlet_amd._lib.require_gpu()
    return scarlet_amd


@pytest.fixture(scope="module")
def g():
    return lc.fixture()


@pytest.fixture(params=["as_it_comes", "streamed"])
def form(request):
    """both forms: the one the shape takes by itself, and the streamed chain forced"""
    if request.param == "as_it_comes":
        yield request.param
        return
    with ll.options(LOWRES_STREAMED=1):
        yield request.param


# ---- the joint batches of tests/test_gpu_lowres.py (its helpers, copied)
def _scenes(g, name, per_scene=False):
    obs, (sed0, morph0, cen0), cw, lo = lc.fit_inputs(g, name)
    if per_scene:
        base = tuple(g[name + "_origin"])
        lo = [lc.geometry(g, name, model_channels=lc.CH5, channels=lc.CH5[3:], images=g[name + "_fit_images_lr"].copy(),
                          origin=(base[0] + 0.5 + dy, base[1] + 0.5 + dx))[0] for dy, dx in PHASES]
    rng = np.random.default_rng(21)
    hr = np.stack([obs[0]["images"] + (0.02 * rng.standard_normal(obs[0]["images"].shape) if s else 0) for s in range(S)])
    lr = np.stack([obs[1]["images"] + (0.02 * rng.standard_normal(obs[1]["images"].shape) if s else 0) for s in range(S)])
    wl = np.stack([obs[1]["weights"] * (1 + 0.2 * s) for s in range(S)])
    sed = np.stack([sed0 * (1 + 0.1 * s) for s in range(S)])
    morph = np.stack([morph0 for s in range(S)])
    cen = np.stack([cen0 for s in range(S)])
    return (hr.astype(np.float32), lr.astype(np.float32), wl.astype(np.float32), sed.astype(np.float32),
            morph.astype(np.float32), cen, obs, cw, lo)


def _batch(scarlet, g, name, counts=None, per_scene=False):
    hr, lr, wl, sed, morph, cen, obs, cw, lo = _scenes(g, name, per_scene)
    hi_b = scarlet.ObservationBatch(hr, band0=0).set_diff_kernel(obs[0]["diff_kernel"])
    lo_b = scarlet.LowResObservationBatch(lr, band0=3, geometry=lo, weights=wl)
    centers = cen if counts is None else [cen[s, :counts[s]] for s in range(S)]
    b = scarlet.BlendBatch.from_observations([hi_b, lo_b], centers, centroid_weight=cw, lowres_products=True)
    b.set_state(sed, morph)
    geos = lo if per_scene else [lo] * S
    return b, dict(hr=hr, lr=lr, wl=wl, diff=obs[0]["diff_kernel"], factors=[x.factors for x in geos])


def lowres_reference(sed, morph, factors, band0, images, weights):
    """float64 rendered / residual / loss of ONE scene's low-resolution observation: the operator as matrix products
    (lowres_common.apply_by_matmul) on the float64 model of sed (K, C) and morph (K, H, W)"""
    B = images.shape[0]
    sed, morph = np.asarray(sed, np.float64), np.asarray(morph, np.float64)
    model = np.einsum("kc,kyx->cyx", sed[:, band0:band0 + B], morph)
    rendered = lc.apply_by_matmul(factors, model)
    images = np.asarray(images, np.float64)
    d = np.asarray(weights, np.float64) * (rendered - images)
    return dict(rendered=rendered, residual=images - rendered, loss=0.5 * (d ** 2).sum(axis=(1, 2)))


def check_lowres(p, i, b, factors, band0, images, weights, where):
    """observation i of the products p against float64 on the batch's own state, scene by scene"""
    sed, morph = pc.state(b)
    got = dict(rendered=p.rendered[i], residual=p.residual[i], loss=p.loss[i])
    worst = {}
    for s in range(b.S):
        w = weights if np.ndim(weights) == 0 else weights[s]
        e = pc.check_scene(got, s, lowres_reference(sed[s], morph[s], factors[s], band0, images[s], w), OBSERVED, where=where)
        worst = {k: max(v, worst.get(k, 0)) for k, v in e.items()}
    print("%s worst: %s" % (where, {k: "%.2e" % v for k, v in worst.items()}))


# ---- 1. the reference's own numbers
def test_reference_fixture(scarlet, g, form):
    """lowres.npz, geometry b: one scene per model of the fixture; K = B components with one-hot SEDs and the model's
    planes as morphologies, so that the model IS b_models[i]"""
    geo, _ = lc.geometry(g, "b")
    models = np.asarray(g["b_models"], dtype=np.float32)                # (n, B, H, W)
    n, B = models.shape[:2]
    h, w = geo.frame.shape[1:]
    images = np.broadcast_to(g["b_images_lr"].astype(np.float32), (n, B, h, w)).copy()
    weights = np.broadcast_to(g["b_weights_lr"].astype(np.float32), (n, B, h, w)).copy()
    lo_b = scarlet.LowResObservationBatch(images, band0=0, geometry=geo, weights=weights)
    b = scarlet.BlendBatch.from_observations([lo_b], np.zeros((n, B, 2), np.int32), symmetric=False, monotonic=False,
                                             lowres_products=True)
    b.set_state(np.broadcast_to(np.eye(B, dtype=np.float32), (n, B, B)), models)
    assert np.array_equal(pc.npy(b.get_model()), models)
    rendered, loss = pc.npy(b.render(obs=0)), pc.npy(b.get_loss())
    assert rendered.shape == (n, B, h, w) and loss.shape == (n,)
    for i in range(n):
        e_render = rel_err(rendered[i], g["b_renders"][i])
        e_loss = abs(loss[i] - g["b_losses"][i]) / g["b_losses"][i]
        print("%s model %d: rendered %.2e loss %.2e" % (form, i, e_render, e_loss))
        assert e_render <= TOL and e_loss <= TOL


# ---- 2. float64 on the state read back
@pytest.mark.parametrize("name,counts,per_scene", [("a", None, False), ("b", None, False), ("b", [2, 1, 2], False),
                                                   ("a", None, True)], ids=["a", "b", "b_ragged", "a_per_scene"])
def test_products_of_a_joint_fit_match_float64(scarlet, g, form, name, counts, per_scene):
    b, data = _batch(scarlet, g, name, counts, per_scene)
    assert b.fit(10, e_rel=0) == 10
    b.raise_on_status()
    p = b.products()
    h, w = data["lr"].shape[2:]
    assert [tuple(x.shape) for x in p.rendered] == [(S, 3) + data["hr"].shape[2:], (S, 2, h, w)]
    assert [tuple(x.shape) for x in p.loss] == [(S, 3), (S, 2)]
    where = "%s %s" % (form, name)
    check_lowres(p, 1, b, data["factors"], 3, data["lr"], data["wl"], where + " low-resolution")
    sed, morph = pc.state(b)
    for s in range(S):
        whole = pc.reference(sed[s], morph[s], np.zeros((5,) + morph.shape[-2:]))
        pc.check_scene(p, s, whole, ("model", "flux"), where=where + " state")
        ref = pc.reference(sed[s][:, :3], morph[s], data["hr"][s], 1.0, data["diff"])
        got = dict(rendered=p.rendered[0], residual=p.residual[0], loss=p.loss[0])
        pc.check_scene(got, s, ref, OBSERVED, where=where + " model grid")
    assert torch.equal(b.render(obs=1), p.rendered[1]) and torch.equal(b.residual(obs=1), p.residual[1])
    only = b.products(model=False, flux=False, obs=[1])
    assert only.rendered[0] is None and torch.equal(only.loss[1], p.loss[1]) and torch.equal(only.rendered[1], p.rendered[1])
    assert torch.equal(b.get_loss(), p.loss[0].sum(dim=1) + p.loss[1].sum(dim=1))


# ---- 3. the kernels' limits
def _limit_batch(scarlet, name, band0, C, K=3, counts=None, seed=31):
    """a joint batch on a LIMITS / LARGE geometry with random factors: a same-grid observation over all C channels and
    the low-resolution one over band0 .. band0 + B - 1"""
    B = ll.spec(name)[5]
    geo, _ = ll.geometry(name, B=B, band0=band0, C=C)
    (H, W), (h, w) = geo.model_shape, geo.frame.shape[1:]
    rng = np.random.default_rng(seed)
    hr, centers, sed, morph = pc.synthetic(seed, S, K, C, H, W)
    lr = rng.random((S, B, h, w)).astype(np.float32)
    wl = (0.5 + rng.random((S, B, h, w))).astype(np.float32)
    lo_b = scarlet.LowResObservationBatch(lr, band0=band0, geometry=geo, weights=wl)
    cen = centers if counts is None else [centers[s, :counts[s]] for s in range(S)]
    b = scarlet.BlendBatch.from_observations([scarlet.ObservationBatch(hr, band0=0), lo_b], cen, symmetric=False, monotonic=False,
                                             lowres_products=True)
    b.set_state(sed, morph)
    return b, dict(hr=hr, lr=lr, wl=wl, factors=[geo.factors] * S, band0=band0, dims=ll.dims(geo))


@pytest.mark.parametrize("name,band0,C", [("j", 1, 5), ("d", 0, 8), ("p", 1, 5)], ids=["j_off_tiles", "d_lds_optin", "p_past_lds"])
def test_kernel_limits(scarlet, form, name, band0, C):
    """j: 17 x 23 / 5 x 7 at B = 3, every GEMM dimension off 16 and off 4; d: 64 x 64 at B = 8, dynamic LDS in the opt-in
    range; p: 96 x 96 at B = 3, which does not fit LDS (streamed in both runs).  band0 > 0 and C > B where B allows it;
    a ragged batch at j"""
    b, data = _limit_batch(scarlet, name, band0, C, counts=[3, 1, 2] if name == "j" else None)
    p = b.products()
    check_lowres(p, 1, b, data["factors"], band0, data["lr"], data["wl"], "%s limits %s" % (form, name))
    # without the state's `model` output the streamed form takes its band models from k_lrs_model: the same bits
    q = b.products(model=False, flux=False, obs=[1])
    for k in OBSERVED:
        assert torch.equal(getattr(q, k)[1], getattr(p, k)[1]), k
    # the form each run took: only the streamed one asks for scratch
    from scarlet_amd import _lib
    out = _lib.ScarletProducts()
    out.rendered = _lib.ptr(p.rendered[1])
    nbytes = _lib.lib.scarlet_lowres_products_scratch_bytes(ctypes.byref(b._c), ctypes.byref(b._observations[1][1]._c),
                                                            ctypes.byref(b._lowres[1][0]), ctypes.byref(out))
    assert (nbytes > 0) == (form == "streamed" or name == "p") and b._scratch.numel() >= nbytes


# ---- 4. bit identities
def _render_large(b, i, model):
    """scarlet_lowres_render_large on the channel slice of observation i of `model` (S, C, H, W) -> (S, B, h, w)"""
    from scarlet_amd import _lib
    o, ob = b._observations[i]
    lr = b._lowres[i][0]
    planes = model[:, o.band0:o.band0 + o.B].contiguous()
    n = b.S * o.B
    band = torch.arange(o.B, dtype=torch.int32, device="cuda").repeat(b.S)
    scene = torch.arange(b.S, dtype=torch.int32, device="cuda").repeat_interleave(o.B)
    out = torch.empty((b.S, o.B) + tuple(o.shape[2:]), dtype=torch.float32, device="cuda")
    nbytes = int(_lib.check(_lib.lib.scarlet_lowres_op_scratch_bytes(n, b.H, b.W, ctypes.byref(lr))))
    scratch = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib.scarlet_lowres_render_large(planes.data_ptr(), n, b.H, b.W, ctypes.byref(lr), band.data_ptr(),
                                                    scene.data_ptr(), out.data_ptr(), scratch.data_ptr(), nbytes,
                                                    _lib.stream_ptr()))
    return out


def _same_bits(p, q, names=OBSERVED, obs=1):
    for k in names:
        assert torch.equal(getattr(p, k)[obs], getattr(q, k)[obs]), k


@pytest.mark.parametrize("name", ["b", "p"])
def test_bit_identities(scarlet, g, form, name):
    """b: the fixture's joint batch (6 band planes); p: 96 x 96, past LDS"""
    if name == "b":
        b, _ = _batch(scarlet, g, "b", counts=[2, 1, 2])
        b.fit(3, e_rel=0)
    else:
        b, _ = _limit_batch(scarlet, "p", 1, 5)
    p = b.products()
    assert torch.equal(p.rendered[1], _render_large(b, 1, p.model))
    keep = [p.loss[1].clone(), p.rendered[1].clone(), p.residual[1].clone()]
    with ll.options(NO_LOWRES_MFMA=1):
        _same_bits(b.products(), p)
    with ll.options(LOWRES_CHUNK=5):                     # 6 (b) or 9 (p) planes: a ragged last chunk
        _same_bits(b.products(), p)
        _same_bits(b.products(model=False, flux=False), p)
    _same_bits(b.products(), p)                          # two calls
    ptrs = [x.data_ptr() for x in (p.loss[1], p.rendered[1], p.residual[1])]
    q = b.products(out=p)                                # out= reuse: the same tensors, the same bits
    assert q is p and ptrs == [x.data_ptr() for x in (p.loss[1], p.rendered[1], p.residual[1])]
    for x, y in zip(keep, (p.loss[1], p.rendered[1], p.residual[1])):
        assert torch.equal(x, y)


def test_all_null_list_is_scarlet_observations_products(scarlet, form):
    from scarlet_amd import _lib
    images, centers, sed, morph = pc.synthetic(41, S, 3, 5, 30, 34)
    b = scarlet.BlendBatch.from_observations([scarlet.ObservationBatch(images[:, :3], band0=0),
                                              scarlet.ObservationBatch(images[:, 3:], band0=3)], centers,
                                             symmetric=False, monotonic=False)
    b.set_state(sed, morph)
    ref = b.products()
    n = 2
    outs = (_lib.ScarletProducts * n)()
    new = {k: [torch.full_like(getattr(ref, k)[i], 7) for i in range(n)] for k in OBSERVED}
    for i in range(n):
        for k in OBSERVED:
            setattr(outs[i], k, _lib.ptr(new[k][i]))
    ps = _lib.ScarletProducts()
    model, flux = torch.full_like(ref.model, 7), torch.full_like(ref.flux, 7)
    ps.model, ps.flux = _lib.ptr(model), _lib.ptr(flux)
    ptrs = (ctypes.POINTER(_lib.ScarletBatch) * n)(*[ctypes.pointer(ob._c) for _, ob in b._observations])
    lows = (ctypes.POINTER(_lib.ScarletLowres) * n)()        # every entry NULL
    band0 = np.array([0, 3], dtype=np.int32)
    scratch = torch.empty((1 << 20,), dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib.scarlet_observations_products_lowres(
        ctypes.byref(b._c), ptrs, lows, band0.ctypes.data_as(ctypes.c_void_p), n, ctypes.byref(ps), outs, scratch.data_ptr(),
        scratch.numel(), _lib.stream_ptr()))
    assert torch.equal(model, ref.model) and torch.equal(flux, ref.flux)
    for i in range(n):
        for k in OBSERVED:
            assert torch.equal(new[k][i], getattr(ref, k)[i]), (k, i)


# ---- 5. read-only
def _bits(t):
    return t.clone().view(torch.uint8) if t.is_floating_point() else t.clone()


def test_read_only(scarlet, g, form):
    def start():
        b, _ = _batch(scarlet, g, "a")
        b.fit(4, e_rel=0)
        return b

    b = start()
    watched = dict(sed0=b.sed[0], sed1=b.sed[1], morph0=b.morph[0], morph1=b.morph[1], cur=b.cur, it=b.it, flags=b.flags,
                   lipschitz=b.lipschitz, active=b.active, status=b.status, mse=b.mse_buf, centers=b.centers, shifts=b.shifts,
                   workspace=b.workspace, lowres_workspace=b._lowres[1][1]["workspace"],
                   hr_workspace=b._observations[0][1].workspace)
    before = {k: _bits(v) for k, v in watched.items()}
    b.products()
    b.get_loss()
    for k, v in watched.items():
        assert torch.equal(_bits(v), before[k]), k
    # four iterations after the call: the bits of eight iterations without it
    b.fit(4, e_rel=0)
    c, _ = _batch(scarlet, g, "a")
    c.fit(8, e_rel=0)
    for k, x, y in (("sed", b.sed_current, c.sed_current), ("morph", b.morph_current, c.morph_current), ("mse", b.mse_buf, c.mse_buf),
                    ("centers", b.centers, c.centers), ("flags", b.flags, c.flags), ("lipschitz", b.lipschitz, c.lipschitz)):
        assert torch.equal(x, y), k


def test_batches_made_without_the_keyword_behave_as_before(scarlet, g):
    """from_observations without lowres_products: the low-resolution products raise as they always did, the rest is
    there, and the fit is the same to the bit"""
    hr, lr, wl, sed, morph, cen, obs, cw, lo = _scenes(g, "a")
    hi_b = scarlet.ObservationBatch(hr, band0=0).set_diff_kernel(obs[0]["diff_kernel"])
    lo_b = scarlet.LowResObservationBatch(lr, band0=3, geometry=lo, weights=wl)
    old = scarlet.BlendBatch.from_observations([hi_b, lo_b], cen, centroid_weight=cw)
    old.set_state(sed, morph)
    new, _ = _batch(scarlet, g, "a")
    old.fit(3, e_rel=0)
    new.fit(3, e_rel=0)
    for call in (old.products, old.get_loss, lambda: old.render(obs=1), lambda: old.residual(obs=1)):
        with pytest.raises(NotImplementedError, match="lowres_products"):
            call()
    p, q = old.products(obs=[0]), new.products()
    assert torch.equal(p.rendered[0], q.rendered[0]) and torch.equal(p.loss[0], q.loss[0]) and p.rendered[1] is None
    assert torch.equal(old.get_model(), q.model) and torch.equal(old.get_flux(), q.flux)
    assert torch.equal(old.morph_current, new.morph_current) and torch.equal(old.mse_buf, new.mse_buf)


# ---- 6. the loss is what the next step records (as tests/test_gpu_products.py states it)
def test_loss_is_what_the_next_step_records(scarlet, g):
    b, _ = _batch(scarlet, g, "b")
    b.fit(5, e_rel=0)
    loss, it0 = pc.npy(b.get_loss()), pc.npy(b.it)
    b.active.fill_(1)
    b.step()
    mse = pc.npy(b.mse_buf)
    assert (pc.npy(b.it) == it0 + 1).all()
    for s in range(b.S):
        e = abs(loss[s] - mse[s, it0[s]]) / mse[s, it0[s]]
        print("scene %d: get_loss %.9g, next mse %.9g (%.2e)" % (s, loss[s], mse[s, it0[s]], e))
        assert e <= TOL


# ---- 7. scenes of every kind
def test_inactive_scenes_and_both_buffers(scarlet, g, form):
    """scene 1 never iterates (inactive, it == 0, buffer 0); scene 2 stops after two iterations (buffer 0), scene 0 after
    three (buffer 1): every one is evaluated, from its own buffer"""
    b, data = _batch(scarlet, g, "a")
    b._ensure_mse_capacity(4)
    b.active[1] = 0
    for it in range(3):
        if it == 2:
            b.active[2] = 0
        b.step(e_rel=0)
    it, cur, active = pc.npy(b.it), pc.npy(b.cur), pc.npy(b.active)
    print("iterations", it.tolist(), "cur", cur.tolist(), "active", active.tolist())
    assert it.tolist() == [3, 0, 2] and set(cur.tolist()) == {0, 1} and (cur == it % 2).all() and active.tolist() == [1, 0, 0]
    assert not torch.equal(b.morph[0][0], b.morph[1][0])          # (the buffer matters)
    p = b.products()
    check_lowres(p, 1, b, data["factors"], 3, data["lr"], data["wl"], "%s mixed scenes" % form)
    assert it.tolist() == pc.npy(b.it).tolist() and active.tolist() == pc.npy(b.active).tolist()


def test_nan_stays_in_its_scene(scarlet, g, form):
    b, _ = _batch(scarlet, g, "b")
    b.fit(2, e_rel=0)
    good = b.products()
    cur = int(b.cur[1].item())
    b.sed[cur][1, 0, 4] = float("nan")                   # a channel of the low-resolution observation, scene 1
    nan = b.products()
    others = [0, 2]
    for k in OBSERVED:
        x, y = getattr(good, k)[1], getattr(nan, k)[1]
        assert torch.equal(x[others], y[others]), k
        assert bool(torch.isnan(y[1]).any()), k
    assert bool(torch.isnan(nan.rendered[1][1, 1]).all()) and not bool(torch.isnan(nan.rendered[1][1, 0]).any())
