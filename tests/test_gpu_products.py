"""GPU: BlendBatch.products (scarlet_batch_products / scarlet_observations_products) -- model, rendered model, residual,
per-band loss, fluxes and component models of a batch's state -- against the reference's own outputs
(tests/golden/grad.npz) and against float64 on the state read back from the device (tests/products_common.py), to the
project's 1e-5 max-norm relative per scene and per array; and that the call is read-only, reproducible to the bit and
keeps a scene's NaN to itself."""
import numpy as np
import pytest

import products_common as pc
from conftest import load_golden, rel_err
from parity_common import TOL

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ALL = ("model", "rendered", "residual", "loss", "flux")


@pytest.fixture(scope="module")
def scarlet():
    import scarlet_amd
    scarlet_amd._lib.require_gpu()
    return scarlet_amd


def check_batch(b, images, weights=None, diff=None, scenes=None, components=None, where=""):
    """every product of a single-observation batch against float64 on its own state"""
    sed, morph = pc.state(b)
    p = b.products(components=components)
    names = ALL + (("component_models",) if components is not None else ())
    for s in range(b.S) if scenes is None else scenes:
        w = 1.0 if weights is None else (weights if np.ndim(weights) == 0 else weights[s])
        d = None if diff is None else (diff if np.ndim(diff) == 3 else diff[s])
        pc.check_scene(p, s, pc.reference(sed[s], morph[s], images[s], w, d), names, components, where)
    return p


# ---- 1. the reference's own outputs
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("psf", [False, True], ids=["nopsf", "psf"])
def test_reference_fixture(scarlet, psf, weighted):
    """grad.npz: B = 3, K = 2, 21 x 25 (H W % 4 != 0; with the PSF the odd width takes the hipFFT chain)"""
    g = load_golden("grad")
    tag = ("psf" if psf else "nopsf") + ("_w" if weighted else "")
    images = g["images"].astype(np.float32)
    b = scarlet.BlendBatch(images[None], np.array([[[10, 12], [5, 6]]], dtype=np.int32),
                           weights=g["weights"].astype(np.float32)[None] if weighted else None, symmetric=False, monotonic=False)
    if psf:
        b.set_diff_kernel(g["diff_" + tag].astype(np.float32))
    b.set_state(g["seds"][None], g["morphs"][None])
    p = b.products()
    e_render = rel_err(pc.npy(p.rendered)[0], g["render_" + tag])
    e_loss = abs(float(p.loss.sum().item()) - float(g["loss_" + tag])) / float(g["loss_" + tag])
    print("%s: rendered %.2e loss %.2e" % (tag, e_render, e_loss))
    assert e_render <= TOL and e_loss <= TOL
    assert rel_err(float(b.get_loss()[0].item()), float(g["loss_" + tag])) <= TOL
    assert rel_err(pc.npy(b.render())[0], g["render_" + tag]) <= TOL


# ---- 2. final states of real fits
def test_final_states_of_the_synthetic_fits(scarlet):
    """fit_synth.npz: 5 x 64 x 64, K = 4, the shape of the fused iteration"""
    from scarlet_amd import synth
    g = load_golden("fit_synth")
    scenes = [synth.make_scene(i) for i in range(3)]
    images = np.stack([s["images"] for s in scenes])
    b = scarlet.BlendBatch(images, np.stack([s["centers"] for s in scenes]))
    pre = ["s%d_f32_" % i for i in range(3)]
    b.set_state(np.stack([g[p + "init_sed"] for p in pre]), np.stack([g[p + "init_morph"] for p in pre]),
                np.stack([g[p + "init_center"] for p in pre]), np.stack([g[p + "init_shift"] for p in pre]))
    b.fit(30, e_rel=0)
    assert rel_err(pc.npy(b.morph_current)[0], g["s0_f32_morph"]) <= TOL
    check_batch(b, images, components=[0, b.K - 1], where="fit_synth")


def test_final_state_of_the_hsc_fit(scarlet):
    """fit_hsc.npz: 5 x 58 x 48, PSF 43 x 43 (the LDS-resident transform)"""
    g, d = load_golden("fit_hsc"), load_golden("hsc_inputs")
    diff = g["diff_kernel"].astype(np.float32)
    b = scarlet.BlendBatch(d["images"][None], g["init_center_f32"][None].astype(np.int32), centroid_weight=g["model_psf"][0])
    b.set_diff_kernel(diff)
    b.set_state(g["init_sed_f32"][None], g["init_morph_f32"][None], shifts=g["init_shift_f32"][None])
    b.fit(50, e_rel=0)
    assert rel_err(pc.npy(b.morph_current)[0], g["morph_f32"]) <= TOL
    check_batch(b, d["images"][None], diff=diff, components=[0, b.K - 1], where="fit_hsc")


# ---- 3. scenes on different buffers
def _mixed_parity_fit(b, e_rel):
    b.fit(60, e_rel=e_rel, check_every=0)
    it, cur = pc.npy(b.it), pc.npy(b.cur)
    print("iterations", it.tolist(), "cur", cur.tolist())
    assert set(cur.tolist()) == {0, 1}, "the scenes must stop on both buffers: %s" % it.tolist()
    assert (cur == it % 2).all()


def _loss_is_what_the_next_step_records(b):
    loss, it0 = pc.npy(b.get_loss()), pc.npy(b.it)
    b.active.fill_(1)
    b.step()
    mse = pc.npy(b.mse_buf)
    assert (pc.npy(b.it) == it0 + 1).all()
    for s in range(b.S):
        e = abs(loss[s] - mse[s, it0[s]]) / mse[s, it0[s]]
        print("scene %d: get_loss %.9g, next mse %.9g (%.2e)" % (s, loss[s], mse[s, it0[s]], e))
        assert e <= TOL


@pytest.mark.parametrize("psf", [False, True], ids=["nopsf", "psf"])
def test_scenes_on_different_buffers(scarlet, psf):
    from parity_common import Workload
    wl = Workload(psf=psf)
    images, centers = wl.scenes(pc.MIXED_SEED[psf], 8)
    b = wl.batch(scarlet, images, centers, 64)
    _mixed_parity_fit(b, pc.MIXED_E_REL)
    check_batch(b, images, diff=wl.diff, where="mixed buffers")
    _loss_is_what_the_next_step_records(b)


def test_two_observations_on_different_buffers(scarlet):
    """band0 = 0 with 3 bands and band0 = 3 with 2 bands, the second with its own kernel"""
    from parity_common import Workload
    wl = Workload(psf=True)
    images, centers = wl.scenes(pc.MIXED_SEED["obs"], 8)
    diff = wl.diff[3:]
    obs = [scarlet.ObservationBatch(images[:, :3], band0=0), scarlet.ObservationBatch(images[:, 3:], band0=3).set_diff_kernel(diff)]
    b = scarlet.BlendBatch.from_observations(obs, centers, centroid_weight=wl.model_psf.astype(np.float32))
    b.init_combined([np.ones(3) * 0.1, np.ones(2) * 0.1], obs_psfs=[None, wl.obs_psfs[3:]], model_psf=wl.model_psf)
    _mixed_parity_fit(b, pc.MIXED_E_REL)
    sed, morph = pc.state(b)
    p = b.products(components=[1, 3])
    assert [tuple(x.shape) for x in p.rendered] == [(8, 3, 64, 64), (8, 2, 64, 64)] and tuple(p.model.shape) == (8, 5, 64, 64)
    for s in range(8):
        whole = pc.reference(sed[s], morph[s], images[s])
        pc.check_scene(p, s, whole, ("model", "flux", "component_models"), [1, 3], "state")
        for i, (band, d) in enumerate(((slice(0, 3), None), (slice(3, 5), diff))):
            ref = pc.reference(sed[s][:, band], morph[s], images[s, band], 1.0, d)
            got = dict(rendered=p.rendered[i], residual=p.residual[i], loss=p.loss[i])
            pc.check_scene(got, s, ref, ("rendered", "residual", "loss"), where="observation %d" % i)
    assert torch.equal(b.render(obs=1), p.rendered[1]) and torch.equal(b.residual(obs=0), p.residual[0])
    only = b.products(model=False, flux=False, obs=[1])
    assert only.rendered[0] is None and torch.equal(only.loss[1], p.loss[1])
    _loss_is_what_the_next_step_records(b)


# ---- 4. shapes where the kernels can go wrong
@pytest.mark.parametrize("K,B,H,W", [(256, 8, 16, 16), (33, 1, 24, 40), (3, 2, 7, 9)], ids=["K256", "K33_B1", "tiny_odd"])
def test_component_and_band_limits(scarlet, K, B, H, W):
    images, centers, sed, morph = pc.synthetic(11, 2, K, B, H, W)
    b = scarlet.BlendBatch(images, centers, symmetric=False, monotonic=False)
    b.set_state(sed, morph)
    check_batch(b, images, components=[K - 1, 0], where="K=%d B=%d" % (K, B))


def test_ragged_batch_and_zero_weights(scarlet):
    """n_components = [1, 3, 2]: absent rows are zeros; per-pixel weights with a block of zeros"""
    S, K, B, H, W = 3, 3, 4, 30, 34
    images, centers, sed, morph = pc.synthetic(12, S, K, B, H, W)
    weights = (0.5 + np.random.default_rng(2).random(images.shape)).astype(np.float32)
    weights[:, 1:, 5:17, 8:20] = 0
    counts = np.array([1, 3, 2], dtype=np.int32)
    b = scarlet.BlendBatch(images, centers, weights=weights, n_components=counts, symmetric=False, monotonic=False)
    b.set_state(sed, morph)
    p = check_batch(b, images, weights=weights, components=[2, 0, 1], where="ragged")
    flux, comp = pc.npy(p.flux), pc.npy(p.component_models)
    for s in range(S):
        assert not flux[s, counts[s]:].any()
        for j, k in enumerate([2, 0, 1]):
            assert (k < counts[s]) == bool(comp[s, j].any())


@pytest.mark.parametrize("H,W", [(32, 32), (21, 25)], ids=["lds", "hipfft"])
def test_per_scene_difference_kernels(scarlet, H, W):
    S, K, B = 3, 2, 3
    images, centers, sed, morph = pc.synthetic(13, S, K, B, H, W)
    diff = pc.kernels(14, (S, B, 11, 11))
    weights = (0.5 + np.random.default_rng(3).random(images.shape)).astype(np.float32)
    b = scarlet.BlendBatch(images, centers, weights=weights, symmetric=False, monotonic=False)
    b.set_diff_kernel(diff)
    b.set_state(sed, morph)
    check_batch(b, images, weights=weights, diff=diff, where="per-scene kernels %dx%d" % (H, W))
    # without a `model` output the unconvolved planes are staged in the scratch: the same bits
    full, part = b.products(), b.products(model=False)
    assert torch.equal(full.rendered, part.rendered) and torch.equal(full.loss, part.loss)


def test_every_tile_boundary_of_a_large_frame(scarlet):
    """one scene of 2 x 1024 x 1000, K = 2"""
    images, centers, sed, morph = pc.synthetic(15, 1, 2, 2, 1024, 1000)
    b = scarlet.BlendBatch(images, centers, symmetric=False, monotonic=False)
    b.set_state(sed, morph)
    check_batch(b, images, where="1024 x 1000")


@pytest.mark.parametrize("path", ["lds", "hipfft"])
def test_scenes_rendered_in_chunks(scarlet, path):
    """batches whose unconvolved planes (and hipFFT buffers) exceed 256 MiB are rendered in chunks of scenes: the scenes
    on both sides of every chunk boundary"""
    import ctypes
    from scarlet_amd import _lib
    S, K, B, side, P = (2100, 1, 8, 64, 11) if path == "lds" else (100, 1, 5, 200, 41)
    gen = torch.Generator(device="cuda").manual_seed(5)
    images = torch.rand((S, B, side, side), device="cuda", generator=gen)
    sed = 0.2 + torch.rand((S, K, B), device="cuda", generator=gen)
    morph = torch.rand((S, K, side, side), device="cuda", generator=gen)
    diff = pc.kernels(16, (B, P, P))
    b = scarlet.BlendBatch(images, np.full((S, K, 2), side // 2, np.int32), symmetric=False, monotonic=False)
    b.set_diff_kernel(diff)
    b.set_state(sed, morph)
    plan = np.zeros(16, np.int32)
    assert (_lib.lib.scarlet_debug_psf_plan(ctypes.byref(b._c), plan.ctypes.data) == 0) == (path == "lds")
    p = b.products(model=False, flux=False)
    per_scene = B * side * side * 4 if path == "lds" else B * (side * side * 4 + 240 * 240 * 4 + 240 * 121 * 8)
    chunk = (256 << 20) // per_scene
    assert S // 2 < chunk < S and b._scratch.numel() <= (256 << 20) + (1 << 20)
    sed, morph, images = pc.npy(sed), pc.npy(morph), pc.npy(images)
    for s in (0, chunk - 1, chunk, S - 1):
        pc.check_scene(p, s, pc.reference(sed[s], morph[s], images[s], 1.0, diff), ("rendered", "residual", "loss"), where=path)


# ---- 5. read-only and reproducible
def _bits(t):
    return t.clone().view(torch.uint8) if t.is_floating_point() else t.clone()


@pytest.mark.parametrize("psf", [False, True], ids=["nopsf", "psf"])
def test_read_only_and_reproducible(scarlet, psf):
    from parity_common import Workload
    wl = Workload(psf=psf, H=64, W=64)
    images, centers = wl.scenes(300, 6)

    def start():
        b = wl.batch(scarlet, images, centers, 32)
        b.fit(3, e_rel=0)
        return b

    b = start()
    watched = dict(sed0=b.sed[0], sed1=b.sed[1], morph0=b.morph[0], morph1=b.morph[1], cur=b.cur, it=b.it, flags=b.flags,
                   lipschitz=b.lipschitz, active=b.active, status=b.status, mse=b.mse_buf, centers=b.centers,
                   shifts=b.shifts, workspace=b.workspace)
    before = {k: _bits(v) for k, v in watched.items()}
    p1 = b.products(components=[0, 3])
    loss1, flux1 = p1.loss.clone(), p1.flux.clone()
    p2 = b.products(components=[0, 3], out=p1)
    assert p2 is p1 and torch.equal(p2.loss, loss1) and torch.equal(p2.flux, flux1)
    p3 = b.products()
    assert torch.equal(p3.loss, loss1) and torch.equal(p3.flux, flux1) and torch.equal(p3.residual, p1.residual)
    for k, v in watched.items():
        assert torch.equal(_bits(v), before[k]), k
    # ten iterations after the call: the bits of ten iterations without it
    b.fit(10, e_rel=0)
    c = start()
    c.fit(10, e_rel=0)
    for x, y in ((b.sed_current, c.sed_current), (b.morph_current, c.morph_current), (b.mse_buf, c.mse_buf), (b.it, c.it)):
        assert torch.equal(x, y)


# ---- 6. a scene's NaN stays its own
@pytest.mark.parametrize("psf", [False, True], ids=["nopsf", "psf"])
def test_nan_stays_in_its_scene(scarlet, psf):
    S, K, B, H, W = 4, 3, 5, 48, 40
    images, centers, sed, morph = pc.synthetic(17, S, K, B, H, W)
    diff = pc.kernels(18, (B, 9, 9)) if psf else None

    def run(m):
        b = scarlet.BlendBatch(images, centers, symmetric=False, monotonic=False)
        if psf:
            b.set_diff_kernel(diff)
        b.set_state(sed, m)
        return b.products(components=[0, 2])

    bad = morph.copy()
    bad[2] = np.nan
    good, nan = run(morph), run(bad)
    others = [0, 1, 3]
    for name in ALL + ("component_models",):
        x, y = getattr(good, name), getattr(nan, name)
        assert torch.equal(x[others], y[others]), name
        assert bool(torch.isnan(y[2]).any()), name


# ---- 7. limits
def test_low_resolution_observation_limits(scarlet):
    import lowres_common as lc
    g = lc.fixture()
    obs, (sed0, morph0, cen0), cw, lo = lc.fit_inputs(g, "a")
    hr = obs[0]["images"][None].astype(np.float32)
    hi_b = scarlet.ObservationBatch(hr, band0=0).set_diff_kernel(obs[0]["diff_kernel"])
    lo_b = scarlet.LowResObservationBatch(obs[1]["images"][None].astype(np.float32), band0=3, geometry=lo)
    b = scarlet.BlendBatch.from_observations([hi_b, lo_b], cen0[None], centroid_weight=cw)
    b.set_state(sed0[None].astype(np.float32), morph0[None].astype(np.float32))
    with pytest.raises(NotImplementedError):
        b.products()
    with pytest.raises(NotImplementedError):
        b.render(obs=1)
    with pytest.raises(NotImplementedError):
        b.get_loss()
    sed, morph = pc.state(b)
    whole = pc.reference(sed[0], morph[0], np.zeros((5,) + morph.shape[-2:]))
    assert rel_err(pc.npy(b.get_model())[0], whole["model"]) <= TOL
    assert rel_err(pc.npy(b.get_flux())[0], whole["flux"]) <= TOL
    # the observation on the model's grid is still there
    ref = pc.reference(sed[0][:, :3], morph[0], hr[0], 1.0, obs[0]["diff_kernel"])
    assert rel_err(pc.npy(b.render(obs=0))[0], ref["rendered"]) <= TOL
    assert rel_err(pc.npy(b.residual(obs=0))[0], ref["residual"]) <= TOL
