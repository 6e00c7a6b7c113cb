"""GPU: batches fitted jointly against several observations (BlendBatch.from_observations, scarlet_fit_observations)
against the CPU oracle (oracle.pgm: `scene.observations`, init_combined_extended_source), started from the device's own
initial state as in tests/parity_common.py: sed, morph and loss history to 1e-5 max-norm relative, centres and
iteration counts exactly."""
import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-5


def _scenes(first, n, B=5, H=64, W=64, K=4, psfs=None):
    from scarlet_amd import synth
    kw = dict(B=B, H=H, W=W, K=K)
    if psfs is not None:
        kw["psfs"] = psfs
    sc = [synth.make_scene(first + i, **kw) for i in range(n)]
    return np.stack([s["images"] for s in sc]), np.stack([s["centers"] for s in sc])


def _check(b, obs_data, n_iter, scenes, approximate_L=False, l0=None, counts=None):
    """obs_data: list of dicts (images (S, B, H, W), band0, weights None / scalar / (S, B, H, W), diff (B, P, P) or None).
    Copies the device state of `scenes`, fits n_iter iterations on the device and in the oracle, compares."""
    from oracle import pgm
    sed0, morph0 = b.sed_current.cpu().numpy(), b.morph_current.cpu().numpy()
    cen0, sh0 = b.centers.cpu().numpy(), b.shifts.cpu().numpy()
    assert b.fit(n_iter, e_rel=0, approximate_L=approximate_L) == n_iter
    b.raise_on_status()
    sed1, morph1 = b.sed_current.cpu().numpy(), b.morph_current.cpu().numpy()
    cen1, it1 = b.centers.cpu().numpy(), b.it.cpu().numpy()
    for s in scenes:
        n = b.K if counts is None else int(counts[s])
        C, H, W = b.B, b.H, b.W
        sh = None if np.isnan(sh0[s, :n]).any() else sh0[s, :n]     # (NaN: no centroid shift yet, as after init_combined)
        sc = pgm.scene_from_state(np.zeros((C, H, W), np.float32), sed0[s, :n], morph0[s, :n], cen0[s, :n], sh,
                                  l0_thresh=l0)
        sc.observations = []
        for o in obs_data:
            w = o.get("weights")
            sc.observations.append(dict(images=o["images"][s], band_slice=slice(o["band0"], o["band0"] + o["images"].shape[1]),
                                        weights=1 if w is None else (w if np.ndim(w) == 0 else w[s]),
                                        diff_kernel=o.get("diff")))
        pgm.fit(sc, n_iter, e_rel=0, approximate_L=approximate_L)
        assert int(it1[s]) == n_iter
        assert rel_err(b.mse(s), sc.mse) < TOL, s
        assert rel_err(sed1[s, :n], np.array([c.sed for c in sc.sources])) < TOL, s
        assert rel_err(morph1[s, :n], np.array([c.morph for c in sc.sources])) < TOL, s
        np.testing.assert_array_equal(cen1[s, :n], np.array([c.center for c in sc.sources]))
        if counts is not None:
            assert not sed1[s, n:].any() and not morph1[s, n:].any()


def _build(obs_data, centers, **kw):
    import scarlet_amd as scarlet
    obs = []
    for o in obs_data:
        ob = scarlet.ObservationBatch(o["images"], band0=o["band0"], weights=o.get("weights"))
        if o.get("diff") is not None:
            ob.set_diff_kernel(o["diff"])
        obs.append(ob)
    return scarlet.BlendBatch.from_observations(obs, centers, **kw)


@pytest.mark.parametrize("layout", ["sliced", "epochs"])
def test_two_observations_match_the_oracle(layout):
    S = 256
    images, centers = _scenes(4000, S)
    if layout == "sliced":
        obs = [dict(images=images[:, :3], band0=0), dict(images=images[:, 3:], band0=3)]
    else:
        images2, _ = _scenes(4000, S)
        rng = np.random.default_rng(3)
        images2 = (images2 + 0.05 * rng.standard_normal(images2.shape)).astype(np.float32)
        obs = [dict(images=images, band0=0), dict(images=images2, band0=0)]
    b = _build(obs, centers)
    if layout == "sliced":
        b.init_combined([np.ones(3) * 0.1, np.ones(2) * 0.1])
    else:
        # (overlapping channels do not tile the model: the start comes from a band-sliced batch's init_combined)
        start = _build([dict(images=images[:, :3], band0=0), dict(images=images[:, 3:], band0=3)], centers)
        start.init_combined([np.ones(3) * 0.1, np.ones(2) * 0.1])
        b.set_state(start.sed_current, start.morph_current)
    _check(b, obs, 6, [0, 1, 77, 255])


def test_weights_and_approximate_L():
    S = 64
    images, centers = _scenes(4100, S)
    rng = np.random.default_rng(5)
    w = (0.5 + rng.random(images[:, :3].shape)).astype(np.float32)
    obs = [dict(images=images[:, :3], band0=0, weights=w), dict(images=images[:, 3:], band0=3, weights=2.0)]
    for approx in (False, True):
        b = _build(obs, centers)
        b.init_combined([np.ones(3) * 0.1, np.ones(2) * 0.1])
        _check(b, obs, 6, [0, 5, 63], approximate_L=approx)


def test_psf_observations_lds_and_hipfft():
    """per-observation PSFs, one observation without: 128 x 128 (LDS-resident convolution) and 200 x 200 (hipFFT)"""
    from scarlet_amd import synth
    from oracle import pgm
    model = synth.gaussian_psf((41, 41), 0.9)
    psf_a = np.array([synth.gaussian_psf((41, 41), 1.2 + 0.15 * b) for b in range(5)])
    diff = pgm.match_psfs(psf_a.astype(np.float32), model[None].astype(np.float32)).astype(np.float32)
    for side, S in ((128, 16), (200, 4)):
        images, centers = _scenes(4200, S, H=side, W=side, psfs=psf_a)
        obs = [dict(images=images[:, :3], band0=0, diff=diff[:3]), dict(images=images[:, 3:], band0=3)]
        b = _build(obs, centers, centroid_weight=model.astype(np.float32))
        b.init_combined([np.ones(3) * 0.1, np.ones(2) * 0.1], obs_psfs=[psf_a[:3], None], model_psf=model)
        _check(b, obs, 4, [0, S - 1])


@pytest.mark.parametrize("K,side,l0", [(12, 64, None), (40, 96, 0.02)])
def test_many_components(K, side, l0):
    S = 4
    images, centers = _scenes(4300, S, H=side, W=side, K=K)
    obs = [dict(images=images[:, :3], band0=0), dict(images=images[:, 3:], band0=3)]
    b = _build(obs, centers, l0_thresh=l0)
    b.init_combined([np.ones(3) * 0.1, np.ones(2) * 0.1])
    _check(b, obs, 3, [0, S - 1], l0=l0)


def test_ragged_and_eight_observations():
    S = 32
    images, centers = _scenes(4400, S, K=6)
    counts = np.array([1 + (s % 6) for s in range(S)])
    lists = [centers[s, :counts[s]] for s in range(S)]
    obs = [dict(images=images[:, :3], band0=0), dict(images=images[:, 3:], band0=3)]
    b = _build(obs, lists)
    b.init_combined([np.ones(3) * 0.1, np.ones(2) * 0.1], obs_idx=1)
    _check(b, obs, 5, [0, 1, 5, 31], counts=counts)
    # eight observations: every band once, three bands twice (epochs)
    obs = [dict(images=images[:, b:b + 1], band0=b) for b in range(5)] + \
          [dict(images=images[:, b:b + 1] * 1.01, band0=b) for b in range(3)]
    b = _build(obs, lists)
    b.set_state(np.ones((S, 6, 5), np.float32) * 0.5, np.full((S, 6, 64, 64), 0.01, np.float32))
    _check(b, obs, 4, [2, 30], counts=counts)


def test_init_combined_matches_the_oracle():
    from oracle import pgm
    S = 8
    images, centers = _scenes(4500, S)
    bg = [np.ones(3) * 0.1, np.ones(2) * 0.1]
    for idx in (0, 1):
        obs = [dict(images=images[:, :3], band0=0), dict(images=images[:, 3:], band0=3)]
        b = _build(obs, centers)
        b.init_combined(bg, obs_idx=idx)
        sed, morph = b.sed_current.cpu().numpy(), b.morph_current.cpu().numpy()
        for s in range(S):
            for k in range(4):
                ws, wm = pgm.init_combined_extended_source(tuple(centers[s, k]), [images[s, :3], images[s, 3:]], bg,
                                                           obs_idx=idx)
                assert rel_err(sed[s, k], ws) < 1e-6
                assert rel_err(morph[s, k], wm) < 1e-5


def test_lipschitz_against_eigvalsh():
    S = 16
    images, centers = _scenes(4600, S)
    obs = [dict(images=images[:, :3], band0=0), dict(images=images[:, 3:], band0=3), dict(images=images, band0=0)]
    b = _build(obs, centers)
    b.set_state(np.random.default_rng(1).random((S, 4, 5)).astype(np.float32),
                np.random.default_rng(2).random((S, 4, 64, 64)).astype(np.float32))
    sed, morph = b.sed_current.cpu().numpy().astype(np.float64), b.morph_current.cpu().numpy().astype(np.float64)
    b.step(e_rel=0)
    L = b.lipschitz.cpu().numpy()
    for s in range(S):
        m = morph[s].reshape(4, -1)
        want_sed = 3 * np.linalg.eigvalsh(m @ m.T).max()
        want_morph = 3 * np.linalg.eigvalsh(sed[s].T @ sed[s]).max()
        assert abs(L[s, 0] - want_sed) <= 1e-7 * want_sed
        assert abs(L[s, 1] - want_morph) <= 1e-7 * want_morph


def test_bad_scenes_leave_the_others_bit_identical():
    S = 16
    images, centers = _scenes(4700, S)
    obs = [dict(images=images[:, :3], band0=0), dict(images=images[:, 3:], band0=3)]
    bg = np.ones((S, 3), np.float32) * 0.1

    def run(bad):
        b = _build(obs, centers)
        g = bg.copy()
        if bad:
            g[5, 1] = 0.0
        b.init_combined([g, np.ones(2) * 0.1])
        if bad:
            b.n_components = b.torch.full((S,), 4, dtype=b.torch.int32, device=b.device)
            b.n_components[9] = 7
            b._fill_struct()
        b.fit(5, e_rel=0)
        return b
    ok, bad = run(False), run(True)
    st = bad.status.cpu().numpy()
    assert st[5] & 8 and st[9] & 4
    with pytest.raises(ValueError):
        bad.raise_on_status()
    keep = [s for s in range(S) if s not in (5, 9)]
    for a, c in ((ok.sed_current, bad.sed_current), (ok.morph_current, bad.morph_current), (ok.mse_buf, bad.mse_buf)):
        np.testing.assert_array_equal(a.cpu().numpy()[keep], c.cpu().numpy()[keep])
