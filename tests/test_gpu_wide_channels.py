"""-m gpu: joint fits over 8 < C <= 32 model channels (BlendBatch.from_observations(..., wide=True),
scarlet_fit_observations_wide: k_obs_contract_wide, k_wide_lmorph; scarlet_observations_products_wide) against the CPU
oracle, exactly as tests/test_gpu_observations.py::_check does: the device's own start state goes to oracle.pgm.fit with
`scene.observations` and `band_slice`; SED, morphology and loss history agree to 1e-5 max-norm relative
(conftest.rel_err), centres, iteration counts and flags are equal.  Shapes are the smallest that reach each path: 3 scenes
of 32 x 32, and 48 x 40 where the last sweep of a tile has to be ragged (1920 pixels: no multiple of 512 or 1024).
"""
import multiprocessing as mp
import os

import numpy as np
import pytest

from conftest import rel_err
import observations_prior_common as oc
import products_common as prc
import wide_channels_common as wc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
TOL = wc.TOL
F32 = np.float32


@pytest.fixture(scope="module")
def env():
    import scarlet_amd
    scarlet_amd._lib.require_gpu()
    from oracle import build as obuild
    obuild.build()
    pool = mp.get_context("spawn").Pool(min(16, os.cpu_count() or 1))
    yield scarlet_amd, pool
    pool.close(); pool.join()


def npy(t):
    return t.detach().cpu().numpy()


def make(scarlet, case, wide=True, **kw):
    obs = []
    for o in case.obs:
        if o.get("lowres") is not None:
            ob = scarlet.LowResObservationBatch(o["images"], band0=o["band0"], geometry=o["lowres"], weights=o.get("weights"))
        else:
            ob = scarlet.ObservationBatch(o["images"], band0=o["band0"], weights=o.get("weights"))
            if o.get("diff") is not None:
                ob.set_diff_kernel(o["diff"])
        obs.append(ob)
    kw = dict(dict(mse_capacity=64, l0_thresh=case.l0, l1_thresh=case.l1), **kw)
    if case.cw is not None:
        kw["centroid_weight"] = case.cw
    centers = case.centers
    if case.ragged:
        centers = [c[:n] for c, n in zip(centers, case.n)]
    b = scarlet.BlendBatch.from_observations(obs, centers, wide=wide, **kw)
    b.set_state(case.sed0, case.morph0)
    for name in ("fix_sed", "fix_morph"):
        f = getattr(case, name)
        if f is not None:
            setattr(b, name, torch.as_tensor(np.ascontiguousarray(f, dtype=np.uint8)).to(b.device))
    b._fill_struct()
    return b


def quad(scarlet, case):
    return scarlet.QuadraticPrior(sed_weight=case.ws, sed_target=case.ts, morph_weight=case.wm, morph_target=case.tm)


def state0(b):
    torch.cuda.synchronize()
    return dict(sed=npy(b.sed_current), morph=npy(b.morph_current), cen=npy(b.centers), sh=npy(b.shifts))


def result(b):
    torch.cuda.synchronize()
    return dict(sed=npy(b.sed_current), morph=npy(b.morph_current), cen=npy(b.centers), it=npy(b.it), flags=npy(b.flags),
                mse=npy(b.mse_buf), status=npy(b.status), L=npy(b.lipschitz), active=npy(b.active),
                Lc=None if b.L_components is None else npy(b.L_components))


def check(case, pool, st0, g, test, per_component=None):
    """every scene of the device's `result` g against the float32 oracle started from st0; returns the oracle's results"""
    ref = pool.map(wc.oracle_fit, [(wc.spec_of(case, st0, i, per_component), case.iters, case.e_rel, F32) for i in range(case.S)])
    assert not g["status"].any(), g["status"]
    for i, r in enumerate(ref):
        n = int(case.n[i])
        e = dict(sed=rel_err(g["sed"][i][:n], r[0]), morph=rel_err(g["morph"][i][:n], r[1]), mse=rel_err(g["mse"][i][:r[4]], r[2]))
        print("%s scene %d: %s iterations %d / %d" % (test, i, e, g["it"][i], r[4]))
        np.testing.assert_array_equal(g["cen"][i][:n], r[3])
        assert g["it"][i] == r[4], (i, g["it"][i], r[4])
        if case.e_rel > 0:
            np.testing.assert_array_equal(g["flags"][i][:n] & 3, np.array(r[5]) & 3)
        assert max(e.values()) <= TOL, (test, i, e)
        assert not g["sed"][i][n:].any() and not g["morph"][i][n:].any()      # absent rows stay zero
    return ref


def fit(scarlet, case, prior=None, check_every=10, **kw):
    b = make(scarlet, case, **kw)
    st0 = state0(b)
    n = b.fit(case.iters, e_rel=case.e_rel, approximate_L=case.approximate_L, check_every=check_every, prior=prior)
    return b, st0, result(b), n


# ------------------------------------------------------------------ channel counts x component counts x constants
# C = 9 (5 + 4: the 16-channel instance), 17 (6 + 4 + 7) and 32 (4 x 8): K = 3, 9 and 40 make min(K, C) = 3, 9, 9, 17
# and 32 for lambda_max of the SED Gram; K = 40 takes its morphology Gram from hugek.h, K = 9 from bigk.h, K = 3 from
# bigk.h too (the wide contraction sums no Gram).  K = 40 runs on 48 x 40: a ragged last sweep.
GRID = [((5, 4), 3, False), ((5, 4), 9, True), ((6, 4, 7), 3, True), ((6, 4, 7), 9, False), ((6, 4, 7), 40, False),
        ((8, 8, 8, 8), 3, False), ((8, 8, 8, 8), 9, True), ((8, 8, 8, 8), 40, False), ((8, 8, 8, 8), 40, True)]


@pytest.mark.parametrize("widths,K,approx", GRID, ids=lambda v: "+".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_channels_components_and_constants(env, widths, K, approx):
    scarlet, pool = env
    big = K == 40
    case = wc.case("grid", 7000 + 10 * len(widths) + K, widths, K=K, H=48 if big else 32, W=40 if big else 32,
                   min_sep=2 if big else (3 if K == 9 else 4), iters=5, approximate_L=approx)
    b, st0, g, n = fit(scarlet, case)
    assert n == 5 and b.B == sum(widths) and tuple(b.sed_current.shape) == (case.S, K, sum(widths))
    check(case, pool, st0, g, "C = %d, K = %d, approximate_L = %s" % (sum(widths), K, approx))


@pytest.mark.parametrize("K,C", [(160, 32), (256, 32)])
def test_two_and_one_wave_instances(env, K, C):
    """K C beyond what four waves' float64 slots hold in LDS: contract_plan takes two waves at K = 160, one at K = 256"""
    scarlet, pool = env
    case = wc.case("waves", 7100 + K, (8,) * (C // 8), S=2, K=K, H=48, W=40, min_sep=1, iters=3)
    b, st0, g, n = fit(scarlet, case)
    check(case, pool, st0, g, "K = %d, C = %d" % (K, C))


def test_lipschitz_against_eigvals(env):
    """lambda_max of the SED Gram for n = min(K, C) = 9, 17, 32 against float64 numpy, and L x n_obs"""
    scarlet, _ = env
    rng = np.random.default_rng(11)
    for K, widths in ((9, (6, 4, 7)), (20, (6, 4, 7)), (40, (8, 8, 8, 8)), (32, (8, 8, 8, 8))):
        case = wc.case("L", 7200 + K, widths, K=K, min_sep=1)
        case.sed0 = rng.random(case.sed0.shape).astype(F32)
        case.morph0 = rng.random(case.morph0.shape).astype(F32)
        b = make(scarlet, case)
        b.step(e_rel=0)
        L = npy(b.lipschitz)
        for s in range(case.S):
            sed, m = case.sed0[s].astype(np.float64), case.morph0[s].reshape(K, -1).astype(np.float64)
            want_sed = len(widths) * np.linalg.eigvalsh(m @ m.T).max()
            want_morph = len(widths) * np.linalg.eigvalsh(sed.T @ sed).max()
            print("K = %d, C = %d, scene %d: L_sed %.3e, L_morph %.3e" % (K, sum(widths), s, abs(L[s, 0] / want_sed - 1),
                                                                          abs(L[s, 1] / want_morph - 1)))
            assert abs(L[s, 0] - want_sed) <= 1e-7 * want_sed
            assert abs(L[s, 1] - want_morph) <= 1e-7 * want_morph


# ------------------------------------------------------------------ layouts of the observations
def test_overlapping_epochs(env):
    """two observations on channels 8 - 12 beside one on 0 - 7, started with set_state"""
    scarlet, pool = env
    images, centers, sed, morph = wc.scenes(7300, 3, 13)
    rng = np.random.default_rng(7)
    second = (images[:, 8:] + 0.05 * rng.standard_normal(images[:, 8:].shape)).astype(F32)
    w = (0.5 + rng.random(second.shape)).astype(F32)
    obs = [dict(images=np.ascontiguousarray(images[:, :8]), band0=0), dict(images=np.ascontiguousarray(images[:, 8:]), band0=8, weights=2.0),
           dict(images=second, band0=8, weights=w)]
    case = oc.Case("epochs", obs, centers, sed, morph, iters=5)
    b, st0, g, _ = fit(scarlet, case)
    check(case, pool, st0, g, "epochs on channels 8 - 12")


def test_psf_observation_past_channel_eight(env):
    """one observation with a PSF at band0 = 10 (its G planes are Fy x Fx, not H x W) beside inline ones"""
    from oracle import pgm
    from scarlet_amd import synth
    scarlet, pool = env
    model = synth.gaussian_psf((11, 11), 0.9)
    psfs = np.array([synth.gaussian_psf((11, 11), 1.2 + 0.15 * b) for b in range(4)])
    diff = pgm.match_psfs(psfs.astype(F32), model[None].astype(F32)).astype(F32)
    images, centers, sed, morph = wc.scenes(7400, 3, 17)
    obs = wc.tiled(images, (6, 4, 4, 3))
    obs[2]["diff"] = diff
    assert obs[2]["band0"] == 10
    case = oc.Case("psf", obs, centers, sed, morph, cw=model.astype(F32), iters=5)
    b, st0, g, _ = fit(scarlet, case)
    check(case, pool, st0, g, "PSF observation at band0 = 10")


def test_low_resolution_observation_past_channel_eight(env):
    """tests/lowres_common.py's geometry "a" (32 x 32 model, 16 x 16 images of 2 bands) at band0 = 9 of 11 channels"""
    import lowres_common as lc
    scarlet, pool = env
    obs, (sed0, morph0, cen0), cw, lo = lc.fit_inputs(lc.fixture(), "a")
    S, K = 3, len(sed0)
    rng = np.random.default_rng(23)
    lr = np.stack([obs[1]["images"] + (0.02 * rng.standard_normal(obs[1]["images"].shape) if s else 0) for s in range(S)])
    wl = np.stack([obs[1]["weights"] * (1 + 0.2 * s) for s in range(S)])
    # the nine channels on the model's grid: the fixture's three high-resolution bands, scaled and with other noise
    scale = np.array([1.0, 0.8, 1.2, 0.6, 1.1, 0.9, 0.7, 1.3, 1.05])
    hr = np.stack([np.stack([obs[0]["images"][c % 3] * scale[c] for c in range(9)]) + 0.02 * rng.standard_normal((9, 32, 32))
                   for s in range(S)])
    sed = np.stack([np.concatenate([sed0[:, [c % 3 for c in range(9)]] * scale[None, :], sed0[:, 3:]], axis=1) * (1 + 0.1 * s)
                    for s in range(S)])
    data = [dict(images=hr[:, :8].astype(F32), band0=0), dict(images=hr[:, 8:].astype(F32), band0=8),
            dict(images=lr.astype(F32), band0=9, weights=wl.astype(F32), lowres=lo)]
    case = oc.Case("lowres", data, np.stack([cen0] * S), sed, np.stack([morph0] * S), cw=np.asarray(cw, F32), iters=5)
    assert case.C == 11 and case.K == K
    b, st0, g, _ = fit(scarlet, case)
    check(case, pool, st0, g, "low-resolution observation at band0 = 9")


# ------------------------------------------------------------------ ragged counts, fixed factors, priors, constraints
def test_ragged_counts_and_fixed_factors(env):
    scarlet, pool = env
    S, K = 4, 4
    images, centers, sed, morph = wc.scenes(7500, S, 17, K=K)
    counts = np.array([4, 1, 3, 2], np.int32)
    present = np.arange(K)[None, :] < counts[:, None]
    sed[~present] = 0
    morph[~present] = 0
    fix_sed, fix_morph = np.zeros((S, K), bool), np.zeros((S, K), bool)
    fix_sed[:, 0] = True
    fix_morph[:, 1] = True
    case = oc.Case("ragged", wc.tiled(images, (6, 4, 7)), centers, sed, morph, counts=counts, fix_sed=fix_sed,
                   fix_morph=fix_morph, iters=5)
    b, st0, g, _ = fit(scarlet, case)
    check(case, pool, st0, g, "ragged counts 4, 1, 3, 2; fix_sed on component 0, fix_morph on 1")
    for buf in range(2):
        assert not npy(b.sed[buf])[~present].any() and not npy(b.morph[buf])[~present].any()


@pytest.mark.parametrize("approx", [False, True])
def test_quadratic_prior(env, approx):
    """a QuadraticPrior with an (S, K, C) SED target and morphology weights, fix_morph on one component; the fit against
    the oracle with the equivalent prior, L_components against the oracle's constants"""
    scarlet, pool = env
    case = wc.case("prior", 7600, (6, 4, 7), K=4, iters=5, approximate_L=approx)
    oc._prior_on(case, (0, 2, 3))
    case.fix_morph = np.zeros((case.S, case.K), bool)
    case.fix_morph[:, 3] = True
    assert case.ts.shape == (case.S, case.K, 17)
    b, st0, g, _ = fit(scarlet, case, prior=quad(scarlet, case))
    ref = check(case, pool, st0, g, "QuadraticPrior, approximate_L = %s" % approx)
    plain = pool.map(wc.oracle_fit, [(wc.spec_of(case, st0, i, prior=False), case.iters, 0.0, F32) for i in range(case.S)])
    moved = [rel_err(p[1], r[1]) for p, r in zip(plain, ref)]
    print("the prior moves the morphologies by", moved)
    assert min(moved) > 1e-3, moved
    for i, r in enumerate(ref):
        e = rel_err(g["Lc"][i], r[6])
        print("scene %d: L_components differ from the oracle's constants by %.2e" % (i, e))
        assert e <= TOL


def test_per_component_constraints(env):
    """symmetric, monotonic and l1_thresh per component"""
    scarlet, pool = env
    case = wc.case("constraints", 7700, (6, 4, 7), K=3, iters=5)
    S, K = case.S, case.K
    pc = dict(symmetric=np.tile(np.array([1, 0, 1], np.uint8), (S, 1)), monotonic=np.tile(np.array([1, 1, 0], np.uint8), (S, 1)),
              l1=np.tile(np.array([-1.0, 0.02, 0.05], F32), (S, 1)))
    b, st0, g, _ = fit(scarlet, case, symmetric=[True, False, True], monotonic=[True, True, False], l1_thresh=[None, 0.02, 0.05])
    assert b.constrained
    check(case, pool, st0, g, "per-component symmetric / monotonic / l1_thresh", per_component=pc)


def test_scenes_stop_on_their_own(env):
    """fit(50, e_rel = 1e-3): iteration counts and flags equal the oracle's (two sources per scene; the float32 oracle
    stops these four scenes after 33, 35, 25 and 23 iterations)"""
    scarlet, pool = env
    case = wc.case("stopping", 7810, (6, 4, 7), S=4, K=2, iters=50, e_rel=1e-3)
    b, st0, g, n = fit(scarlet, case, check_every=5)
    check(case, pool, st0, g, "fit(50, e_rel = 1e-3)")
    print("iterations:", g["it"], "launched", n)
    assert len(np.unique(g["it"])) > 1 and g["it"].max() < 50 and not g["active"].any()


# ------------------------------------------------------------------ the same bits
def test_wide_with_five_channels_is_the_batch_of_today(env):
    scarlet, _ = env
    case = wc.case("same", 7900, (3, 2), K=3, iters=6)
    for prior in (False, True):
        if prior:
            oc._prior_on(case, (0, 2))
        out = []
        for wide in (True, False):
            b, _, g, _ = fit(scarlet, case, prior=quad(scarlet, case) if prior else None, wide=wide)
            out.append(g)
            assert (g["it"] == 6).all()
        for key in ("sed", "morph", "mse", "L", "cen", "it", "flags") + (("Lc",) if prior else ()):
            np.testing.assert_array_equal(out[0][key], out[1][key], err_msg=key)


@pytest.mark.parametrize("widths,K", [((6, 4, 7), 3), ((8, 8, 8, 8), 40)])
def test_a_wide_fit_is_reproducible_to_the_bit(env, widths, K):
    scarlet, _ = env
    case = wc.case("twice", 8000 + K, widths, K=K, min_sep=4 if K == 3 else 1, iters=4)
    a, c = fit(scarlet, case)[2], fit(scarlet, case)[2]
    for key in ("sed", "morph", "mse", "L", "cen", "it", "flags"):
        np.testing.assert_array_equal(a[key], c[key], err_msg=key)


# ------------------------------------------------------------------ products
def test_products_of_a_seventeen_channel_batch(env):
    scarlet, _ = env
    case = wc.case("products", 8100, (6, 4, 7), S=3, K=4, H=48, W=40, iters=3)
    rng = np.random.default_rng(3)
    case.obs[1]["weights"] = (0.5 + rng.random(case.obs[1]["images"].shape)).astype(F32)
    counts = np.array([4, 2, 3], np.int32)
    case.ragged, case.n = True, counts
    present = np.arange(case.K)[None, :] < counts[:, None]
    case.sed0[~present] = 0
    case.morph0[~present] = 0
    b = make(scarlet, case)
    b.fit(3, e_rel=0)
    sed, morph = prc.state(b)
    before = result(b)
    p = b.products(components=[2, 0])
    q = b.products(components=[2, 0])
    assert tuple(p.model.shape) == (3, 17, 48, 40) and tuple(p.flux.shape) == (3, 4, 17)
    assert tuple(p.component_models.shape) == (3, 2, 17, 48, 40)
    np.testing.assert_array_equal(npy(p.flux), npy(q.flux))
    for i in range(3):
        np.testing.assert_array_equal(npy(p.loss[i]), npy(q.loss[i]))
    for s in range(case.S):
        whole = prc.reference(sed[s], morph[s], np.zeros((17, 48, 40)))
        prc.check_scene(p, s, whole, ("model", "flux", "component_models"), components=[2, 0], where="state")
        for i, o in enumerate(case.obs):
            sl = slice(o["band0"], o["band0"] + o["images"].shape[1])
            w = o.get("weights")
            ref = prc.reference(sed[s][:, sl], morph[s], o["images"][s], 1.0 if w is None else w[s])
            prc.check_scene(dict(rendered=p.rendered[i], residual=p.residual[i], loss=p.loss[i]), s, ref,
                            ("rendered", "residual", "loss"), where="observation %d" % i)
    assert not npy(p.flux)[~present].any()
    # the named shortcuts
    assert rel_err(npy(b.get_model()), npy(p.model)) == 0 and rel_err(npy(b.get_flux()), npy(p.flux)) == 0
    assert rel_err(npy(b.render(obs=2)), npy(p.rendered[2])) == 0 and rel_err(npy(b.residual(obs=1)), npy(p.residual[1])) == 0
    np.testing.assert_array_equal(npy(b.get_loss()), npy(sum(x.sum(dim=1) for x in p.loss)))
    np.testing.assert_array_equal(npy(b.component_models([2, 0])), npy(p.component_models))
    # read-only: the state is as it was, and a fit continued after products() equals one that never called it
    after = result(b)
    for key in before:
        if before[key] is not None:
            np.testing.assert_array_equal(before[key], after[key], err_msg=key)
    b.fit(2, e_rel=0)
    c = make(scarlet, case)
    c.fit(3, e_rel=0)
    c.fit(2, e_rel=0)
    for key, x in result(b).items():
        if x is not None:
            np.testing.assert_array_equal(x, result(c)[key], err_msg=key)
    # the next iteration records the loss that get_loss reported
    assert rel_err(npy(b.mse_buf)[:, 3], npy(sum(x.sum(dim=1) for x in p.loss))) <= TOL


def test_init_combined_over_seventeen_channels(env):
    from oracle import pgm
    scarlet, _ = env
    images, centers, _, _ = wc.scenes(8200, 3, 17)
    obs = wc.tiled(images, (6, 4, 7))
    b = scarlet.BlendBatch.from_observations([scarlet.ObservationBatch(o["images"], band0=o["band0"]) for o in obs], centers,
                                             wide=True)
    bg = [np.ones(6) * 0.1, np.ones(4) * 0.1, np.ones(7) * 0.1]
    b.init_combined(bg, obs_idx=2)
    sed, morph = npy(b.sed_current), npy(b.morph_current)
    for s in range(3):
        for k in range(centers.shape[1]):
            ws, wm = pgm.init_combined_extended_source(tuple(centers[s, k]), [o["images"][s] for o in obs], bg, obs_idx=2)
            assert rel_err(sed[s, k], ws) < 1e-6
            assert rel_err(morph[s, k], wm) < 1e-5
