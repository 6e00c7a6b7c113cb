"""-m gpu: batches whose components carry priors (scarlet_fit_prior, scarlet_backward_step_prior, k_prior_step)
against the reference's fixture and the CPU oracle with the same hook (`s.prior = (grad, lip)`, oracle/pgm.py:747-764),
started from the device's own initial state.

Tolerance: rel_err (max-norm relative) <= 1e-5 on SED, morphology and loss history; centres, iteration counts and
flags equal.  A scene beyond 1e-5 passes only through the float64-anchored threshold rule of tests/parity_common.py
(restated with the prior in tests/prior_common.py), at most ONE scene per case, every use printed by log_exemptions.
"""
import multiprocessing as mp
import os

import numpy as np
import pytest

from conftest import rel_err, load_golden
import parity_common as pc
import prior_common as prc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
TOL = pc.TOL
BG = 0.1


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


class Case(object):
    """one batch + its priors; `make(sl)` builds the initialised batch of the scenes in slice `sl`"""

    def __init__(self, scarlet, wl, images, centers, n=None, weights=None, group=None, fix_sed=None, fix_morph=None,
                 approximate_L=False, init="extended"):
        self.scarlet, self.wl, self.images, self.centers = scarlet, wl, images, centers
        self.S, self.K = len(images), centers.shape[1]
        self.n = np.full(self.S, self.K, np.int32) if n is None else np.asarray(n, np.int32)
        self.ragged = n is not None
        self.weights, self.group, self.fix_sed, self.fix_morph = weights, group, fix_sed, fix_morph
        self.approximate_L, self.init = approximate_L, init
        self.ws = self.wm = self.ts = self.tm = None

    def make(self, sl=slice(None), mse_capacity=256):
        wl = self.wl
        kw = dict(mse_capacity=mse_capacity, l0_thresh=wl.l0)
        if self.ragged:
            kw["n_components"] = self.n[sl]
        if self.group is not None:
            kw["group"] = self.group[sl]
        if self.weights is not None:
            kw["weights"] = self.weights[sl]
        if wl.psf:
            kw["centroid_weight"] = wl.model_psf.astype(np.float32)
        b = self.scarlet.BlendBatch(self.images[sl], self.centers[sl], **kw)
        if wl.psf:
            b.set_diff_kernel(wl.diff)
        if self.init == "sources":
            b.init_sources(np.ones(wl.B, np.float32) * BG, flux_percentiles=[30])
        else:
            b.init_extended(np.ones(wl.B) * BG, sed_scale=wl.scale)
        for name in ("fix_sed", "fix_morph"):
            f = getattr(self, name)
            if f is not None:
                setattr(b, name, torch.as_tensor(np.ascontiguousarray(f[sl], dtype=np.uint8)).to(b.device))
        b._fill_struct()
        return b

    def prior(self, sl=slice(None)):
        cut = lambda a: None if a is None else a[sl]
        return self.scarlet.QuadraticPrior(sed_weight=cut(self.ws), sed_target=cut(self.ts), morph_weight=cut(self.wm),
                                           morph_target=cut(self.tm))

    def spec(self, st0, i):
        n = int(self.n[i])
        okw = self.wl.oracle_kwargs()
        if self.weights is not None:
            okw["weights"] = self.weights[i]
        cut = lambda a: None if a is None else a[i][:n]
        return dict(images=self.images[i], sed0=st0["sed"][i][:n], morph0=st0["morph"][i][:n], cen0=st0["cen"][i][:n],
                    sh0=st0["sh"][i][:n], ws=cut(self.ws), wm=cut(self.wm), ts=cut(self.ts), tm=cut(self.tm),
                    fix_sed=cut(self.fix_sed), fix_morph=cut(self.fix_morph), group=cut(self.group), okw=okw,
                    approximate_L=self.approximate_L)


def state0(b):
    torch.cuda.synchronize()
    return dict(sed=npy(b.sed_current), morph=npy(b.morph_current), cen=npy(b.centers), sh=npy(b.shifts))


def result(b):
    torch.cuda.synchronize()
    return dict(sed=npy(b.sed_current), morph=npy(b.morph_current), cen=npy(b.centers), it=npy(b.it), flags=npy(b.flags),
                mse=npy(b.mse_buf), status=npy(b.status), L=npy(b.lipschitz),
                Lc=None if b.L_components is None else npy(b.L_components))


def check_against_oracle(case, pool, st0, g, iters, e_rel, test, cap=1, support=False, scenes=None):
    """every scene of `g` (a `result`) against the float32 oracle; returns the oracle's results"""
    S = case.S
    idx = list(range(S)) if scenes is None else list(scenes)
    ref = pool.map(prc.oracle_fit, [(case.spec(st0, i), iters, e_rel, np.float32) for i in idx])
    assert not g["status"].any(), g["status"]
    exempt = []
    worst = dict(sed=0.0, morph=0.0, mse=0.0)
    for i, r in zip(idx, ref):
        n = int(case.n[i])
        np.testing.assert_array_equal(g["cen"][i][:n], r[3])
        assert g["it"][i] == r[4], (i, g["it"][i], r[4])
        if e_rel > 0:
            np.testing.assert_array_equal(g["flags"][i][:n] & 3, np.array(r[5]) & 3)
        e = dict(sed=rel_err(g["sed"][i][:n], r[0]), morph=rel_err(g["morph"][i][:n], r[1]),
                 mse=rel_err(g["mse"][i][:r[4]], r[2]))
        same_support = np.array_equal(g["morph"][i][:n] == 0, r[1] == 0)
        if max(e.values()) <= TOL and (same_support or not support):
            for k in worst:
                worst[k] = max(worst[k], e[k])
            continue
        # the float64-anchored rule, on a per-iteration re-run of the scene alone
        b1 = case.make(slice(i, i + 1))
        p1 = case.prior(slice(i, i + 1))
        snaps = []
        for _ in range(int(r[4])):
            b1.fit(1, e_rel=0, approximate_L=case.approximate_L, prior=p1)
            snaps.append(npy(b1.morph_current)[0][:n].copy())
        ok, msg = prc.straddles_threshold(snaps, case.spec(st0, i), int(r[4]))
        assert ok, "scene %d beyond 1e-5 (%s, same support %s) and not a threshold straddle: %s" % (i, e, same_support, msg)
        exempt.append((i, e, msg))
    pc.log_exemptions(test, exempt, cap)
    assert len(exempt) <= cap, exempt
    print("%s: %d scenes, worst errors %s" % (test, len(idx), worst))
    return dict(zip(idx, ref))


# ------------------------------------------------------------------ 1. the reference's own fixture
def test_reference_fixture(env):
    """synth scene 3, ExtendedSource starts, quadratic prior on component 1 only (weights 0.3 / 2.0, target 0), 8
    iterations: what the reference itself computed (tests/golden/fit_extras.npz, prior_*)"""
    scarlet, _ = env
    from scarlet_amd import synth
    scn = synth.make_scene(3)
    b = scarlet.BlendBatch(scn["images"][None], scn["centers"][None]).init_extended(np.ones(5) * BG)
    n = b.fit(8, e_rel=0, prior=scarlet.QuadraticPrior(sed_weight=[0, 0.3, 0, 0], morph_weight=[0, 2.0, 0, 0]))
    assert n == 8
    r = result(b)
    g = load_golden("fit_extras")
    e = dict(mse=rel_err(r["mse"][0][:8], g["prior_mse"]), morph=rel_err(r["morph"][0], g["prior_morph"]),
             sed=rel_err(r["sed"][0], g["prior_sed"]))
    print("reference fixture:", e)
    assert max(e.values()) <= TOL, e
    np.testing.assert_array_equal(r["cen"][0], g["prior_center"])
    # the constants: the scene's, plus the weights on component 1
    L = r["L"][0]
    for k in range(4):
        ws, wm = (0.3, 2.0) if k == 1 else (0.0, 0.0)
        assert r["Lc"][0, k, 0] == (np.float32(L[0]) + np.float32(ws) if ws else L[0])
        assert r["Lc"][0, k, 1] == (np.float32(L[1]) + np.float32(wm) if wm else L[1])


# ------------------------------------------------------------------ 2. / 3. / 7. a batch of 64 scenes
def batch64(scarlet, l0=None):
    wl = pc.Workload(l0=l0)
    images, centers = wl.scenes(0, 64)
    case = Case(scarlet, wl, images, centers)
    S, K = 64, 4
    s, k = np.mgrid[:S, :K]
    case.ws = (20.0 * (k % 2)).astype(np.float32)
    case.wm = np.array([0.0, 1000.0, 4000.0], np.float32)[(s + k) % 3]
    return case


def fit64(case, iters, e_rel, check_every=10):
    b = case.make()
    st0 = state0(b)
    case.ts, case.tm = st0["sed"].copy(), st0["morph"].copy()          # targets = the initial state
    b.fit(iters, e_rel=e_rel, check_every=check_every, prior=case.prior())
    return st0, result(b)


def plain_oracle(case, pool, st0, iters, scenes):
    keep = case.ws, case.wm
    case.ws = case.wm = None
    try:
        return pool.map(prc.oracle_fit, [(case.spec(st0, i), iters, 0.0, np.float32) for i in scenes])
    finally:
        case.ws, case.wm = keep


def test_batch_of_64_scenes(env):
    scarlet, pool = env
    case = batch64(scarlet)
    st0, g = fit64(case, 10, 0.0)
    ref = check_against_oracle(case, pool, st0, g, 10, 0.0, "prior, 64 scenes x 10 iterations")
    # the weights are large enough to matter: a prior that is silently dropped cannot pass
    plain = plain_oracle(case, pool, st0, 10, range(16))
    for i in range(16):
        ds, dm = rel_err(plain[i][0], ref[i][0]), rel_err(plain[i][1], ref[i][1])
        assert ds > 1e-3 and dm > 1e-3, (i, ds, dm)


def test_sparsity_cut_uses_the_components_own_step(env):
    """l0_thresh = 0.05: the cut is thresh / L_morph,k (update.py:71-82); the supports equal the oracle's"""
    scarlet, pool = env
    case = batch64(scarlet, l0=0.05)
    st0, g = fit64(case, 10, 0.0)
    check_against_oracle(case, pool, st0, g, 10, 0.0, "prior + l0, 64 scenes x 10 iterations", support=True)


def test_scenes_stop_on_their_own(env):
    scarlet, pool = env
    case = batch64(scarlet)
    st0, g = fit64(case, 200, 1e-3, check_every=10)
    _, g0 = fit64(case, 200, 1e-3, check_every=0)
    for key in ("it", "flags", "sed", "morph", "cen"):
        np.testing.assert_array_equal(g[key], g0[key])
    check_against_oracle(case, pool, st0, g, 200, 1e-3, "prior, 64 scenes to e_rel = 1e-3")
    print("iterations: min %d median %d max %d" % (g["it"].min(), np.median(g["it"]), g["it"].max()))
    assert len(np.unique(g["it"])) > 1 and g["it"].max() < 200


# ------------------------------------------------------------------ 4. every gradient path
PATHS = [
    ("k8", dict(K=8), {}),
    ("k12_128", dict(K=12, H=128, W=128), {}),
    ("k40", dict(K=40, min_sep=2), {}),
    ("psf", dict(psf=True), {}),
    ("approximate_L", dict(), dict(approximate_L=True)),
    ("pixel_weights", dict(), dict(pixel_weights=True)),
]


@pytest.mark.parametrize("name,wkw,ckw", PATHS, ids=[p[0] for p in PATHS])
def test_every_gradient_path(env, name, wkw, ckw):
    scarlet, pool = env
    wl = pc.Workload(**wkw)
    images, centers = wl.scenes(0, 4)
    weights = None
    if ckw.get("pixel_weights"):
        weights = np.random.default_rng(7).uniform(0.5, 1.5, images.shape).astype(np.float32)
    case = Case(scarlet, wl, images, centers, weights=weights, approximate_L=bool(ckw.get("approximate_L")))
    even = (np.arange(wl.K) % 2 == 0).astype(np.float32)
    case.ws, case.wm = np.tile(20.0 * even, (4, 1)), np.tile(2000.0 * even, (4, 1))
    b = case.make()
    st0 = state0(b)
    case.ts, case.tm = st0["sed"].copy(), st0["morph"].copy()
    b.fit(5, e_rel=0, approximate_L=case.approximate_L, prior=case.prior())
    g = result(b)
    ref = check_against_oracle(case, pool, st0, g, 5, 0.0, "prior on path %s, 4 scenes x 5 iterations" % name)
    plain = plain_oracle(case, pool, st0, 5, range(4))
    moved = [rel_err(plain[i][1], ref[i][1]) for i in range(4)]
    print("the prior moves the morphologies by", moved)
    assert min(moved) > 1e-3


# ------------------------------------------------------------------ 5. ragged counts, fixed factors, groups
def test_ragged_fixed_and_grouped(env):
    scarlet, pool = env
    from scarlet_amd import synth
    wl = pc.Workload(K=5)
    counts = np.array([5, 2, 3, 1, 4, 5], np.int32)
    S, K = len(counts), 5
    imgs, cens = [], np.zeros((S, K, 2), np.int32)
    for i, n in enumerate(counts):
        sc = synth.make_scene(700 + i, K=int(n))
        imgs.append(sc["images"]); cens[i, :n] = sc["centers"]
    images = np.stack(imgs)
    s, k = np.mgrid[:S, :K]
    fix_sed, fix_morph = (s + k) % 4 == 1, (s + k) % 4 == 2
    case = Case(scarlet, wl, images, cens, n=counts, fix_sed=fix_sed, fix_morph=fix_morph)
    case.ws = np.full((S, K), 20.0, np.float32)                        # every component, the fixed ones included
    case.wm = np.full((S, K), 2000.0, np.float32)
    b = case.make()
    st0 = state0(b)
    case.ts, case.tm = st0["sed"].copy(), st0["morph"].copy()
    b.L_components = torch.full((S, K, 2), -7.0, dtype=torch.float64, device=b.device)    # to see what is written
    b.fit(6, e_rel=0, prior=case.prior())
    g = result(b)
    check_against_oracle(case, pool, st0, g, 6, 0.0, "prior, ragged counts and fixed factors")
    present = k < counts[:, None]
    for buf in range(2):
        assert not npy(b.sed[buf])[~present].any() and not npy(b.morph[buf])[~present].any()
    assert (g["Lc"][~present] == -7.0).all()                           # absent components: not written
    Lc, L = g["Lc"], g["L"]
    # a fixed factor keeps the scene's constant; the others add the weight in float32, the frame's dtype
    want_s = np.where(fix_sed, L[:, :1], (L[:, :1].astype(np.float32) + np.float32(20.0)).astype(np.float64))
    want_m = np.where(fix_morph, L[:, 1:], (L[:, 1:].astype(np.float32) + np.float32(2000.0)).astype(np.float64))
    np.testing.assert_array_equal(Lc[..., 0][present], want_s[present])
    np.testing.assert_array_equal(Lc[..., 1][present], want_m[present])


def test_group_with_a_prior(env):
    """one scene with a two-layer multi-component source: the prior belongs to a component, the centre to the group"""
    scarlet, pool = env
    from scarlet_amd import synth
    scn = synth.make_scene(5)
    c = scn["centers"]
    centers = np.array([[c[0], c[0], c[1], c[2]]], np.int32)
    group = np.array([[0, 0, -1, -1]], np.int32)
    case = Case(scarlet, pc.Workload(), scn["images"][None], centers, group=group, init="sources")
    case.ws = np.array([[0.0, 20.0, 20.0, 0.0]], np.float32)
    case.wm = np.array([[2000.0, 0.0, 2000.0, 0.0]], np.float32)
    b = case.make()
    st0 = state0(b)
    case.ts, case.tm = st0["sed"].copy(), st0["morph"].copy()
    b.fit(8, e_rel=0, prior=case.prior())
    g = result(b)
    ref = check_against_oracle(case, pool, st0, g, 8, 0.0, "prior on the layers of a group", cap=0)
    plain = plain_oracle(case, pool, st0, 8, [0])
    assert rel_err(plain[0][1], ref[0][1]) > 1e-3


# ------------------------------------------------------------------ 6. the three forms agree
def test_three_forms_agree(env):
    scarlet, pool = env
    from scarlet_amd import _lib
    case = batch64(scarlet, l0=0.05)
    case.images, case.centers, case.S, case.n = case.images[:8], case.centers[:8], 8, case.n[:8]
    case.ws, case.wm = case.ws[:8], case.wm[:8]
    b = case.make()
    st0 = state0(b)
    case.ts, case.tm = st0["sed"].copy(), st0["morph"].copy()
    dev = lambda a: torch.as_tensor(a).to(b.device)
    ws, wm, ts, tm = dev(case.ws), dev(case.wm), dev(case.ts), dev(case.tm)

    def given(sed, morph):
        return dict(grad_sed=ws[..., None] * (sed - ts), grad_morph=wm[..., None, None] * (morph - tm), L_sed=ws, L_morph=wm)

    b.fit(10, e_rel=0, prior=case.prior())                             # scarlet_fit_prior
    quad = result(b)
    b2 = case.make()
    b2.fit(10, e_rel=0, prior=given)                                   # the callable, once per iteration
    call = result(b2)
    b3 = case.make()
    for _ in range(10):                                                # given tensors recomputed by the caller
        b3.step(e_rel=0, prior=given(b3.sed_current, b3.morph_current))
    step = result(b3)
    for name, other in (("callable", call), ("step", step)):
        e = {key: rel_err(other[key], quad[key]) for key in ("sed", "morph", "mse", "Lc")}
        print("quadratic form vs %s: %s" % (name, e))
        assert max(e.values()) <= TOL, (name, e)
        for key in ("cen", "it", "flags"):
            np.testing.assert_array_equal(other[key], quad[key])
    # all weights zero: the plain fit on the unfused path, and L_comp = lipschitz
    case.ws, case.wm = np.zeros_like(case.ws), np.zeros_like(case.wm)
    b4 = case.make()
    b4.fit(10, e_rel=0, prior=case.prior())
    zero = result(b4)
    prev = _lib.set_option("NO_FUSED", 1)
    try:
        b5 = case.make()
        b5.fit(10, e_rel=0)
        plain = result(b5)
    finally:
        _lib.set_option("NO_FUSED", prev)
    e = {key: rel_err(zero[key], plain[key]) for key in ("sed", "morph", "mse")}
    print("zero weights vs the plain fit:", e)
    assert max(e.values()) <= TOL, e
    for key in ("cen", "it", "flags"):
        np.testing.assert_array_equal(zero[key], plain[key])
    np.testing.assert_array_equal(zero["Lc"], np.repeat(zero["L"][:, None, :], 4, axis=1))
    np.testing.assert_array_equal(zero["L"], plain["L"])


# ------------------------------------------------------------------ 8. no round trip per iteration
def test_callable_runs_once_per_iteration_without_host_sync(env):
    scarlet, _ = env
    wl = pc.Workload()
    images, centers = wl.scenes(100, 8)
    b = wl.batch(scarlet, images, centers, 64)
    w = torch.full((8, 4), 5.0, device=b.device)
    calls = []

    def fn(sed, morph):
        calls.append(1)
        assert sed.shape == (8, 4, 5) and morph.shape == (8, 4, 64, 64) and sed.is_cuda
        return dict(grad_sed=w[..., None] * sed, L_sed=w)

    assert b.fit(12, e_rel=1e-3, check_every=0, prior=fn) == 12
    assert len(calls) == 12
    # the same loop under torch's synchronisation check, where this build has one: any synchronising torch call
    # inside it raises.  (fit() itself looks at `it` once before the loop to size the loss history, so the check
    # wraps the loop it then runs.)
    b.active.fill_(1)
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
    except Exception as exc:                                            # not supported here: the loop was counted above
        print("set_sync_debug_mode unavailable:", exc)
        return
    try:
        n = b._fit_prior(fn, 12, 1e-3, 0, 0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert n == 12 and len(calls) == 24
    print("12 iterations with a callable prior under set_sync_debug_mode('error'): no synchronising call")
