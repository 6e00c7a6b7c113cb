"""-m gpu: batches fitted jointly against several observations whose components carry priors
(BlendBatch.from_observations + fit(prior=) / step(prior=), scarlet_fit_observations_prior, k_obs_contract<KS, true>,
k_obs_head<true>) against the CPU oracle with `scene.observations` and `s.prior` in the same loop (oracle/pgm.py:719-777),
started from the device's own state.  The cases live in tests/observations_prior_common.py; each is the smallest shape
that reaches its code path.

Tolerance: rel_err (max-norm relative) <= 1e-5 on SED, morphology and loss history; centres, iteration counts and flags
equal.  A scene beyond 1e-5 passes only through the float64-anchored threshold rule of tests/prior_common.py (restated
with the observations in the helper), at most ONE scene per test, every use printed by log_exemptions.
"""
import multiprocessing as mp
import os

import numpy as np
import pytest

from conftest import rel_err
import parity_common as pc
import observations_prior_common as oc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
TOL = oc.TOL
SENTINEL = -7.0


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


def make(scarlet, case, sl=slice(None), state=True):
    """the batch of the scenes in slice `sl` with the case's start loaded"""
    obs = []
    for o in case.obs:
        w = o.get("weights")
        w = w if w is None or np.ndim(w) == 0 else w[sl]
        if o.get("lowres") is not None:
            ob = scarlet.LowResObservationBatch(o["images"][sl], band0=o["band0"], geometry=o["lowres"], weights=w)
        else:
            ob = scarlet.ObservationBatch(o["images"][sl], band0=o["band0"], weights=w)
            if o.get("diff") is not None:
                ob.set_diff_kernel(o["diff"])
        obs.append(ob)
    kw = dict(mse_capacity=64, l0_thresh=case.l0, l1_thresh=case.l1)
    if case.group is not None:
        kw["group"] = case.group[sl]
    if case.cw is not None:
        kw["centroid_weight"] = case.cw
    centers = case.centers[sl]
    if case.ragged:
        centers = [c[:n] for c, n in zip(centers, case.n[sl])]
    b = scarlet.BlendBatch.from_observations(obs, centers, **kw)
    b.set_state(case.sed0[sl], case.morph0[sl])
    for name in ("fix_sed", "fix_morph"):
        f = getattr(case, name)
        if f is not None:
            setattr(b, name, torch.as_tensor(np.ascontiguousarray(f[sl], dtype=np.uint8)).to(b.device))
    b._fill_struct()
    return b


def quad(scarlet, case, sl=slice(None)):
    cut = lambda a: None if a is None else a[sl]
    return scarlet.QuadraticPrior(sed_weight=cut(case.ws), sed_target=cut(case.ts), morph_weight=cut(case.wm),
                                  morph_target=cut(case.tm))


def state0(b):
    torch.cuda.synchronize()
    return dict(sed=npy(b.sed_current), morph=npy(b.morph_current), cen=npy(b.centers), sh=npy(b.shifts))


def result(b):
    torch.cuda.synchronize()
    return dict(sed=npy(b.sed_current), morph=npy(b.morph_current), cen=npy(b.centers), it=npy(b.it), flags=npy(b.flags),
                mse=npy(b.mse_buf), status=npy(b.status), L=npy(b.lipschitz), active=npy(b.active),
                Lc=None if b.L_components is None else npy(b.L_components))


def check_against_oracle(scarlet, case, pool, st0, g, test, cap=1, support=False):
    """every scene of `g` (a `result`) against the float32 oracle; returns the oracle's results"""
    iters, e_rel = case.iters, case.e_rel
    ref = pool.map(oc.oracle_fit, [(case.spec(st0, i), iters, e_rel, np.float32) for i in range(case.S)])
    assert not g["status"].any(), g["status"]
    exempt = []
    worst = dict(sed=0.0, morph=0.0, mse=0.0)
    for i, r in enumerate(ref):
        n = int(case.n[i])
        np.testing.assert_array_equal(g["cen"][i][:n], r[3])
        assert g["it"][i] == r[4], (i, g["it"][i], r[4])
        if e_rel > 0:
            np.testing.assert_array_equal(g["flags"][i][:n] & 3, np.array(r[5]) & 3)
        e = dict(sed=rel_err(g["sed"][i][:n], r[0]), morph=rel_err(g["morph"][i][:n], r[1]),
                 mse=rel_err(g["mse"][i][:r[4]], r[2]))
        print("%s scene %d: %s" % (test, i, e))
        same_support = np.array_equal(g["morph"][i][:n] == 0, r[1] == 0)
        if max(e.values()) <= TOL and (same_support or not support):
            for k in worst:
                worst[k] = max(worst[k], e[k])
            continue
        # the float64-anchored rule, on a per-iteration re-run of the scene alone
        b1 = make(scarlet, case, slice(i, i + 1))
        p1 = quad(scarlet, case, slice(i, i + 1))
        snaps = []
        for _ in range(int(r[4])):
            b1.fit(1, e_rel=0, approximate_L=case.approximate_L, prior=p1)
            snaps.append(npy(b1.morph_current)[0][:n].copy())
        ok, msg = oc.straddles_threshold(snaps, case.spec(st0, i), int(r[4]))
        assert ok, "scene %d beyond 1e-5 (%s, same support %s) and not a threshold straddle: %s" % (i, e, same_support, msg)
        exempt.append((i, e, msg))
    pc.log_exemptions(test, exempt, cap)
    assert len(exempt) <= cap, exempt
    print("%s: %d scenes, worst errors %s" % (test, case.S, worst))
    return ref


def fit_case(scarlet, case, check_every=10):
    b = make(scarlet, case)
    st0 = state0(b)
    n = b.fit(case.iters, e_rel=case.e_rel, approximate_L=case.approximate_L, check_every=check_every, prior=quad(scarlet, case))
    return b, st0, result(b), n


def prior_moves(case, pool, st0, ref):
    """a prior that is silently dropped cannot pass: the oracle without it ends elsewhere"""
    plain = pool.map(oc.oracle_fit, [(case.spec(st0, i, prior=False), case.iters, 0.0, np.float32) for i in range(case.S)])
    moved = [rel_err(p[1], r[1]) for p, r in zip(plain, ref)]
    print("the prior moves the morphologies by", moved)
    assert min(moved) > 1e-3, moved


# ------------------------------------------------------------------ 1. - 5., 8.: every path against the oracle
PATHS = ["sliced_30x34", "epochs_30x34", "two_tiles_72x60", "k9", "k33", "approximate_L", "psf_mixed", "lowres"]


@pytest.mark.parametrize("name", PATHS)
def test_path_matches_the_oracle(env, name):
    """sliced / epochs 30 x 34: H W = 1020 is no multiple of 4 (the sweep's tail), inline residuals; 72 x 60: two tiles,
    the head sums their partials; K = 9: k_obs_contract<0, true> and the bigk constants; K = 33: hugek; approximate_L:
    OBS_PARTIALS, then OBS_STEP with the prior; psf_mixed: a G plane and an inline observation in one pass; lowres: a
    low-resolution observation's G planes beside a model-grid observation"""
    scarlet, pool = env
    case = oc.CASES[name]()
    b, st0, g, n = fit_case(scarlet, case)
    assert n == case.iters
    ref = check_against_oracle(scarlet, case, pool, st0, g, "observations + prior, %s" % name)
    prior_moves(case, pool, st0, ref)
    # the constants: the scene's (x n_obs, no prior in them) plus the weights, added in float32
    L, Lc = g["L"], g["Lc"]
    for j, w in ((0, case.ws), (1, case.wm)):
        want = np.where(w != 0, (L[:, j:j + 1].astype(np.float32) + w).astype(np.float64), L[:, j:j + 1])
        np.testing.assert_array_equal(Lc[..., j], want)


# ------------------------------------------------------------------ 6. ragged counts, fixed factors, a group
def test_ragged_fixed_and_grouped(env):
    scarlet, pool = env
    case = oc.CASES["ragged"]()
    S, K = case.S, case.K
    b = make(scarlet, case)
    st0 = state0(b)
    b.L_components = torch.full((S, K, 2), SENTINEL, dtype=torch.float64, device=b.device)    # to see what is written
    assert b.fit(case.iters, e_rel=0, prior=quad(scarlet, case)) == case.iters
    g = result(b)
    ref = check_against_oracle(scarlet, case, pool, st0, g, "observations + prior, ragged / fixed / grouped", cap=0)
    prior_moves(case, pool, st0, ref)
    present = np.arange(K)[None, :] < case.n[:, None]
    for buf in range(2):
        assert not npy(b.sed[buf])[~present].any() and not npy(b.morph[buf])[~present].any()
    assert (g["Lc"][~present] == SENTINEL).all()                       # absent components: not written
    Lc, L = g["Lc"], g["L"]
    # a fixed factor reports the scene's constant; the others add the weight in float32, the frame's dtype
    want_s = np.where(case.fix_sed, L[:, :1], (L[:, :1].astype(np.float32) + case.ws).astype(np.float64))
    want_m = np.where(case.fix_morph, L[:, 1:], (L[:, 1:].astype(np.float32) + case.wm).astype(np.float64))
    np.testing.assert_array_equal(Lc[..., 0][present], want_s[present])
    np.testing.assert_array_equal(Lc[..., 1][present], want_m[present])
    # a scene made inactive beforehand: its rows of L_comp and its state stay as they were (step() leaves `active` alone)
    b2 = make(scarlet, case)
    b2.L_components = torch.full((S, K, 2), SENTINEL, dtype=torch.float64, device=b2.device)
    b2.active[1] = 0
    before = result(b2)
    b2.step(e_rel=0, prior=quad(scarlet, case))
    after = result(b2)
    assert (after["Lc"][1] == SENTINEL).all() and (after["Lc"][0][present[0]] != SENTINEL).all()
    for key in ("sed", "morph", "L", "it", "mse"):
        np.testing.assert_array_equal(after[key][1], before[key][1])
    assert after["it"][0] == 1 and after["it"][1] == 0


# ------------------------------------------------------------------ 7. the sparsity cut
@pytest.mark.parametrize("name", ["l0", "l1"])
def test_sparsity_cut_uses_the_components_own_step(env, name):
    """l0_thresh / l1_thresh = 0.05: the cut is thresh / L_morph,k with L_morph,k = L_morph n_obs + w (update.py:71-82);
    the supports equal the oracle's, which cuts with the component's own step"""
    scarlet, pool = env
    case = oc.CASES[name]()
    b, st0, g, n = fit_case(scarlet, case)
    check_against_oracle(scarlet, case, pool, st0, g, "observations + prior + %s" % name, support=True)
    # the constant the cut divides by is the component's own: the scene's plus the weight (2000 on components 0 and 2)
    with_prior = case.wm != 0
    own = (g["L"][:, 1:].astype(np.float32) + case.wm).astype(np.float64)
    np.testing.assert_array_equal(g["Lc"][..., 1][with_prior], own[with_prior])
    assert (own[with_prior] >= np.broadcast_to(g["L"][:, 1:], own.shape)[with_prior] + 1999).all()


# ------------------------------------------------------------------ 9. / 10. the three forms, and a zero prior
def test_three_forms_agree_bit_for_bit(env):
    scarlet, _ = env
    case = oc.CASES["forms"]()
    b = make(scarlet, case)
    dev = lambda a: torch.as_tensor(a).to(b.device)
    ws, wm, ts, tm = dev(case.ws), dev(case.wm), dev(case.ts), dev(case.tm)

    def given(sed, morph):
        return dict(grad_sed=ws[..., None] * (sed - ts), grad_morph=wm[..., None, None] * (morph - tm), L_sed=ws, L_morph=wm)

    assert b.fit(case.iters, e_rel=0, prior=quad(scarlet, case)) == case.iters      # one library call
    q = result(b)
    b2 = make(scarlet, case)
    assert b2.fit(case.iters, e_rel=0, prior=given) == case.iters                   # the callable, once per iteration
    call = result(b2)
    b3 = make(scarlet, case)
    for _ in range(case.iters):                                                     # given tensors recomputed by the caller
        b3.step(e_rel=0, prior=given(b3.sed_current, b3.morph_current))
    step = result(b3)
    assert not q["status"].any() and (q["it"] == case.iters).all()
    for name, other in (("callable", call), ("step", step)):
        for key in ("sed", "morph", "mse", "Lc", "L", "cen", "it", "flags"):
            np.testing.assert_array_equal(other[key], q[key], err_msg="%s: %s" % (name, key))


def test_a_zero_prior_changes_nothing(env):
    scarlet, _ = env
    case = oc.CASES["forms"]()
    case.ws, case.wm = np.zeros_like(case.ws), np.zeros_like(case.wm)
    b = make(scarlet, case)
    b.fit(case.iters, e_rel=0, prior=quad(scarlet, case))
    zero = result(b)
    b2 = make(scarlet, case)
    b2.fit(case.iters, e_rel=0)
    plain = result(b2)
    for key in ("sed", "morph", "mse", "L", "cen", "it", "flags"):
        np.testing.assert_array_equal(zero[key], plain[key], err_msg=key)
    # prior_L hands L through unrounded when the prior's constant is 0
    np.testing.assert_array_equal(zero["Lc"], np.repeat(zero["L"][:, None, :], case.K, axis=1))


# ------------------------------------------------------------------ 11. one observation: two device paths
def test_one_observation_agrees_with_the_single_observation_batch(env):
    scarlet, _ = env
    case = oc.CASES["sliced_30x34"]()
    images = np.concatenate([o["images"] for o in case.obs], axis=1)
    case.obs = [dict(images=images, band0=0)]
    b = make(scarlet, case)
    b.fit(case.iters, e_rel=0, prior=quad(scarlet, case))
    joint = result(b)
    b1 = scarlet.BlendBatch(images, case.centers, mse_capacity=64)
    b1.set_state(case.sed0, case.morph0)
    b1.fit(case.iters, e_rel=0, prior=quad(scarlet, case))
    single = result(b1)
    e = {key: rel_err(joint[key], single[key]) for key in ("sed", "morph", "mse", "Lc", "L")}
    print("from_observations([a]) vs BlendBatch(images):", e)
    assert max(e.values()) <= TOL, e
    for key in ("cen", "it", "flags"):
        np.testing.assert_array_equal(joint[key], single[key])


# ------------------------------------------------------------------ 12. scenes stop on their own
def test_scenes_stop_on_their_own(env):
    scarlet, pool = env
    case = oc.CASES["stopping"]()
    b, st0, g, _ = fit_case(scarlet, case, check_every=2)
    _, _, g0, n0 = fit_case(scarlet, case, check_every=0)
    assert n0 == case.iters
    for key in ("it", "flags", "sed", "morph", "cen"):
        np.testing.assert_array_equal(g[key], g0[key])
    check_against_oracle(scarlet, case, pool, st0, g, "observations + prior to e_rel = %g" % case.e_rel)
    print("iterations:", g["it"])
    assert len(np.unique(g["it"])) > 1 and g["it"].max() < case.iters and not g["active"].any()


# ------------------------------------------------------------------ 13. no round trip per iteration
def test_callable_runs_once_per_iteration_without_host_sync(env):
    scarlet, _ = env
    case = oc.CASES["sliced_30x34"]()
    b = make(scarlet, case)
    S, K, C, H, W = case.S, case.K, case.C, case.H, case.W
    w = torch.full((S, K), 5.0, device=b.device)
    calls = []

    def fn(sed, morph):
        calls.append(1)
        assert sed.shape == (S, K, C) and morph.shape == (S, K, H, W) and sed.is_cuda
        return dict(grad_sed=w[..., None] * sed, L_sed=w)

    assert b.fit(10, e_rel=1e-3, check_every=0, prior=fn) == 10
    assert len(calls) == 10
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
        n = b._fit_prior(fn, 10, 1e-3, 0, 0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert n == 10 and len(calls) == 20
    print("10 iterations of the joint fit with a callable prior under set_sync_debug_mode('error'): no synchronising call")
