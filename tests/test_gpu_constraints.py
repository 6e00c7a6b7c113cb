"""-m gpu: batches whose components carry their own constraint switches (scarlet_constraints: symmetric, monotonic,
l0_thresh, l1_thresh per component) against the CPU oracle, whose sources have always had them (oracle/pgm.py:525-573).

Every oracle comparison starts the oracle from the device's own state after the start (sed, morph, centres, shifts), as
tests/parity_common.py does, sets the four switches on each oracle Source from the same arrays and fits.  Tolerance:
parity_common.TOL = 1e-5 max-norm relative on sed, morph and the loss history; centres, iteration counts and flags
bit-exact; the shifts of components without `symmetric` still NaN.

No threshold-straddle exemption: the cap is 0 scenes.  The seeds below were chosen on the CPU so that the reference
alone stays inside that cap -- for each scene, from the oracle's own starts, the float32 and the float64 oracle agree
on the support of every morphology after every iteration and differ by at most 1e-6
(constraints_common.seed_is_decided; tools/pick_constraint_seeds.py repeats the search and prints this table).

Setting pattern (constraints_common.pattern): component k of scene s takes the (symmetric, monotonic) pair
((1,1), (0,1), (1,0), (0,0))[(k + s) % 4]; component 0 of scene 0 has l0_thresh = 0.3, component 1 of scene 1 (scene 0
of a one-scene batch) l1_thresh = 0.2."""
import contextlib
import ctypes

import numpy as np
import pytest

from conftest import rel_err
import constraints_common as cc
from constraints_common import box_fallback
import parity_common as pc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
TOL = pc.TOL

SEEDS = {
    "fused_k4_b3": [5000, 5001, 5002, 5003],
    "fused_k3_b3": [5100, 5101, 5102, 5103],
    "fused_k4_b6": [5200, 5201, 5202, 5203],
    "fused_k4_b8": [6300, 6301, 6302, 6303],
    "box_72x80": [5300, 5301],
    "tile_128": [5400, 5401],
    "plane_160x144": [5500],
    "streamed_272x48": [5600],
    "k9_32": [5700, 5701],
    "ragged": [5800, 5801, 5802],
    "group": [5900, 5901],
    "prior": [6000, 6001],
    "two_obs": [6100, 6101],
    "blend_32": [6200],
    "blend_obs_32": [6400],
}
RAGGED_COUNTS = (2, 4, 3)
PRIOR_WEIGHTS = (0.3, 2.0)


@pytest.fixture(scope="module")
def scarlet():
    import scarlet_amd
    scarlet_amd._lib.require_gpu()
    from oracle import build as obuild
    obuild.build()
    return scarlet_amd


@contextlib.contextmanager
def option(scarlet, name, value=1):
    old = scarlet._lib.set_option(name, value)
    try:
        yield
    finally:
        scarlet._lib.set_option(name, old)


def scenes(name, K, B, H, W, counts=None):
    """images (S, B, H, W) and centres (S, K, 2) of the case's seeds; scene s of a ragged case has counts[s] sources"""
    from scarlet_amd import synth
    imgs, cens = [], []
    for s, seed in enumerate(SEEDS[name]):
        n = K if counts is None else counts[s]
        sc = synth.make_scene(seed, B=B, H=H, W=W, K=n, min_sep=3 if K > 4 else 4)
        c = np.zeros((K, 2), np.int32)
        c[:n] = sc["centers"]
        imgs.append(sc["images"]); cens.append(c)
    return np.stack(imgs), np.stack(cens)


def state(b):
    torch.cuda.synchronize()
    return dict(sed=b.sed_current.cpu().numpy(), morph=b.morph_current.cpu().numpy(), cen=b.centers.cpu().numpy(),
                shifts=b.shifts.cpu().numpy(), flags=b.flags.cpu().numpy(), mse=b.mse_buf.cpu().numpy(),
                it=b.it.cpu().numpy(), status=b.status.cpu().numpy(), lipschitz=b.lipschitz.cpu().numpy())


def assert_identical(a, b, what):
    for key in a:
        assert np.array_equal(a[key], b[key], equal_nan=True), "%s: %s differs" % (what, key)


def check_against_oracle(st0, st1, images, settings, iters, counts=None, extra=None, label=""):
    """every scene of the device run st0 -> st1 against the oracle started from st0[s] with the scene's own switches"""
    sym, mono, l0, l1 = settings
    S, K = sym.shape
    worst = 0.0
    assert int(np.abs(st1["status"]).sum()) == 0, st1["status"]
    for s in range(S):
        n = K if counts is None else int(counts[s])
        ex = {} if extra is None else extra(s, n)
        spec = cc.spec_of(images[s], st0["sed"][s, :n], st0["morph"][s, :n], st0["cen"][s, :n], st0["shifts"][s, :n],
                          sym[s, :n], mono[s, :n], l0[s, :n], l1[s, :n], **ex)
        ref = cc.oracle_fit(spec, iters)
        assert int(st1["it"][s]) == iters == ref["it"]
        np.testing.assert_array_equal(st1["cen"][s, :n], ref["cen"], err_msg="%s scene %d: centres" % (label, s))
        np.testing.assert_array_equal(st1["flags"][s, :n], ref["flags"], err_msg="%s scene %d: flags" % (label, s))
        e = dict(sed=rel_err(st1["sed"][s, :n], ref["sed"]), morph=rel_err(st1["morph"][s, :n], ref["morph"]),
                 mse=rel_err(st1["mse"][s, :iters], ref["mse"]))
        print("%s scene %d: %s" % (label, s, e))
        assert max(e.values()) <= TOL, "%s scene %d beyond 1e-5: %s" % (label, s, e)
        worst = max(worst, max(e.values()))
        grouped = ex.get("group")
        for k in range(n):
            if not sym[s, k] or (grouped is not None and grouped[k] >= 0 and iters < 5):
                continue
            assert np.isfinite(st1["shifts"][s, k]).all(), "%s scene %d: symmetric component %d has no shift" % (label, s, k)
        for k in range(n):                           # no symmetry, no centroid: the shift is never written
            if not sym[s, k]:
                assert np.isnan(st1["shifts"][s, k]).all(), "%s scene %d: component %d is not symmetric but has a shift" % (label, s, k)
        if counts is not None:
            assert not st1["sed"][s, n:].any() and not st1["morph"][s, n:].any() and not st1["flags"][s, n:].any()
    return worst


def run_extended(scarlet, name, K, B, H, W, iters, approximate_L=False, profile=False):
    """ExtendedSource starts with each component's own switches, `iters` iterations at e_rel = 0, oracle comparison"""
    images, centers = scenes(name, K, B, H, W)
    S = len(images)
    settings = cc.pattern(S, K)
    b = scarlet.BlendBatch(images, centers, symmetric=settings[0], monotonic=settings[1], l0_thresh=settings[2],
                           l1_thresh=settings[3], mse_capacity=iters + 1)
    assert b.constrained and b.symmetric and b.monotonic and b.l0_thresh is None and b.l1_thresh is None
    b.init_extended(np.ones(B) * cc.BG)
    st0 = state(b)
    L = scarlet._lib.lib
    if profile:
        scarlet._lib.check(L.scarlet_profile_begin(iters))
    assert b.fit(iters, e_rel=0, approximate_L=approximate_L, check_every=0) == iters
    counts = None
    if profile:
        ms, counts = (ctypes.c_double * 8)(), (ctypes.c_int64 * 8)()
        scarlet._lib.check(L.scarlet_profile_end(ms, counts))
        counts = list(counts)
    st1 = state(b)
    if H > 64 or W > 64:
        st1["fallback"], st1["mono"] = box_fallback(b), settings[1]
    check_against_oracle(st0, st1, images, settings, iters, extra=lambda s, n: dict(approximate_L=approximate_L),
                         label="%s%s" % (name, " approximate_L" if approximate_L else ""))
    return st1, counts


# ---------------------------------------------------------------------------------------------- 1, 2: small scenes
@pytest.mark.parametrize("name,K,B", [("fused_k4_b3", 4, 3), ("fused_k3_b3", 3, 3), ("fused_k4_b6", 4, 6), ("fused_k4_b8", 4, 8)])
def test_fused_per_component_instance(scarlet, name, K, B):
    """K <= 4, 24 x 32, no PSF, exact L: one launch per iteration of the four-wave kernel's per-component instance
    (profile class 4) and nothing else -- a silent fall to the general path fails here.  K = 3 leaves one wave idle;
    B = 3 would take the eight-wave kernels with scalars, B = 6 the four-wave one; B = 8 takes the second per-component
    instance, k_iterate<4, 8, FusedArgsPC>."""
    _, counts = run_extended(scarlet, name, K, B, 24, 32, 10, profile=True)
    assert counts == [0, 0, 0, 0, 10, 0, 0, 0], counts


@pytest.mark.parametrize("name,K,B", [("fused_k4_b3", 4, 3), ("fused_k3_b3", 3, 3), ("fused_k4_b6", 4, 6)])
def test_wave_per_component_general_kernel(scarlet, name, K, B):
    """the same scenes with approximate_L: the general path, k_source_update_w (one wave per component)"""
    _, counts = run_extended(scarlet, name, K, B, 24, 32, 10, approximate_L=True, profile=True)
    assert counts[4] == 0 and counts[2] == 10, counts


# ---------------------------------------------------------------------------------------------- 3 - 5: larger frames
def test_box_kernels_and_full_path_fallback(scarlet):
    """72 x 80: the monotonic components run on the box around their peak, the others are flagged and go through the
    full-frame kernel (only_flagged); with NO_BOX every component takes k_source_update<0>.  Both against the oracle and
    against each other to 1e-6.  That the components without `monotonic` were left to the full-frame kernel is read from
    the box kernels' own flags in the workspace (`box_fallback`: what only_flagged points at); that the full-frame kernel
    then processed exactly those has no hook of its own and shows only in the results: a flagged component nobody
    processed would keep its stepped, unnormalised morphology and miss the oracle."""
    a, _ = run_extended(scarlet, "box_72x80", 3, 2, 72, 80, 10)
    assert (a["fallback"][a["mono"] == 0] == 1).all(), a["fallback"]         # no sweep, no box: flagged every iteration
    assert (a["fallback"][a["mono"] == 1] == 0).any(), a["fallback"]         # the box served monotonic components
    with option(scarlet, "NO_BOX"):
        b, _ = run_extended(scarlet, "box_72x80", 3, 2, 72, 80, 10)
    for key in ("sed", "morph", "mse"):
        assert rel_err(a[key], b[key]) <= 1e-6, key
    for key in ("cen", "flags", "it"):
        assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(np.isnan(a["shifts"]), np.isnan(b["shifts"]))


def test_two_pipelines_offset_the_arrays_per_half(scarlet):
    """1024 scenes with a PSF kernel run as two half-batches on two streams (split_views): each half reads its own part
    of the four arrays.  Bit for bit the run with NO_PIPELINE, and the tiled copies of a scene -- whose settings repeat
    with them -- agree wherever they sit."""
    K, B, iters, U, S = 3, 2, 3, 8, 1024
    from scarlet_amd import synth
    sc = [synth.make_scene(6500 + i, B=B, H=24, W=32, K=K) for i in range(U)]
    images = np.tile(np.stack([x["images"] for x in sc]), (S // U, 1, 1, 1))
    centers = np.tile(np.stack([x["centers"] for x in sc]), (S // U, 1, 1))
    sym, mono, l0, l1 = cc.pattern(U, K)
    tile = lambda a: np.tile(a, (S // U, 1))
    y, x = np.mgrid[:5, :5]
    k = np.exp(-((y - 2) ** 2 + (x - 2) ** 2) / 2.0).astype(np.float32)
    diff = np.stack([k / k.sum()] * B)

    def run():
        b = scarlet.BlendBatch(images, centers, symmetric=tile(sym), monotonic=tile(mono), l0_thresh=tile(l0),
                               l1_thresh=tile(l1), mse_capacity=iters + 1)
        b.set_diff_kernel(diff)
        b.init_extended(np.ones(B) * cc.BG)
        n = int(scarlet._lib.lib.scarlet_batch_pipelines(ctypes.byref(b._c)))
        assert b.fit(iters, e_rel=0, check_every=0) == iters
        return n, state(b)

    n2, two = run()
    with option(scarlet, "NO_PIPELINE"):
        n1, one = run()
    assert (n2, n1) == (2, 1)
    assert int(np.abs(two["status"]).sum()) == 0 and (two["it"] == iters).all()
    assert_identical(one, two, "two pipelines")
    for key in ("sed", "morph", "cen", "shifts", "mse"):
        v = two[key].reshape((S // U, U) + two[key].shape[1:])
        assert np.array_equal(v, np.broadcast_to(v[:1], v.shape), equal_nan=True), key
    # the settings took effect in the second half too: shifts exactly where the component is symmetric
    assert np.array_equal(np.isnan(two["shifts"][..., 0]), tile(sym) == 0)


def test_tile_in_lds_scratch_in_hbm(scarlet):
    """128 x 128: box kernels for the monotonic components, k_source_update<1> for the rest"""
    run_extended(scarlet, "tile_128", 3, 2, 128, 128, 5)


@pytest.mark.parametrize("name,H,W", [("plane_160x144", 160, 144), ("streamed_272x48", 272, 48)])
def test_plane_in_hbm_and_streamed_box(scarlet, name, H, W):
    """160 x 144: k_source_update<2> (plane in HBM) behind the banded box; 272 x 48: the streamed box instance"""
    run_extended(scarlet, name, 3, 2, H, W, 5)


# ---------------------------------------------------------------------------------------------- 6: K > 8
def test_indexing_with_many_components(scarlet):
    """K = 9 (chunked gradient kernels): the pairs repeat along k, the arrays are indexed [s][k] with K = 9"""
    run_extended(scarlet, "k9_32", 9, 3, 32, 32, 10)


# ---------------------------------------------------------------------------------------------- 7: combinations
def test_ragged_counts(scarlet):
    K, B, iters = 4, 3, 6
    images, centers = scenes("ragged", K, B, 24, 32, counts=RAGGED_COUNTS)
    settings = cc.pattern(3, K)
    rows = lambda a, off=None: [[(None if (off is not None and v < 0) else v) for v in a[s, :n].tolist()]
                                for s, n in enumerate(RAGGED_COUNTS)]
    b = scarlet.BlendBatch(images, [c[:n] for c, n in zip(centers, RAGGED_COUNTS)], symmetric=rows(settings[0]),
                           monotonic=rows(settings[1]), l0_thresh=rows(settings[2], True), l1_thresh=rows(settings[3], True),
                           mse_capacity=iters + 1)
    assert b.constrained and b.n_components.tolist() == list(RAGGED_COUNTS)
    b.init_extended(np.ones(B) * cc.BG)
    st0 = state(b)
    assert b.fit(iters, e_rel=0, check_every=0) == iters
    check_against_oracle(st0, state(b), images, settings, iters, counts=RAGGED_COUNTS, label="ragged")


def test_two_layer_group_beside_a_source(scarlet):
    """a two-layer source sharing (1, 1) beside a (0, 1) source, against pgm.MultiSource"""
    K, B, iters = 3, 3, 6
    from scarlet_amd import synth
    imgs, cens = [], []
    for seed in SEEDS["group"]:
        sc = synth.make_scene(seed, B=B, H=24, W=32, K=2)
        imgs.append(sc["images"]); cens.append(sc["centers"][[0, 0, 1]])
    images, centers = np.stack(imgs), np.stack(cens)
    S = len(images)
    sym = np.tile(np.array([1, 1, 0], np.uint8), (S, 1)); mono = np.ones((S, K), np.uint8)
    off = np.full((S, K), -1.0, np.float32)
    group = np.tile(np.array([0, 0, -1], np.int32), (S, 1))
    with pytest.raises(ValueError):                    # the layers must agree
        scarlet.BlendBatch(images, centers, symmetric=[1, 0, 0], group=group)
    b = scarlet.BlendBatch(images, centers, symmetric=sym, monotonic=[1, 1, 1], group=group, mse_capacity=iters + 1)
    assert b.constrained
    b.init_sources(np.ones(B) * cc.BG)
    b.raise_on_status()
    st0 = state(b)
    assert np.isnan(st0["shifts"][:, 2]).all() and np.isfinite(st0["shifts"][:, :2]).all()
    assert b.fit(iters, e_rel=0, check_every=0) == iters
    check_against_oracle(st0, state(b), images, (sym, mono, off, off), iters,
                         extra=lambda s, n: dict(group=group[s]), label="group")


def test_quadratic_prior_and_the_component_step(scarlet):
    """a QuadraticPrior on component 0, which also has l0 set: its cut uses the component's own step 1 / L_comp"""
    K, B, iters = 4, 3, 6
    images, centers = scenes("prior", K, B, 24, 32)
    S = len(images)
    settings = cc.pattern(S, K)
    b = scarlet.BlendBatch(images, centers, symmetric=settings[0], monotonic=settings[1], l0_thresh=settings[2],
                           l1_thresh=settings[3], mse_capacity=iters + 1)
    b.init_extended(np.ones(B) * cc.BG)
    st0 = state(b)
    ws, wm = np.zeros(K), np.zeros(K)
    ws[0], wm[0] = PRIOR_WEIGHTS
    assert b.fit(iters, e_rel=0, check_every=0, prior=scarlet.QuadraticPrior(sed_weight=ws, morph_weight=wm)) == iters
    check_against_oracle(st0, state(b), images, settings, iters, extra=lambda s, n: dict(ws=ws, wm=wm), label="prior")
    # the prior's constant is in the step of component 0 and of no other
    Lc = b.L_components.cpu().numpy()
    assert (Lc[:, 0, 1] > Lc[:, 1, 1]).all() and (Lc[:, 1:, 1] == Lc[:, 1:2, 1]).all()


def test_two_observations(scarlet):
    K, B, iters = 4, 3, 6
    images, centers = scenes("two_obs", K, B, 24, 32)
    S = len(images)
    settings = cc.pattern(S, K)
    obs = [scarlet.ObservationBatch(images[:, :2], band0=0), scarlet.ObservationBatch(images[:, 2:], band0=2)]
    b = scarlet.BlendBatch.from_observations(obs, centers, symmetric=settings[0], monotonic=settings[1],
                                             l0_thresh=settings[2], l1_thresh=settings[3], mse_capacity=iters + 1)
    assert b.constrained
    b.init_combined([np.ones(2) * cc.BG, np.ones(1) * cc.BG])
    st0 = state(b)
    assert b.fit(iters, e_rel=0, check_every=0) == iters
    extra = lambda s, n: dict(observations=[dict(images=images[s, :2], band_slice=slice(0, 2)),
                                            dict(images=images[s, 2:], band_slice=slice(2, 3))])
    check_against_oracle(st0, state(b), np.zeros_like(images), settings, iters, extra=extra, label="two observations")


# ---------------------------------------------------------------------------------------------- 8: constructors
def test_constructors_honour_each_components_settings(scarlet):
    """init_extended on a constrained batch = the oracle's init_extended_source + source_update(it = 0) with the
    source's own switches; through init_sources a scene with a bad bg_rms row keeps STATUS_BAD_INIT and is not touched
    by the update call, which ignores `active`"""
    K, B = 4, 3
    images, centers = scenes("fused_k4_b3", K, B, 24, 32)
    S = len(images)
    sym, mono, l0, l1 = settings = cc.pattern(S, K)
    kw = dict(symmetric=sym, monotonic=mono, l0_thresh=l0, l1_thresh=l1)

    def check(st, s):
        sed, morph, cen, sh = cc.oracle_start(images[s], centers[s], sym[s], mono[s], l0[s], l1[s])
        assert rel_err(st["sed"][s], sed) <= TOL and rel_err(st["morph"][s], morph) <= TOL, s
        np.testing.assert_array_equal(st["cen"][s], cen)
        assert np.array_equal(np.isnan(st["shifts"][s]), np.isnan(sh)), (st["shifts"][s], sh)
        assert np.array_equal(np.isnan(sh[:, 0]), sym[s] == 0)
        ok = ~np.isnan(sh)
        assert np.abs(st["shifts"][s][ok] - sh[ok]).max() <= 1e-4

    b = scarlet.BlendBatch(images, centers, **kw).init_extended(np.ones(B) * cc.BG)
    st = state(b)
    for s in range(S):
        check(st, s)
    # run_update=False leaves the start as the scalar batch's
    plain = scarlet.BlendBatch(images, centers).init_extended(np.ones(B) * cc.BG, run_update=False)
    noup = scarlet.BlendBatch(images, centers, **kw).init_extended(np.ones(B) * cc.BG, run_update=False)
    assert_identical(state(plain), state(noup), "run_update=False")

    bg = np.ones((S, B), np.float32) * cc.BG
    bg[1, 2] = 0.0                                              # scene 1: bad input
    b = scarlet.BlendBatch(images, centers, **kw)
    mark_sed = np.full((S, K, B), 2.0, np.float32)
    mark_morph = np.full((S, K, 24, 32), 0.5, np.float32)       # (an update would normalise this to 1)
    b.set_state(mark_sed, mark_morph)
    b.init_sources(bg)
    st = state(b)
    assert st["status"][1] & scarlet._lib.STATUS_BAD_INIT and not (st["status"][[0, 2, 3]] & scarlet._lib.STATUS_BAD_INIT).any()
    assert int(b.active[1].item()) == 0
    assert (st["sed"][1] == 2.0).all() and (st["morph"][1] == 0.5).all() and np.isnan(st["shifts"][1]).all()
    np.testing.assert_array_equal(st["cen"][1], centers[1])
    for s in (0, 2, 3):
        check(st, s)
    # ... and a later update_sources() call leaves it alone too
    b.update_sources()
    st = state(b)
    assert (st["sed"][1] == 2.0).all() and (st["morph"][1] == 0.5).all() and np.isnan(st["shifts"][1]).all()

    # a count outside 1..K found on the device: STATUS_BAD_COUNT, the scene untouched by start, update and fit
    b = scarlet.BlendBatch(images, centers, n_components=[K] * S, **kw)
    b.set_state(mark_sed, mark_morph)
    b.n_components[2] = K + 1
    b.init_extended(np.ones(B) * cc.BG)
    b.update_sources()
    b.fit(2, e_rel=0, check_every=0)
    st = state(b)
    assert st["status"][2] == scarlet._lib.STATUS_BAD_COUNT and not st["status"][[0, 1, 3]].any()
    assert int(b.active[2].item()) == 0 and st["it"][2] == 0 and (st["it"][[0, 1, 3]] == 2).all()
    assert (st["sed"][2] == 2.0).all() and (st["morph"][2] == 0.5).all() and np.isnan(st["shifts"][2]).all()
    np.testing.assert_array_equal(st["cen"][2], centers[2])


# ---------------------------------------------------------------------------------------------- 9: nothing else moved
@pytest.mark.parametrize("sym,mono,l0,l1", [(True, True, None, None), (False, True, 0.3, None), (True, False, None, 0.2)])
@pytest.mark.parametrize("path", ["general", "fused"])
def test_arrays_of_the_scalars_equal_the_scalar_call(scarlet, path, sym, mono, l0, l1):
    """arrays filled with the batch's scalars give, bit for bit, what the scalar call gives: every factor, centre, shift,
    flag and loss.  General path: approximate_L.  Fused path: against the scalar call with FUSED_V1 on, which is the
    same four-wave kernel."""
    K, B, iters = 4, 3, 6
    images, centers = scenes("fused_k4_b3", K, B, 24, 32)
    S = len(images)
    approx = path == "general"

    def run(**kw):
        b = scarlet.BlendBatch(images, centers, mse_capacity=iters + 1, **kw).init_extended(np.ones(B) * cc.BG)
        start = state(b)
        assert b.fit(iters, e_rel=0, approximate_L=approx, check_every=0) == iters
        b.step(e_rel=0, approximate_L=approx)                 # ... and the three phases called one by one
        return b, start, state(b)

    with option(scarlet, "FUSED_V1", 0 if approx else 1):
        b0, start0, end0 = run(symmetric=sym, monotonic=mono, l0_thresh=l0, l1_thresh=l1)
    b1, start1, end1 = run(symmetric=scarlet.batch.constraint_arrays(sym, S, K, "symmetric"),
                           monotonic=scarlet.batch.constraint_arrays(mono, S, K, "monotonic"),
                           l0_thresh=scarlet.batch.constraint_arrays(l0, S, K, "l0_thresh"),
                           l1_thresh=scarlet.batch.constraint_arrays(l1, S, K, "l1_thresh"))
    assert not b0.constrained and b1.constrained
    assert_identical(start0, start1, "start")
    assert_identical(end0, end1, "fit + step")
    for x, y in zip(b0.sed + b0.morph, b1.sed + b1.morph):     # both buffers, on the device
        assert torch.equal(x, y)
    assert torch.equal(b0.centers, b1.centers) and torch.equal(b0.flags, b1.flags) and torch.equal(b0.mse_buf, b1.mse_buf)


# ---------------------------------------------------------------------------------------------- 10: single-scene Blend
def test_blend_of_sources_that_disagree(scarlet):
    """two ExtendedSources, one symmetric=False and one monotonic=False: the blend stays on the device pipeline and
    agrees with the per-source Python update() pipeline"""
    from scarlet_amd import synth
    scn = synth.make_scene(SEEDS["blend_32"][0], B=3, H=32, W=32, K=2)
    images = scn["images"]
    frame = scarlet.Frame(images.shape)
    bg = np.ones(3) * cc.BG
    npy = lambda t: t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)

    def blend(python_pipeline):
        obs = scarlet.Observation(images).match(frame)
        cen = [tuple(int(v) for v in p) for p in scn["centers"]]
        srcs = [scarlet.ExtendedSource(frame, cen[0], obs, bg, symmetric=False),
                scarlet.ExtendedSource(frame, cen[1], obs, bg, monotonic=False)]
        bl = scarlet.Blend(srcs, obs)
        bl.python_pipeline = python_pipeline
        return bl

    dev, ref = blend(False), blend(True)
    assert dev._builtin_pipeline() and not ref._builtin_pipeline()
    dev.fit(10, e_rel=0)
    ref.fit(10, e_rel=0)
    assert dev._batch.constrained and not ref._batch.constrained
    assert len(dev.mse) == len(ref.mse) == 10
    assert rel_err(dev.mse, ref.mse) <= TOL
    for a, b in zip(dev.components, ref.components):
        assert rel_err(npy(a.sed), npy(b.sed)) <= TOL and rel_err(npy(a.morph), npy(b.morph)) <= TOL
        assert tuple(a.pixel_center) == tuple(b.pixel_center)
    # the source without symmetry never got a shift; the other one did
    sh = dev._batch.shifts[0].cpu().numpy()
    assert np.isnan(sh[0]).all() and np.isfinite(sh[1]).all()


def test_blend_of_sources_that_disagree_with_two_observations(scarlet):
    """the same pair of sources fitted against two band slices of the data (Blend(sources, [obs_a, obs_b])): the device
    loop is scarlet_fit_observations_constrained, the Python pipeline combines the gradients on the host"""
    from scarlet_amd import synth
    scn = synth.make_scene(SEEDS["blend_obs_32"][0], B=3, H=32, W=32, K=2)
    images, ch = scn["images"], list("gri")
    frame = scarlet.Frame(images.shape, channels=ch)
    bg = np.ones(3) * cc.BG
    npy = lambda t: t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)

    def blend(python_pipeline):
        full = scarlet.Observation(images, channels=ch).match(frame)
        obs = [scarlet.Observation(images[:2], channels=ch[:2]).match(frame),
               scarlet.Observation(images[2:], channels=ch[2:]).match(frame)]
        cen = [tuple(int(v) for v in p) for p in scn["centers"]]
        srcs = [scarlet.ExtendedSource(frame, cen[0], full, bg, symmetric=False),
                scarlet.ExtendedSource(frame, cen[1], full, bg, monotonic=False)]
        bl = scarlet.Blend(srcs, obs)
        bl.python_pipeline = python_pipeline
        return bl

    dev, ref = blend(False), blend(True)
    assert dev._builtin_pipeline() and not ref._builtin_pipeline()
    dev.fit(10, e_rel=0)
    ref.fit(10, e_rel=0)
    assert dev._batch.constrained and dev._batch._observations is not None and len(dev.mse) == len(ref.mse) == 10
    assert rel_err(dev.mse, ref.mse) <= TOL
    for a, b in zip(dev.components, ref.components):
        assert rel_err(npy(a.sed), npy(b.sed)) <= TOL and rel_err(npy(a.morph), npy(b.morph)) <= TOL
        assert tuple(a.pixel_center) == tuple(b.pixel_center)
    sh = dev._batch.shifts[0].cpu().numpy()
    assert np.isnan(sh[0]).all() and np.isfinite(sh[1]).all()
