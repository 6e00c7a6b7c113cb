"""GPU: the low-resolution operator past its LDS limit -- the streamed form of csrc/lowres_stream.h (k_lrs_gemm and the
elementwise kernels between its launches) behind the *_large entry points -- at the smallest shapes at which it can go
wrong (lowres_large_common.LARGE, lowres_common.LIMITS):

  j   17 x 23 / 5 x 7: every GEMM dimension off 16 and off 4, one ragged tile per product (LOWRES_STREAMED)
  d   64 x 64 at B = 8: several tiles per product, where the LDS form runs too (LOWRES_STREAMED)
  p   96 x 96 / 48 x 48 at B = 3: the first shape past LDS
  n   100 x 90 / 30 x 27: non-square, past LDS
  r   256 x 256 / 48 x 48, ratio 5: K-loops of 17 steps, 8 x 5 tiles a plane

against float64 (resampling.apply_factors / adjoint_factors, lowres_common.fit).  Parity is the project's 1e-5 max-norm
relative; a float32 emulation of the sandwich on the CPU predicts 0.7e-6 to 1.7e-6 for the operator.  The fits run S = 3
scenes for 6 iterations at e_rel = 0; their seeds were chosen on the CPU by tools/pick_lowres_large_seeds.py: the
float32 and the float64 restatement agree on the support of every morphology after every iteration and differ by at most
1e-6, so the reference alone is decided and no exemption is used."""
import functools

import numpy as np
import pytest

import lowres_common as lc
import lowres_large_common as ll
import test_gpu_lowres_limits as lim
from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-5
S = lim.S
ITERS = lim.ITERS


@functools.lru_cache(maxsize=None)
def _geometries(name, per_scene, B, n_scenes=S):
    if not per_scene:
        return ll.geometry(name, B=B)[0]
    if name in lc.LIMITS:
        return lim._geometries(name, True, B)
    # per scene: the observation cut half a pixel further in plus the scene's phase; p, which spans its model frame, gets
    # an observation one pixel smaller (47 x 47)
    (h, w), org = ll.LARGE[name][1], ll.LARGE[name][3]
    shape = (h - 1, w - 1) if name == "p" else (h, w)
    return [ll.geometry(name, B=B, lr_shape=shape, origin=(org[0] + 0.5 + dy, org[1] + 0.5 + dx))[0]
            for dy, dx in lim.PHASES[:n_scenes]]


# (geometry, LOWRES_STREAMED, scenes, bands)
OPERATOR_SHAPES = [("j", 1, 3, 3), ("d", 1, 3, 8), ("p", 0, 3, 3), ("n", 0, 3, 3), ("r", 0, 2, 2)]


@pytest.mark.parametrize("per_scene", [False, True], ids=["shared", "per_scene"])
@pytest.mark.parametrize("name,streamed,n_scenes,B", OPERATOR_SHAPES, ids=[s[0] for s in OPERATOR_SHAPES])
def test_operator_and_adjoint_match_float64(name, streamed, n_scenes, B, per_scene):
    from scarlet_amd import resampling as rs
    geo = _geometries(name, per_scene, B, n_scenes)
    x, y, band, scene = ll.planes(geo, n_scenes, B)
    with ll.options(LOWRES_STREAMED=streamed):
        Tx, Ty = ll.operate(geo, n_scenes, B, x, y, band, scene)
    worst = np.zeros((n_scenes, 3))
    for p in range(n_scenes * B):
        f = (geo[scene[p]] if per_scene else geo).factors
        f = dict(f, dhat=f["dhat"][band[p]:band[p] + 1])
        e1, e2 = rel_err(Tx[p], rs.apply_factors(f, x[p:p + 1])[0]), rel_err(Ty[p], rs.adjoint_factors(f, y[p:p + 1])[0])
        # <T x, y> = <x, T^T y>, each side with the float32 rounding of one pass through the GEMM chain
        lhs, rhs = np.sum(Tx[p] * y[p]), np.sum(x[p].astype(np.float64) * Ty[p])
        e3 = abs(lhs - rhs) / (np.linalg.norm(Tx[p]) * np.linalg.norm(y[p]))
        worst[scene[p]] = np.maximum(worst[scene[p]], (e1, e2, e3))
    for s in range(n_scenes):
        print("streamed: geometry %s %s B = %d scene %d, worst band: render %.3e adjoint %.3e identity %.3e"
              % ((name, "per scene" if per_scene else "shared", B, s) + tuple(worst[s])))
    assert worst.max() <= TOL


# ------------------------------------------------------------------------------------------------- the forms against each other
@pytest.mark.parametrize("name", ["d", "j"])
def test_streamed_form_agrees_with_the_lds_form(name):
    B = lc.LIMITS[name][5]
    geo = _geometries(name, False, B)
    x, y, band, scene = ll.planes(geo, S, B, seed=8)
    lds = ll.operate(geo, S, B, x, y, band, scene, large=False)
    with ll.options(LOWRES_STREAMED=1):
        streamed = ll.operate(geo, S, B, x, y, band, scene)
    for what, a, b in (("render", streamed[0], lds[0]), ("adjoint", streamed[1], lds[1])):
        print("geometry %s %s: streamed vs LDS form %.3e" % (name, what, rel_err(a, b)))
        assert rel_err(a, b) <= TOL


@pytest.mark.parametrize("name", ["d", "j"])
def test_new_entry_points_are_the_old_ones_where_lds_holds(name):
    """LOWRES_STREAMED off: the *_large calls launch the LDS-resident kernels, bit for bit"""
    B = lc.LIMITS[name][5]
    geo = _geometries(name, False, B)
    x, y, band, scene = ll.planes(geo, S, B, seed=9)
    old = ll.operate(geo, S, B, x, y, band, scene, large=False)
    with ll.options(LOWRES_STREAMED=0):
        new = ll.operate(geo, S, B, x, y, band, scene)
    np.testing.assert_array_equal(new[0], old[0])
    np.testing.assert_array_equal(new[1], old[1])


# ------------------------------------------------------------------------------------------------- the switches
@pytest.mark.parametrize("name,streamed", [("j", 1), ("p", 0)])
def test_plain_fma_form_of_the_streamed_operator_is_bit_identical(name, streamed):
    B = ll.spec(name)[5]
    geo = _geometries(name, False, B)
    x, y, band, scene = ll.planes(geo, S, B, seed=8)
    with ll.options(LOWRES_STREAMED=streamed, NO_LOWRES_MFMA=0):
        mfma = ll.operate(geo, S, B, x, y, band, scene)
    with ll.options(LOWRES_STREAMED=streamed, NO_LOWRES_MFMA=1):
        plain = ll.operate(geo, S, B, x, y, band, scene)
    for what, a, b in (("render", mfma[0], plain[0]), ("adjoint", mfma[1], plain[1])):
        print("geometry %s %s: streamed MFMA vs plain FMA %.3e" % (name, what, rel_err(a, b)))
        np.testing.assert_array_equal(a, b)


def test_chunks_of_five_planes_are_bit_identical():
    """12 planes (S = 4, B = 3 at 96 x 96) in chunks of 5, 5 and 2 against one chunk"""
    geo = _geometries("p", False, 3)
    x, y, band, scene = ll.planes(geo, 4, 3, seed=10)
    with ll.options(LOWRES_CHUNK=0):
        whole = ll.operate(geo, 4, 3, x, y, band, scene)
    with ll.options(LOWRES_CHUNK=5):
        chunked = ll.operate(geo, 4, 3, x, y, band, scene)
    np.testing.assert_array_equal(whole[0], chunked[0])
    np.testing.assert_array_equal(whole[1], chunked[1])


# ------------------------------------------------------------------------------------------------- the joint fits
class Case(lim.Case):
    """lim.Case whose low-resolution observations may carry one geometry per scene ("geo": a list of S)"""

    def __init__(self, model_shape, C, centers, observations, seed, centroid_weight, **kw):
        first = [dict(o, geo=o["geo"][0]) if isinstance(o.get("geo"), list) else o for o in observations]
        lim.Case.__init__(self, model_shape, C, centers, first, seed, centroid_weight, **kw)
        for mine, given in zip(self.obs, observations):
            if isinstance(given.get("geo"), list):
                mine["geos"] = given["geo"]

    def _with_scene(self, s):
        return [dict(o, geo=o["geos"][s]) if "geos" in o else o for o in self.obs]

    def oracle(self, s, dt=np.float32, trace=None):
        keep, self.obs = self.obs, self._with_scene(s)
        try:
            return lim.Case.oracle(self, s, dt, trace)
        finally:
            self.obs = keep

    def batch(self):
        keep, self.obs = self.obs, [dict(o, geo=o["geos"]) if "geos" in o else o for o in self.obs]
        try:
            return lim.Case.batch(self)
        finally:
            self.obs = keep


def _lo(name, band0, C, B=2, per_scene=False, weights="map"):
    if per_scene:
        (h, w), org = ll.LARGE[name][1], ll.LARGE[name][3]
        shape = (h - 1, w - 1) if name == "p" else (h, w)
        geo = [ll.geometry(name, B=B, band0=band0, C=C, lr_shape=shape, origin=(org[0] + 0.5 + dy, org[1] + 0.5 + dx))[0]
               for dy, dx in lim.PHASES]
    else:
        geo = ll.geometry(name, B=B, band0=band0, C=C)[0]
    return dict(geo=geo, band0=band0, B=B, weights=weights, wscale=1.0)


def _centers(name, K):
    H, W = ll.LARGE[name][0]
    return [(int(fy * H), int(fx * W)) for fy, fx in lim.CEN5[:K]]


def _cw(name):
    return lc.limit_psfs(ll.LARGE[name][4], 1)[0][0]


# the seeds: tools/pick_lowres_large_seeds.py
SEEDS = {"joint": 51, "ragged": 53, "constrained": 53, "per_scene": 54, "inactive": 55, "nonsquare": 56}


def _joint(seed=None):
    """96 x 96: a same-grid observation with a PSF on channels 0 - 2, the low-resolution one on channels 3 - 4"""
    return Case(ll.LARGE["p"][0], 5, _centers("p", 3), [lim._hi(0, 3, psf=True), _lo("p", 3, 5)],
                SEEDS["joint"] if seed is None else seed, _cw("p"), sigma=3.0)


def _ragged(seed=None):
    """the same with K = 5; the scenes use 5, 2 and 3 of them"""
    return Case(ll.LARGE["p"][0], 5, _centers("p", 5), [lim._hi(0, 3, psf=True), _lo("p", 3, 5)],
                SEEDS["ragged"] if seed is None else seed, _cw("p"), sigma=3.0, counts=[5, 2, 3])


def _constrained(seed=None):
    """the same with K = 3 components that carry their own switches, an l1 threshold on one and fix_sed on one (no
    fix_morph at e_rel = 0: test_gpu_lowres_limits._constrained says why)"""
    return Case(ll.LARGE["p"][0], 5, _centers("p", 3), [lim._hi(0, 3, psf=True), _lo("p", 3, 5)],
                SEEDS["constrained"] if seed is None else seed, _cw("p"), sigma=3.0,
                symmetric=[True, False, True], monotonic=[True, True, False], l1_thresh=[None, 0.05, None],
                fix_sed=[False, False, True])


def _per_scene(seed=None):
    """every scene with its own vy, vx and dhat (47 x 47 observations cut at different sub-pixel phases)"""
    return Case(ll.LARGE["p"][0], 5, _centers("p", 3), [lim._hi(0, 3, psf=True), _lo("p", 3, 5, per_scene=True)],
                SEEDS["per_scene"] if seed is None else seed, _cw("p"), sigma=3.0)


def _inactive(seed=None):
    return Case(ll.LARGE["p"][0], 4, _centers("p", 3), [lim._hi(0, 2), _lo("p", 2, 4)],
                SEEDS["inactive"] if seed is None else seed, _cw("p"), sigma=3.0)


def _nonsquare(seed=None):
    """100 x 90 with a 30 x 27 observation, the low-resolution observation first in the list"""
    return Case(ll.LARGE["n"][0], 4, _centers("n", 3), [_lo("n", 0, 4, B=3), lim._hi(2, 2)],
                SEEDS["nonsquare"] if seed is None else seed, _cw("n"), sigma=3.0)


CASES = {"joint": _joint, "ragged": _ragged, "constrained": _constrained, "per_scene": _per_scene, "nonsquare": _nonsquare}


@pytest.mark.parametrize("which", sorted(CASES))
def test_joint_fit_matches_the_float_restatement(which):
    case = CASES[which]()
    b = case.batch()
    assert b.fit(ITERS, e_rel=0) == ITERS
    b.raise_on_status()
    for s in range(S):
        lim._compare(b, s, case.oracle(s), case.n(s), "streamed " + which)


def _outputs(b):
    return [t.cpu().numpy() for t in (b.sed_current, b.morph_current, b.mse_buf, b.centers, b.flags, b.lipschitz, b.it)]


def test_inactive_scene_stays_untouched():
    """Scene 1 inactive: no kernel of the streamed form writes its gradient planes or losses, its factors stay, and the
    other scenes fit as ever"""
    import torch
    case = _inactive()
    b = case.batch()
    work = b._lowres[1][1]["workspace"]
    work.fill_(0x5a)
    H, W = ll.LARGE["p"][0]
    B = 2
    planes = work[:S * B * H * W * 4].view(S, B * H * W * 4)
    losses = work[(S * B * H * W * 4 + 15) // 16 * 16:][:S * B * 8].view(S, B * 8)
    b._ensure_mse_capacity(ITERS)
    b.active.fill_(1)
    b.active[1] = 0
    before = [t.clone() for t in (b.sed[0], b.sed[1], b.morph[0], b.morph[1])]
    b._lib_fit(None, ITERS, 0.0, False, 0)
    torch.cuda.synchronize()
    assert bool((planes[1] == 0x5a).all()) and bool((losses[1] == 0x5a).all())
    assert not bool((planes[0] == 0x5a).all()) and not bool((losses[2] == 0x5a).all())
    for t0, t1 in zip(before, (b.sed[0], b.sed[1], b.morph[0], b.morph[1])):
        assert torch.equal(t0[1], t1[1])
    assert int(b.it[1].item()) == 0
    for s in (0, 2):
        lim._compare(b, s, case.oracle(s), case.n(s), "streamed inactive")


def test_fit_is_deterministic():
    """the same fit twice: every output array bit-identical (the loss sums have a fixed order, no atomics)"""
    def run():
        b = _ragged().batch()
        assert b.fit(ITERS, e_rel=0) == ITERS
        return _outputs(b)
    for a, b in zip(run(), run()):
        np.testing.assert_array_equal(a, b)


def test_switches_leave_a_fit_unchanged():
    """NO_LOWRES_MFMA and LOWRES_CHUNK = 5 (6 planes: a ragged last chunk) on a joint fit at 96 x 96: bit-identical"""
    def run():
        b = _joint().batch()
        assert b.fit(ITERS, e_rel=0) == ITERS
        return _outputs(b)
    base = run()
    for values in (dict(NO_LOWRES_MFMA=1), dict(LOWRES_CHUNK=5)):
        with ll.options(**values):
            for a, b in zip(base, run()):
                np.testing.assert_array_equal(a, b)


def test_streamed_fit_agrees_with_the_lds_fit():
    """geometry d at C = 8, K = 5 (test_gpu_lowres_limits' largest fit) through LOWRES_STREAMED: the band models are
    projected instead of the components, so the two forms differ by rounding only"""
    def run():
        b = lim._at_the_limit("d").batch()
        assert b.fit(ITERS, e_rel=0) == ITERS
        return _outputs(b)
    lds = run()
    with ll.options(LOWRES_STREAMED=1):
        streamed = run()
    for what, a, b in zip(("sed", "morph", "mse"), streamed, lds):
        print("fit at geometry d, %s: streamed vs LDS form %.3e" % (what, rel_err(a, b)))
        assert rel_err(a, b) <= TOL
    for a, b in zip(streamed[3:5], lds[3:5]):
        np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------------------------------------- the reference API
def test_render_loss_and_blend_at_96_match_the_fixture():
    """The public single-observation interface past LDS, against tests/golden/lowres_large.npz: LowResObservation.render /
    get_loss at 96 x 96 and 256 x 256; a batch of one scene from the fixture's start against the reference's 5-iteration
    Blend.fit (2e-5: the float32 bound of the comparisons with the reference's own float32 fits, tests/test_lowres_host.py);
    and a Blend of CombinedExtendedSources on the 96 x 96 frame, which is that batch of one bit for bit"""
    import scarlet_amd as scarlet
    from conftest import load_golden
    g = load_golden("lowres_large")
    for name in ("p", "r"):
        ch = ("r", "i")[:len(g[name + "_lr_psfs"])]
        obs, _ = lc.geometry(g, name, model_channels=ch, channels=ch)
        model = g[name + "_models"][0]
        e_render = rel_err(obs.render(model).cpu().numpy(), g[name + "_renders"][0])
        e_loss = abs(float(obs.get_loss(model)) - g[name + "_losses"][0]) / g[name + "_losses"][0]
        print("fixture %s: render %.3e loss %.3e" % (name, e_render, e_loss))
        assert max(e_render, e_loss) <= TOL
    name = "p"
    obs, (sed0, morph0, cen0), cw, lo = lc.fit_inputs(g, name)
    hi_b = scarlet.ObservationBatch(obs[0]["images"][None], band0=0).set_diff_kernel(obs[0]["diff_kernel"])
    lo_b = scarlet.LowResObservationBatch(obs[1]["images"][None], band0=3, geometry=lo, weights=obs[1]["weights"][None])
    b = scarlet.BlendBatch.from_observations([hi_b, lo_b], cen0[None], centroid_weight=cw)
    b.set_state(sed0[None], morph0[None])
    assert b.fit(5, e_rel=0) == 5
    errs = (rel_err(b.mse(0), g[name + "_fit_mse"]), rel_err(b.sed_current[0].cpu().numpy(), g[name + "_fit_sed"]),
            rel_err(b.morph_current[0].cpu().numpy(), g[name + "_fit_morph"]))
    print("fixture p, fit against the reference's: mse %.3e sed %.3e morph %.3e" % errs)
    assert max(errs) <= 2e-5
    np.testing.assert_array_equal(b.centers[0].cpu().numpy(), g[name + "_fit_centers"])
    np.testing.assert_array_equal(b.flags[0].cpu().numpy(), g[name + "_fit_flags"])
    # Blend
    lo, frame = lc.geometry(g, name, model_channels=lc.CH5, channels=lc.CH5[3:], images=g[name + "_fit_images_lr"].copy())
    hi = scarlet.Observation(g[name + "_fit_images_hr"].copy(), psfs=g[name + "_hr_psfs"].copy(), channels=lc.CH5[:3]).match(frame)
    bg = [np.ones(3, np.float32) * 0.01, np.ones(2, np.float32) * 0.01]
    centers = [tuple(int(v) for v in c) for c in cen0]
    sources = [scarlet.CombinedExtendedSource(frame, c, [hi, lo], bg, symmetric=True, monotonic=True) for c in centers]
    sed0 = np.stack([np.asarray(s.sed.cpu()) for s in sources])
    morph0 = np.stack([np.asarray(s.morph.cpu()) for s in sources])
    blend = scarlet.Blend(sources, [hi, lo]).fit(5, e_rel=0)
    hi_b = scarlet.ObservationBatch(hi.images[None], band0=0).set_diff_kernel(np.asarray(hi._diff_kernels.image, dtype=np.float32))
    lo_b = scarlet.LowResObservationBatch(lo.images[None], band0=3, geometry=lo, weights=lo.weights[None])
    b = scarlet.BlendBatch.from_observations([hi_b, lo_b], np.array(centers, dtype=np.int32)[None])
    b.set_state(sed0[None], morph0[None])
    assert b.fit(5, e_rel=0) == 5
    np.testing.assert_array_equal(np.stack([np.asarray(s.sed.cpu()) for s in sources]), b.sed_current[0].cpu().numpy())
    np.testing.assert_array_equal(np.stack([np.asarray(s.morph.cpu()) for s in sources]), b.morph_current[0].cpu().numpy())
    assert blend.mse == b.mse(0) and len(blend.mse) == 5
