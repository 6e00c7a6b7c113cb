"""GPU: the low-resolution operator (lowres.h: k_lowres_planes, k_lowres_render, k_lowres_adjoint, lr_gemm) where the
fixture geometries of test_gpu_lowres.py never take it -- lowres_common.LIMITS:

  d, g, f, e  133 - 158 KiB of dynamic LDS, the opt-in range above 48 KiB, at their largest B (8, 8, 6, 2)
  h           the scratch buffers sized by h x ldw instead of 2 nfy x ld2x (the p region then holds another buffer Y)
  i, j        non-square frames; j with every GEMM dimension off 16 and off 4

against float64 (resampling.apply_factors / adjoint_factors, lowres_common.fit): operator and adjoint with every band
index and the planes in shuffled order, NO_LOWRES_MFMA against the MFMA form bit for bit, and joint fits that take the
branches of k_lowres_planes the fixture fits leave out (scalar weight, zero weights, the low-resolution observation
first / alone / twice in the list, channels shared with a same-grid observation, K = 3 and 5, per-component constraints,
fix_sed, ragged counts).  Parity is the project's 1e-5 max-norm relative; S = 3 scenes, 6 iterations.

No scene passes through parity_common's threshold exemption (the cap is 0).  The seeds were checked on the CPU before
any device run, by the rule of constraints_common: the float32 and the float64 restatement agree on the support of every
morphology after every iteration and differ by at most 1e-6 (`seed_is_decided` below), so the reference alone is
decided and a device result beyond 1e-5 is a defect."""
import ctypes

import numpy as np
import pytest

import lowres_common as lc
from conftest import rel_err
from oracle import pgm

pytestmark = pytest.mark.gpu
TOL = 1e-5
S = 3
ITERS = 6
PHASES = ((0.0, 0.0), (0.3, -0.4), (-0.2, 0.45))      # sub-pixel cuts of the three scenes, model pixels (y, x)


def _geometries(name, per_scene, B):
    if not per_scene:
        return lc.limit_geometry(name, B=B)[0]
    # per scene: the observation cut half a pixel further in plus the scene's phase.  d, e and g, which span their model
    # frame, get an observation one pixel smaller (31 x 31, 41 x 41, 35 x 35: odd sizes besides); LowResObservationBatch
    # refuses a geometry that does not cover
    (h, w), org = lc.LIMITS[name][1], lc.LIMITS[name][3]
    shape = (h - 1, w - 1) if name in "deg" else (h, w)
    return [lc.limit_geometry(name, B=B, lr_shape=shape, origin=(org[0] + 0.5 + dy, org[1] + 0.5 + dx))[0] for dy, dx in PHASES]


def _operate(geo, B, x, y, band, scene):
    """scarlet_lowres_render of the planes x and scarlet_lowres_adjoint of the planes y as float64 arrays"""
    import torch
    import scarlet_amd as scarlet
    from scarlet_amd import _lib
    n, H, W = x.shape
    h, w = y.shape[1:]
    lo = scarlet.LowResObservationBatch(np.zeros((S, B, h, w), np.float32), geometry=geo)
    lr, keep = lo.lowres_struct("cuda")
    bd, sd = torch.as_tensor(band.astype(np.int32)).cuda(), torch.as_tensor(scene.astype(np.int32)).cuda()
    xd, yd = torch.as_tensor(x).cuda(), torch.as_tensor(y).cuda()
    Tx = torch.empty((n, h, w), dtype=torch.float32, device="cuda")
    Ty = torch.empty((n, H, W), dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib.scarlet_lowres_render(xd.data_ptr(), n, H, W, ctypes.byref(lr), bd.data_ptr(), sd.data_ptr(),
                                              Tx.data_ptr(), _lib.stream_ptr()))
    _lib.check(_lib.lib.scarlet_lowres_adjoint(yd.data_ptr(), n, H, W, ctypes.byref(lr), bd.data_ptr(), sd.data_ptr(),
                                               Ty.data_ptr(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return Tx.cpu().numpy().astype(np.float64), Ty.cpu().numpy().astype(np.float64)


def _planes(geo, B, seed=7):
    """S x B planes in shuffled order: plane p carries band band[p] of scene scene[p]; every (scene, band) occurs once"""
    g0 = geo[0] if isinstance(geo, list) else geo
    (H, W), (h, w) = g0.model_shape, g0.frame.shape[1:]
    rng = np.random.default_rng(seed)
    order = rng.permutation(S * B)
    x = rng.random((S * B, H, W)).astype(np.float32)
    y = rng.standard_normal((S * B, h, w)).astype(np.float32)
    return x, y, order % B, order // B


@pytest.mark.parametrize("per_scene", [False, True], ids=["shared", "per_scene"])
@pytest.mark.parametrize("name", sorted(lc.LIMITS))
def test_operator_and_adjoint_match_float64(name, per_scene):
    from scarlet_amd import resampling as rs
    B = lc.LIMITS[name][5]
    geo = _geometries(name, per_scene, B)
    x, y, band, scene = _planes(geo, B)
    Tx, Ty = _operate(geo, B, x, y, band, scene)
    worst = np.zeros((S, 3))
    for p in range(S * B):
        f = (geo[scene[p]] if per_scene else geo).factors
        f = dict(f, dhat=f["dhat"][band[p]:band[p] + 1])
        e1, e2 = rel_err(Tx[p], rs.apply_factors(f, x[p:p + 1])[0]), rel_err(Ty[p], rs.adjoint_factors(f, y[p:p + 1])[0])
        # <T x, y> = <x, T^T y>: both sides carry the float32 rounding of one pass through the GEMM chain, bounded by
        # the parity bar times the norms
        lhs, rhs = np.sum(Tx[p] * y[p]), np.sum(x[p].astype(np.float64) * Ty[p])
        e3 = abs(lhs - rhs) / (np.linalg.norm(Tx[p]) * np.linalg.norm(y[p]))
        worst[scene[p]] = np.maximum(worst[scene[p]], (e1, e2, e3))
    for s in range(S):
        print("geometry %s %s B = %d scene %d, worst band: render %.3e adjoint %.3e identity %.3e"
              % ((name, "per scene" if per_scene else "shared", B, s) + tuple(worst[s])))
    assert worst.max() <= TOL


# ------------------------------------------------------------------------------------------------- the joint fits
def _blob(shape, cy, cx, sy, sx):
    y, x = np.mgrid[:shape[0], :shape[1]]
    return np.exp(-((y - cy) ** 2 / (2 * sy ** 2) + (x - cx) ** 2 / (2 * sx ** 2)))


def _hr_kernels(B):
    """difference kernels of a same-grid observation of B bands with 11-pixel PSFs, as lowres_common.fit_inputs"""
    model_psf = lc.limit_psfs((11, 9), 1)[0]
    hr = np.array([lc.gauss(11, 1.1 + 0.1 * b) for b in range(B)]).astype(np.float32)
    return pgm.match_psfs(hr, model_psf).astype(np.float32)


class Case(object):
    """One joint fit of S scenes.  observations: dicts with band0, B and either geo (a matched LowResObservation:
    low-resolution; weights None, "map" (0.5 .. 1.5 times wscale) or "zeros" = a map with about 3 % zeros) or diff (same grid; None or kernels)."""

    def __init__(self, model_shape, C, centers, observations, seed, centroid_weight, sigma=2.2, counts=None, **settings):
        from scarlet_amd import resampling as rs
        H, W = model_shape
        rng = np.random.default_rng(seed)
        self.K, self.C, self.counts, self.cw = len(centers), C, counts, centroid_weight
        K = self.K
        self.cen = np.array(centers, dtype=np.int32)
        truth_sed = 0.3 + rng.random((K, C))
        truth = np.einsum("kc,kyx->cyx", truth_sed, np.array([_blob((H, W), cy + 0.3, cx - 0.2, sigma, 0.8 * sigma) for cy, cx in centers]))
        self.sed0 = (truth_sed[None] * (0.7 + 0.6 * rng.random((S, K, C)))).astype(np.float32)
        self.morph0 = np.broadcast_to(np.array([_blob((H, W), cy, cx, 1.2 * sigma, 1.2 * sigma) for cy, cx in centers]), (S, K, H, W)).astype(np.float32)
        self.obs = []
        for o in observations:
            o = dict(o)
            sl = slice(o["band0"], o["band0"] + o["B"])
            clean = rs.apply_factors(o["geo"].factors, truth[sl]) if "geo" in o else truth[sl]
            o["images"] = (clean[None] + 0.01 * rng.standard_normal((S,) + clean.shape)).astype(np.float32)
            if o.get("weights") is not None:
                wmap = o.get("wscale", 1.0) * (0.5 + rng.random(o["images"].shape))
                if o["weights"] == "zeros":
                    wmap[rng.random(wmap.shape) < 0.03] = 0
                o["weights"] = wmap.astype(np.float32)
            self.obs.append(o)
        # per-component settings of BlendBatch (symmetric, monotonic, l1_thresh: (K,) lists) and fix_sed / fix_morph (K,)
        self.settings = settings

    def n(self, s):
        return self.K if self.counts is None else self.counts[s]

    def oracle(self, s, dt=np.float32, trace=None):
        """lowres_common.fit of scene s in `dt`; trace: a list that receives the morphologies after every iteration"""
        n, st = self.n(s), self.settings
        sc = pgm.scene_from_state(np.zeros((self.C,) + self.morph0.shape[2:], dt), self.sed0[s, :n], self.morph0[s, :n],
                                  self.cen[:n], None, centroid_weight=self.cw)
        for k, src in enumerate(sc.sources):
            for name in ("symmetric", "monotonic", "l1_thresh", "fix_sed", "fix_morph"):
                if name in st:
                    setattr(src, name, st[name][k])
        obs = []
        for o in self.obs:
            d = dict(images=o["images"][s], band_slice=slice(o["band0"], o["band0"] + o["B"]),
                     weights=1 if o.get("weights") is None else o["weights"][s])
            if "geo" in o:
                d["factors"] = o["geo"].factors
            else:
                d["diff_kernel"] = None if o["diff"] is None else o["diff"].astype(dt)
            obs.append(d)
        if trace is None:
            return lc.fit(sc, obs, ITERS)
        for _ in range(ITERS):
            lc.fit(sc, obs, 1)
            trace.append(np.array([c.morph.copy() for c in sc.sources]))
        return sc

    def seed_is_decided(self):
        """constraints_common.seed_is_decided for every scene of the case (CPU; run when a seed is chosen)"""
        for s in range(S):
            t32, t64 = [], []
            self.oracle(s, np.float32, t32), self.oracle(s, np.float64, t64)
            for a, b in zip(t32, t64):
                if ((a == 0) != (b == 0)).any() or not np.isfinite(a).all() or rel_err(a, b) > 1e-6:
                    return False
        return True

    def batch(self):
        import torch
        import scarlet_amd as scarlet
        obs = []
        for o in self.obs:
            if "geo" in o:
                obs.append(scarlet.LowResObservationBatch(o["images"], band0=o["band0"], geometry=o["geo"], weights=o.get("weights")))
            else:
                ob = scarlet.ObservationBatch(o["images"], band0=o["band0"])
                obs.append(ob if o["diff"] is None else ob.set_diff_kernel(o["diff"]))
        cen = np.broadcast_to(self.cen, (S,) + self.cen.shape)
        centers = cen if self.counts is None else [cen[s, :self.counts[s]] for s in range(S)]
        kw = {k: v for k, v in self.settings.items() if k in ("symmetric", "monotonic", "l1_thresh")}
        b = scarlet.BlendBatch.from_observations(obs, centers, centroid_weight=self.cw, **kw)
        b.set_state(self.sed0, self.morph0)
        for name in ("fix_sed", "fix_morph"):
            if name in self.settings:
                mask = np.broadcast_to(np.array(self.settings[name], dtype=np.uint8), (S, self.K)).copy()
                setattr(b, name, torch.as_tensor(mask).cuda())
        b._fill_struct()
        return b


def _lo(name, band0, C, weights="map", wscale=1.0):
    B = lc.LIMITS[name][5]
    return dict(geo=lc.limit_geometry(name, B=B, band0=band0, C=C)[0], band0=band0, B=B, weights=weights, wscale=wscale)


def _hi(band0, B, psf=False):
    return dict(band0=band0, B=B, diff=_hr_kernels(B) if psf else None)


def _cw(name):
    return lc.limit_psfs(lc.LIMITS[name][4], 1)[0][0]


CEN5 = ((0.30, 0.33), (0.62, 0.55), (0.25, 0.72), (0.73, 0.27), (0.5, 0.8))     # K <= 5 centres, fractions of the frame


def _centers(name, K):
    H, W = lc.LIMITS[name][0]
    return [(int(fy * H), int(fx * W)) for fy, fx in CEN5[:K]]


def _at_the_limit(name):
    """C = 8, K = 5: a same-grid observation with a PSF on channels 0 - 2 and the low-resolution one on ALL 8 (shared
    channels; the largest LDS footprint a fit can have: 132.8 KiB at d, 156.3 KiB at g)"""
    return Case(lc.LIMITS[name][0], 8, _centers(name, 5), [_hi(0, 3, psf=True), _lo(name, 0, 8)], 31, _cw(name), sigma=2.6)


def _weights(kind):
    """geometry e (158.1 KiB): scalar weight 1 (weights == NULL in k_lowres_planes) / a map with about 3 % zeros"""
    return Case(lc.LIMITS["e"][0], 4, _centers("e", 3), [_hi(0, 2), _lo("e", 2, 4, weights=kind)], 32, _cw("e"), sigma=2.6)


def _layout(kind):
    if kind == "first":          # geometry i, the low-resolution observation before the same-grid one
        return Case(lc.LIMITS["i"][0], 5, _centers("i", 3), [_lo("i", 0, 5), _hi(3, 2)], 33, _cw("i"))
    if kind == "only":           # ... and alone
        return Case(lc.LIMITS["i"][0], 3, _centers("i", 3), [_lo("i", 0, 3)], 34, _cw("i"))
    # two low-resolution observations of different geometry around a same-grid one: the fixture's a (16 x 16, ratio 2)
    # on channels 0 - 1 and b (12 x 12, ratio 2.5, offset) on channels 3 - 4 of a 32 x 32 frame
    g = lc.fixture()
    a = lc.geometry(g, "a", model_channels=lc.CH5, channels=lc.CH5[:2])[0]
    b = lc.geometry(g, "b", model_channels=lc.CH5, channels=lc.CH5[3:])[0]
    obs = [dict(geo=a, band0=0, B=2, weights="map"), _hi(2, 1), dict(geo=b, band0=3, B=2, weights="map")]
    return Case((32, 32), 5, [(12, 13), (20, 18), (9, 22)], obs, 35, g["a_model_psf"][0])


def _constrained(seed=36):
    """geometry f at its 6 bands beside a same-grid observation on channels 0 - 1 (shared): K = 3 components with their
    own switches, an l1 threshold on one and fix_sed on one.  No fix_morph at e_rel = 0: a fixed morphology is a fixed
    point of the constraints up to its last bit, and MORPH_NOT_CONVERGED then asks whether that bit moved (in the float32
    oracle 315 pixels of such a component move by one ulp in iteration 5, on the device none does; the values agree to
    2.4e-7).  tests/test_gpu_engine.py has fix_morph on every gradient path, without the flags."""
    return Case(lc.LIMITS["f"][0], 6, _centers("f", 3), [_hi(0, 2), _lo("f", 0, 6)], seed, _cw("f"), sigma=2.6,
                symmetric=[True, False, True], monotonic=[True, True, False], l1_thresh=[None, 0.05, None],
                fix_sed=[False, False, True])


def _other_layout():
    """geometry h, the h x ldw layout: channels 1 - 2 at low resolution, 0 - 1 on the model's grid"""
    return Case(lc.LIMITS["h"][0], 3, _centers("h", 3), [_hi(0, 2), _lo("h", 1, 3)], 37, _cw("h"))


def _ragged(seed=38, wscale=0.25):
    """geometry j (17 x 23 frame, 5 x 7 observation): K = 3, the scenes use 3, 1 and 2 of them"""
    return Case(lc.LIMITS["j"][0], 3, [(5, 6), (11, 16), (9, 11)], [_lo("j", 0, 3, wscale=wscale), _hi(0, 2)], seed, _cw("j"), sigma=1.3,
                counts=[3, 1, 2])


CASES = {"limit_d": lambda: _at_the_limit("d"), "limit_g": lambda: _at_the_limit("g"),
         "weights_none": lambda: _weights(None), "weights_zeros": lambda: _weights("zeros"),
         "first": lambda: _layout("first"), "only": lambda: _layout("only"), "two_lowres": lambda: _layout("two"),
         "constrained": _constrained, "other_layout_h": _other_layout, "ragged_j": _ragged}


def _compare(b, s, sc, n, what_for):
    """test_gpu_lowres._compare"""
    sed, morph = b.sed_current.cpu().numpy(), b.morph_current.cpu().numpy()
    assert int(b.it[s].item()) == sc.it
    errs = [rel_err(got, want) for got, want in ((b.mse(s), sc.mse), (sed[s, :n], np.array([c.sed for c in sc.sources])),
                                                 (morph[s, :n], np.array([c.morph for c in sc.sources])))]
    print("fit %s scene %d: mse %.3e sed %.3e morph %.3e" % ((what_for, s) + tuple(errs)))
    assert max(errs) <= TOL, (s, errs)
    np.testing.assert_array_equal(b.centers.cpu().numpy()[s, :n], np.array([c.center for c in sc.sources]))
    np.testing.assert_array_equal(b.flags.cpu().numpy()[s, :n], np.array([c.flags for c in sc.sources]))
    assert not sed[s, n:].any() and not morph[s, n:].any()


@pytest.mark.parametrize("which", sorted(CASES))
def test_joint_fit_matches_the_float_restatement(which):
    case = CASES[which]()
    b = case.batch()
    assert b.fit(ITERS, e_rel=0) == ITERS
    b.raise_on_status()
    for s in range(S):
        _compare(b, s, case.oracle(s), case.n(s), which)


# ------------------------------------------------------------------------------------------------- NO_LOWRES_MFMA
def _with_option(value, fn):
    from scarlet_amd import _lib
    old = _lib.set_option("NO_LOWRES_MFMA", value)
    try:
        return fn()
    finally:
        _lib.set_option("NO_LOWRES_MFMA", old)


@pytest.mark.parametrize("name", ["d", "h", "j"])
def test_plain_fma_form_of_the_operator_is_bit_identical(name):
    """scarlet_hip.h: "NO_LOWRES_MFMA (the GEMMs of a low-resolution observation as plain FMA chains, bit-identical)" """
    B = lc.LIMITS[name][5]
    geo = _geometries(name, False, B)
    x, y, band, scene = _planes(geo, B, seed=8)
    mfma = _with_option(0, lambda: _operate(geo, B, x, y, band, scene))
    plain = _with_option(1, lambda: _operate(geo, B, x, y, band, scene))
    for what, a, b in (("render", mfma[0], plain[0]), ("adjoint", mfma[1], plain[1])):
        print("geometry %s %s: MFMA vs plain FMA %.3e" % (name, what, rel_err(a, b)))
        np.testing.assert_array_equal(a, b)


def test_plain_fma_form_of_a_joint_fit_is_bit_identical():
    def run():
        b = _at_the_limit("d").batch()
        assert b.fit(ITERS, e_rel=0) == ITERS
        return [t.cpu().numpy() for t in (b.sed_current, b.morph_current, b.mse_buf, b.centers, b.flags, b.lipschitz)]
    for a, b in zip(_with_option(0, run), _with_option(1, run)):
        np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------------------------------------- what the fits exposed
@pytest.mark.parametrize("K,B,H,W", [(3, 3, 48, 64), (4, 5, 64, 64), (4, 3, 40, 40)])
def test_lipschitz_constant_of_equal_separated_sources(K, B, H, W):
    """The fits on geometry i ("first", "only") missed 1e-5 by a factor of 3 in the loss of iteration 2, whatever the
    list order: three equal blobs far apart make a Gram matrix with a triple top eigenvalue, and the characteristic-
    polynomial solver (engine.h: lambda_max_charpoly4) stepped from rounding noise to as much as 1e-3 below it (restated
    on the CPU: 4 I comes out 9 % low), so L_sed was too small.  Here directly: L_sed of one iteration from equal blobs
    against numpy's eigenvalues of the float64 Gram matrix.  The device sums the Gram matrix in float32 partial sums
    (~1e-7) and the solver starts within the off-diagonal sums above the root (5e-6 at 40 x 40, where the blobs are
    closest; below 1e-7 otherwise): the bound is TOL."""
    import scarlet_amd as scarlet
    cen = [(int(fy * H), int(fx * W)) for fy, fx in ((0.25, 0.25), (0.72, 0.3), (0.3, 0.75), (0.75, 0.72))[:K]]
    rng = np.random.default_rng(41)
    morph = np.array([_blob((H, W), cy, cx, 2.6, 2.6) for cy, cx in cen], dtype=np.float32)
    sed = (0.3 + rng.random((K, B))).astype(np.float32)
    images = (np.einsum("kc,kyx->cyx", sed, morph) + 0.01 * rng.standard_normal((B, H, W))).astype(np.float32)
    single = scarlet.BlendBatch(np.stack([images] * S), np.stack([cen] * S))
    joint = scarlet.BlendBatch.from_observations([scarlet.ObservationBatch(np.stack([images[:2]] * S), band0=0),
                                                  scarlet.ObservationBatch(np.stack([images[2:]] * S), band0=2)], np.stack([cen] * S))
    M = morph.reshape(K, -1).astype(np.float64)
    want = np.linalg.eigvalsh(M @ M.T).max()
    for what, b, n_obs in (("one observation", single, 1), ("two observations", joint, 2)):
        b.set_state(np.stack([sed] * S), np.stack([morph] * S))
        assert b.fit(1, e_rel=0) == 1
        got = b.lipschitz.cpu().numpy()[:, 0] / n_obs
        print("K = %d, %d x %d, %s: L_sed rel err %s" % (K, H, W, what, np.array2string(got / want - 1, precision=2)))
        assert np.abs(got / want - 1).max() <= TOL
