"""Batches whose components use the stock update functions' other options (BlendBatch(update=UpdateOptions(...))): the
cases shared by tests/test_update_option_cases.py (CPU: every case is admissible in the oracle, every option set moves the
result) and tests/test_gpu_update_options.py (-m gpu: the device against the composed oracle).  numpy and oracle.pgm only.

The expected result is NOT oracle.pgm.fit (which runs the stock pipeline): it is the oracle's pieces composed here, in the
order of source.py:402-440 -- loss_and_gradients, lipschitz, the step, then per component max_pixel, (every fifth
iteration) psf_weighted_centroid, update_symmetric(algorithm=, strength=), update_monotonic(use_nearest=, thresh=),
prox_plus on the SED and / or the morphology, normalize(kind) -- and check_convergence.  The nearest-neighbour operator is
float64-only in the reference: the float32 pipeline casts up, sweeps and casts down (min is exact).

A case is a frame, K, B, PSF or not, one or two observations.  Shapes are the smallest that reach each form of the
constraint update (tests/frame_cases.py update_form): wave 40 x 40 (K = 2, and K = 12 for the chunked gradient passes), tile
72 x 80, tile_gscratch 96 x 96, plane PLANE_SIDE^2, one PSF case at 48 x 48 and one joint fit of two observations (3 + 2
channels) at 40 x 40.  B = 3, 6 iterations.  The scenes are blends in the strict sense: K elliptical Gaussians in one
cluster (`_blend_scene` says why isolated sources would not do).  The wave and tile cases end in the hand-placed scene of frame_cases: sources
on (h - 1, w - 1) and (2, 2) (`hand`: that scene's seed, 0 = the case has none).

The last band of every scene holds no source, only an over-subtracted sky (noise - SKY): the best-fit SED of that band is
negative, so positive="morph" (which does not clamp the SED) differs from the stock pipeline there.
"""
import collections

import numpy as np

import frame_cases

BG = 0.1
NOISE = 0.1
SKY = 0.3
NEIGHBOUR = 25.0     # peak of the hand scenes' undetected neighbours
ITERS = 6
CONVERGED_CAP = 120  # iteration cap of the one converged run (wave, soft, e_rel = 1e-3): its scenes stop before

Case = collections.namedtuple("Case", "name H W B K seeds psf joint hand min_sep")
PLANE_SIDE = frame_cases.PLANE_SIDE
CASES = collections.OrderedDict((c.name, c) for c in [
    Case("wave", 40, 40, 3, 2, (1100, 1102), False, False, 1150, 4),
    Case("wave_k12", 40, 40, 3, 12, (1300, 1302), False, False, 0, 3),
    Case("tile", 72, 80, 3, 3, (1400, 1401), False, False, 1450, 4),
    Case("tile_gscratch", 96, 96, 3, 2, (1500, 1501), False, False, 0, 4),
    Case("plane", PLANE_SIDE, PLANE_SIDE, 3, 2, (1600, 1601), False, False, 0, 4),
    Case("psf", 48, 48, 3, 2, (1700, 1701), True, False, 0, 4),
    Case("joint", 40, 40, 5, 2, (1800, 1801), False, True, 0, 4),
])
JOINT_SPLIT = 3                      # the joint case: observation 0 = channels 0..2, observation 1 = channels 3..4
assert [frame_cases.update_form(c.H, c.W) for c in CASES.values()] == \
    ["wave", "wave", "tile", "tile_gscratch", "plane", "wave", "wave"]

DEFAULTS = dict(symmetry="kspace", strength=0.5, use_nearest=False, monotonic_thresh=0.0, positive="both",
                normalization="morph_max")
# option set -> the options of component k (the mixed set: component 0 keeps the defaults, odd and even ones differ)
_MIXED = (dict(), dict(symmetry="sdss", use_nearest=True),
          dict(symmetry="soft", strength=0.3, monotonic_thresh=0.05, positive="morph", normalization="morph"))
OPTION_SETS = collections.OrderedDict([
    ("soft", lambda k: dict(symmetry="soft", strength=0.5)),
    ("sdss", lambda k: dict(symmetry="sdss")),
    ("thresh", lambda k: dict(monotonic_thresh=0.1)),
    ("nearest", lambda k: dict(use_nearest=True)),
    ("norm_morph", lambda k: dict(normalization="morph")),
    ("norm_sed", lambda k: dict(normalization="sed")),
    ("pos_morph", lambda k: dict(positive="morph")),
    ("mixed", lambda k: _MIXED[0] if k == 0 else _MIXED[1 + (k + 1) % 2]),
])


def component_options(optset, k):
    """the full options of component k under `optset` (None: the stock pipeline)"""
    o = dict(DEFAULTS)
    if optset is not None:
        o.update(OPTION_SETS[optset](k))
    return o


def update_kwargs(optset, K):
    """UpdateOptions(**update_kwargs(...)) of a batch with K components per scene: one (K,) sequence per field"""
    per = [component_options(optset, k) for k in range(K)]
    return {name: [p[name] for p in per] for name in DEFAULTS}


def psfs(c):
    return frame_cases.psfs(c)


def _blend_scene(c, seed):
    """K elliptical Gaussians in ONE cluster: every source lies min_sep .. min_sep + 3 pixels from another one, at least 5
    pixels inside the frame.  Isolated sources would not do: their SEDs reach the fixed point of the float32 arithmetic
    within the 6 iterations (the exact step size solves a lone source's SED in one step), and whether a factor moved by
    one last bit or by none -- the convergence flags at e_rel = 0 -- is then undecided between two float32 evaluations."""
    rng = np.random.Generator(np.random.PCG64(seed))
    H, W, m = c.H, c.W, 5
    peaks = [(int(rng.integers(H // 2 - 4, H // 2 + 5)), int(rng.integers(W // 2 - 4, W // 2 + 5)))]
    while len(peaks) < c.K:
        py, px = peaks[int(rng.integers(len(peaks)))]
        r, th = rng.uniform(c.min_sep, c.min_sep + 3), rng.uniform(0, 2 * np.pi)
        q = (int(round(py + r * np.sin(th))), int(round(px + r * np.cos(th))))
        if m <= q[0] < H - m and m <= q[1] < W - m and all((q[0] - a) ** 2 + (q[1] - b) ** 2 >= c.min_sep ** 2 for a, b in peaks):
            peaks.append(q)
    yy, xx = np.mgrid[:H, :W].astype(np.float64)
    model = np.zeros((c.B, H, W))
    for cy, cx in peaks:
        smaj, q, th = rng.uniform(1.5, 3.0), rng.uniform(0.5, 1.0), rng.uniform(0, np.pi)
        dy, dx = yy - cy, xx - cx
        u, v = np.cos(th) * dx + np.sin(th) * dy, -np.sin(th) * dx + np.cos(th) * dy
        amp = np.exp(rng.uniform(np.log(20.0), np.log(50.0)))
        model += (amp * rng.uniform(0.2, 1.0, size=c.B))[:, None, None] * np.exp(-0.5 * ((u / smaj) ** 2 + (v / (smaj * q)) ** 2))
    if c.psf:
        from scipy.signal import fftconvolve
        obs = psfs(c)[0]
        model = np.array([fftconvolve(model[b], obs[b], mode="same") for b in range(c.B)])
    return (model + rng.normal(0.0, NOISE, size=model.shape)).astype(np.float32), np.array(peaks, np.int32)


_cache = {}


def scenes(c):
    """[(images (B, H, W) float32, centres (K, 2) int32)] of the case; shared, read-only"""
    if c.name not in _cache:
        out = []
        n = len(c.seeds) + (1 if c.hand else 0)
        for i in range(n):
            if c.hand and i == n - 1:
                images, centers = frame_cases._hand_scene(c, c.H, c.W, c.hand)
                if c.K > 2:      # (the hand scene has two sources: one more, in the middle of the frame)
                    yy, xx = np.mgrid[:c.H, :c.W].astype(np.float64)
                    blob = 30.0 * np.exp(-0.5 * (((yy - c.H // 2) / 2.5) ** 2 + ((xx - c.W // 2) / 3.0) ** 2))
                    images = images + (np.array([1.0, 0.6, 0.3])[:c.B, None, None] * blob).astype(np.float32)
                    centers = np.concatenate([centers[:1], [[c.H // 2, c.W // 2]], centers[1:]]).astype(np.int32)
                # an undetected neighbour of another colour three pixels inside of either source: a lone source's SED is
                # solved in one step (see _blend_scene), with the neighbour it follows the morphology's slow changes
                yy, xx = np.mgrid[:c.H, :c.W].astype(np.float64)
                for (cy, cx), d in zip(centers, (-3, 3, 3)):
                    blob = NEIGHBOUR * np.exp(-0.5 * (((yy - cy - d) / 2.0) ** 2 + ((xx - cx - d) / 2.0) ** 2))
                    images = images + (np.linspace(0.2, 1.0, c.B)[:, None, None] * blob).astype(np.float32)
            else:
                images, centers = _blend_scene(c, c.seeds[i])
            images = np.array(images, np.float32)
            rng = np.random.Generator(np.random.PCG64(c.seeds[0] + 900 + i))
            images[-1] = (rng.normal(0.0, NOISE, size=images[-1].shape) - SKY).astype(np.float32)
            images.setflags(write=False)
            out.append((images, np.asarray(centers, np.int32)))
        _cache[c.name] = out
    return _cache[c.name]


def stacked(c):
    sc = scenes(c)
    return np.stack([im for im, _ in sc]), np.stack([cen for _, cen in sc])


# ---- the composed oracle
def source_update(src, it, o):
    """PointSource / ExtendedSource.update (source.py:402-440) with the stock functions' options `o`"""
    from oracle import pgm
    src.center = pgm.max_pixel(src.morph, src.center)
    if src.symmetric:
        if it % 5 == 0:
            src.center, src.shift = pgm.psf_weighted_centroid(src.morph, src.centroid_weight, src.center)
        pgm.update_symmetric(src.morph, src.center, src.shift, algorithm=o["symmetry"], strength=o["strength"])
    if src.monotonic:
        if o["use_nearest"]:
            if o["monotonic_thresh"] != 0:
                raise ValueError("Thresholding does not work with nearest neighbor monotonicity")
            m64 = np.ascontiguousarray(src.morph, dtype=np.float64)      # the binding is float64-only
            pgm.update_monotonic(m64, src.center, use_nearest=True)
            src.morph[:] = m64
        else:
            pgm.update_monotonic(src.morph, src.center, thresh=o["monotonic_thresh"])
    if src.l0_thresh is not None:
        pgm.prox_hard(src.morph, 1 / src.L_morph, src.l0_thresh)
    if src.l1_thresh is not None:
        pgm.prox_soft(src.morph, 1 / src.L_morph, src.l1_thresh)
    if o["positive"] in ("both", "sed"):
        pgm.prox_plus(src.sed)
    if o["positive"] in ("both", "morph"):
        pgm.prox_plus(src.morph)
    if o["normalization"] != "none":
        pgm.normalize(src.sed, src.morph, o["normalization"])


def composed_fit(scene, iters, e_rel, opts):
    """Blend.fit (blend.py:65-102) from the oracle's pieces, the sources updated with opts[k]"""
    from oracle import pgm
    for _ in range(iters):
        seds = [c.sed for c in scene.sources]
        morphs = [c.morph for c in scene.sources]
        extra = getattr(scene, "observations", None)
        if extra is None:
            loss, gs, gm = pgm.loss_and_gradients(seds, morphs, scene.images, scene.weights, scene.diff_kernel)
            n_obs = 1
        else:
            loss = 0
            gs = [np.zeros_like(sd) for sd in seds]
            gm = [np.zeros_like(m) for m in morphs]
            for ob in extra:
                sl = ob["band_slice"]
                l_, gs_, gm_ = pgm.loss_and_gradients([sd[sl] for sd in seds], morphs, ob["images"], 1, None)
                loss = loss + l_
                for k in range(len(seds)):
                    gs[k][sl] += gs_[k]
                    gm[k] = gm[k] + gm_[k]
            n_obs = len(extra)
        scene.mse.append(loss)
        L_sed, L_morph = pgm.lipschitz(seds, morphs, n_obs, False, scene.mse)
        for c, g_s, g_m in zip(scene.sources, gs, gm):
            c.L_sed, c.L_morph = L_sed, L_morph
            c.sed = c.sed - (1 / c.L_sed) * g_s
            c.morph = c.morph - (1 / c.L_morph) * g_m
        it = scene.it
        for k, c in enumerate(scene.sources):
            source_update(c, it, opts[k])
        # the relative change of every factor in this iteration, (K, 2): what check_convergence compares with e_rel
        with np.errstate(invalid="ignore", divide="ignore"):
            scene.change = np.array([[np.sqrt(((c.last_sed - c.sed) ** 2).sum() / (c.sed ** 2).sum()),
                                      np.sqrt(((c.last_morph - c.morph) ** 2).sum() / (c.morph ** 2).sum())] for c in scene.sources],
                                    dtype=np.float64)
        if pgm.check_convergence(scene, e_rel):
            break
    return scene


def oracle_kwargs(c, dt):
    if not c.psf:
        return {}
    _, model, diff, _ = psfs(c)
    return dict(diff_kernel=diff.astype(dt), centroid_weight=model.astype(np.float32))


def oracle_start(c, s, optset, dt=np.float32):
    """the constructors' state of scene s in the oracle: init_extended_source and the constructor's update() (it = 0) with
    the component's options; the joint case starts as CombinedExtendedSource does, without an update.  Returns sed (K, B),
    morph (K, H, W), centres (K, 2), shifts (K, 2; NaN = none)."""
    from oracle import pgm
    images, centers = scenes(c)[s]
    images = images.astype(dt)
    seds, morphs, cens, shifts = [], [], [], []
    kw = {}
    cw = pgm.default_centroid_weight()
    if c.psf:
        obs, model, _, _ = psfs(c)
        kw = dict(obs_psfs=obs.astype(dt), frame_psf=model.astype(dt))
        cw = model.astype(np.float32)
    for k, px in enumerate(centers):
        px = (int(px[0]), int(px[1]))
        if c.joint:
            sed, morph = pgm.init_combined_extended_source(px, [images[:JOINT_SPLIT], images[JOINT_SPLIT:]],
                                                           [np.ones(JOINT_SPLIT) * BG, np.ones(c.B - JOINT_SPLIT) * BG])
            src = pgm.Source(sed, morph, px, dt, centroid_weight=cw)
        else:
            sed, morph = pgm.init_extended_source(px, images, np.ones(c.B) * BG, **kw)
            src = pgm.Source(sed, morph, px, dt, centroid_weight=cw)
            source_update(src, 0, component_options(optset, k))
        seds.append(src.sed); morphs.append(src.morph); cens.append(src.center)
        shifts.append((np.nan, np.nan) if src.shift is None else src.shift)
    return np.array(seds), np.array(morphs), np.array(cens), np.array(shifts, dtype=np.float64)


def oracle_run(c, s, optset, state, iters=ITERS, e_rel=0.0, dt=np.float32):
    """the composed fit of scene s from `state` = (sed, morph, centres, shifts); returns a dict of results"""
    from oracle import pgm
    images = scenes(c)[s][0].astype(dt)
    sed0, morph0, cen0, sh0 = state
    sh = [None if np.isnan(v[0]) else v for v in np.asarray(sh0, dtype=np.float64)]
    sc = pgm.scene_from_state(images, np.asarray(sed0).astype(dt), np.asarray(morph0).astype(dt), cen0, None,
                              **oracle_kwargs(c, dt))
    for src, v in zip(sc.sources, sh):
        if v is not None:
            src.shift = (float(v[0]), float(v[1]))
    if c.joint:
        sc.observations = [dict(images=images[:JOINT_SPLIT], band_slice=slice(0, JOINT_SPLIT)),
                           dict(images=images[JOINT_SPLIT:], band_slice=slice(JOINT_SPLIT, c.B))]
    composed_fit(sc, iters, e_rel, [component_options(optset, k) for k in range(len(sc.sources))])
    return dict(sed=np.array([x.sed for x in sc.sources]), morph=np.array([x.morph for x in sc.sources]),
                mse=np.array(sc.mse), cen=np.array([x.center for x in sc.sources]), it=len(sc.mse),
                flags=np.array([int(x.flags) for x in sc.sources]), change=sc.change)


# ---- the nearest-neighbour sweep, ring by ring (what the device runs; numpy)
def nearest_ring_reference(shape, center):
    """per pixel the flat index of its reference pixel in closed form: one step towards the peak along the major axis, and
    along the minor axis too iff (A + b)^2 > 2 A^2 (A, b = the larger and the smaller of |dy|, |dx|); the peak itself"""
    H, W = shape
    cy, cx = int(center[0]), int(center[1])
    Y, X = np.mgrid[:H, :W]
    Y, X = Y - cy, X - cx
    ay, ax = np.abs(Y), np.abs(X)
    A, b = np.maximum(ay, ax), np.minimum(ay, ax)
    diag = (A + b) ** 2 > 2 * A ** 2
    sy = np.where((ay == A) | diag, -np.sign(Y), 0)
    sx = np.where((ax == A) | diag, -np.sign(X), 0)
    return ((Y + cy + sy) * W + (X + cx + sx)).reshape(-1)


def ring_sweep(X, center):
    """x = min(x, x_ref) ring by ring (Chebyshev rings around the peak), every ring at once; in place"""
    H, W = X.shape
    cy, cx = int(center[0]), int(center[1])
    ref = nearest_ring_reference(X.shape, center)
    Y_, X_ = np.mgrid[:H, :W]
    ring = np.maximum(np.abs(Y_ - cy), np.abs(X_ - cx)).reshape(-1)
    flat = X.reshape(-1)
    for a in range(1, int(ring.max()) + 1):
        idx = np.nonzero(ring == a)[0]
        cur, r = flat[idx], flat[ref[idx]]
        flat[idx] = np.where(r < cur, r, cur)            # std::min(cur, ref)
    return X
