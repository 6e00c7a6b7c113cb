"""Catalogue batches whose sources carry the stock update functions' options (BlendBatch.from_catalog with SourceSpec
options or update=): the cases shared by tests/test_catalog_option_cases.py (CPU: every case x option set x scene is
admissible in the oracle, every option set moves the result, zero-weight padding is not the own-frame result) and
tests/test_gpu_catalog_options.py (-m gpu: the device against the composed oracle).  numpy, oracle.pgm and the cases of
catalog_cases, update_option_cases and frame_cases only.

The cases are catalog_cases' wave (40 x 40 padded), tile (72 x 80), plane (PLANE_SIDE) and psf (48 x 48) -- the smallest
shapes that reach each form of the constraint update -- and one tile_gscratch case (96 x 96).  Every case keeps a scene
with w % 4 != 0 and one with w % 4 == 0 and w < W; every scene of the plane and tile_gscratch cases holds at least two
sources (catalog_cases' plane scenes hold one).  As in update_option_cases the last band of every scene holds no source,
only an over-subtracted sky (noise - SKY): the best-fit SED of that band is negative, so positive="morph" differs from the
stock pipeline there.  B = 3, 6 iterations.

Option sets: update_option_cases.OPTION_SETS, applied per SOURCE -- source i of a scene takes the set's options of index
i + 1, so that under "mixed" (whose index 0 keeps the defaults) the first source of every catalogue, a multi source, gets
non-default options.  The layers of a multi source share their source's options.

The expected result is the oracle's pieces composed here: pgm.fit's loop (blend.py:65-102) with the tree update
  point / extended source: update_option_cases.source_update (source.py:402-440 with the stock functions' options);
  multi source: the shared centre is max_pixel of sum_layers morph * sed.sum(), every fifth iteration (if symmetric) the
      centroid of that sum, exactly as pgm.multi_source_update does it and before any option acts; each layer then gets
      update.symmetric(layer, centre, algorithm=, strength=) with NO shift (k-space therefore falls back to soft symmetry
      with strength 1), update.monotonic(use_nearest=, thresh=), the positivity variant and normalized(type=).
Each scene runs alone on its own (B, h_s, w_s) frame.
"""
import collections

import numpy as np

import catalog_cases as cc
import frame_cases as fc
import update_option_cases as uo

BG = cc.BG
NOISE = uo.NOISE
SKY = uo.SKY
ITERS = 6
CONVERGED_CAP = 120     # iteration cap of the one converged run (wave, soft, e_rel = 1e-3): its scenes stop before
E, P, M, M3 = cc.E, cc.P, cc.M, cc.M3
OPTION_SETS = uo.OPTION_SETS
PLANE_SIDE = fc.PLANE_SIDE

# (the names differ from catalog_cases': its scene cache is keyed by the name)
_w, _t, _p = cc.CASES["wave"], cc.CASES["tile"], cc.CASES["psf"]
CASES = collections.OrderedDict([
    ("wave", _w._replace(name="options_wave")),
    ("tile", _t._replace(name="options_tile")),
    ("tile_gscratch", cc.Case("options_tile_gscratch", 3, ((96, 96), (70, 50), (33, 88)), ((M, P), (M, E), (M, P)), False, 1611, 8, None)),
    ("plane", cc.Case("options_plane", 3, ((PLANE_SIDE, PLANE_SIDE), (40, 30), (25, 36)), ((M, E), (M, P), (M, E)), False, 1707, 8, None)),
    ("psf", _p._replace(name="options_psf")),
])


# uniform cut-outs with multi sources and options (the same route with frame_hw = NULL); not one of the ragged cases above
UNIFORM = cc.Case("options_uniform", 3, ((40, 40),) * 3, ((M, P, E), (M, E), (M, P)), False, 1800, 8, None)
ALL_CASES = collections.OrderedDict(list(CASES.items()) + [("uniform", UNIFORM)])


def padded_shape(c):
    return cc.padded_shape(c)


def n_components(c, s):
    return cc.n_components(c, s)


def psfs(c):
    return fc.psfs(c)


def one_component(c, s):
    """scene s holds a single component (see make_scene)"""
    return n_components(c, s) == 1


# per case the seed of every scene (catalog_cases seeds scene s with the case's seed + s).  The first entries are those;
# a scene that was not admissible under some option set (tests/test_catalog_option_cases.py: float32 against float64, the
# centres, the flags, the DECIDED rule, and for wave the converged run) took the next seed that is, counting up from there.
SEEDS = {
    "options_wave": (1100, 1102, 1102, 1105, 1105, 1105),
    "options_tile": (1204, 1204, 1206, 1206),
    "options_tile_gscratch": (1613, 1613, 1613),
    "options_plane": (1712, 1708, 1710),
    "options_psf": (1503, 1504, 1505),
    "options_uniform": (1802, 1802, 1805),
}
LONE_D, LONE_PEAK = 3, uo.NEIGHBOUR      # the lone source's undetected neighbour: offset along both axes, peak
_cache = {}


def make_scene(c, s, seed):
    """scene s of the case as catalog_cases makes it from `seed` (its hand-placed star included), with the last band
    replaced by noise - SKY: (images (B, h, w) float32, centres (n_sources, 2) int32), read-only"""
    star = None if c.star is None or c.star[0] != s else (0, c.star[1])
    one = c._replace(name="%s_scene%d_seed%d" % (c.name, s, seed), shapes=(c.shapes[s],), catalog=(c.catalog[s],), seed=seed, star=star)
    im, cen = cc.scenes(one)[0]
    images = np.array(im, np.float32)
    if one_component(c, s):
        # A scene of ONE component is degenerate under the exact step sizes: with sed * morph = c * (the best fit), the SED
        # step divides the SED by c and the morphology step divides the morphology by c, so c -> 1 / c every iteration.
        # Started by its constructor (c = 1 at the peak) it sits on the fixed point to float64 round-off -- its last change
        # was 1e-14 .. 1e-9 under each of 80 seeds, never decided -- and anything that takes it off the fixed point leaves
        # it in that 2-cycle for good.  As in update_option_cases' hand scenes it gets an undetected neighbour of another
        # colour LONE_D pixels towards the middle of the frame: the 6-iteration runs are then decided under every option
        # set, and the converged run of this scene alone never stops (tests/test_catalog_option_cases.py
        # test_converged_run_is_admissible says what is asserted for it instead)
        (cy, cx), (h, w) = cen[0], c.shapes[s]
        yy, xx = np.mgrid[:h, :w].astype(np.float64)
        ny, nx = cy + (LONE_D if cy < h / 2 else -LONE_D), cx + (LONE_D if cx < w / 2 else -LONE_D)
        blob = LONE_PEAK * np.exp(-0.5 * (((yy - ny) / 2.0) ** 2 + ((xx - nx) / 2.0) ** 2))
        images = images + (np.linspace(0.2, 1.0, c.B)[:, None, None] * blob).astype(np.float32)
    rng = np.random.Generator(np.random.PCG64(seed + 900))
    images[-1] = (rng.normal(0.0, NOISE, size=images[-1].shape) - SKY).astype(np.float32)
    images.setflags(write=False)
    return images, cen


def scenes(c):
    """[(images (B, h, w) float32, centres (n_sources, 2) int32)] of the case's scenes, catalogue order; shared, read-only"""
    if c.name not in _cache:
        _cache[c.name] = [make_scene(c, s, seed) for s, seed in enumerate(SEEDS[c.name])]
    return _cache[c.name]


def catalog(c):
    """per scene a list of (centre (y, x), kind, percentiles or None), catalogue order"""
    return [[((int(cen[i][0]), int(cen[i][1])), kind, perc) for i, (kind, perc) in enumerate(cat)]
            for (_, cen), cat in zip(scenes(c), c.catalog)]


def source_options(optset, i):
    """the full options of source i of a scene under `optset` (None: the stock pipeline)"""
    return uo.component_options(optset, i + 1)


def spec_kwargs(optset, i):
    """the SourceSpec keywords of source i: only what `optset` sets (None elsewhere, the batch's default)"""
    return {} if optset is None else dict(OPTION_SETS[optset](i + 1))


def component_options(c, s, optset):
    """the options of every component of scene s, layers sharing their source's"""
    out = []
    for i, (kind, perc) in enumerate(c.catalog[s]):
        out += [source_options(optset, i)] * (1 if perc is None else len(perc) + 1)
    return out


# ---- the composed oracle
def _sweep_positive_normalize(src, center, o):
    """update.monotonic(use_nearest=, thresh=), the positivity variant, normalized(type=) of one component"""
    from oracle import pgm
    if src.monotonic:
        if o["use_nearest"]:
            if o["monotonic_thresh"] != 0:
                raise ValueError("Thresholding does not work with nearest neighbor monotonicity")
            m64 = np.ascontiguousarray(src.morph, dtype=np.float64)      # the binding is float64-only
            pgm.update_monotonic(m64, center, use_nearest=True)
            src.morph[:] = m64
        else:
            pgm.update_monotonic(src.morph, center, thresh=o["monotonic_thresh"])
    if o["positive"] in ("both", "sed"):
        pgm.prox_plus(src.sed)
    if o["positive"] in ("both", "morph"):
        pgm.prox_plus(src.morph)
    if o["normalization"] != "none":
        pgm.normalize(src.sed, src.morph, o["normalization"])


def multi_source_update(ms, it, o):
    """MultiComponentSource.update (source.py:605-641) with the stock functions' options `o` for every layer"""
    from oracle import pgm
    _morph = np.sum([c.morph * c.sed.sum() for c in ms.components], axis=0)
    ms.center = pgm.max_pixel(_morph, ms.center)
    if ms.symmetric and it % 5 == 0:
        ms.center, ms.shift = pgm.psf_weighted_centroid(_morph, ms.centroid_weight, ms.center)
    for c in ms.components:
        if ms.symmetric:
            pgm.update_symmetric(c.morph, ms.center, None, algorithm=o["symmetry"], strength=o["strength"])
        c.monotonic = ms.monotonic
        _sweep_positive_normalize(c, ms.center, o)
        c.center = ms.center


def tree_update(t, it, o):
    from oracle import pgm
    if isinstance(t, pgm.MultiSource):
        multi_source_update(t, it, o)
    else:
        uo.source_update(t, it, o)


def composed_fit(scene, iters, e_rel, opts):
    """pgm.fit's loop (single observation) with tree_update(tree i, it, opts[i])"""
    from oracle import pgm
    for _ in range(iters):
        seds = [c.sed for c in scene.sources]
        morphs = [c.morph for c in scene.sources]
        loss, gs, gm = pgm.loss_and_gradients(seds, morphs, scene.images, scene.weights, scene.diff_kernel)
        scene.mse.append(loss)
        L_sed, L_morph = pgm.lipschitz(seds, morphs, 1, False, scene.mse)
        for c, g_s, g_m in zip(scene.sources, gs, gm):
            c.L_sed, c.L_morph = L_sed, L_morph
            c.sed = c.sed - (1 / c.L_sed) * g_s
            c.morph = c.morph - (1 / c.L_morph) * g_m
        it = scene.it
        for t, o in zip(scene.trees, opts):
            tree_update(t, it, o)
        with np.errstate(invalid="ignore", divide="ignore"):
            scene.change = np.array([[np.sqrt(((c.last_sed - c.sed) ** 2).sum() / (c.sed ** 2).sum()),
                                      np.sqrt(((c.last_morph - c.morph) ** 2).sum() / (c.morph ** 2).sum())] for c in scene.sources],
                                    dtype=np.float64)
        if pgm.check_convergence(scene, e_rel):
            break
    return scene


def _psf_setup(c, dt):
    """(observed PSFs, model PSF, difference kernel, centroid weight) of the case in dtype dt; Nones without a PSF"""
    from oracle import pgm
    if not c.psf:
        return None, None, None, pgm.default_centroid_weight()
    o, m, _, _ = psfs(c)
    obs, model = o.astype(np.float32), m.astype(np.float32)
    diff = pgm.match_psfs(obs, model[None])
    return obs, model, diff.astype(dt), model


def _result(sc, trees):
    from oracle import pgm
    shifts = []
    for t in trees:
        n = len(t.components) if isinstance(t, pgm.MultiSource) else 1
        shifts += [(np.nan, np.nan) if t.shift is None else t.shift] * n
    return dict(sed=np.array([x.sed for x in sc.sources]), morph=np.array([x.morph for x in sc.sources]),
                cen=np.array([x.center for x in sc.sources], np.int32), shifts=np.array(shifts, np.float64),
                flags=np.array([int(x.flags) for x in sc.sources]), mse=np.array(sc.mse, np.float64), it=len(sc.mse),
                change=getattr(sc, "change", None))


def _padded(c, s, images):
    """scene s zero-padded to the case's padded frame, and the weights that are zero outside its own frame"""
    H, W = padded_shape(c)
    h, w = images.shape[1:]
    pad = np.zeros((c.B, H, W), np.float32)
    pad[:, :h, :w] = images
    weights = np.zeros((c.B, H, W), np.float32)
    weights[:, :h, :w] = 1
    return pad, weights


def oracle_start(c, s, optset, how="own"):
    """the constructors' state of scene s (float32): every source by its own constructor WITHOUT its update, then the
    composed update once at it = 0 with the source's options.  how = "padded": on the zero-padded frame."""
    from oracle import pgm
    images = np.array(scenes(c)[s][0])
    if how == "padded":
        images, _ = _padded(c, s, images)
    obs, model, _, cw = _psf_setup(c, np.float32)
    bg = np.ones(c.B) * BG
    trees, flat = [], []
    for i, (px, kind, perc) in enumerate(catalog(c)[s]):
        if kind == "multi":
            seds, morphs = pgm.init_multicomponent_source(px, images, bg, list(perc), obs, model)
            comps = [pgm.Source(seds[j], morphs[j], px, images.dtype, centroid_weight=cw) for j in range(len(seds))]
            t = pgm.MultiSource(comps, px, centroid_weight=cw)
            flat += comps
        else:
            if kind == "point":
                sed, morph = cc._point_start(pgm, images, px, obs, model)
            else:
                sed, morph = pgm.init_extended_source(px, images, bg, obs, model)
            t = pgm.Source(sed, morph, px, images.dtype, centroid_weight=cw)
            flat.append(t)
        tree_update(t, 0, source_options(optset, i))
        trees.append(t)
    sc = pgm.Scene(images, flat, 1, None)
    return _result(sc, trees)


def oracle_run(c, s, optset, state, iters=ITERS, e_rel=0.0, dt=np.float32, how="own"):
    """the composed fit of scene s alone from `state` (sed, morph, cen, shifts of its components; what oracle_start
    returns, or the device's own start) in dtype dt"""
    from oracle import pgm
    images = np.array(scenes(c)[s][0])
    weights = 1
    if how == "padded":
        images, weights = _padded(c, s, images)
    images = images.astype(dt)
    _, _, diff, cw = _psf_setup(c, dt)
    trees, flat, k = [], [], 0
    for i, (px, kind, perc) in enumerate(catalog(c)[s]):
        n = 1 if perc is None else len(perc) + 1
        comps = [pgm.Source(np.asarray(state["sed"][k + j]).astype(dt), np.asarray(state["morph"][k + j]).astype(dt),
                            state["cen"][k + j], dt, centroid_weight=cw) for j in range(n)]
        sh = np.asarray(state["shifts"][k], np.float64)
        if kind == "multi":
            t = pgm.MultiSource(comps, state["cen"][k], centroid_weight=cw)
        else:
            t = comps[0]
        t.shift = None if np.isnan(sh[0]) else (float(sh[0]), float(sh[1]))
        trees.append(t)
        flat += comps
        k += n
    sc = pgm.Scene(images, flat, weights, diff)
    sc.trees = trees
    composed_fit(sc, iters, e_rel, [source_options(optset, i) for i in range(len(trees))])
    return _result(sc, trees)


def oracle_job(args):
    """worker: (case key, scene, option set, state or None, iters, e_rel, dtype name, how) -> (start, fit); the start is
    the oracle's own where `state` is None"""
    key, s, optset, state, iters, e_rel, dt, how = args
    c = ALL_CASES[key]
    start = oracle_start(c, s, optset, how) if state is None else state
    return start, oracle_run(c, s, optset, start, iters, e_rel, np.dtype(dt).type, how)
