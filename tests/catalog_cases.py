"""Catalogue batches (BlendBatch.from_catalog): ragged-frame scenes that hold point sources, extended sources and
multi-component sources.  The cases shared by tests/test_catalog_cases.py (CPU: every scene is admissible in the oracle,
and zero-weight padding is NOT the reference's result for a grouped source) and tests/test_gpu_catalog.py (-m gpu: the
device against the oracle run of each scene alone on its own frame).  numpy, scarlet_amd.synth and oracle.pgm only.

A case is a list of scene shapes (h, w) and, per scene, its catalogue: a tuple of sources (kind, percentiles), kind one of
"extended", "point", "multi" (percentiles None except for multi).  The centres come from synth.make_scene (8 px inside
the scene's own frame), in catalogue order; `star` places one more point source by hand.  The padded frame is what
scarlet_amd.batch.pad_frames makes of the shapes (H = max h, W = max w rounded up to a multiple of 4).  The shapes are the
smallest that reach each form of the constraint update (frame_cases.update_form) and of the init kernels' tile:
  wave      40 x 40     one wave per component; ragged counts (1 to 4 components per scene)
  tile      72 x 80     one workgroup per component, tile and scratch in LDS
  plane     PLANE_SIDE  the update's plane form; the init kernels' float64 tile still fits LDS (8 H (W + 1) bytes)
  plane_gt  141 x 141   the smallest square whose float64 init tile leaves LDS: the init kernels' HBM-tile (GT) form
  psf       48 x 48     the difference kernels and the model PSF of parity_common.Workload(psf=True); a point source 2 px
                        from its scene's own last row and column, in a scene with w < W
Every case has a scene with w % 4 != 0 and one with w % 4 == 0 and w < W.  The default centroid PSF is 41 px wide, so
every grouped source lies within its radius (20 px) of an end of its own frame.
"""
import collections

import numpy as np

import frame_cases as fc

BG = fc.BG
ITERS = 6
E, P, M = ("extended", None), ("point", None), ("multi", (25.0,))
M3 = ("multi", (20.0, 60.0))

Case = collections.namedtuple("Case", "name B shapes catalog psf seed min_sep star")

INIT_TILE_LIMIT = fc.LDS_LIMIT                  # launch_plan.h init_tile_plan: 8 H (W + 1) bytes of LDS, or the HBM tile
GT_SIDE = next(n for n in range(65, 1025) if 8 * n * (-(-n // 4) * 4 + 1) > INIT_TILE_LIMIT)

CASES = collections.OrderedDict((c.name, c) for c in [
    Case("wave", 3, ((40, 40), (24, 40), (40, 27), (17, 23), (33, 20), (31, 26)),
         ((M, P, E), (M3, E), (M, P), (E,), (M,), (M, E)), False, 1100, 8, None),
    Case("tile", 3, ((72, 80), (65, 33), (20, 70), (66, 76)), ((M, P), (M, P), (M, P), (M, P)), False, 1202, 8, None),
    Case("plane", 3, ((fc.PLANE_SIDE, fc.PLANE_SIDE), (40, 30), (25, 36)), ((M,), (M,), (M,)), False, 1307, 8, None),
    Case("plane_gt", 3, ((GT_SIDE, GT_SIDE), (40, 30), (25, 36)), ((M,), (M,), (M,)), False, 1439, 8, None),
    # star: (scene, (y, x)) -- a point source 2 px from the own last row and column of the 24 x 44 scene
    Case("psf", 3, ((48, 48), (24, 44), (41, 27)), ((M, E), (M, P), (M, P)), True, 1503, 10, (1, (21, 41))),
])


def padded_shape(c):
    return max(h for h, _ in c.shapes), -(-max(w for _, w in c.shapes) // 4) * 4


def n_components(c, s):
    return sum(1 if p is None else len(p) + 1 for _, p in c.catalog[s])


def init_tile_in_lds(c):
    H, W = padded_shape(c)
    return 8 * H * (W + 1) <= INIT_TILE_LIMIT


def psfs(c):
    return fc.psfs(c)


_cache = {}


def scenes(c):
    """[(images (B, h, w) float32, centres (n_sources, 2) int32)] of the case's scenes, catalogue order; shared, read-only"""
    if c.name not in _cache:
        from scarlet_amd import synth
        out = []
        for s, ((h, w), cat) in enumerate(zip(c.shapes, c.catalog)):
            hand = c.star is not None and c.star[0] == s
            n = len(cat) - (1 if hand else 0)
            kw = dict(B=c.B, H=h, W=w, K=n, min_sep=c.min_sep)
            if c.psf:
                kw["psfs"] = psfs(c)[0]
            sc = synth.make_scene(c.seed + s, **kw)
            images, centers = sc["images"], sc["centers"]
            if hand:                               # the star is the catalogue's last source
                assert cat[-1] == P
                y, x = c.star[1]
                obs = psfs(c)[0]
                R = obs.shape[1] // 2
                flux = np.array([30.0, 24.0, 18.0])[:c.B]
                for b in range(c.B):
                    for dy in range(-R, R + 1):
                        for dx in range(-R, R + 1):
                            if 0 <= y + dy < h and 0 <= x + dx < w:
                                images[b, y + dy, x + dx] += np.float32(flux[b] * obs[b, R + dy, R + dx])
                centers = np.concatenate([centers, np.array([[y, x]], np.int32)])
            images.setflags(write=False)
            out.append((images, centers.astype(np.int32)))
        _cache[c.name] = out
    return _cache[c.name]


def catalog(c):
    """per scene a list of (centre (y, x), kind, percentiles or None): what the tests turn into SourceSpecs"""
    return [[((int(cen[i][0]), int(cen[i][1])), kind, perc) for i, (kind, perc) in enumerate(cat)]
            for (_, cen), cat in zip(scenes(c), c.catalog)]


def grouped_components(c, s):
    """indices of scene s's components that are layers of a multi source"""
    out, k = [], 0
    for kind, perc in c.catalog[s]:
        n = 1 if perc is None else len(perc) + 1
        if kind == "multi":
            out += list(range(k, k + n))
        k += n
    return out


# ---- the oracle: every source by its own constructor, then Blend.fit, for one scene alone
def _point_start(pgm, images, px, obs, model):
    """PointSource as tests/test_gpu_init_sources.py states it: the model PSF pasted on the pixel and clipped to the
    frame (a single 1 without one), SED = pixel / observed PSF peaks"""
    _, H, W = images.shape
    py, px_ = px
    morph = np.zeros((H, W), np.float32)
    if model is not None:
        R = model.shape[0] // 2
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                if 0 <= py + dy < H and 0 <= px_ + dx < W:
                    morph[py + dy, px_ + dx] = model[R + dy, R + dx]
    else:
        morph[py, px_] = 1
    sed = images[:, py, px_].copy()
    if obs is not None:
        sed /= obs.max(axis=(1, 2))
    return sed, morph


def oracle_scene(c, images, cat, weights=1):
    """the constructors' scene: (pgm.Scene with .trees, the list of trees)"""
    from oracle import pgm
    obs = model = diff = None
    cw = pgm.default_centroid_weight()
    if c.psf:
        o, m, _, _ = psfs(c)
        obs, model = o.astype(np.float32), m.astype(np.float32)
        diff = pgm.match_psfs(obs, model[None])
        cw = model
    bg = np.ones(c.B) * BG
    trees, flat = [], []
    for px, kind, perc in cat:
        if kind == "multi":
            seds, morphs = pgm.init_multicomponent_source(px, images, bg, list(perc), obs, model)
            comps = [pgm.Source(seds[j], morphs[j], px, images.dtype, centroid_weight=cw) for j in range(len(seds))]
            t = pgm.MultiSource(comps, px, centroid_weight=cw)
            pgm.multi_source_update(t, 0)
            flat += comps
        else:
            if kind == "point":
                sed, morph = _point_start(pgm, images, px, obs, model)
            else:
                sed, morph = pgm.init_extended_source(px, images, bg, obs, model)
            t = pgm.Source(sed, morph, px, images.dtype, centroid_weight=cw)
            pgm.source_update(t, 0)
            flat.append(t)
        trees.append(t)
    sc = pgm.Scene(images, flat, weights, diff)
    sc.trees = trees
    return sc


def _snapshot(sc, crop=None):
    from oracle import pgm
    h, w = crop if crop is not None else sc.images.shape[1:]
    shift_none = []
    for t in sc.trees:
        n = len(t.components) if isinstance(t, pgm.MultiSource) else 1
        shift_none += [t.shift is None] * n
    return dict(sed=np.array([x.sed for x in sc.sources]), morph=np.array([x.morph[:h, :w] for x in sc.sources]),
                centers=np.array([x.center for x in sc.sources], np.int32), flags=np.array([int(x.flags) for x in sc.sources]),
                shift_none=np.array(shift_none), mse=np.array(sc.mse, np.float64), it=sc.it)


def oracle_run(args):
    """worker: scene `s` of case `name`, started and fitted alone -> (start, fit) snapshots.  how = "own": on its own frame;
    "padded": zero-padded to the case's padded frame with zero weights outside, what a user without the ragged route
    would do (morphologies cropped back to the scene)"""
    from oracle import pgm
    name, s, iters, how = args
    c = CASES[name]
    images, _ = scenes(c)[s]
    images = np.array(images)
    cat = catalog(c)[s]
    h, w = images.shape[1:]
    weights = 1
    if how == "padded":
        H, W = padded_shape(c)
        pad = np.zeros((c.B, H, W), np.float32)
        pad[:, :h, :w] = images
        weights = np.zeros((c.B, H, W), np.float32)
        weights[:, :h, :w] = 1
        images = pad
    sc = oracle_scene(c, images, cat, weights)
    start = _snapshot(sc, (h, w))
    pgm.fit(sc, iters, e_rel=0)
    return start, _snapshot(sc, (h, w))
