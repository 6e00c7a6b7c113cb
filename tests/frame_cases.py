"""Batches whose scenes have their own frame sizes (BlendBatch(frame_shapes=...)): the cases shared by
tests/test_frame_cases.py (CPU: every scene is admissible in the oracle, and zero-weight padding is NOT the reference's
result) and tests/test_gpu_frames.py (-m gpu: the device against the oracle run of each scene on its own frame).
numpy, scarlet_amd.synth and oracle.pgm only.

A case is a padded frame, per-scene shapes (h, w), per-scene source counts, K, B, PSF or not, iterations.  The shapes
are the smallest that reach each form of the constraint update (launch_plan.h update_plan, restated in `update_form`):
  wave            40 x 40   one wave per component; K = 2: the register-tiled gradient kernels
  wave_k6         40 x 40   the same frames, K = 6 (the K <= 8 instance of the gradient kernels)
  wave_k12        40 x 40   K = 12: the chunked (big-K) gradient passes
  tile            72 x 80   one workgroup per component, tile and scratch in LDS
  tile_gscratch   96 x 96   the tile in LDS, the symmetry scratch in HBM
  plane           PLANE_SIDE, the smallest square whose form is the plane form: operators in place in HBM
  psf             48 x 48   the difference kernels of parity_common.Workload(psf=True)
Every case has a scene with w % 4 != 0 and one with w % 4 == 0 and w < W.  A small frame cannot hold K well-separated
sources (synth.make_scene keeps them 8 px inside): such scenes carry fewer sources, so the K = 6 and K = 12 cases are
ragged in their counts as well.  wave, tile and psf end in a hand-placed scene with one source centred on the frame's
last pixel (h - 1, w - 1) and one on row and column 2 -- the limits of the reference's max_pixel, as tests/edge_cases.py
uses them for uniform frames.
"""
import collections

import numpy as np

BG = 0.1
NOISE = 0.1

Case = collections.namedtuple("Case", "name H W B K shapes counts psf iters seed hand")


# ---- launch_plan.h update_plan / prox_ops.h, restated (host arithmetic only)
def _tile_stride(W):
    return ((W - 2 + 31) // 32) * 32 + 2


def _scratch_stride(wp):
    return ((wp + 31) // 32) * 32 + 16


def _round16(v):
    return (v + 15) & ~15


def _symmetry_vec_floats(H, W):
    return 2 * _round16(H) + 5 * _round16(W)


def update_lds_bytes(H, W):
    return 4 * (H * _tile_stride(W) + _round16(H) * _scratch_stride(_round16(W)) + _symmetry_vec_floats(H, W))


def tile_stage_lds_bytes(H, W):
    hp, wp = _round16(H), _round16(W)
    return 4 * H * _tile_stride(W) + 4 * (_symmetry_vec_floats(H, W) + max(16 * _tile_stride(wp), hp * 16))


LDS_LIMIT = 160 * 1024 - 1024


def update_form(H, W):
    """the form update_plan picks for a workspace-backed launch: wave, tile, tile_gscratch or plane"""
    if H <= 64 and W <= 64:
        return "wave"
    if update_lds_bytes(H, W) > LDS_LIMIT:
        return "plane"
    if update_lds_bytes(H, W) > 80 * 1024 and tile_stage_lds_bytes(H, W) <= 78 * 1024:
        return "tile_gscratch"
    return "tile"


PLANE_SIDE = next(n for n in range(65, 1025) if update_form(n, n) == "plane")

_WAVE_SHAPES = ((40, 40), (24, 40), (40, 27), (17, 23), (33, 20), (20, 36))
CASES = collections.OrderedDict((c.name, c) for c in [
    Case("wave", 40, 40, 3, 2, _WAVE_SHAPES + ((31, 26),), (2,) * 7, False, 6, 100, True),
    Case("wave_k6", 40, 40, 3, 6, _WAVE_SHAPES, (6, 4, 4, 2, 3, 4), False, 6, 200, False),
    Case("wave_k12", 40, 40, 3, 12, _WAVE_SHAPES, (12, 5, 5, 2, 3, 4), False, 6, 300, False),
    Case("tile", 72, 80, 3, 3, ((72, 80), (65, 33), (20, 70), (66, 76), (61, 78)), (3, 3, 3, 3, 2), False, 6, 400, True),
    Case("tile_gscratch", 96, 96, 3, 2, ((96, 96), (50, 91), (90, 40)), (2, 2, 2), False, 6, 500, False),
    Case("plane", PLANE_SIDE, PLANE_SIDE, 3, 2, ((PLANE_SIDE, PLANE_SIDE), (40, 30), (25, 36)), (2, 2, 2), False, 6, 600, False),
    Case("psf", 48, 48, 3, 2, ((48, 48), (24, 44), (41, 27), (37, 30)), (2,) * 4, True, 6, 700, True),
])
assert update_form(40, 40) == "wave" and update_form(72, 80) == "tile" and update_form(96, 96) == "tile_gscratch"
assert update_form(PLANE_SIDE - 1, PLANE_SIDE - 1) != "plane"


def psfs(c):
    """(observed PSFs, model PSF, difference kernel, SED scale) as parity_common.Workload(psf=True) builds them"""
    from oracle import pgm
    from scarlet_amd import synth
    obs = np.array([synth.gaussian_psf((41, 41), 1.2 + 0.15 * b) for b in range(c.B)])
    model = synth.gaussian_psf((41, 41), 0.9)
    diff = pgm.match_psfs(obs.astype(np.float32), model[None].astype(np.float32))
    scale = (model.max() / obs.max(axis=(1, 2))).astype(np.float32)
    return obs, model, diff, scale


def _hand_scene(c, h, w, seed):
    """two elliptical Gaussians, one centred on (h - 1, w - 1), one on (2, 2)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    peaks = [(h - 1, w - 1), (2, 2)]
    yy, xx = np.mgrid[:h, :w].astype(np.float64)
    model = np.zeros((c.B, h, w))
    for k, (cy, cx) in enumerate(peaks):
        smaj, q, th = rng.uniform(1.5, 3.5), rng.uniform(0.5, 1.0), rng.uniform(0, np.pi)
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
    """[(images (B, h, w) float32, centres (n, 2) int32)] of the case's scenes; shared, read-only"""
    if c.name not in _cache:
        from scarlet_amd import synth
        out = []
        for i, ((h, w), n) in enumerate(zip(c.shapes, c.counts)):
            if c.hand and i == len(c.shapes) - 1:
                images, centers = _hand_scene(c, h, w, c.seed + i)
            else:
                kw = dict(B=c.B, H=h, W=w, K=n, min_sep=4 if c.K <= 3 else 3)
                if c.psf:
                    kw["psfs"] = psfs(c)[0]
                sc = synth.make_scene(c.seed + i, **kw)
                images, centers = sc["images"], sc["centers"]
            images.setflags(write=False)
            out.append((images, centers))
        _cache[c.name] = out
    return _cache[c.name]


def padded(c):
    """(images (S, B, H, W) zero-padded, frame_shapes (S, 2), centres (S, K, 2), counts (S,)) of the case"""
    sc = scenes(c)
    S = len(sc)
    images = np.zeros((S, c.B, c.H, c.W), np.float32)
    centers = np.zeros((S, c.K, 2), np.int32)
    for s, (im, cen) in enumerate(sc):
        images[s, :, :im.shape[1], :im.shape[2]] = im
        centers[s, :len(cen)] = cen
    return images, np.array(c.shapes, np.int32), centers, np.array(c.counts, np.int32)


def oracle_kwargs(c):
    if not c.psf:
        return {}
    _, model, diff, _ = psfs(c)
    return dict(diff_kernel=diff, centroid_weight=model.astype(np.float32))


def oracle_start(c, images, centers, weights=1):
    """the constructors' scene in the oracle: ExtendedSource per catalogue pixel, each with its update()"""
    from oracle import pgm
    kw = {}
    if c.psf:
        obs, model, _, _ = psfs(c)
        kw = dict(obs_psfs=obs.astype(np.float32), frame_psf=model.astype(np.float32))
    return pgm.make_extended_scene(images, centers, np.ones(c.B) * BG, weights=weights, **kw)


def oracle_own_frame(args):
    """worker: scene `s` of case `name` started and fitted on its own frame -> (sed, morph, mse, centres)"""
    from oracle import pgm
    name, s, iters = args
    c = CASES[name]
    images, centers = scenes(c)[s]
    sc = oracle_start(c, np.array(images), centers)
    pgm.fit(sc, iters, e_rel=0)
    return (np.array([x.sed for x in sc.sources]), np.array([x.morph for x in sc.sources]), np.array(sc.mse),
            np.array([x.center for x in sc.sources]))


def oracle_zero_weight_padded(args):
    """worker: the same scene padded to the case's frame with weights = 0 outside it, fitted on the padded frame -- what
    a user without frame_shapes would do; morphologies cropped back to the scene"""
    from oracle import pgm
    name, s, iters = args
    c = CASES[name]
    images, centers = scenes(c)[s]
    h, w = images.shape[1:]
    pad = np.zeros((c.B, c.H, c.W), np.float32)
    pad[:, :h, :w] = images
    wgt = np.zeros((c.B, c.H, c.W), np.float32)
    wgt[:, :h, :w] = 1
    sc = oracle_start(c, pad, centers, weights=wgt)
    pgm.fit(sc, iters, e_rel=0)
    return (np.array([x.sed for x in sc.sources]), np.array([x.morph[:h, :w] for x in sc.sources]), np.array(sc.mse),
            np.array([x.center for x in sc.sources]))
