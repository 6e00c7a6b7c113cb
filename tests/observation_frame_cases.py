"""Joint fits of scenes with their own frame sizes (ObservationBatch(frame_shapes=...) -> BlendBatch.from_observations): the
cases shared by tests/test_observation_frame_cases.py (CPU: every scene is admissible in the oracle, float32 and float64
agree far inside the GPU tolerance, and zero-weight padding is NOT the reference's result) and
tests/test_gpu_observations_frames.py (-m gpu: the device against the oracle run of each scene on its own frame).
numpy, tests/frame_cases.py and oracle.pgm only.

The scenes are those of frame_cases, seen through two observations on the model's pixel grid:
  wave      40 x 40, 7 scenes, the last hand-placed on the frame's edge   wave form of the update, small contraction
  psf       48 x 48, observation a has difference kernels, b has none     per-observation PSF
  tile      72 x 80                                                        tile form
  wave_k12  K = 12 with ragged counts                                      the any-K contraction, the big-K Gram passes
  epochs    wave with both observations at band0 = 0                       overlapping channels; starts via set_state
  wide      the wave frames with C = 9, observations of 5 + 4 bands        the wide contraction
The first four split the three bands 2 + 1; `epochs` shows all three bands twice, the second time with fresh noise.  Every
case runs 6 iterations.  The start is the reference's CombinedExtendedSource on each scene's own frame
(pgm.init_combined_extended_source, morphology from observation 0, no update()); `epochs`, whose observations do not tile
the channels, starts from the state that the band-sliced observations of `wave` give.
"""
import collections

import numpy as np

import frame_cases as fc

BG = fc.BG
ITERS = 6
EPOCH_NOISE = 0.05

# base: the frame_cases case whose scenes are used (None: made here);  bands: [(band0, B)] per observation;
# start: the band split that init_combined sees (the observations' own where they tile the channels)
Case = collections.namedtuple("Case", "name base H W C K shapes counts psf bands start iters seed")


def _from(name, base, bands, start=None):
    c = fc.CASES[base]
    return Case(name, base, c.H, c.W, c.B, c.K, c.shapes, c.counts, c.psf, bands, start or bands, ITERS, c.seed)


_SPLIT = ((0, 2), (2, 1))
CASES = collections.OrderedDict((c.name, c) for c in [
    _from("wave", "wave", _SPLIT),
    _from("psf", "psf", _SPLIT),
    _from("tile", "tile", _SPLIT),
    _from("wave_k12", "wave_k12", _SPLIT),
    _from("epochs", "wave", ((0, 3), (0, 3)), start=_SPLIT),
    Case("wide", None, 40, 40, 9, 2, fc._WAVE_SHAPES, (2,) * 6, False, ((0, 5), (5, 4)), ((0, 5), (5, 4)), ITERS, 800),
])

_cache = {}


def scenes(c):
    """[(images (C, h, w) float32 over the model's channels, centres (n, 2) int32)] of the case's scenes; read-only"""
    if c.base is not None:
        return fc.scenes(fc.CASES[c.base])
    if c.name not in _cache:
        from scarlet_amd import synth
        out = []
        for i, ((h, w), n) in enumerate(zip(c.shapes, c.counts)):
            sc = synth.make_scene(c.seed + i, B=c.C, H=h, W=w, K=n, min_sep=4)
            sc["images"].setflags(write=False)
            out.append((sc["images"], sc["centers"]))
        _cache[c.name] = out
    return _cache[c.name]


def diff_kernels(c):
    """per observation None or (B_o, P, P) float32: observation a of `psf` carries the difference kernels of its bands"""
    if not c.psf:
        return [None] * len(c.bands)
    diff = fc.psfs(fc.CASES[c.base])[2].astype(np.float32)
    return [diff[b0:b0 + nb] if o == 0 else None for o, (b0, nb) in enumerate(c.bands)]


def centroid_weight(c):
    """None (the default) or the model PSF, as frame_cases.oracle_kwargs gives it"""
    return fc.psfs(fc.CASES[c.base])[1].astype(np.float32) if c.psf else None


def scene_observations(c, s):
    """the images (B_o, h, w) float32 of scene s as each observation sees them"""
    images = np.asarray(scenes(c)[s][0])
    out = []
    for o, (b0, nb) in enumerate(c.bands):
        im = images[b0:b0 + nb]
        if c.name == "epochs" and o == 1:       # a second epoch of the same bands: the same sky, fresh noise
            rng = np.random.Generator(np.random.PCG64(c.seed + 50 + s))
            im = (im + EPOCH_NOISE * rng.standard_normal(im.shape)).astype(np.float32)
        out.append(np.ascontiguousarray(im))
    return out


def padded(c, fill=0.0):
    """(obs_data, frame_shapes (S, 2), centres (S, K, 2), counts (S,)): obs_data is one dict per observation with the
    padded images (S, B_o, H, W) (padding = fill), band0 and diff"""
    S = len(c.shapes)
    centers = np.zeros((S, c.K, 2), np.int32)
    obs = [dict(images=np.full((S, nb, c.H, c.W), fill, np.float32), band0=b0, diff=d)
           for (b0, nb), d in zip(c.bands, diff_kernels(c))]
    for s in range(S):
        cen = scenes(c)[s][1]
        centers[s, :len(cen)] = cen
        for o, im in zip(obs, scene_observations(c, s)):
            o["images"][s, :, :im.shape[1], :im.shape[2]] = im
    return obs, np.array(c.shapes, np.int32), centers, np.array(c.counts, np.int32)


def oracle_start(c, s, dtype=np.float32):
    """(sed (n, C), morph (n, h, w), centres) of scene s as init_combined starts it on its own frame"""
    from oracle import pgm
    images, cen = scenes(c)[s]
    images = np.asarray(images).astype(dtype)
    parts = [images[b0:b0 + nb] for b0, nb in c.start]
    bg = [np.ones(nb) * BG for _, nb in c.start]
    seds, morphs = [], []
    for px in cen:
        sed, morph = pgm.init_combined_extended_source((int(px[0]), int(px[1])), parts, bg, obs_idx=0)
        seds.append(sed)
        morphs.append(morph)
    return np.array(seds, dtype), np.array(morphs, dtype), np.array(cen, np.int32)


def oracle_scene(c, obs_images, sed0, morph0, cen0, shifts=None, dtype=np.float32, weights=None):
    """the oracle's scene of given per-observation images (each (B_o, h, w)) from a given state; weights: None, or one
    entry per observation (scalar or (B_o, h, w))"""
    from oracle import pgm
    cw = centroid_weight(c)
    h, w = obs_images[0].shape[1:]
    sc = pgm.scene_from_state(np.zeros((c.C, h, w), dtype), np.asarray(sed0, dtype), np.asarray(morph0, dtype), cen0, shifts,
                              centroid_weight=None if cw is None else cw.astype(dtype))
    sc.observations = []
    for o, ((b0, nb), d) in enumerate(zip(c.bands, diff_kernels(c))):
        sc.observations.append(dict(images=np.asarray(obs_images[o]).astype(dtype), band_slice=slice(b0, b0 + nb),
                                    weights=1 if weights is None else weights[o],
                                    diff_kernel=None if d is None else d.astype(dtype)))
    return sc


def _result(sc):
    return (np.array([x.sed for x in sc.sources]), np.array([x.morph for x in sc.sources]), np.array(sc.mse),
            np.array([x.center for x in sc.sources]), len(sc.mse), [int(x.flags) for x in sc.sources])


def oracle_own_frame(args):
    """worker: scene `s` of case `name` started and fitted on its own frame in float32 or float64 -> (sed, morph, mse,
    centres, iterations, flags)"""
    from oracle import pgm
    name, s, iters, dtype = args
    c, dt = CASES[name], np.dtype(dtype).type
    sed0, morph0, cen0 = oracle_start(c, s, dt)
    sc = oracle_scene(c, scene_observations(c, s), sed0, morph0, cen0, None, dt)
    pgm.fit(sc, iters, e_rel=0)
    return _result(sc)


def oracle_zero_weight_padded(args):
    """worker: the same scene padded to the case's frame with weights = 0 outside it, started and fitted on the padded
    frame -- what a user without frame shapes would do; morphologies cropped back to the scene"""
    from oracle import pgm
    name, s, iters = args
    c = CASES[name]
    h, w = c.shapes[s]
    cen = scenes(c)[s][1]
    pads, wgts = [], []
    for im in scene_observations(c, s):
        p = np.zeros((im.shape[0], c.H, c.W), np.float32)
        p[:, :h, :w] = im
        g = np.zeros_like(p)
        g[:, :h, :w] = 1
        pads.append(p)
        wgts.append(g)
    assert c.start == c.bands, "the start of the padded run comes from the observations themselves"
    bg = [np.ones(nb) * BG for _, nb in c.start]
    start = [pgm.init_combined_extended_source((int(px[0]), int(px[1])), pads, bg, obs_idx=0) for px in cen]
    sc = oracle_scene(c, pads, np.array([x[0] for x in start]), np.array([x[1] for x in start]), cen, None, np.float32, wgts)
    pgm.fit(sc, iters, e_rel=0)
    r = _result(sc)
    return (r[0], r[1][:, :h, :w]) + r[2:]


def oracle_fit_from(args):
    """worker (never touches the GPU): scene `s` of case `name` fitted from a given state (the device's own start) ->
    (sed, morph, mse, centres, iterations, flags).  weights: None or one entry per observation"""
    from oracle import pgm
    name, s, sed0, morph0, cen0, sh0, iters, e_rel, approximate_L, weights = args
    c = CASES[name]
    sh = None if sh0 is None or np.isnan(sh0).any() else sh0       # (NaN: no centroid shift yet, as after init_combined)
    sc = oracle_scene(c, scene_observations(c, s), sed0, morph0, cen0, sh, np.float32, weights)
    pgm.fit(sc, iters, e_rel=e_rel, approximate_L=approximate_L)
    return _result(sc)
