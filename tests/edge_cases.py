"""Scenes whose sources sit on the frame's borders, for every single-observation launch form: the cases of
tests/test_edge_cases.py (CPU: every scene is proved admissible against the oracle), tests/test_gpu_edges.py (-m gpu:
the device against the oracle) and the reference fixture tests/golden/fit_edges.npz (oracle/gen_golden.py edges).
numpy, launch_form_cases, constraints_common and oracle.pgm (scarlet_amd.synth for the PSFs); the GPU only in make_batch.

Cases.  Every `fit` case of launch_form_cases.CASES (01 to 23: shape, options, batch keywords, iterations) and two PSF
cases the table lacks, built the way parity_common.Workload(psf=True) builds its batches: 30 (k_psf_conv, the three-pass
form, 9 x 9 PSFs) and 31 (41 x 41 PSFs: the centroid weight is the model PSF, so its window is clipped from radius 20
down to 0).  Each case runs 2 scenes for max(case.iters or 0, 6) iterations -- the centroid fires at it % 5 == 0, so
iteration 5 recentres and iteration 6 applies a non-zero shift -- and 11 on the 16 x 16 / 16 x 20 frames and in the
persistent 64 x 64 case; a fused case of exactly one iteration is launched once per iteration.

Peaks.  The reference's max_pixel refuses a centre with a coordinate below 2 (its 5 x 5 window starts at c - 2) and
clips the window at the high edges, so the limits are 2 and H - 1 / W - 1.  Truth peaks come from the corners (2, 2),
(2, W-1), (H-1, 2), (H-1, W-1) and the mid-edges (2, W/2), (H-1, W/2), (H/2, 2), (H/2, W-1):
  scene 0: a corner (alternating (2, 2) / (H-1, W-1) along the table), an adjacent corner, then mid-edges; its
           catalogue pixels sit on the truth.  The corner opposite the first one stays free: it is the broad source's
           farthest pixel, and a compact source on it takes that pixel's flux from the first iteration on;
  scene 1: the two corners of the other diagonal -- all four corners where K = 4 -- then mid-edges; its catalogue
           pixels sit one pixel towards the interior, so the tracker has to move onto the border.
Every scene has a peak on a low limit and one on a high one, the two scenes use different corners, scene 1 has two
corner peaks on opposite sides (two clipped boxes that overlap in the interior).  The grouped case keeps its two-layer
source on the first corner.

Sources.  Component 0 of scene 0 is broad: amplitude 40, profile exp(-r / (max(H, W) / 2)).  It stays positive at the
pixel farthest from its peak after every iteration, so the monotonic sweep never meets three quiet levels and runs to
its last level (from a corner of a 64 x 64 frame: level 2 * 61 + 61 = 183 from (2, 2), 189 from (63, 63)); beyond
64 px it keeps a positive pixel farther than 63 px (Chebyshev) from its peak, so neither box of boxupdate.h is complete
and the full-frame kernel takes it.  The others are the elliptical Gaussians of synth.make_scene with amplitudes in
20 .. 50 (a fainter one on the broad source's slope would have its maximum pulled off its own centre).  Scene 1's are
narrower (major sigma up to 2.5), of near-equal amplitude (36 .. 44) and have one band of their own each (1 there,
0.05 .. 0.15 elsewhere; K <= B in every case).  That is what moves a tracker: the constructor's symmetry and sweep
leave the maximum on the catalogue pixel, and max_pixel leaves it only if one gradient step lifts the true peak above
it.  The morphologies step with 1 / lambda_max of the SEDs' Gram matrix; with SEDs alike that is the full step for
the brightest source of a scene and a fraction of it for the others, which then stay on their catalogue pixels (one
source in three moved with the SEDs of make_scene).  Under a PSF the step is shorter still, by the squared norm of the
difference kernel, and the constraints pin the maximum where it starts: no tracker of the two PSF cases left its
catalogue pixel within 31 iterations, whatever the width.  Their scene 1 therefore keeps its catalogue pixels on the
truth; the centroid's clipped window is met there all the same (radius 2 on a low limit, 0 on a high one).  Noise 0.1.

Seeds.  `SEEDS` holds one seed per scene.  tests/test_edge_cases.py asserts the admissibility conditions for each of
them; a scene that fails one gets the next seed here, before any device run (`python tests/edge_cases.py` repeats the
search and prints the table).
"""
import collections
import functools

import numpy as np

import launch_form_cases as lf

BG = lf.BG
NOISE = 0.1
S = 2
BROAD_AMPLITUDE = 40.0
WIDE, NARROW = (1.5, 3.5), (1.5, 2.5)          # major sigma: synth.make_scene's, scene 1's
LONG_ITERS = 11
MIN_ITERS = 6
PSF = {"30_psf_three_pass_9": 9, "31_psf_41_centroid": 41}          # side of the PSFs of the two PSF cases

CASES = collections.OrderedDict((c.name, c) for c in [c for c in lf.CASES.values() if c.kind == "fit"] + [
    lf._c("30_psf_three_pass_9", 3, 3, 32, 40),
    lf._c("31_psf_41_centroid", 4, 5, 64, 64),
])
INDEX = {name: i for i, name in enumerate(CASES)}

# the scenes' seeds: {case: (scene 0, scene 1)}; default 9000 + 10 * index + scene.  The scenes listed failed with their
# default: a tracker of scene 1 stayed on its catalogue pixel (03, 17, 19, 23), the group's came within 1 px of row 0 (23)
SEEDS = {
    "03_exact_one_iteration": (9020, 9023),
    "17_tile_gscratch_96": (9160, 9163),
    "19_box_128": (9180, 9185),
    "23_group": (9220, 9225),
}


def seeds(c):
    return SEEDS.get(c.name, (9000 + 10 * INDEX[c.name], 9001 + 10 * INDEX[c.name]))


def iterations(c):
    if max(c.H, c.W) <= 20 or c.name == "04_exact_persistent":
        return LONG_ITERS
    return max(c.iters or 0, MIN_ITERS)


def one_launch_per_iteration(c):
    return c.iters == 1


def grouped(c):
    return c.batch.get("group") is not None


def corners(c):
    return [(2, 2), (2, c.W - 1), (c.H - 1, 2), (c.H - 1, c.W - 1)]


def mid_edges(c):
    return [(2, c.W // 2), (c.H - 1, c.W // 2), (c.H // 2, 2), (c.H // 2, c.W - 1)]


def truth_peaks(c, s):
    """the truth peak of every component of scene s; the layers of a group share theirs"""
    i, cor, mid = INDEX[c.name], corners(c), mid_edges(c)
    n = c.K - 1 if grouped(c) else c.K
    if s == 0:
        a = 0 if i % 2 == 0 else 3
        peaks = [cor[a], cor[1 if i % 4 < 2 else 2]] + [mid[(i + j) % 4] for j in range(2)]
    else:
        a = 2 if i % 4 < 2 else 1
        peaks = [cor[a], cor[3 - a]] + ([cor[0], cor[3]] if n == 4 else [mid[(i + 2 + j) % 4] for j in range(2)])
    peaks = peaks[:n]
    return [peaks[0]] + peaks if grouped(c) else peaks


def inward(c, p):
    """the pixel one step from a limit towards the interior"""
    step = lambda v, n: v + 1 if v == 2 else (v - 1 if v == n - 1 else v)
    return (step(p[0], c.H), step(p[1], c.W))


def displaced(c, s):
    """scene s starts its trackers one pixel inside the truth"""
    return s == 1 and c.name not in PSF


def catalogue(c, s, peaks=None):
    peaks = truth_peaks(c, s) if peaks is None else peaks
    return np.array([inward(c, p) for p in peaks] if displaced(c, s) else peaks, np.int32)


def psfs(c):
    """(observed PSFs, model PSF, difference kernel, SED scale) of a PSF case as parity_common.Workload builds them"""
    from oracle import pgm
    from scarlet_amd import synth
    P = PSF[c.name]
    obs = np.array([synth.gaussian_psf((P, P), 1.2 + 0.15 * b) for b in range(c.B)])
    model = synth.gaussian_psf((P, P), 0.9)
    diff = pgm.match_psfs(obs.astype(np.float32), model[None].astype(np.float32))
    scale = (model.max() / obs.max(axis=(1, 2))).astype(np.float32)
    return obs, model, diff, scale


def render(c, seed, peaks, broad, peaked=False):
    """images (B, H, W) float32 of one scene: the sources at `peaks` (equal neighbours = the layers of one source),
    the first one broad if asked, convolved with the observed PSFs in a PSF case, plus noise"""
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[:c.H, :c.W].astype(np.float64)
    model = np.zeros((c.B, c.H, c.W))
    for k, (cy, cx) in enumerate(peaks):
        if k and tuple(peaks[k - 1]) == (cy, cx):
            continue
        dy, dx = yy - cy, xx - cx
        if broad and k == 0:
            morph, amp = np.exp(-np.hypot(dy, dx) / (max(c.H, c.W) / 2.0)), BROAD_AMPLITUDE
        else:
            smaj, q, th = rng.uniform(*(NARROW if peaked else WIDE)), rng.uniform(0.5, 1.0), rng.uniform(0, np.pi)
            u, v = np.cos(th) * dx + np.sin(th) * dy, -np.sin(th) * dx + np.cos(th) * dy
            morph = np.exp(-0.5 * ((u / smaj) ** 2 + (v / (smaj * q)) ** 2))
            amp = rng.uniform(36.0, 44.0) if peaked else np.exp(rng.uniform(np.log(20.0), np.log(50.0)))
        colour = rng.uniform(0.2, 1.0, size=c.B)
        if peaked:                                          # one band of its own per source
            colour = rng.uniform(0.05, 0.15, size=c.B)
            colour[k % c.B] = 1.0
        model += (amp * colour)[:, None, None] * morph
    if c.name in PSF:
        from scipy.signal import fftconvolve
        obs = psfs(c)[0]
        model = np.array([fftconvolve(model[b], obs[b], mode="same") for b in range(c.B)])
    return (model + rng.normal(0.0, NOISE, size=model.shape)).astype(np.float32)


_scene_cache = {}


def scene(c, s):
    """(images (B, H, W) float32, catalogue pixels (K, 2) int32, truth peaks) of scene s; shared, read-only"""
    key = (c.name, s, seeds(c)[s])
    if key not in _scene_cache:
        peaks = truth_peaks(c, s)
        images = render(c, seeds(c)[s], peaks, broad=(s == 0), peaked=(s == 1))
        images.setflags(write=False)
        _scene_cache[key] = (images, catalogue(c, s, peaks), peaks)
    return _scene_cache[key]


def scenes(c):
    """images (S, B, H, W), catalogue pixels (S, K, 2) of the case's two scenes"""
    sc = [scene(c, s) for s in range(S)]
    return np.stack([x[0] for x in sc]), np.stack([x[1] for x in sc])


options, state = lf.options, lf.state


def make_batch(scarlet, c, images, centers, mse_capacity=None):
    """the case's freshly initialised batch of the given scenes (any number of them): launch_form_cases.make_batch,
    and for a PSF case what parity_common.Workload(psf=True).batch does"""
    cap = iterations(c) + 1 if mse_capacity is None else mse_capacity
    bg = np.ones(c.B) * BG
    if c.name in PSF:
        _, model, diff, scale = psfs(c)
        b = scarlet.BlendBatch(images, centers, mse_capacity=cap, centroid_weight=model.astype(np.float32))
        b.set_diff_kernel(diff)
        return b.init_extended(bg, sed_scale=scale)
    kw = dict(c.batch)
    if grouped(c):
        kw["group"] = [c.batch["group"][0]] * len(images)
    b = scarlet.BlendBatch(images, centers, mse_capacity=cap, **kw)
    return b.init_sources(bg) if b.group is not None else b.init_extended(bg)


REFUSED = (1, 10)


def refused_scene(c):
    """scene 1's layout with its last source moved to (1, 10), a centre the reference's max_pixel refuses, and every
    catalogue pixel on its truth"""
    peaks = truth_peaks(c, 1)[:-1] + [REFUSED]
    return render(c, seeds(c)[1] + 5, peaks, broad=False, peaked=True), np.array(peaks, np.int32)


# ---------------------------------------------------------------------------------------- the settings of a case
def settings(c):
    """(symmetric, monotonic, l0, l1) per component, (K,) each, as the case's batch keywords set them"""
    sym = np.broadcast_to(np.asarray(c.batch.get("symmetric", True), np.uint8), (c.K,)).copy()
    mono = np.broadcast_to(np.asarray(c.batch.get("monotonic", True), np.uint8), (c.K,)).copy()
    off = np.full((c.K,), -1.0, np.float32)
    return sym, mono, off, off.copy()


def oracle_keywords(c):
    """the `okw` of a spec: the difference kernel and the centroid weight of a PSF case"""
    if c.name not in PSF:
        return {}
    _, model, diff, _ = psfs(c)
    return dict(diff_kernel=diff, centroid_weight=model.astype(np.float32))


def spec(c, images, sed0, morph0, cen0, sh0):
    """the scene description constraints_common.build_scene takes: a state and the case's settings"""
    sym, mono, l0, l1 = settings(c)
    group = c.batch["group"][0] if grouped(c) else None
    return dict(images=images, sed0=sed0, morph0=morph0, cen0=cen0, sh0=sh0, sym=sym, mono=mono, l0=l0, l1=l1,
                group=group, okw=oracle_keywords(c), approximate_L=False)


def oracle_start(c, s, dt):
    """the constructors' state of scene s in the oracle (ExtendedSource per catalogue pixel, MultiComponentSource for
    the group; each with its constructor's update()): sed, morph, centres, shifts (NaN = none)"""
    from oracle import pgm
    images, pixels, _ = scene(c, s)
    images = images.astype(dt)
    bg = np.ones(c.B) * BG
    sym, mono, _, _ = settings(c)
    kw, cw = {}, pgm.default_centroid_weight()
    if c.name in PSF:
        obs, model, _, _ = psfs(c)
        kw, cw = dict(obs_psfs=obs.astype(dt), frame_psf=model.astype(dt)), model.astype(dt)
    out, k = [], 0
    while k < c.K:
        px = (int(pixels[k][0]), int(pixels[k][1]))
        if grouped(c) and c.batch["group"][s][k] >= 0:
            seds, morphs = pgm.init_multicomponent_source(px, images, bg)
            ms = pgm.MultiSource([pgm.Source(seds[j], morphs[j], px, dt) for j in range(len(seds))], px)
            pgm.multi_source_update(ms, 0)
            out += [(x.sed, x.morph, ms.center, ms.shift) for x in ms.components]
            k += len(seds)
            continue
        sed, morph = pgm.init_extended_source(px, images, bg, monotonic=bool(mono.any()), **kw)
        src = pgm.Source(sed, morph, px, dt, symmetric=bool(sym[k]), monotonic=bool(mono[k]), centroid_weight=cw)
        pgm.source_update(src, 0)
        out.append((src.sed, src.morph, src.center, src.shift))
        k += 1
    shifts = np.array([(np.nan, np.nan) if o[3] is None else o[3] for o in out], np.float64)
    return np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out]), shifts


def fit_from(sp, iters, dt=np.float32, trace=False):
    """the oracle's fit of one scene from the state in `sp`; with `trace` also, per iteration, the centres, the
    morphologies, the stepped morphologies and the morphologies as prox_plus saw them"""
    import constraints_common as cc
    from oracle import pgm
    sc = cc.build_scene(sp, dt)
    post, cens = [], []
    if trace:
        for src in sc.sources:
            src.trace = dict(step=[], pre_plus=[])

    def look(scn):
        post.append(np.array([x.morph.copy() for x in scn.sources]))
        cens.append(np.array([x.center for x in scn.sources]))

    pgm.fit(sc, iters, e_rel=0, approximate_L=False, callback=look if trace else None)
    out = dict(sed=np.array([x.sed for x in sc.sources]), morph=np.array([x.morph for x in sc.sources]),
               mse=np.array(sc.mse), cen=np.array([x.center for x in sc.sources]), it=len(sc.mse),
               flags=np.array([int(x.flags) for x in sc.sources]), post=post, centers=cens)
    if trace and not grouped_spec(sp):
        out["pre"] = [(np.array([x.trace["step"][t] for x in sc.sources]), np.array([x.trace["pre_plus"][t] for x in sc.sources]))
                      for t in range(iters)]
    return out


def grouped_spec(sp):
    return sp.get("group") is not None and (np.asarray(sp["group"]) >= 0).any()


def oracle_worker(args):
    """for a spawned pool (never touches the GPU): (spec, iters) -> sed, morph, mse, centres, it, flags"""
    sp, iters = args
    r = fit_from(sp, iters)
    return r["sed"], r["morph"], r["mse"], r["cen"], r["it"], r["flags"].tolist()


@functools.lru_cache(maxsize=None)
def _own_fit(name, s, dtname, seed):
    c, dt = CASES[name], np.dtype(dtname).type
    sed0, morph0, cen0, sh0 = oracle_start(c, s, dt)
    r = fit_from(spec(c, scene(c, s)[0], sed0, morph0, cen0, sh0), iterations(c), dt, trace=True)
    r["start"] = (sed0, morph0, cen0, sh0)
    return r


def own_fit(c, s, dt=np.float32):
    """the oracle's fit of scene s from its own constructors' state, traced; shared, computed once"""
    return _own_fit(c.name, s, np.dtype(dt).name, seeds(c)[s])


def on_limit(c, p, q):
    """the peak p of the table lies on limits; q lies on the same ones"""
    ok = True
    for v, w, n in ((p[0], q[0], c.H), (p[1], q[1], c.W)):
        if v == 2 or v == n - 1:
            ok = ok and w == v
    return ok


def farthest(c, p):
    return (0 if p[0] > c.H // 2 else c.H - 1, 0 if p[1] > c.W // 2 else c.W - 1)


def admissible(c, s):
    """the conditions of tests/test_edge_cases.py for one scene: None, or the first one that fails"""
    from conftest import rel_err
    try:
        a, b = own_fit(c, s, np.float32), own_fit(c, s, np.float64)
    except Exception as e:                                   # (the reference raises for a centre it refuses)
        return "the fit did not complete: %r" % (e,)
    iters, peaks = iterations(c), scene(c, s)[2]
    if a["it"] != iters or b["it"] != iters:
        return "the fit stopped early"
    for r in (a, b):
        if min(int(x.min()) for x in r["centers"] + [r["start"][2]]) < 2:
            return "a centre came closer than 2 px to a low edge"
    for k, p in enumerate(peaks):
        if not on_limit(c, p, a["cen"][k]):
            return "component %d ended on %s, its peak is %s" % (k, tuple(a["cen"][k]), p)
    if not (np.array_equal(a["cen"], b["cen"]) and np.array_equal(a["flags"], b["flags"]) and
            all(np.array_equal(x, y) for x, y in zip(a["centers"], b["centers"]))):
        return "float32 and float64 differ in centres or flags"
    for key in ("sed", "morph", "mse"):
        if not rel_err(a[key], b[key]) <= 1e-5:
            return "float32 and float64 differ by %.2e in %s" % (rel_err(a[key], b[key]), key)
    if s == 0:
        for t in range(iters):
            cy, cx = a["centers"][t][0]
            for r in (a, b):
                m = r["post"][t][0]
                if max(c.H, c.W) <= 64:
                    if not m[farthest(c, (cy, cx))] > 0:
                        return "iteration %d: the broad component is not positive at its farthest pixel" % (t + 1)
                else:
                    yy, xx = np.mgrid[:c.H, :c.W]
                    if not (m[np.maximum(np.abs(yy - cy), np.abs(xx - cx)) > 63] > 0).any():
                        return "iteration %d: the broad component has no positive pixel beyond 63 px" % (t + 1)
    return None


if __name__ == "__main__":                                   # the seed search: the first admissible seed of every scene
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for c in CASES.values():
        row = list(seeds(c))
        for s in range(S):
            for _ in range(20):
                SEEDS[c.name] = tuple(row)
                why = admissible(c, s)
                if why is None:
                    break
                print("#", c.name, s, row[s], why)
                row[s] += 2
        print('    "%s": (%d, %d),' % (c.name, row[0], row[1]))
