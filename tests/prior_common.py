"""Oracle side of tests/test_gpu_prior.py: the CPU oracle's fit of ONE scene whose components carry quadratic priors
(`s.prior = (grad, lip)`, oracle/pgm.py:747-764), as a worker for a spawned pool (it never touches the GPU), and the
float64-anchored threshold rule of tests/parity_common.py restated with the prior.

A scene is described by a dict `spec`:
  images (B, H, W); sed0 (n, B), morph0 (n, H, W), cen0 (n, 2), sh0 (n, 2): the device's own initial state
  ws, wm (n,): the prior's weights; ts (n, B), tm (n, H, W) or None: its targets (None = 0)
  fix_sed, fix_morph (n,) bool or None; group (n,) or None (-1 = a source of its own, g >= 0 = a layer of source g)
  okw: weights / diff_kernel / centroid_weight / l0_thresh of pgm.scene_from_state;  approximate_L
"""
import numpy as np

from conftest import rel_err

TOL = 1e-5


def build_scene(spec, dt):
    from oracle import pgm
    okw = dict(spec.get("okw") or {})
    for key in ("diff_kernel", "weights"):
        if okw.get(key) is not None and np.ndim(okw[key]):
            okw[key] = np.asarray(okw[key]).astype(dt)
    sc = pgm.scene_from_state(spec["images"].astype(dt), spec["sed0"].astype(dt), spec["morph0"].astype(dt),
                              spec["cen0"], spec["sh0"], **okw)
    n = len(sc.sources)
    ws, wm = spec.get("ws"), spec.get("wm")
    for k, s in enumerate(sc.sources):
        if spec.get("fix_sed") is not None:
            s.fix_sed = bool(spec["fix_sed"][k])
        if spec.get("fix_morph") is not None:
            s.fix_morph = bool(spec["fix_morph"][k])
        a = dt(0 if ws is None else ws[k])
        c = dt(0 if wm is None else wm[k])
        if a == 0 and c == 0:
            continue
        ts = dt(0) if spec.get("ts") is None else spec["ts"][k].astype(dt)
        tm = dt(0) if spec.get("tm") is None else spec["tm"][k].astype(dt)
        s.prior = ((lambda sed, morph, a=a, c=c, ts=ts, tm=tm: (a * (sed - ts), c * (morph - tm))),
                   (lambda sed, morph, a=a, c=c: (a, c)))
    group = spec.get("group")
    if group is not None and (np.asarray(group) >= 0).any():
        trees, k = [], 0
        while k < n:
            if group[k] < 0:
                trees.append(sc.sources[k]); k += 1
                continue
            m = 1
            while k + m < n and group[k + m] == group[k]:
                m += 1
            cw = okw.get("centroid_weight")
            trees.append(pgm.MultiSource(sc.sources[k:k + m], sc.sources[k].center, centroid_weight=cw))
            k += m
        sc.trees = trees
    return sc


def oracle_fit(args):
    """(spec, iters, e_rel, dtype) -> sed, morph, mse, centres, it, flags"""
    from oracle import pgm
    spec, iters, e_rel, dt = args
    sc = build_scene(spec, dt)
    pgm.fit(sc, iters, e_rel=e_rel, approximate_L=bool(spec.get("approximate_L")))
    return (np.array([s.sed for s in sc.sources]), np.array([s.morph for s in sc.sources]), np.array(sc.mse),
            np.array([s.center for s in sc.sources]), len(sc.mse), [int(s.flags) for s in sc.sources])


def oracle_trace(spec, iters, dt):
    """per iteration: the morphologies after it, and (stepped, as prox_plus saw them)"""
    from oracle import pgm
    sc = build_scene(spec, dt)
    for s in sc.sources:
        s.trace = dict(step=[], pre_plus=[])
    post = []
    pgm.fit(sc, iters, e_rel=0, approximate_L=bool(spec.get("approximate_L")),
            callback=lambda scn: post.append(np.array([s.morph.copy() for s in scn.sources])))
    pre = [(np.array([s.trace["step"][t] for s in sc.sources]), np.array([s.trace["pre_plus"][t] for s in sc.sources]))
           for t in range(iters)]
    return post, pre


def straddles_threshold(gpu_snaps, spec, iters):
    """parity_common.straddles_threshold with the prior in both oracles.  gpu_snaps[t]: the scene's morphologies
    (n, H, W) after iteration t + 1 of a per-iteration re-run on the device from the same state.  Accepts the scene
    only if GPU and float32 oracle agree within 1e-5 before t0, disagree about the SUPPORT in a pixel at t0, and the
    float64 trajectory's value at that pixel at one of the two threshold tests of t0 lies within 1e-5 x max|morph| of
    0.  Returns (ok, message)."""
    o32, _ = oracle_trace(spec, iters, np.float32)
    o64, pre64 = oracle_trace(spec, iters, np.float64)
    for t in range(iters):
        gm = gpu_snaps[t]
        mismatch = (gm == 0) != (o32[t] == 0)
        close = rel_err(gm, o32[t]) <= TOL
        if mismatch.any():
            scale = np.abs(o64[t]).max()
            near = np.minimum(np.abs(pre64[t][0][mismatch]), np.abs(pre64[t][1][mismatch]))
            on_threshold = near <= TOL * scale
            if on_threshold.any():
                k, y, x = (int(v[np.argmax(on_threshold)]) for v in np.nonzero(mismatch))
                return True, ("iteration %d, component %d pixel (%d, %d): float64 values at the threshold tests: stepped "
                              "%.3e, before prox_plus %.3e (tolerance 1e-5 x %.3g); gpu %.3e, float32 oracle %.3e" % (
                                  t + 1, k, y, x, pre64[t][0][k, y, x], pre64[t][1][k, y, x], scale, gm[k, y, x],
                                  o32[t][k, y, x]))
        if not close:
            return False, "iteration %d: gpu and float32 oracle differ by %.2e with no pixel on a threshold" % (
                t + 1, rel_err(gm, o32[t]))
    return False, "no divergence found when re-running the scene alone"
