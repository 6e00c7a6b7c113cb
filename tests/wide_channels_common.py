"""Shared by tests/test_gpu_wide_channels.py: joint fits over more than 8 model channels
(BlendBatch.from_observations(..., wide=True)) and their oracle.  The cases are tests/observations_prior_common.py's
`Case`s -- host data, a host start, the oracle oracle.pgm.fit with `scene.observations` and `band_slice`, which is plain
numpy and has no channel limit -- with per-component constraint switches and the constants of the last iteration added."""
import numpy as np

import observations_prior_common as oc

F32 = np.float32
TOL = oc.TOL


def scenes(first, S, C, H=32, W=32, K=3, min_sep=4):
    """(images (S, C, H, W), centres, start SEDs (S, K, C), start morphologies) of S synthetic scenes"""
    return oc._scenes(first, S, C=C, H=H, W=W, K=K, min_sep=min_sep)


def tiled(images, widths):
    """observations that tile the channels in order, e.g. widths (6, 4, 7) for 17 channels"""
    assert sum(widths) == images.shape[1] and max(widths) <= 8
    out, at = [], 0
    for w in widths:
        out.append(dict(images=np.ascontiguousarray(images[:, at:at + w]), band0=at))
        at += w
    return out


def case(name, first, widths, S=3, K=3, H=32, W=32, min_sep=4, **kw):
    images, centers, sed, morph = scenes(first, S, sum(widths), H=H, W=W, K=K, min_sep=min_sep)
    return oc.Case(name, tiled(images, widths), centers, sed, morph, **kw)


def spec_of(c, st0, i, per_component=None, prior=True):
    """scene i for `oracle_fit`; per_component: dict symmetric / monotonic / l1 -> (S, K) arrays (l1 < 0: off)"""
    spec = c.spec(st0, i, prior=prior)
    if per_component is not None:
        n = int(c.n[i])
        spec["per_component"] = {k: np.asarray(v)[i][:n] for k, v in per_component.items()}
    return spec


def oracle_fit(args):
    """(spec, iters, e_rel, dtype) -> sed, morph, mse, centres, it, flags, the constants (n, 2) of the last iteration
    (a worker of a spawned pool: no GPU)"""
    spec, iters, e_rel, dt = args
    sc = oc.build_scene(spec, dt)
    pc = spec.get("per_component")
    if pc is not None:
        for k, s in enumerate(sc.sources):
            s.symmetric, s.monotonic = bool(pc["symmetric"][k]), bool(pc["monotonic"][k])
            s.l1_thresh = None if pc["l1"][k] < 0 else float(pc["l1"][k])
    oc.run(sc, spec, iters, e_rel)
    return (np.array([s.sed for s in sc.sources]), np.array([s.morph for s in sc.sources]), np.array(sc.mse),
            np.array([s.center for s in sc.sources]), len(sc.mse), [int(s.flags) for s in sc.sources],
            np.array([[float(s.L_sed), float(s.L_morph)] for s in sc.sources]))
