"""Shared machinery of tests/test_gpu_constraints.py: the mixed setting pattern, the CPU oracle's fit of ONE scene whose
sources carry their own switches (oracle/pgm.py:525-573), and the rule by which the test's seeds were chosen.

The pattern: component k of scene s takes the (symmetric, monotonic) pair PAIRS[(k + s) % 4], so every scene mixes the
pairs and the pairs rotate by one per scene; component 0 of scene 0 has l0_thresh = L0 and component 1 of the next scene
(the same scene when there is only one) has l1_thresh = L1.

Seeds.  The algorithm compares pixel values with 0 in two places (tests/parity_common.py) and a pixel that sits on the
threshold to within float32 rounding may land on either side.  These tests take no such exemption (the cap is 0
scenes): every seed used was chosen ON THE CPU, before any device run, so that the reference alone is decided --
`seed_is_decided`: started from the oracle's own ExtendedSource starts, the float32 and the float64 oracle agree on the
support of every morphology after every iteration and differ by at most 1e-6 max-norm relative.
tools/pick_constraint_seeds.py repeats the search.
"""
import numpy as np

from conftest import rel_err
import prior_common

PAIRS = ((1, 1), (0, 1), (1, 0), (0, 0))
L0, L1 = 0.3, 0.2
BG = 0.1
SEED_TOL = 1e-6


def pattern(S, K, thresholds=True):
    """(sym, mono) uint8 (S, K) and (l0, l1) float32 (S, K), -1 = off"""
    sym = np.zeros((S, K), np.uint8)
    mono = np.zeros((S, K), np.uint8)
    for s in range(S):
        for k in range(K):
            sym[s, k], mono[s, k] = PAIRS[(k + s) % 4]
    l0 = np.full((S, K), -1.0, np.float32)
    l1 = np.full((S, K), -1.0, np.float32)
    if thresholds:
        l0[0, 0] = L0
        l1[1 if S > 1 else 0, 1] = L1
    return sym, mono, l0, l1


def build_scene(spec, dt):
    """prior_common.build_scene (state, priors, groups) plus the per-source switches sym / mono / l0 / l1 (n,) of `spec`
    and, for several observations, spec["observations"] = [dict(images, band_slice)]"""
    from oracle import pgm
    sc = prior_common.build_scene(spec, dt)
    for k, s in enumerate(sc.sources):
        s.symmetric, s.monotonic = bool(spec["sym"][k]), bool(spec["mono"][k])
        s.l0_thresh = None if spec["l0"][k] < 0 else float(spec["l0"][k])
        s.l1_thresh = None if spec["l1"][k] < 0 else float(spec["l1"][k])
        if not s.symmetric or s.shift is None or np.isnan(s.shift[0]):
            s.shift = None
    for t in getattr(sc, "trees", None) or []:
        if isinstance(t, pgm.MultiSource):                      # the layers agree: the first one's value
            t.symmetric, t.monotonic = t.components[0].symmetric, t.components[0].monotonic
    if spec.get("observations") is not None:
        sc.observations = [dict(images=o["images"].astype(dt), band_slice=o["band_slice"], weights=1, diff_kernel=None)
                           for o in spec["observations"]]
    return sc


def oracle_fit(spec, iters, dt=np.float32, trace=False):
    from oracle import pgm
    sc = build_scene(spec, dt)
    post = []
    cb = (lambda scn: post.append(np.array([s.morph.copy() for s in scn.sources]))) if trace else None
    pgm.fit(sc, iters, e_rel=0, approximate_L=bool(spec.get("approximate_L")), callback=cb)
    return dict(sed=np.array([s.sed for s in sc.sources]), morph=np.array([s.morph for s in sc.sources]),
                mse=np.array(sc.mse), cen=np.array([s.center for s in sc.sources]), it=len(sc.mse),
                flags=np.array([int(s.flags) for s in sc.sources]), post=post)


def oracle_start(images, centers, sym, mono, l0, l1, dt=np.float32):
    """ExtendedSource starts of one scene in the oracle: init_extended_source, then the constructor's update() with the
    source's own switches (source.py:444-492).  Returns sed (n, B), morph (n, H, W), centres, shifts (NaN = none)."""
    from oracle import pgm
    B = images.shape[0]
    seds, morphs, cens, shifts = [], [], [], []
    for k, px in enumerate(centers):
        px = (int(px[0]), int(px[1]))
        sed, morph = pgm.init_extended_source(px, images.astype(dt), np.ones(B) * BG, symmetric=True, monotonic=bool(mono.any()))
        s = pgm.Source(sed, morph, px, dt, symmetric=bool(sym[k]), monotonic=bool(mono[k]),
                       centroid_weight=pgm.default_centroid_weight(),
                       l0_thresh=None if l0[k] < 0 else float(l0[k]), l1_thresh=None if l1[k] < 0 else float(l1[k]))
        pgm.source_update(s, 0)
        seds.append(s.sed); morphs.append(s.morph); cens.append(s.center)
        shifts.append((np.nan, np.nan) if s.shift is None else s.shift)
    return np.array(seds), np.array(morphs), np.array(cens), np.array(shifts, dtype=np.float64)


def seed_is_decided(spec, iters):
    """the seed criterion of the module docstring for one scene (spec: its state and switches)"""
    o32 = oracle_fit(spec, iters, np.float32, trace=True)["post"]
    o64 = oracle_fit(spec, iters, np.float64, trace=True)["post"]
    for a, b in zip(o32, o64):
        if ((a == 0) != (b == 0)).any() or not np.isfinite(a).all() or rel_err(a, b) > SEED_TOL:
            return False
    return len(o32) == iters


def _box_regions(b):
    """byte offsets of the convergence sums and of the box kernels' flags in the workspace (ws_layout in
    scarlet_hip.hip): behind the per-tile partials.  Valid for K <= 32 without a difference kernel; PSF batches and
    K > 32 lay their workspace out differently."""
    assert b.K <= 32 and getattr(b, "diff_kernel", None) is None, "workspace layout of K <= 32 without a difference kernel only"
    tiles = (b.H * b.W + 4095) // 4096
    partials = 1 + b.K * b.B + b.K * (b.K + 1) // 2
    conv = 8 * b.S * tiles * partials
    return conv, conv + 8 * b.S * b.K * 4


def box_fallback(b):
    """the per-component flags the box kernels leave in the workspace (1 = left to the full-frame kernel): the int region
    behind the per-tile partials and the convergence sums (ws_layout in scarlet_hip.hip; K <= 32)"""
    torch = b.torch
    _, at = _box_regions(b)
    torch.cuda.synchronize()
    return b.workspace[at:at + 4 * b.S * b.K].view(torch.int32).cpu().numpy().reshape(b.S, b.K)


def box_conv(b):
    """the convergence sums the last in-iteration update left, directly in front of those flags: (S, K, 4) float64 =
    {d2 sed, n2 sed, d2 morph, n2 morph}, d2 = |previous - new|^2, n2 = |new|^2"""
    torch = b.torch
    at, end = _box_regions(b)
    torch.cuda.synchronize()
    return b.workspace[at:end].view(torch.float64).cpu().numpy().reshape(b.S, b.K, 4)


def spec_of(images, sed0, morph0, cen0, sh0, sym, mono, l0, l1, **extra):
    d = dict(images=images, sed0=sed0, morph0=morph0, cen0=cen0, sh0=sh0, sym=sym, mono=mono, l0=l0, l1=l1)
    d.update(extra)
    return d
