"""Cases of tests/test_gpu_box_update.py and tests/test_box_update_cases.py: stepped morphologies for ONE constraint
update on frames beyond 64 px (scarlet_amd/csrc/boxupdate.h), whose outcome in the CPU oracle -- and with it the stage
that has to serve each component -- is known before any device run.  numpy and oracle.pgm only.

The plane.  level(y, x) = 2 max(|y - cy|, |x - cx|) + min(|y - cy|, |x - cx|) (prox_ops.h sweep_level).  A crafted
plane is exp(-r / 40) + 0.02 * uniform noise where level <= Lp0 inside a footprint mask, and -1 everywhere else.  The
peak holds 1 + noise, every other pixel at most exp(-1 / 40) + 0.02 < 1, so max_pixel finds the peak from any start
centre within two pixels.  Behind the footprint the sweep's caps are averages that contain the -1 floor: it dies at
once, and the last level Lp on which the oracle's output is positive is a property of the plane and not of rounding.
Masks: the full disc, the four 90-degree wedges about the axes (the x-major and y-major walkers of wave_monotonic and
their two halves), two opposite quadrants, one octant; each sector united with the 5 x 5 core around the peak.  The
sectors matter because the sweep's "three quiet levels" count is an OR over lanes that serve different wedges.
Half of the swept cases without symmetry have a RIM: 0.5 + noise instead of -1 on every level beyond Lp0 + 3.  A pixel's strictly closer
neighbours lie one to three levels below its own, so behind a moat of three levels of -1 the reference caps the whole
rim at negative averages and zeroes it: Lp does not move.  The kernels, which stop at level Lp + 3, never sweep the rim;
only the cut of their write-back (`axmax`, `rowstep`, the scalar form) keeps it out of the result, and a cut that is one
level generous shows as a positive pixel where the reference has none.  With -1 everywhere outside no cut is visible.
Symmetric cases keep the plain plane: the cut comes after the symmetry and is the same code with and without it, and a
rim fills the k-space symmetry's window, up to 1013 columns wide at 72 x 1024, with values of 0.5 whose float32 sums the
box and the full-frame kernel take in different orders -- with a rim on 72x1024/31 (iteration 5) the two differed by
1.013e-6 in the morphology (7.2e-7 without; each within 1.5e-6 of the oracle), past the 1e-6 the runs are held to.

Which stage serves a component (boxupdate.h ub_component, wave_ops.h wave_monotonic, prox_ops.h monotonic_tile).
Let Lp be the last level with a positive value after the sweep.  Both sweeps count `quiet`, the consecutive levels
without a positive value, and stop INSIDE the third one: wave_monotonic leaves its loop with `done = ell` before
`++ell`, monotonic_tile returns `ell` when `ell - lastpos >= 3`.  So a sweep that stops reports Lp + 3, and it stops
only if it gets to run level Lp + 3.
  * 63 x 63 box (R = 31): wave_monotonic(level_cap = 2 R = 62) runs the levels 1 .. min(Lall, 62), Lall being the
    largest level of the CLIPPED box: 2 max(my, mx) + min(my, mx) with my = max(min(cy, R), min(H - 1 - cy, R)), mx
    alike.  It serves the component iff Lp + 3 <= min(Lall, 62); otherwise done stays 1 << 30 and the component is
    flagged and listed.  In a frame with both sides >= 63 Lall >= 62: the small box serves Lp <= 59.
  * 127 x 127 box (R = 63): wave_monotonic without a cap sweeps the compact levels 1 .. min(Lall, 46); if that did
    not stop, monotonic_tile continues from level 47 up to Lall and returns Lp + 3 or, past the last level, 1 << 30;
    `if (lstop > 2 R) lstop = 1 << 30` then refuses what the box does not hold.  Served iff Lp + 3 <= min(Lall, 126):
    60 <= Lp <= 123 in a frame that holds the whole box, fewer where the frame is short (66 x 24, peak (30, 17):
    Lall = 2 * 35 + 17 = 87, so Lp = 84 is the last one served).
  * everything else is flagged and taken by the full-frame kernel; so are a component without `monotonic` (no sweep
    bounds its footprint) and a symmetric component without a shift whose centre is (H / 2, W / 2): the soft flip
    then runs about the array middle and leaves the box (`mode == 2 && sw.centered`).  Neither is listed for the
    second box.
A box of half-size R holds every pixel of the levels <= 2 R and none of level > 3 R; SAFETY is the weaker statement
that a component with Lp > 2 R is never served by that box (its output would be truncated), PINNED the table above.
With l0_thresh / l1_thresh the stage follows the sweep, which runs before the cut: Lp is then taken from the oracle
with the thresholds off.

`decided(case, phase)` is constraints_common.seed_is_decided for one update: the float32 and the float64 oracle give
the same support and the same centre, finite values, and differ by at most 1e-6 max-norm relative.  No case is
exempt; a case that is not decided gets another seed in RESEED (tests/test_box_update_cases.py checks all of them on
the CPU).

Phases.  "ctor": the constructors' update (it = 0: centroid, k-space symmetry), L = 1.  "it0" / "it4": the update inside
iteration it + 1 with the step 1 / LIP: it0 has no centroid yet, so a symmetric component takes the soft flip; it4
(iteration 5) measures the centroid and takes the k-space symmetry.
"""
import functools

import numpy as np

from conftest import rel_err
import constraints_common as cc

NOISE, SCALE, FLOOR = 0.02, 40.0, -1.0
RIM, MOAT = 0.5, 3              # cases with a rim: 0.5 + noise on every level beyond Lp0 + 3
LIP = 2.5                       # lipschitz[:, 1] of the in-iteration phases: the cuts are thresh / LIP
L0, L1 = 0.1, 0.06              # cuts 0.1 / 0.06 (ctor) and 0.04 / 0.024: above the noise, below exp(-65 / 40) = 0.197
B = 2
SMALL, LARGE, FULL = 0, 1, 2
STAGE_NAMES = ("63-box", "127-box", "full frame")
R_SMALL, R_LARGE = 31, 63
PHASES = {"ctor": 0, "it0": 1, "it4": 5}          # the iteration number the oracle's source_update sees

# name, H, W, instance of k_source_update_box, option the batch runs under
FRAMES = (
    ("72x80", 72, 80, "<8,0>", None),              # W / 4 = 20: float4 write-back without rowstep
    ("128x128", 128, 128, "<8,128>", None),        # rowstep
    ("128x128_generic", 128, 128, "<8,0>", "NO_EXACT"),
    ("144x200", 144, 200, "<16,0>", None),
    ("256x256", 256, 256, "<16,256>", None),
    ("130x258", 130, 258, "<0,0>", None),          # W % 4 != 0: scalar write-back, streamed
    ("264x136", 264, 136, "<0,0>", None),          # H over 256
    ("72x1024", 72, 1024, "<0,0>", None),          # W / 4 = 256: rowstep with one row per step
    ("100x90", 100, 90, "<8,0>", None),            # scalar write-back
    ("66x24", 66, 24, "<8,0>", None),              # a short side: the boxes' own Lall ends the sweeps
    ("73x81", 73, 81, "<8,0>", None),              # odd sides: (36, 40) is the exact middle
)
FRAME = {f[0]: f for f in FRAMES}

MASKS = {
    "disc": lambda dy, dx: np.ones(dy.shape, bool),
    "right": lambda dy, dx: dx >= np.abs(dy),
    "up": lambda dy, dx: -dy >= np.abs(dx),
    "left": lambda dy, dx: -dx >= np.abs(dy),
    "down": lambda dy, dx: dy >= np.abs(dx),
    "quadrants": lambda dy, dx: dy * dx >= 0,
    "octant": lambda dy, dx: (dy >= 0) & (dx >= dy),
}
MASK_ORDER = ("disc", "right", "up", "left", "down", "quadrants", "octant")
CRITICAL = (59, 60, 62, 63, 123, 124, 126, 127)   # either side of: small box serves / holds, large box serves / holds
OTHERS = (56, 58, 61, 66, 120, 122, 125, 130)

# a case that `decided` refuses gets another seed here: {case id: seed}
RESEED = {}


def level_map(H, W, cy, cx):
    y, x = np.mgrid[:H, :W]
    ay, ax = np.abs(y - cy), np.abs(x - cx)
    return 2 * np.maximum(ay, ax) + np.minimum(ay, ax)


def peaks(H, W):
    """every peak at least 3 px from the low edges and 5 from the high ones (max_pixel's window stays in the frame)"""
    p = dict(inner=(H // 2 - 3, W // 2 + 5), mid=(H // 2, W // 2), edge=(12, W // 2 + 2), side=(H // 2 + 1, 9),
             c00=(5, 7), c11=(H - 6, W - 8))
    if W > 512:
        p["far"] = (40, 700)
    return p


PEAK_ORDER = ("inner", "c00", "edge", "c11", "side")


def footprint(H, W, peak, mask, Lp0):
    y, x = np.mgrid[:H, :W]
    dy, dx = y - peak[0], x - peak[1]
    core = (np.abs(dy) <= 2) & (np.abs(dx) <= 2)
    return (level_map(H, W, *peak) <= Lp0) & (MASKS[mask](dy, dx) | core)


def holds(H, W, peak, mask, Lp0):
    """the footprint has a pixel on level Lp0 inside the frame; a sector at least three (a lone pixel at a sector's rim
    is capped below zero by the floor beside it)"""
    return int((footprint(H, W, peak, mask, Lp0) & (level_map(H, W, *peak) == Lp0)).sum()) >= (1 if mask == "disc" else 3)


def _case(frame, n, Lp0, peak, mask, off=(0, 0), sym=0, mono=1, l0=-1.0, l1=-1.0):
    cid, fi = "%s/%02d" % (frame, n), [f[0] for f in FRAMES].index(frame)
    # rim: half of the swept cases without symmetry, moving with the frame, so that each level has it at some frames and
    # not at others (the cut it probes comes after the symmetry and does not depend on it; see the docstring)
    return dict(id=cid, frame=frame, Lp0=Lp0, peak=peak, start=(peak[0] + off[0], peak[1] + off[1]), mask=mask,
                sym=sym, mono=mono, l0=l0, l1=l1, rim=int(bool(mono) and not sym and (n + fi) % 4 in (0, 1)),
                seed=RESEED.get(cid, 7000 + 100 * fi + n))


def _place(H, W, Lp0, fi, i, want_peak=None, want_mask=None):
    """the first (peak, mask) pair, in an order rotated by the frame and the case number, that holds level Lp0"""
    pk = peaks(H, W)
    names = [want_peak] if want_peak else [PEAK_ORDER[(i + fi + j) % len(PEAK_ORDER)] for j in range(len(PEAK_ORDER))]
    masks = [want_mask] if want_mask else [MASK_ORDER[(i + 2 * fi + j) % len(MASK_ORDER)] for j in range(len(MASK_ORDER))]
    for m in masks:
        for p in names:
            if holds(H, W, pk[p], m, Lp0):
                return pk[p], m
    if want_peak or want_mask:
        return _place(H, W, Lp0, fi, i)
    raise ValueError("no peak of the %d x %d frame holds level %d" % (H, W, Lp0))


OFFSETS = ((0, 0), (1, -2), (-1, 1), (0, 2), (2, 0), (-2, -1))


@functools.lru_cache(maxsize=None)
def frame_cases(frame):
    """{phase: [scene][component] cases} of one frame.  ctor: 18 components in scenes of three -- the eight CRITICAL
    levels without symmetry, the eight OTHERS (four of them symmetric, with a start centre off the peak), one symmetric
    component at the frame's middle and one without `monotonic`; thresholds on four of them.  it0, it4: six components
    in scenes of two."""
    _, H, W, _, _ = FRAME[frame]
    fi = [f[0] for f in FRAMES].index(frame)
    pk = peaks(H, W)
    short = frame == "66x24"
    others = (56, 66, 83, 84, 85, 61, 87, 120) if short else tuple(OTHERS[(fi + j) % 8] for j in range(8))
    ctor = []
    for i, Lp0 in enumerate(CRITICAL):
        peak, mask = _place(H, W, Lp0, fi, i)
        ctor.append(_case(frame, len(ctor), Lp0, peak, mask, off=OFFSETS[(i + fi) % 6] if i % 3 == 2 else (0, 0),
                          l0=L0 if i == (fi % 8) else -1.0, l1=L1 if i == ((fi + 3) % 8) else -1.0))
    for j, Lp0 in enumerate(others):
        sym = 1 if j in (0, 2, 4, 6) and not short else 0
        if short:                                   # the boxes' own Lall: the interior peak, whose 127-box ends at level 87
            peak, mask = _place(H, W, Lp0, fi, j, want_peak="inner", want_mask=("disc", "quadrants", "down", "disc", "disc", "disc", "disc", "disc")[j])
        elif sym:                                   # k-space symmetry: a small window (c00), a clipped box (c11), an interior peak
            p, m = ("c00", None, "c11", None, "inner", None, "edge")[j], ("disc", None, "quadrants", None, "disc", None, "quadrants")[j]
            peak, mask = _place(H, W, Lp0, fi, j, want_peak=p, want_mask=m if holds(H, W, pk[p], m, Lp0) else None)
        else:
            peak, mask = _place(H, W, Lp0, fi, j + 3)
        ctor.append(_case(frame, len(ctor), Lp0, peak, mask, off=OFFSETS[1 + (j + fi) % 5] if sym else (0, 0), sym=sym,
                          l0=L0 if j in (1, 6) else -1.0, l1=L1 if j == 3 else -1.0))
    if short:                                       # ... and one symmetric component in the short frame too
        ctor[8]["sym"], ctor[8]["rim"], ctor[8]["start"] = 1, 0, (ctor[8]["peak"][0] + 1, ctor[8]["peak"][1] - 1)
    ctor.append(_case(frame, len(ctor), 58, pk["mid"], "disc", sym=1))                # centred: the k-space call is a no-op
    ctor.append(_case(frame, len(ctor), 56, pk["side"], "disc", mono=0))              # no sweep: always flagged
    lo, hi = (59, 60), ((83, 84, 85, 62) if short else (123, 124, 126, 62))
    it0 = [
        _case(frame, 20, 58, pk["c00"], "quadrants", off=(1, -1), sym=1),             # soft flip in a window smaller than the box
        _case(frame, 21, 56, pk["mid"], "disc", sym=1),                               # soft flip about the array middle: flagged
        _case(frame, 22, hi[0], *_place(H, W, hi[0], fi, 1), l1=L1),
        _case(frame, 23, 56, pk["inner"], "right", sym=1, mono=0),
        _case(frame, 24, hi[3], *_place(H, W, hi[3], fi, 2, want_peak="side" if not short else None), off=(0, 2)),
        _case(frame, 25, hi[1], *_place(H, W, hi[1], fi, 0, want_mask="disc"), sym=1),
    ]
    it4 = [
        _case(frame, 30, lo[0], pk["inner"], "disc", off=(1, -2), sym=1),
        _case(frame, 31, OTHERS[5] if not short else 80, *_place(H, W, OTHERS[5] if not short else 80, fi, 3, want_mask="quadrants"), off=(-1, 1), sym=1),
        _case(frame, 32, lo[1], *_place(H, W, lo[1], fi, 4), l0=L0),
        _case(frame, 33, hi[2], *_place(H, W, hi[2], fi, 5)),
        _case(frame, 34, 56, pk["edge"], "disc", sym=1, mono=0),
        _case(frame, 35, 61, pk["mid"], "disc", sym=1),                               # centred with a shift: mode 0
    ]
    group = lambda cs, k: [cs[i:i + k] for i in range(0, len(cs), k)]
    return {"ctor": group(ctor, 3), "it0": group(it0, 2), "it4": group(it4, 2)}


def all_cases():
    """(case, phase) of every frame"""
    return [(c, ph) for f in FRAMES for ph, scenes in frame_cases(f[0]).items() for sc in scenes for c in sc]


def plane(case):
    _, H, W, _, _ = FRAME[case["frame"]]
    rng = np.random.RandomState(case["seed"])
    y, x = np.mgrid[:H, :W]
    r = np.hypot(y - case["peak"][0], x - case["peak"][1])
    noise = NOISE * rng.rand(H, W)
    outside = np.where(case["rim"] & (level_map(H, W, *case["peak"]) > case["Lp0"] + MOAT), RIM + noise, FLOOR)
    return np.where(footprint(H, W, case["peak"], case["mask"], case["Lp0"]), np.exp(-r / SCALE) + noise, outside).astype(np.float32)


def sed(case):
    """(B,) float32 in 0.5 .. 1.5; every third case has a negative entry (positivity of the SED)"""
    s = (0.5 + np.random.RandomState(case["seed"] + 1).rand(B)).astype(np.float32)
    if case["seed"] % 3 == 0:
        s[1] = -0.25
    return s


@functools.lru_cache(maxsize=None)
def _oracle(cid, phase, dtname, thresholds):
    from oracle import pgm
    case = CASE[cid]
    dt = np.dtype(dtname).type
    on = lambda v: None if (v < 0 or not thresholds) else float(v)
    s = pgm.Source(sed(case), plane(case), case["start"], dt, symmetric=bool(case["sym"]), monotonic=bool(case["mono"]),
                   centroid_weight=pgm.default_centroid_weight(), l0_thresh=on(case["l0"]), l1_thresh=on(case["l1"]))
    if phase != "ctor":
        s.L_morph = LIP
    pgm.source_update(s, PHASES[phase])
    _, H, W, _, _ = FRAME[case["frame"]]
    pos = s.morph > 0
    Lp = int(level_map(H, W, *s.center)[pos].max()) if pos.any() else -1
    shift = (np.nan, np.nan) if s.shift is None else tuple(float(v) for v in s.shift)
    for a in (s.morph, s.sed):
        a.setflags(write=False)
    return dict(morph=s.morph, sed=s.sed, center=tuple(int(v) for v in s.center), shift=shift, Lp=Lp)


def oracle(case, phase, dt=np.float32, thresholds=True):
    """pgm.source_update of the case's plane: morph, sed (read-only, shared), center, shift (NaN = none), Lp"""
    has = case["l0"] >= 0 or case["l1"] >= 0
    return _oracle(case["id"], phase, np.dtype(dt).name, bool(thresholds) or not has)


def decided(case, phase):
    a, b = oracle(case, phase, np.float32), oracle(case, phase, np.float64)
    return bool(np.array_equal(a["morph"] == 0, b["morph"] == 0) and np.isfinite(a["morph"]).all() and
                np.isfinite(a["sed"]).all() and rel_err(a["morph"], b["morph"]) <= cc.SEED_TOL and
                a["center"] == b["center"])


def box_lall(H, W, center, R):
    """the largest sweep level of the box of half-size R around `center`, clipped to the frame"""
    my = max(min(center[0], R), min(H - 1 - center[0], R))
    mx = max(min(center[1], R), min(W - 1 - center[1], R))
    return 2 * max(my, mx) + min(my, mx)


def sweep_lp(case, phase, dt=np.float64):
    """the last positive level behind the sweep (the thresholds cut after it), and the centre it is counted from"""
    o = oracle(case, phase, dt, thresholds=False)
    return o["Lp"], o["center"]


def expected_stage(case, phase, dt=np.float64):
    _, H, W, _, _ = FRAME[case["frame"]]
    Lp, cen = sweep_lp(case, phase, dt)
    if not case["mono"]:
        return FULL
    if phase == "it0" and case["sym"] and cen == (H // 2, W // 2):       # no shift yet: soft flip about the array middle
        return FULL
    if Lp + 3 <= min(box_lall(H, W, cen, R_SMALL), 2 * R_SMALL):
        return SMALL
    if Lp + 3 <= min(box_lall(H, W, cen, R_LARGE), 2 * R_LARGE):
        return LARGE
    return FULL


def is_sweep(case, phase):
    """the stage was decided by a sweep (not by a missing `monotonic` or the centred soft flip)"""
    _, H, W, _, _ = FRAME[case["frame"]]
    return bool(case["mono"]) and not (phase == "it0" and case["sym"] and oracle(case, phase)["center"] == (H // 2, W // 2))


CASE = {c["id"]: c for c, _ in all_cases()}
