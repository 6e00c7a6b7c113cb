"""-m gpu: ONE constraint update (scarlet_source_update_constrained) on frames beyond 64 px, driven directly on the
crafted planes of tests/box_update_cases.py, against pgm.source_update per component.  The planes put footprints either
side of the levels at which a component passes from the 63 x 63 box to the 127 x 127 box and from there to the
full-frame kernel (scarlet_amd/csrc/boxupdate.h; the derivation is in box_update_cases' docstring), in whole, clipped
and short boxes, at the smallest frame that selects each instance of k_source_update_box.

Per batch, three runs: default options, NO_BOX2 and NO_BOX.  Each against the float32 oracle -- morphology and SED to
parity_common.TOL = 1e-5 max-norm relative, support identical, centres bit-exact, shifts of symmetric components to
1e-6 absolute and NaN for the others, status 0 -- and against each other to 1e-6.  The flags the box kernels leave
(constraints_common.box_fallback) give the stage that served each component: under NO_BOX2 a flag says the small box
declined, under the default options that both did.  SAFETY: a component with Lp > 2 R was not served by the box of
half-size R.  PINNED: the stage is box_update_cases.expected_stage.  Every frame shows its instance and the _listed twin
both serving and declining a swept component.

Inside an iteration (in_iteration = 1; it = 0: no centroid, soft flip; it = 4: centroid, k-space) the crafted plane is
the stepped buffer 1 - cur and another case's constructor result the previous buffer `cur`; the four convergence sums
per component (constraints_common.box_conv) are compared with float64 sums over the device's own output and the
previous buffer to (H W / 256 + 8) 2^-23 relative -- each thread adds at most H W / 256 (+ the float4 tail) non-negative
float32 terms before the float64 reduction, every one rounded a few times -- and scarlet_check_convergence must set
and clear the flags for e_rel a factor 2 either side of a component's ratio.

Every max-norm error is printed (`box_update ...` lines; profiles/box_update_rel_err.txt is a run's collection)."""
import contextlib
import ctypes

import numpy as np
import pytest

from conftest import rel_err
import box_update_cases as bc
from constraints_common import box_conv, box_fallback
import parity_common as pc
from test_gpu_constraints import option

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
TOL = pc.TOL
FRAME_NAMES = [f[0] for f in bc.FRAMES]
SHIFT_TOL = 1e-6
CROSS_TOL = 1e-6


@pytest.fixture(scope="module")
def scarlet():
    import scarlet_amd
    scarlet_amd._lib.require_gpu()
    from oracle import build as obuild
    obuild.build()
    return scarlet_amd


def grid(scenes, fn, dtype):
    return np.array([[fn(c) for c in sc] for sc in scenes], dtype=dtype)


def previous_state(frame, scenes):
    """the previous buffer of the in-iteration phases: the float32 oracle's constructor results of the frame's first
    cases, one per component -- decided planes that differ from the crafted ones"""
    ctor = [c for sc in bc.frame_cases(frame)["ctor"] for c in sc]
    ref = [bc.oracle(c, "ctor") for c in ctor]
    K = len(scenes[0])
    idx = [[s * K + k for k in range(K)] for s in range(len(scenes))]
    return (np.array([[ref[i]["sed"] for i in row] for row in idx], np.float32),
            np.array([[ref[i]["morph"] for i in row] for row in idx], np.float32))


def run(scarlet, frame, phase, **opts):
    """the batch of (frame, phase), loaded and updated once under `opts` (and the frame's own option)"""
    _, H, W, _, frame_opt = bc.FRAME[frame]
    scenes = bc.frame_cases(frame)[phase]
    S, K = len(scenes), len(scenes[0])
    images = np.random.RandomState(1).rand(S, bc.B, H, W).astype(np.float32)          # (the update does not read them)
    starts = grid(scenes, lambda c: c["start"], np.int32)
    if frame_opt:
        opts = dict(opts, **{frame_opt: 1})
    with contextlib.ExitStack() as stack:
        for name, value in opts.items():
            stack.enter_context(option(scarlet, name, value))
        b = scarlet.BlendBatch(images, starts, symmetric=grid(scenes, lambda c: c["sym"], np.uint8),
                               monotonic=grid(scenes, lambda c: c["mono"], np.uint8),
                               l0_thresh=grid(scenes, lambda c: c["l0"], np.float32),
                               l1_thresh=grid(scenes, lambda c: c["l1"], np.float32))
        assert b.constrained and b.monotonic
        sed, morph = grid(scenes, bc.sed, np.float32), grid(scenes, bc.plane, np.float32)
        nan = np.full((S, K, 2), np.nan)
        out = {}
        if phase == "ctor":
            b.set_state(sed, morph, centers=starts, shifts=nan)
            b.update_sources()
            w = 0
        else:
            psed, pmorph = previous_state(frame, scenes)
            b.set_state(psed, pmorph, centers=starts, shifts=nan)                      # both buffers; cur = 0
            b.sed[1].copy_(torch.as_tensor(sed)); b.morph[1].copy_(torch.as_tensor(morph))
            b.lipschitz[:, 1] = bc.LIP
            b.it.fill_(bc.PHASES[phase] - 1)
            b._lib_update(None, 1)
            w = 1
            out.update(prev_sed=psed, prev_morph=pmorph, conv=box_conv(b))
            assert np.array_equal(b.morph[0].cpu().numpy(), pmorph) and np.array_equal(b.sed[0].cpu().numpy(), psed)
        torch.cuda.synchronize()
        out.update(sed=b.sed[w].cpu().numpy(), morph=b.morph[w].cpu().numpy(), cen=b.centers.cpu().numpy(),
                   shifts=b.shifts.cpu().numpy(), status=b.status.cpu().numpy(), fallback=box_fallback(b).copy(), batch=b)
    return out


def against_oracle(frame, phase, label, res, stages):
    """every component of one run against pgm.source_update; prints the largest errors per serving stage"""
    scenes = bc.frame_cases(frame)[phase]
    assert int(np.abs(res["status"]).sum()) == 0, res["status"]
    worst = {}
    for s, sc in enumerate(scenes):
        for k, case in enumerate(sc):
            ref = bc.oracle(case, phase)
            what = "%s %s %s" % (case["id"], phase, label)
            em, es = rel_err(res["morph"][s, k], ref["morph"]), rel_err(res["sed"][s, k], ref["sed"])
            w = worst.setdefault(stages[s][k], [0.0, 0.0, 0.0, 0])
            w[0], w[1], w[3] = max(w[0], em), max(w[1], es), w[3] + 1
            assert np.array_equal(res["morph"][s, k] == 0, ref["morph"] == 0), "%s: support differs" % what
            assert em <= TOL and es <= TOL, "%s beyond 1e-5: morph %.3e sed %.3e" % (what, em, es)
            assert tuple(res["cen"][s, k]) == ref["center"], "%s: centre %s, oracle %s" % (what, res["cen"][s, k], ref["center"])
            if case["sym"] and phase != "it0":
                d = float(np.abs(res["shifts"][s, k] - np.array(ref["shift"])).max())
                w[2] = max(w[2], d)
                assert d <= SHIFT_TOL, "%s: shift %s, oracle %s" % (what, res["shifts"][s, k], ref["shift"])
            else:
                assert np.isnan(ref["shift"]).all() and np.isnan(res["shifts"][s, k]).all(), "%s: a shift was written" % what
    for st in sorted(worst):
        m, e, d, n = worst[st]
        print("box_update %-16s %-5s %-8s %-10s n=%2d  morph %.3e  sed %.3e  shift %.1e" % (frame, phase, label, bc.STAGE_NAMES[st], n, m, e, d))


def three_ways(scarlet, frame, phase):
    """default options, NO_BOX2, NO_BOX: each against the oracle and against each other, the stages read from the flags"""
    _, H, W, inst, _ = bc.FRAME[frame]
    scenes = bc.frame_cases(frame)[phase]
    dflt, nb2, nobox = run(scarlet, frame, phase), run(scarlet, frame, phase, NO_BOX2=1), run(scarlet, frame, phase, NO_BOX=1)
    d, n = dflt["fallback"], nb2["fallback"]
    assert set(np.unique(d)) <= {0, 1} and set(np.unique(n)) <= {0, 1}
    assert not (d & ~n).any(), "a component the small box served alone was flagged with both boxes:\n%s\n%s" % (d, n)
    got = np.where(n == 0, bc.SMALL, np.where(d == 0, bc.LARGE, bc.FULL))
    against_oracle(frame, phase, "default", dflt, got)
    against_oracle(frame, phase, "NO_BOX2", nb2, np.where(n == 0, bc.SMALL, bc.FULL))
    against_oracle(frame, phase, "NO_BOX", nobox, np.full(n.shape, bc.FULL))
    for a, b, name in ((dflt, nb2, "default / NO_BOX2"), (dflt, nobox, "default / NO_BOX")):
        for key in ("sed", "morph"):
            e = rel_err(a[key], b[key])
            print("box_update %-16s %-5s %s: %s %.3e" % (frame, phase, name, key, e))
            assert e <= CROSS_TOL, (name, key, e)
        assert np.array_equal(a["cen"], b["cen"]) and np.array_equal(np.isnan(a["shifts"]), np.isnan(b["shifts"])), name
        assert np.abs(np.nan_to_num(a["shifts"]) - np.nan_to_num(b["shifts"])).max() <= CROSS_TOL, name
    seen = set()
    for s, sc in enumerate(scenes):
        for k, case in enumerate(sc):
            Lp, _ = bc.sweep_lp(case, phase, np.float32)
            want = bc.expected_stage(case, phase, np.float32)
            what = "%s %s (Lp0 %d, Lp %d, %s, peak %s)" % (case["id"], phase, case["Lp0"], Lp, case["mask"], case["peak"])
            print("box_update %-16s stage of %s: %s" % (frame, what, bc.STAGE_NAMES[got[s, k]]))
            if not case["mono"]:
                assert n[s, k] == 1 and d[s, k] == 1, "%s has no sweep and was not flagged" % what
                continue
            # safety: a box of half-size R is complete for the levels <= 2 R only
            assert not (Lp > 2 * bc.R_SMALL and n[s, k] == 0), "%s was served by the 63 x 63 box" % what
            assert not (Lp > 2 * bc.R_LARGE and d[s, k] == 0), "%s was served by the 127 x 127 box" % what
            assert got[s, k] == want, "%s: served by the %s, expected the %s" % (what, bc.STAGE_NAMES[got[s, k]], bc.STAGE_NAMES[want])
            if bc.is_sweep(case, phase):
                seen.add(("small", bool(n[s, k])))
                if n[s, k]:
                    seen.add(("listed", bool(d[s, k])))
    return dflt, seen


@pytest.mark.parametrize("frame", FRAME_NAMES)
def test_constructor_update(scarlet, frame):
    """in_iteration = 0 on 18 components per frame; k_source_update_box<instance> and its _listed twin each serve and
    decline a swept component, read from the flags under NO_BOX2 and the default options"""
    _, seen = three_ways(scarlet, frame, "ctor")
    assert seen == {("small", False), ("small", True), ("listed", False), ("listed", True)}, (bc.FRAME[frame][3], seen)


@pytest.mark.parametrize("it", [0, 4])
@pytest.mark.parametrize("frame", FRAME_NAMES)
def test_update_inside_an_iteration(scarlet, frame, it):
    _, H, W, _, _ = bc.FRAME[frame]
    phase = "it%d" % it
    res, _ = three_ways(scarlet, frame, phase)
    # ---- the convergence sums against float64 sums over the device's own output and the previous buffer
    f8 = lambda a: a.astype(np.float64)
    want = np.stack([((f8(res["prev_sed"]) - f8(res["sed"])) ** 2).sum(-1), (f8(res["sed"]) ** 2).sum(-1),
                     ((f8(res["prev_morph"]) - f8(res["morph"])) ** 2).sum((-2, -1)), (f8(res["morph"]) ** 2).sum((-2, -1))], axis=-1)
    bound = (H * W / 256.0 + 8) * 2.0 ** -23
    err = np.abs(res["conv"] - want) / want
    print("box_update %-16s %-5s convergence sums: largest relative error %.3e (bound %.3e)" % (frame, phase, err.max(), bound))
    assert (want > 0).all() and (err <= bound).all(), (err, bound)
    if it == 0:
        return                                           # (iteration 1 runs no convergence test)
    # ---- scarlet_check_convergence: e_rel a factor 2 either side of the ratio of two components
    b, L = res["batch"], scarlet._lib
    S, K = want.shape[:2]
    ratio = np.sqrt(np.stack([want[..., 0] / want[..., 1], want[..., 2] / want[..., 3]], axis=-1))      # (S, K, {sed, morph})
    bits = np.array([L.FLAG_SED_NOT_CONVERGED, L.FLAG_MORPH_NOT_CONVERGED])
    for (s, k, j) in ((0, 0, 1), (S - 1, K - 1, 0)):
        for factor in (2.0, 0.5):
            e_rel = factor * ratio[s, k, j]
            # no component sits on the threshold to within what the sums are good for (d2 <= e_rel^2 n2, each to `bound`)
            assert (np.abs((ratio / e_rel) ** 2 - 1) > 2 * bound).all(), (ratio, e_rel)
            not_conv = ((ratio > e_rel) * bits).sum(-1)
            b.flags.copy_(torch.as_tensor((3 - not_conv).astype(np.int32)))     # every flag has to flip
            b.it.fill_(it); b.cur.zero_(); b.active.fill_(1)
            L.check(L.lib.scarlet_check_convergence(ctypes.byref(b._c), float(e_rel), L.stream_ptr()))
            torch.cuda.synchronize()
            flags = b.flags.cpu().numpy()
            assert np.array_equal(flags, not_conv), (e_rel, flags, not_conv)
            assert bool(flags[s, k] & bits[j]) == (factor < 1)
            assert (b.it.cpu().numpy() == it + 1).all() and (b.cur.cpu().numpy() == 1).all()
            assert np.array_equal(b.active.cpu().numpy(), (not_conv != 0).any(-1).astype(np.int32))
