"""CPU: the ragged-frame cases of tests/fused_frame_cases.py are admissible -- the oracle starts and fits every scene on
its own frame with finite results -- the case table holds what its docstring promises, and the library's plan
(scarlet_debug_fused_plan, host-only) routes each case to the four-wave kernel's ragged-frames instance and every batch
outside that kernel's conditions to the general path."""
import ctypes
import multiprocessing as mp
import os

import numpy as np
import pytest

import fused_frame_cases as ffc

FAKE = 0x1000          # a non-NULL pointer that is never dereferenced: the plan reads the structs' own fields only
LDS_LIMIT = 160 * 1024 - 1024


@pytest.fixture(scope="module")
def pool():
    from oracle import build as obuild
    obuild.build()
    p = mp.get_context("spawn").Pool(min(16, os.cpu_count() or 1))
    yield p
    p.close(); p.join()


def ffc_pgm():
    from oracle import pgm
    return pgm


def _check_admissible(out, shape, n, iters, what):
    sed, morph, mse, cen = out
    h, w = shape
    assert morph.shape == (n, h, w) and len(mse) == iters, what
    assert np.isfinite(sed).all() and np.isfinite(morph).all() and np.isfinite(mse).all(), what
    assert (morph.max(axis=(1, 2)) > 0).all(), what
    assert ((cen >= 0) & (cen < np.array([h, w]))).all(), what


@pytest.mark.parametrize("name", list(ffc.CASES))
def test_every_scene_is_admissible_on_its_own_frame(pool, name):
    """no SourceInitError, no refused max_pixel window (either would raise in the worker), finite results"""
    c = ffc.CASES[name]
    out = pool.map(ffc.oracle_own_frame, [(name, s, c.iters) for s in range(len(c.shapes))])
    for s, o in enumerate(out):
        _check_admissible(o, c.shapes[s], c.counts[s], c.iters, (name, s))


def test_thin_and_tiny_frames(pool):
    """frames down to 3 x 3 start and fit in the oracle; a frame with h < 3 or w < 3 admits no centre at all: the
    reference has no result there"""
    jobs = [(shape, peaks, 1400 + i, 6) for i, (shape, peaks) in enumerate(ffc.THIN_FRAMES)]
    for (shape, peaks, _, iters), o in zip(jobs, pool.map(ffc.oracle_hand_frame, jobs)):
        _check_admissible(o, shape, len(peaks), iters, shape)
    # every centre of such a frame lies on a row or column < 2, where max_pixel's window starts at a negative index:
    # the oracle raises, or the centre it returns has left the frame
    for shape, centre in ffc.NO_REFERENCE_FRAMES + (((2, 3), (1, 1)), ((3, 2), (1, 1)), ((5, 2), (2, 1))):
        try:
            cen = ffc.oracle_hand_frame((shape, (centre,), 1500, 1))[3]
        except (ValueError, IndexError, ffc_pgm().SourceInitError):
            continue
        assert not ((cen >= 0) & (cen < np.array(shape))).all(), (shape, cen)


def test_the_case_table_holds_what_it_promises():
    assert list(ffc.CASES) == ["k4_64", "b6_k3", "b8_k4", "switches", "weights"]
    for c in ffc.CASES.values():
        assert c.shapes[0] == (c.H, c.W) and max(c.counts) == c.K and len(c.counts) == len(c.shapes), c.name
        assert all(3 <= h <= c.H and 3 <= w <= c.W for h, w in c.shapes), c.name
        assert c.H <= 64 and c.W <= 64 and c.W % 4 == 0 and c.K <= 4 and c.B <= 8, c.name
        assert any(w % 4 for _, w in c.shapes) and any(h < c.H for h, _ in c.shapes), c.name
        assert c.iters == (10 if c.name == "k4_64" else 6)
        for (h, w), n, (im, cen) in zip(c.shapes, c.counts, ffc.scenes(c)):
            assert im.shape == (c.B, h, w) and cen.shape == (n, 2)
            assert (cen >= 2).all() and (cen < np.array([h, w])).all(), (c.name, h, w)       # max_pixel's window
    k4 = ffc.CASES["k4_64"]
    assert {w % 4 for _, w in k4.shapes} == {0, 1, 2, 3}
    h, w = k4.shapes[0]
    assert h * ((w + 3) // 4) == 1024                                   # every group of the kernel's walk
    assert (3, 3) in k4.shapes and (3, 64) in k4.shapes and (64, 3) in k4.shapes and (5, 5) in k4.shapes
    cen = [ffc.scenes(k4)[i][1].tolist() for i in range(len(k4.shapes))]
    assert [2, 2] in cen[0] and [63, 63] in cen[0] and len(cen[0]) == 4
    assert [c[0] for c in cen[5]] == [2, 2] and cen[9] == [[30, 25], [2, 2]]
    assert ffc.CASES["b6_k3"].B == 6 and ffc.CASES["b6_k3"].K == 3 and ffc.CASES["b8_k4"].B == 8
    assert ffc.CASES["switches"].shapes == ffc.CASES["b6_k3"].shapes and ffc.CASES["weights"].shapes == ffc.CASES["b8_k4"].shapes
    # switches: a component without `monotonic` in a scene with w % 4 != 0 (the whole-plane maximum over partial
    # groups), and one with an L1 cut
    c = ffc.CASES["switches"]
    sym, mono, l0, l1 = ffc.switches(c)
    assert any(w % 4 and not mono[s, :n].all() for s, ((_, w), n) in enumerate(zip(c.shapes, c.counts)))
    assert any((l1[s, :n] >= 0).any() for s, n in enumerate(c.counts)) and any((l0[s, :n] >= 0).any() for s, n in enumerate(c.counts))
    assert any(not sym[s, :n].all() for s, n in enumerate(c.counts))
    wg = ffc.weights(ffc.CASES["weights"])
    assert all(x.shape == (8, h, w) and x.min() >= 0.5 and x.max() <= 1.5 for x, (h, w) in zip(wg, ffc.CASES["weights"].shapes))


def _batch(c, S=None, **over):
    from scarlet_amd import _lib
    b = _lib.ScarletBatch()
    b.S, b.K, b.B, b.H, b.W = S or len(c.shapes), c.K, c.B, c.H, c.W
    for f in ("images", "weights", "cur", "centers", "shifts", "flags", "lipschitz", "mse", "it", "active", "status", "workspace",
              "centroid_psf", "n_components"):
        setattr(b, f, FAKE)
    for i in range(2):
        b.sed[i] = FAKE
        b.morph[i] = FAKE
    b.mse_capacity, b.weight_scalar, b.symmetric, b.monotonic, b.l0_thresh, b.l1_thresh, b.centroid_P = 16, 1.0, 1, 1, -1.0, -1.0, 11
    for k, v in over.items():
        setattr(b, k, v)
    return b


def _plan(b, frames=True, cons=False, approximate_L=0, n_iter=10):
    from scarlet_amd import _lib
    f = _lib.ScarletFrames()
    f.frame_hw = FAKE if frames else None
    cs = _lib.ScarletConstraints()
    if cons:
        cs.symmetric = cs.monotonic = cs.l0_thresh = cs.l1_thresh = FAKE
    out = np.full(8, -7, np.int32)
    rc = _lib.lib.scarlet_debug_fused_plan(ctypes.byref(b), ctypes.byref(f), ctypes.byref(cs), approximate_L, n_iter,
                                           out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    return out.tolist()


@pytest.mark.parametrize("name", list(ffc.CASES))
def test_the_plan_routes_each_case_to_the_frames_instance(name):
    """(fails where the library has no scarlet_debug_fused_plan: ragged frames had no one-launch kernel then)"""
    c = ffc.CASES[name]
    lds = ffc.fused_lds_bytes(c.K, c.H, c.W)
    for cons in (False, True):
        assert _plan(_batch(c), cons=cons or c.switches) == [c.kernel, 256, lds, 1, LDS_LIMIT, 1, 0, 0], (name, cons)
    assert c.kernel == (ffc.FUSED_FRAMES_B6 if c.B <= 6 else ffc.FUSED_FRAMES_B8)
    # the same struct without frames: what it gave before -- the eight-wave kernel for B <= 5, the four-wave kernel
    # above, its per-component instance with constraints
    plain, pc = _plan(_batch(c), frames=False), _plan(_batch(c), frames=False, cons=True)
    assert plain[0] == (5 if c.B <= 5 else 6 if c.B <= 6 else 7) and plain[1] == (512 if c.B <= 5 else 256) and plain[5] == 0
    assert pc[:3] == [1 if c.B <= 6 else 2, 256, lds] and pc[5] == 0
    if c.B > 5:
        assert plain[2] == lds


def test_the_plan_keeps_the_general_path_outside_the_kernels_conditions():
    from scarlet_amd import _lib
    c = ffc.CASES["k4_64"]
    none = [ffc.FUSED_NONE, 256, 0, 1, LDS_LIMIT, 1, 0, 0]
    assert _plan(_batch(c))[0] == ffc.FUSED_FRAMES_B6
    assert _plan(_batch(c, B=5))[0] == ffc.FUSED_FRAMES_B6           # B <= 5 too: no eight-wave kernel takes ragged frames
    assert _plan(_batch(c, B=7))[0] == ffc.FUSED_FRAMES_B8
    assert _plan(_batch(c, K=5)) == none
    assert _plan(_batch(c, H=68)) == none
    assert _plan(_batch(c, W=68)) == none
    assert _plan(_batch(c, W=62)) == none                             # W % 4
    assert _plan(_batch(c, H=2, W=8)) == none
    assert _plan(_batch(c, diff_kernel=FAKE, psf_h=11, psf_w=11)) == none
    assert _plan(_batch(c), approximate_L=1) == none
    assert _plan(_batch(c, group=FAKE)) == none
    assert _lib.set_option("NO_FUSED", 1) == 0
    try:
        assert _plan(_batch(c)) == none
        assert _plan(_batch(c), frames=False)[0] == ffc.FUSED_NONE
    finally:
        _lib.set_option("NO_FUSED", 0)
    assert _plan(_batch(c))[0] == ffc.FUSED_FRAMES_B6
    # the headline shape keeps its kernels: persistent for several iterations, the exact instance for one
    head = _batch(c, B=5, weights=None)
    assert _plan(head, frames=False, n_iter=10)[:2] == [3, 512] and _plan(head, frames=False, n_iter=1)[:2] == [4, 512]
    assert _lib.lib.scarlet_debug_fused_plan(None, None, None, 0, 1, None) == -1
