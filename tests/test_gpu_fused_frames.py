"""-m gpu: ragged-frame batches on the one-launch iteration (the four-wave kernel's ragged-frames instance).

The cases are those of tests/fused_frame_cases.py.  Checked here:
  1. every iteration of every case is ONE launch of profile class 4;
  2. every scene against the oracle run of its cropped arrays, started from the batch's own initial state, at
     tests/parity_common.py's TOL with NO threshold-straddle exemption; centres and iteration counts bit-exact;
  3. a converged run of k4_64: flags and iteration counts as the oracle's, scenes stopping at different iterations;
  4. pixels outside a scene's frame stay exactly zero in both morphology buffers and in the products;
  5. isolation: copies of a scene agree bitwise wherever they sit; frames the reference has no result for, and a NaN
     scene, leave their neighbours' bits alone;
  6. the general path (NO_FUSED) keeps its coverage of the K <= 4 wave form of the constraint update.
"""
import ctypes
import multiprocessing as mp
import os

import numpy as np
import pytest

from conftest import rel_err
import frame_cases as fc
import fused_frame_cases as ffc
import parity_common as pc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
TOL = pc.TOL


@pytest.fixture(scope="module")
def env():
    import scarlet_amd
    scarlet_amd._lib.require_gpu()
    from oracle import build as obuild
    obuild.build()
    pool = mp.get_context("spawn").Pool(min(16, os.cpu_count() or 1))
    yield scarlet_amd, pool
    pool.close(); pool.join()


def _make(scarlet, c, images, shapes, centers, counts, mse_capacity=16, **kw):
    if (np.asarray(counts) != c.K).any():
        kw["n_components"] = counts
    b = scarlet.BlendBatch(images, centers, frame_shapes=shapes, mse_capacity=mse_capacity, **kw)
    b.init_extended(np.ones(c.B) * ffc.BG)
    return b


def _case_batch(scarlet, c, mse_capacity=16):
    images, shapes, centers, n = ffc.padded(c)
    return _make(scarlet, c, images, shapes, centers, n, mse_capacity=mse_capacity, **ffc.batch_kwargs(c))


def _state(b):
    torch.cuda.synchronize()
    return dict(sed=[t.cpu().numpy() for t in b.sed], morph=[t.cpu().numpy() for t in b.morph],
                cur=b.cur.cpu().numpy(), cen=b.centers.cpu().numpy(), shifts=b.shifts.cpu().numpy(),
                flags=b.flags.cpu().numpy(), mse=b.mse_buf.cpu().numpy(), it=b.it.cpu().numpy(),
                status=b.status.cpu().numpy(), active=b.active.cpu().numpy(), lip=b.lipschitz.cpu().numpy())


def _outside(shapes, H, W):
    sh = np.asarray(shapes)
    return ((np.arange(H)[None, :, None] >= sh[:, 0, None, None]) | (np.arange(W)[None, None, :] >= sh[:, 1, None, None]))[:, None]


def _assert_outside_zero(b, shapes, what):
    torch.cuda.synchronize()
    out = _outside(shapes, b.H, b.W)
    for i in range(2):
        m = b.morph[i].cpu().numpy()
        sel = m[np.broadcast_to(out, m.shape)]
        assert np.array_equal(sel.view(np.uint32), np.zeros(sel.size, np.uint32)), "%s: morph[%d] is not +0 outside the frames" % (what, i)


def _profiled_fit(scarlet, b, iters, **kw):
    L = scarlet._lib.lib
    torch.cuda.synchronize()
    scarlet._lib.check(L.scarlet_profile_begin(iters))
    try:
        n = b.fit(iters, **kw)
    finally:
        ms, counts = (ctypes.c_double * 8)(), (ctypes.c_int64 * 8)()
        scarlet._lib.check(L.scarlet_profile_end(ms, counts))
    return n, list(counts)


_runs = {}


def _run(scarlet, name):
    """the case's batch after init (st0) and after its fixed-iteration fit under the profile recorder (st, counts);
    shared by the tests below, read-only"""
    if name not in _runs:
        c = ffc.CASES[name]
        b = _case_batch(scarlet, c, mse_capacity=c.iters + 1)
        st0 = _state(b)
        n, counts = _profiled_fit(scarlet, b, c.iters, e_rel=0, check_every=0)
        assert n == c.iters
        _runs[name] = dict(b=b, st0=st0, st=_state(b), counts=counts)
    return _runs[name]


def _oracle_jobs(c, st0, iters, e_rel):
    sc, wg, sw = ffc.scenes(c), ffc.weights(c), ffc.switches(c)
    jobs = []
    for i, ((h, w), n) in enumerate(zip(c.shapes, c.counts)):
        c0 = st0["cur"][i]
        jobs.append((np.array(sc[i][0]), st0["sed"][c0][i][:n], st0["morph"][c0][i][:n, :h, :w], st0["cen"][i][:n],
                     st0["shifts"][i][:n], iters, e_rel, 1 if wg is None else wg[i],
                     None if sw is None else tuple(a[i][:n] for a in sw)))
    return jobs


def _compare(c, b, st, ref, what, flags=False):
    """every scene against the oracle's result: TOL on sed / morph / loss, centres and iteration counts bit-exact"""
    assert not st["status"].any(), st["status"]
    worst = 0.0
    for i, ((h, w), n) in enumerate(zip(c.shapes, c.counts)):
        cur = st["cur"][i]
        sed, morph = st["sed"][cur][i][:n], st["morph"][cur][i][:n, :h, :w]
        got = b.scene(i)
        assert np.array_equal(got[1].cpu().numpy(), morph) and np.array_equal(got[0].cpu().numpy(), sed), (what, i)
        np.testing.assert_array_equal(st["cen"][i][:n], ref[i][3])
        assert st["it"][i] == ref[i][4], (what, i, st["it"][i], ref[i][4])
        if flags:
            assert np.array_equal(st["flags"][i][:n] & 3, np.array(ref[i][5]) & 3), (what, i, st["flags"][i], ref[i][5])
        e = dict(sed=rel_err(sed, ref[i][0]), morph=rel_err(morph, ref[i][1]), mse=rel_err(st["mse"][i][:st["it"][i]], ref[i][2]))
        print("%s scene %d %s: %s" % (what, i, (h, w), e))
        worst = max(worst, max(e.values()))
        assert max(e.values()) <= TOL, "%s: scene %d %s beyond 1e-5: %s" % (what, i, (h, w), e)
    print("%s: worst max-norm relative error %.3e" % (what, worst))


# ------------------------------------------------------------------ 1. one launch per iteration
@pytest.mark.parametrize("name", list(ffc.CASES))
def test_one_launch_per_iteration(env, name):
    """(fails where ragged frames take the general path: the counts land in classes 0 - 3)"""
    scarlet, _ = env
    c = ffc.CASES[name]
    r = _run(scarlet, name)
    assert r["counts"] == [0, 0, 0, 0, c.iters, 0, 0, 0], r["counts"]
    assert (r["st"]["it"] == c.iters).all()


# ------------------------------------------------------------------ 2. parity
@pytest.mark.parametrize("name", list(ffc.CASES))
def test_scenes_match_the_oracle_on_their_own_frames(env, name):
    scarlet, pool = env
    c = ffc.CASES[name]
    r = _run(scarlet, name)
    ref = pool.map(ffc.oracle_fit_state, _oracle_jobs(c, r["st0"], c.iters, 0.0))
    _compare(c, r["b"], r["st"], ref, "fused ragged frames " + name)


# ------------------------------------------------------------------ 3. converged run
def test_converged_run_matches_the_oracle(env):
    scarlet, pool = env
    c = ffc.CASES["k4_64"]
    b = _case_batch(scarlet, c, mse_capacity=201)
    st0 = _state(b)
    b.fit(200, e_rel=1e-3, check_every=10)
    st = _state(b)
    ref = pool.map(ffc.oracle_fit_state, _oracle_jobs(c, st0, 200, 1e-3))
    _compare(c, b, st, ref, "fused ragged frames k4_64 converged", flags=True)
    print("iterations:", st["it"].tolist())
    assert (st["it"] < 200).any(), "no scene stopped before 200 iterations: the run tests nothing"
    assert st["it"].max() > st["it"].min(), "no scene went on after another had stopped: the inactive-scene return is not exercised"
    assert (st["active"][st["it"] < 200] == 0).all()
    _assert_outside_zero(b, ffc.padded(c)[1], "converged")


# ------------------------------------------------------------------ 4. outside pixels
@pytest.mark.parametrize("name", list(ffc.CASES))
def test_outside_pixels_stay_zero(env, name):
    scarlet, _ = env
    c = ffc.CASES[name]
    shapes = ffc.padded(c)[1]
    b = _case_batch(scarlet, c)
    _assert_outside_zero(b, shapes, name + " init")
    b.fit(3, e_rel=0)
    _assert_outside_zero(b, shapes, name + " fit")
    b.fit(2, e_rel=0)
    _assert_outside_zero(b, shapes, name + " second fit")
    p = b.products()
    torch.cuda.synchronize()
    out = _outside(shapes, c.H, c.W)
    for key in ("model", "rendered", "residual"):
        x = getattr(p, key).cpu().numpy()
        assert not np.any(x[np.broadcast_to(out, x.shape)]), "%s: products().%s is not zero outside the frames" % (name, key)
        assert np.isfinite(x).all()


# ------------------------------------------------------------------ 5. isolation
def _scene_bits(st, i):
    cur = st["cur"][i]
    return dict(sed=st["sed"][cur][i], morph=st["morph"][cur][i], cen=st["cen"][i], shifts=st["shifts"][i], flags=st["flags"][i],
                mse=st["mse"][i], it=st["it"][i], status=st["status"][i], lip=st["lip"][i])


def _assert_same_scene(a, b, what):
    for key in a:
        assert np.array_equal(a[key], b[key], equal_nan=True), "%s: %s differs" % (what, key)


def test_copies_of_a_scene_agree_wherever_they_sit(env):
    scarlet, _ = env
    c = ffc.CASES["k4_64"]
    images, shapes, centers, n = ffc.padded(c)
    order = np.random.default_rng(3).permutation(64) % len(images)
    b = _make(scarlet, c, images[order], shapes[order], centers[order], n[order], mse_capacity=c.iters + 1)
    n_it, counts = _profiled_fit(scarlet, b, c.iters, e_rel=0, check_every=0)
    assert counts == [0, 0, 0, 0, c.iters, 0, 0, 0]
    st, own = _state(b), _run(scarlet, "k4_64")["st"]
    assert not st["status"].any() and (st["it"] == c.iters).all()
    for i, src in enumerate(order):
        _assert_same_scene(_scene_bits(st, i), _scene_bits(own, src), "copy %d of scene %d" % (i, src))
    _assert_outside_zero(b, shapes[order], "k4_64 x 64")


def test_frames_without_a_reference_leave_their_neighbours_alone(env):
    """frames (2, 7), (64, 1), (1, 1): the ABI allows 1 <= h, w, the reference has no result for them; nothing is
    asserted about their own values"""
    scarlet, _ = env
    c = ffc.CASES["k4_64"]
    images, shapes, centers, n = ffc.padded(c)
    S = len(images)
    extra = len(ffc.NO_REFERENCE_FRAMES)
    images = np.concatenate([images, np.zeros((extra,) + images.shape[1:], np.float32)])
    centers = np.concatenate([centers, np.zeros((extra,) + centers.shape[1:], np.int32)])
    for j, ((h, w), cen) in enumerate(ffc.NO_REFERENCE_FRAMES):
        images[S + j, :, :h, :w] = ffc.hand_scene(c.B, h, w, (cen,), 1600 + j)[0]
        centers[S + j, 0] = cen
    shapes = np.concatenate([shapes, np.array([s for s, _ in ffc.NO_REFERENCE_FRAMES], np.int32)])
    n = np.concatenate([n, np.ones(extra, np.int32)])
    b = _make(scarlet, c, images, shapes, centers, n, mse_capacity=c.iters + 1)
    _assert_outside_zero(b, shapes, "init")
    _, counts = _profiled_fit(scarlet, b, c.iters, e_rel=0, check_every=0)
    assert counts == [0, 0, 0, 0, c.iters, 0, 0, 0]
    st, own = _state(b), _run(scarlet, "k4_64")["st"]
    for i in range(S):
        assert st["status"][i] == 0
        _assert_same_scene(_scene_bits(st, i), _scene_bits(own, i), "scene %d beside the three" % i)
    _assert_outside_zero(b, shapes, "fit")


def test_a_nan_scene_leaves_its_neighbours_alone(env):
    """one scene of b6_k3 with a NaN image pixel inside its frame, away from its centres"""
    scarlet, _ = env
    c = ffc.CASES["b6_k3"]
    images, shapes, centers, n = ffc.padded(c)
    bad = 2                                       # (24, 29): a row tail that straddles the frame's edge
    h, w = shapes[bad]
    images = images.copy()
    y, x = 1, int(w) - 1                          # the last column of the frame, in its straddling group
    assert all(max(abs(int(cy) - y), abs(int(cx) - x)) >= 4 for cy, cx in centers[bad][:n[bad]])
    b = _make(scarlet, c, images, shapes, centers, n, mse_capacity=c.iters + 1)        # (init from clean data)
    b.images[bad, 1, y, x] = float("nan")
    b.fit(c.iters, e_rel=0, check_every=0)
    st = _state(b)
    clean = _case_batch(scarlet, c, mse_capacity=c.iters + 1)
    clean.fit(c.iters, e_rel=0, check_every=0)
    ref = _state(clean)
    for i in range(len(images)):
        if i != bad:
            assert st["status"][i] == 0
            _assert_same_scene(_scene_bits(st, i), _scene_bits(ref, i), "scene %d beside the NaN scene" % i)
    cur = st["cur"][bad]
    assert np.isnan(st["morph"][cur][bad][:n[bad], :h, :w]).any(), "the NaN never reached the scene: the test tests nothing"
    _assert_outside_zero(b, shapes, "NaN scene")


# ------------------------------------------------------------------ 6. the general path keeps its coverage
def test_general_path_under_no_fused(env):
    """case wave of tests/frame_cases.py (K = 2, 40 x 40) under NO_FUSED: k_source_update_w_ragged with K <= 4, which
    approximate_L and NO_FUSED users still take, against the oracle at TOL"""
    scarlet, pool = env
    c = fc.CASES["wave"]
    images, shapes, centers, n = fc.padded(c)
    prev = scarlet._lib.set_option("NO_FUSED", 1)
    try:
        b = scarlet.BlendBatch(images, centers, frame_shapes=shapes, mse_capacity=c.iters + 1)
        b.init_extended(np.ones(c.B) * fc.BG)
        st0 = _state(b)
        _, counts = _profiled_fit(scarlet, b, c.iters, e_rel=0, check_every=0)
        st = _state(b)
    finally:
        scarlet._lib.set_option("NO_FUSED", prev)
    print("NO_FUSED launch counts per class:", counts)
    assert counts[4] == 0 and counts[2] > 0 and counts[3] > 0, counts
    sc = fc.scenes(c)
    jobs = []
    for i, (h, w) in enumerate(shapes):
        c0 = st0["cur"][i]
        jobs.append((np.array(sc[i][0]), st0["sed"][c0][i][:n[i]], st0["morph"][c0][i][:n[i], :h, :w], st0["cen"][i][:n[i]],
                     st0["shifts"][i][:n[i]], c.iters, 0.0, 1, None))
    ref = pool.map(ffc.oracle_fit_state, jobs)
    cc = ffc.Case("wave", c.H, c.W, c.B, c.K, c.shapes, c.counts, c.iters, c.seed, {}, False, False, 0)
    _compare(cc, b, st, ref, "general path (NO_FUSED) wave")
    _assert_outside_zero(b, shapes, "NO_FUSED wave")
