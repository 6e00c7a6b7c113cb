"""-m gpu: ragged frames -- scenes of different frame sizes in one BlendBatch (frame_shapes / a list of images).

Scene s lies in the top-left corner of its padded planes and must come out as the reference fits the (B, h_s, w_s) scene
alone.  The cases are those of tests/frame_cases.py (every form of the constraint update, the K <= 4, K <= 8 and big-K
gradient paths, a PSF).  Checked here:
  1. every scene against the oracle run of its cropped arrays started from the batch's own initial state
     (tests/parity_common.py tolerances, at most one logged threshold-straddle exemption per test), and one converged run;
  2. the initialisation alone against the oracle's constructors on each scene's own frame;
  3. pixels outside a scene's frame are exactly zero in both morphology buffers after every call, and in the products;
  4. shapes that all equal (H, W) give the bits of frame_shapes=None on the paths both share;
  5. every copy of a scene gives the same bits wherever it sits and whatever its neighbours' shapes are;
  6. shapes outside 1..H x 1..W on the device set STATUS_BAD_FRAME and leave those scenes untouched;
  7. products() against its definition on each cropped scene.
"""
import multiprocessing as mp
import os

import numpy as np
import pytest

from conftest import rel_err
import frame_cases as fc
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


def _workload(c):
    return pc.Workload(B=c.B, H=c.H, W=c.W, K=c.K, psf=c.psf)


def _make(scarlet, c, images, shapes, centers, counts, mse_capacity=16, init=True, **kw):
    """the case's batch of the given padded scenes; shapes None: a uniform batch"""
    wl = _workload(c)
    if (np.asarray(counts) != c.K).any():
        kw["n_components"] = counts
    if c.psf:
        kw["centroid_weight"] = wl.model_psf.astype(np.float32)
    b = scarlet.BlendBatch(images, centers, frame_shapes=shapes, mse_capacity=mse_capacity, **kw)
    if c.psf:
        b.set_diff_kernel(wl.diff)
    if init:
        b.init_extended(np.ones(c.B) * fc.BG, sed_scale=wl.scale)
    return b


def _state(b):
    torch.cuda.synchronize()
    return dict(sed=[t.cpu().numpy() for t in b.sed], morph=[t.cpu().numpy() for t in b.morph],
                cur=b.cur.cpu().numpy(), cen=b.centers.cpu().numpy(), shifts=b.shifts.cpu().numpy(),
                flags=b.flags.cpu().numpy(), mse=b.mse_buf.cpu().numpy(), it=b.it.cpu().numpy(),
                status=b.status.cpu().numpy(), active=b.active.cpu().numpy(), lip=b.lipschitz.cpu().numpy())


def _assert_identical(a, b, what, keep=None):
    for key in a:
        xs, ys = (a[key], b[key]) if isinstance(a[key], list) else ([a[key]], [b[key]])
        for i, (x, y) in enumerate(zip(xs, ys)):
            if keep is not None:
                x, y = x[keep], y[keep]
            assert np.array_equal(x, y, equal_nan=True), "%s: %s[%d] differs" % (what, key, i)


def _outside(shapes, H, W):
    """(S, 1, H, W) bool: the pixels outside each scene's own frame"""
    sh = np.asarray(shapes)
    return ((np.arange(H)[None, :, None] >= sh[:, 0, None, None]) | (np.arange(W)[None, None, :] >= sh[:, 1, None, None]))[:, None]


def _assert_outside_zero(b, shapes, what):
    torch.cuda.synchronize()
    out = _outside(shapes, b.H, b.W)
    for i in range(2):
        m = b.morph[i].cpu().numpy()
        assert np.array_equal(m[np.broadcast_to(out, m.shape)], np.zeros(int(np.broadcast_to(out, m.shape).sum()), np.float32)), \
            "%s: morph[%d] is not zero outside the frames" % (what, i)


# ------------------------------------------------------------------ 1. every scene against the oracle on its own frame
def _vs_oracle(scarlet, pool, c, iters, e_rel, test, max_exempt=1):
    images, shapes, centers, n = fc.padded(c)
    b = _make(scarlet, c, images, shapes, centers, n, mse_capacity=iters + 1)
    st0 = _state(b)
    _assert_outside_zero(b, shapes, test + " after init")
    b.fit(iters, e_rel=e_rel, check_every=10)
    st = _state(b)
    _assert_outside_zero(b, shapes, test + " after fit")
    wl = _workload(c)
    sc = fc.scenes(c)
    S = len(sc)
    jobs = []
    for i in range(S):
        h, w = shapes[i]
        c0 = st0["cur"][i]
        jobs.append((np.array(sc[i][0]), st0["sed"][c0][i][:n[i]], st0["morph"][c0][i][:n[i], :h, :w], st0["cen"][i][:n[i]],
                     st0["shifts"][i][:n[i]], iters, e_rel, np.float32, wl.oracle_kwargs()))
    ref = pool.map(pc.oracle_fit, jobs)
    assert not st["status"].any(), st["status"]
    exempt = []
    for i in range(S):
        h, w = shapes[i]
        cur = st["cur"][i]
        sed, morph = st["sed"][cur][i][:n[i]], st["morph"][cur][i][:n[i], :h, :w]
        assert np.array_equal(b.scene(i)[1].cpu().numpy(), morph) and np.array_equal(b.scene(i)[0].cpu().numpy(), sed)
        np.testing.assert_array_equal(st["cen"][i][:n[i]], ref[i][3])
        assert st["it"][i] == ref[i][4], (i, st["it"][i], ref[i][4])
        if e_rel > 0:
            flags = st["flags"][i][:n[i]] & 3
            assert np.array_equal(flags, np.array(ref[i][5]) & 3), (i, flags, ref[i][5])
        e = dict(sed=rel_err(sed, ref[i][0]), morph=rel_err(morph, ref[i][1]), mse=rel_err(st["mse"][i][:st["it"][i]], ref[i][2]))
        print("%s scene %d %s: %s" % (test, i, tuple(shapes[i]), e))
        if max(e.values()) <= TOL:
            continue
        assert e_rel == 0, "scene %d %s beyond 1e-5 in a converged run: %s" % (i, tuple(shapes[i]), e)
        ok, msg = pc.straddles_threshold(scarlet, wl, np.array(sc[i][0]), sc[i][1], iters)
        assert ok, "scene %d %s beyond 1e-5 (%s) and not a threshold straddle: %s" % (i, tuple(shapes[i]), e, msg)
        exempt.append((i, e, msg))
    pc.log_exemptions(test, exempt, max_exempt)
    assert len(exempt) <= max_exempt, exempt
    return st


@pytest.mark.parametrize("name", list(fc.CASES))
def test_scenes_match_the_oracle_on_their_own_frames(env, name):
    scarlet, pool = env
    c = fc.CASES[name]
    st = _vs_oracle(scarlet, pool, c, c.iters, 0.0, "ragged frames " + name)
    assert (st["it"] == c.iters).all()


def test_converged_run_matches_the_oracle(env):
    scarlet, pool = env
    st = _vs_oracle(scarlet, pool, fc.CASES["wave"], 200, 1e-3, "ragged frames wave converged", max_exempt=0)
    assert (st["active"] == 0).any(), "no scene converged within 200 iterations: the run tests nothing"


# ------------------------------------------------------------------ 2. the initialisation alone
@pytest.mark.parametrize("name", ["wave", "tile"])
def test_init_extended_on_each_scenes_own_frame(env, name):
    scarlet, _ = env
    c = fc.CASES[name]
    images, shapes, centers, n = fc.padded(c)
    b = _make(scarlet, c, images, shapes, centers, n)
    st = _state(b)
    assert not st["status"].any()
    for i, (im, cen) in enumerate(fc.scenes(c)):
        h, w = shapes[i]
        ref = fc.oracle_start(c, np.array(im), cen)
        cur = st["cur"][i]
        assert rel_err(st["sed"][cur][i][:n[i]], np.array([s.sed for s in ref.sources])) <= TOL, (name, i)
        assert rel_err(st["morph"][cur][i][:n[i], :h, :w], np.array([s.morph for s in ref.sources])) <= TOL, (name, i)
        np.testing.assert_array_equal(st["cen"][i][:n[i]], np.array([s.center for s in ref.sources]))
        np.testing.assert_array_equal(st["flags"][i][:n[i]], np.array([int(s.flags) for s in ref.sources]))
    # init_sources (per-scene noise rows) starts the same extended sources
    b2 = _make(scarlet, c, images, shapes, centers, n, init=False)
    b2.init_sources(np.ones((len(images), c.B)) * fc.BG)
    _assert_identical(st, _state(b2), name + ": init_sources against init_extended")


# ------------------------------------------------------------------ 3. outside stays zero
@pytest.mark.parametrize("name", ["wave", "psf"])
def test_outside_pixels_stay_zero(env, name):
    scarlet, _ = env
    c = fc.CASES[name]
    images, shapes, centers, n = fc.padded(c)
    # padding that is not zero: the batch masks data and weights itself
    dirty = images.copy()
    dirty[np.broadcast_to(_outside(shapes, c.H, c.W), dirty.shape)] = 7.0
    b = _make(scarlet, c, dirty, shapes, centers, n)
    _assert_outside_zero(b, shapes, "init")
    b.fit(3, e_rel=0)
    _assert_outside_zero(b, shapes, "fit")
    b.step(e_rel=0)
    _assert_outside_zero(b, shapes, "step")
    ref = _make(scarlet, c, images, shapes, centers, n)
    ref.fit(3, e_rel=0)
    ref.step(e_rel=0)
    _assert_identical(_state(ref), _state(b), name + ": dirty padding against zero padding")
    rng = np.random.default_rng(11)
    b.set_state(rng.uniform(0.5, 1.5, size=(b.S, b.K, b.B)).astype(np.float32),
                rng.uniform(0.1, 1.0, size=(b.S, b.K, b.H, b.W)).astype(np.float32))
    _assert_outside_zero(b, shapes, "set_state")
    b.fit(2, e_rel=0)
    _assert_outside_zero(b, shapes, "set_state + fit")
    before = _state(b)
    p = b.products()
    torch.cuda.synchronize()
    out = _outside(shapes, c.H, c.W)
    for key in ("model", "rendered", "residual"):
        x = getattr(p, key).cpu().numpy()
        assert not np.any(x[np.broadcast_to(out, x.shape)]), "%s: products().%s is not zero outside the frames" % (name, key)
        assert np.isfinite(x).all()
    _assert_identical(before, _state(b), name + ": products() is read-only")


# ------------------------------------------------------------------ 4. full-size shapes change nothing
@pytest.mark.parametrize("K,psf", [(6, False), (4, True)], ids=["general_k6", "psf_k4"])
def test_full_size_shapes_give_the_bits_of_none(env, K, psf):
    scarlet, _ = env
    wl = pc.Workload(B=5, H=64, W=64, K=K, psf=psf)
    S = 4
    images, centers = wl.scenes(9800 + K, S)
    out = []
    for shapes in (None, np.tile(np.array([[64, 64]], np.int32), (S, 1))):
        kw = dict(mse_capacity=8, frame_shapes=shapes)
        if psf:
            kw["centroid_weight"] = wl.model_psf.astype(np.float32)
        b = scarlet.BlendBatch(images, centers, **kw)
        if psf:
            b.set_diff_kernel(wl.diff)
        b.init_extended(np.ones(5) * 0.1, sed_scale=wl.scale)
        b.fit(5, e_rel=0, check_every=3)
        out.append(_state(b))
        del b
    _assert_identical(out[0], out[1], "full-size frame_shapes")
    assert (out[0]["it"] == 5).all()


# ------------------------------------------------------------------ 5. isolation
def _tiled(c, S, seed):
    images, shapes, centers, n = fc.padded(c)
    order = np.random.default_rng(seed).permutation(S) % len(images)
    return images[order], shapes[order], centers[order], n[order], order


def _assert_copies_agree(st, order, what):
    for src in np.unique(order):
        idx = np.nonzero(order == src)[0]
        first = idx[0]
        for key in ("sed", "morph"):
            cur = [st[key][st["cur"][i]][i] for i in idx]
            for x in cur[1:]:
                assert np.array_equal(x, cur[0], equal_nan=True), (what, key, src)
        for key in ("cen", "shifts", "flags", "mse", "it", "status", "lip"):
            assert np.array_equal(st[key][idx], np.broadcast_to(st[key][first], st[key][idx].shape), equal_nan=True), (what, key, src)


def test_copies_of_a_scene_agree_wherever_they_sit(env):
    scarlet, _ = env
    c = fc.CASES["wave"]
    images, shapes, centers, n, order = _tiled(c, 64, 1)
    b = _make(scarlet, c, images, shapes, centers, n)
    b.fit(6, e_rel=0)
    st = _state(b)
    assert not st["status"].any() and (st["it"] == 6).all()
    _assert_copies_agree(st, order, "wave x 64")
    # ... and equal the case's own batch, scene for scene
    i0, s0, c0, n0 = fc.padded(c)
    small = _make(scarlet, c, i0, s0, c0, n0)
    small.fit(6, e_rel=0)
    ss = _state(small)
    for i, src in enumerate(order):
        assert np.array_equal(st["morph"][st["cur"][i]][i], ss["morph"][ss["cur"][src]][src]), (i, src)
        assert np.array_equal(st["mse"][i], ss["mse"][src]), (i, src)


def test_copies_agree_across_the_two_half_batch_pipelines(env):
    import ctypes
    scarlet, _ = env
    c = fc.CASES["psf"]
    images, shapes, centers, n, order = _tiled(c, 1024, 2)
    b = _make(scarlet, c, images, shapes, centers, n, mse_capacity=8)
    assert scarlet._lib.lib.scarlet_batch_pipelines(ctypes.byref(b._c)) == 2
    b.fit(5, e_rel=0)
    st = _state(b)
    assert not st["status"].any() and (st["it"] == 5).all()
    _assert_copies_agree(st, order, "psf x 1024")
    _assert_outside_zero(b, shapes, "psf x 1024")


# ------------------------------------------------------------------ 6. bad shapes on the device
@pytest.mark.parametrize("name", ["wave", "tile", "psf"])
def test_bad_shapes_on_device(env, name):
    """the device check runs before any kernel reads a plane: the two scenes are refused and never touched"""
    scarlet, _ = env
    from scarlet_amd import _lib
    c = fc.CASES[name]
    images, shapes, centers, n = fc.padded(c)
    images, shapes, centers, n = (np.concatenate([x, x]) for x in (images, shapes, centers, n))
    S = len(images)
    assert S - 1 not in (1, 3)
    out = []
    for corrupt in (False, True):
        b = _make(scarlet, c, images, shapes, centers, n, init=False)
        if corrupt:
            b.frame_shapes[1, 0] = 0
            b.frame_shapes[3, 0] = c.H + 1
        st0 = _state(b)
        b.init_extended(np.ones(c.B) * fc.BG, sed_scale=_workload(c).scale)
        b.fit(4, e_rel=0, check_every=3)
        b.step(e_rel=0)
        p = b.products()
        assert np.isfinite(p.model.cpu().numpy()).all()
        out.append((st0, _state(b)))
        if corrupt:
            with pytest.raises(ValueError, match=r"scenes \[1, 3\]"):
                b.raise_on_status()
    (_, good), (st0, badst) = out
    for i in (1, 3):
        assert badst["status"][i] == _lib.STATUS_BAD_FRAME and badst["active"][i] == 0 and badst["it"][i] == 0
        for key in ("sed", "morph"):
            for j in range(2):
                assert not np.any(badst[key][j][i])
        for key in ("cen", "shifts", "flags", "mse", "cur", "lip"):
            assert np.array_equal(badst[key][i], st0[key][i], equal_nan=True), key
    keep = np.ones(S, bool); keep[[1, 3]] = False
    assert not good["status"].any()
    _assert_identical(good, badst, name + ": the other scenes", keep=keep)


# ------------------------------------------------------------------ 7. products against their definition
def test_products_against_their_definition(env):
    """case psf after one iteration: model, rendered, residual and loss of every scene against the float64 evaluation of
    its cropped factors and data (tests/products_common.py), and the loss against what the next iteration records"""
    import products_common as prc
    scarlet, _ = env
    c = fc.CASES["psf"]
    wl = _workload(c)
    images, shapes, centers, n = fc.padded(c)
    b = _make(scarlet, c, images, shapes, centers, n)
    b.fit(1, e_rel=0)
    p = b.products()
    torch.cuda.synchronize()
    for i, (im, _) in enumerate(fc.scenes(c)):
        h, w = shapes[i]
        sed, morph = (x.cpu().numpy() for x in b.scene(i))
        ref = prc.reference(sed, morph, np.array(im), 1.0, wl.diff)
        got = dict(model=p.model[:, :, :h, :w], rendered=p.rendered[:, :, :h, :w], residual=p.residual[:, :, :h, :w], loss=p.loss)
        prc.check_scene(got, i, ref, ("model", "rendered", "residual", "loss"), where="ragged frames psf")
    b.fit(1, e_rel=0)
    torch.cuda.synchronize()
    assert rel_err(p.loss.sum(dim=1).cpu().numpy(), b.mse_buf.cpu().numpy()[:, 1]) <= TOL


# ------------------------------------------------------------------ the refusals that need a batch
def test_refusals_on_a_ragged_frame_batch(env):
    scarlet, _ = env
    from scarlet_amd import prior as sp
    c = fc.CASES["wave"]
    images, shapes, centers, n = fc.padded(c)
    b = _make(scarlet, c, images, shapes, centers, n)
    assert b.frame_shapes.dtype == torch.int32 and tuple(b.frame_shapes.shape) == (len(images), 2)
    assert b.weights is not None and tuple(b.weights.shape) == tuple(images.shape)
    out = _outside(shapes, c.H, c.W)
    assert not np.any(b.weights.cpu().numpy()[np.broadcast_to(out, images.shape)])
    for call in (lambda: b.fit(1, prior=sp.QuadraticPrior(morph_weight=0.1)), lambda: b.step(prior=sp.QuadraticPrior(morph_weight=0.1)),
                 lambda: b.init_sources(np.ones(c.B) * fc.BG, kind=np.zeros((b.S, b.K), np.int32)),
                 lambda: b.init_combined([np.ones(c.B) * fc.BG])):
        with pytest.raises(NotImplementedError):
            call()
    # the list form is the padded form
    b2 = scarlet.BlendBatch([np.array(im) for im, _ in fc.scenes(c)], centers, mse_capacity=16)
    b2.init_extended(np.ones(c.B) * fc.BG)
    _assert_identical(_state(b), _state(b2), "list of images against padded block")
    with pytest.raises(ValueError):
        b.set_state(b.sed_current, b.morph_current, centers=np.full((b.S, b.K, 2), 39, np.int32))      # outside 17 x 23
