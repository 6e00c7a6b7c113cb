"""-m gpu: joint fits of scenes with their own frame sizes -- BlendBatch.from_observations on observations that carry
frame_shapes (scarlet_fit_observations_frames, scarlet_observations_products_frames).

Scene s lies in the top-left corner of its padded planes in every observation and must come out as the reference fits the
(C, h_s, w_s) scene alone against its cropped observations.  The cases are those of tests/observation_frame_cases.py.
Checked here:
  1. every scene against the oracle run of its cropped arrays started from the batch's own initial state: sed, morph and
     loss history to parity_common.TOL, centres, iteration counts and flags exactly.  NO threshold-straddle exemption:
     tests/test_observation_frame_cases.py shows that the float32 and float64 oracles agree to 1e-6 with equal supports
     on every scene, so none is needed;
  2. init_combined alone against the oracle's CombinedExtendedSource on each scene's own frame;
  3. pixels outside a scene's frame are exactly zero in both morphology buffers after every call; dirty padding changes no bit;
  4. shapes that all equal (H, W) give the bits of the uniform joint batch;
  5. every copy of a scene gives the same bits wherever it sits and whatever its neighbours' shapes are;
  6. a shape outside 1..H x 1..W on the device sets STATUS_BAD_FRAME and leaves that scene untouched;
  7. products() per observation against its definition on each cropped scene; read-only;
  8. a converged run;
  9. the refusals that need a batch.
"""
import multiprocessing as mp
import os

import numpy as np
import pytest

from conftest import rel_err
import observation_frame_cases as oc
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


def _build(scarlet, c, obs, shapes, centers, counts, bands=None, weights=None, mse_capacity=16, **kw):
    """the joint batch of the padded observations `obs`; shapes None: the uniform batch of the padded block;
    weights: None or one entry per observation (scalar, block or per-scene list)"""
    batches = []
    for i, o in enumerate(obs):
        ob = scarlet.ObservationBatch(o["images"], band0=o["band0"], weights=None if weights is None else weights[i],
                                      frame_shapes=shapes)
        if o.get("diff") is not None:
            ob.set_diff_kernel(o["diff"])
        batches.append(ob)
    if (np.asarray(counts) != c.K).any():
        kw["n_components"] = counts
    if c.psf:
        kw["centroid_weight"] = oc.centroid_weight(c)
    if c.C > 8:
        kw["wide"] = True
    return scarlet.BlendBatch.from_observations(batches, centers, mse_capacity=mse_capacity, **kw)


def _bg(bands):
    return [np.ones(nb) * oc.BG for _, nb in bands]


def _start(scarlet, c, b, obs, shapes, centers, counts):
    """the case's start: init_combined where the observations tile the channels, otherwise (`epochs`) the state that
    init_combined gives the band-sliced observations of the same scenes, loaded with set_state"""
    if c.start == c.bands:
        b.init_combined(_bg(c.bands))
        return b
    assert c.name == "epochs"
    full = obs[0]["images"]
    sliced = [dict(images=np.ascontiguousarray(full[:, b0:b0 + nb]), band0=b0, diff=None) for b0, nb in c.start]
    start = _build(scarlet, c, sliced, shapes, centers, counts)
    start.init_combined(_bg(c.start))
    b.set_state(start.sed_current, start.morph_current)
    return b


def _make(scarlet, c, fill=0.0, uniform=False, **kw):
    obs, shapes, centers, counts = oc.padded(c, fill=fill)
    b = _build(scarlet, c, obs, None if uniform else shapes, centers, counts, **kw)
    return _start(scarlet, c, b, obs, None if uniform else shapes, centers, counts)


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
        sel = np.broadcast_to(out, m.shape)
        assert np.array_equal(m[sel], np.zeros(int(sel.sum()), np.float32)), "%s: morph[%d] is not zero outside the frames" % (what, i)


# ------------------------------------------------------------------ 1. every scene against the oracle on its own frame
def _vs_oracle(env, name, test, iters=None, e_rel=0.0, approximate_L=False, weights=None, oracle_weights=None):
    scarlet, pool = env
    c = oc.CASES[name]
    iters = c.iters if iters is None else iters
    obs, shapes, centers, n = oc.padded(c)
    b = _build(scarlet, c, obs, shapes, centers, n, weights=weights, mse_capacity=iters + 1)
    _start(scarlet, c, b, obs, shapes, centers, n)
    st0 = _state(b)
    assert not st0["status"].any(), st0["status"]
    _assert_outside_zero(b, shapes, test + " after the start")
    b.fit(iters, e_rel=e_rel, approximate_L=approximate_L, check_every=10)
    b.raise_on_status()
    st = _state(b)
    _assert_outside_zero(b, shapes, test + " after fit")
    S = len(c.shapes)
    jobs = []
    for i in range(S):
        h, w = shapes[i]
        c0 = st0["cur"][i]
        jobs.append((name, i, st0["sed"][c0][i][:n[i]], st0["morph"][c0][i][:n[i], :h, :w], st0["cen"][i][:n[i]],
                     st0["shifts"][i][:n[i]], iters, e_rel, approximate_L, None if oracle_weights is None else oracle_weights[i]))
    ref = pool.map(oc.oracle_fit_from, jobs)
    errors = []
    for i in range(S):
        h, w = shapes[i]
        cur = st["cur"][i]
        sed, morph = st["sed"][cur][i][:n[i]], st["morph"][cur][i][:n[i], :h, :w]
        assert np.array_equal(b.scene(i)[1].cpu().numpy(), morph) and np.array_equal(b.scene(i)[0].cpu().numpy(), sed)
        e = dict(sed=rel_err(sed, ref[i][0]), morph=rel_err(morph, ref[i][1]), mse=rel_err(st["mse"][i][:st["it"][i]], ref[i][2]))
        print("%s scene %d %s: %s" % (test, i, tuple(shapes[i]), {k: "%.2e" % v for k, v in e.items()}))
        errors.append(e)
    for i in range(S):
        np.testing.assert_array_equal(st["cen"][i][:n[i]], ref[i][3])
        assert st["it"][i] == ref[i][4], (i, st["it"][i], ref[i][4])
        assert np.array_equal(st["flags"][i][:n[i]] & 3, np.array(ref[i][5]) & 3), (i, st["flags"][i], ref[i][5])
        assert not st["sed"][st["cur"][i]][i][n[i]:].any() and not st["morph"][st["cur"][i]][i][n[i]:].any()
        assert max(errors[i].values()) <= TOL, "%s scene %d %s: %s" % (test, i, tuple(shapes[i]), errors[i])
    return st


@pytest.mark.parametrize("name", list(oc.CASES))
def test_scenes_match_the_oracle_on_their_own_frames(env, name):
    st = _vs_oracle(env, name, "ragged observations " + name)
    assert (st["it"] == oc.CASES[name].iters).all()


def test_approximate_L(env):
    st = _vs_oracle(env, "wave", "ragged observations wave approximate_L", approximate_L=True)
    assert (st["it"] == 6).all()


def test_per_scene_weight_lists(env):
    """weights given as per-scene (B_o, h_s, w_s) arrays, observation b a scalar"""
    c = oc.CASES["wave"]
    rng = np.random.default_rng(21)
    wa = [(0.5 + rng.random((2, h, w))).astype(np.float32) for h, w in c.shapes]
    st = _vs_oracle(env, "wave", "ragged observations wave weight lists", weights=[wa, 2.0],
                    oracle_weights=[[wa[s], 2.0] for s in range(len(c.shapes))])
    assert (st["it"] == 6).all()


def test_from_frames_is_the_padded_block(env):
    scarlet, _ = env
    c = oc.CASES["wave"]
    obs, shapes, centers, n = oc.padded(c)
    lists = [scarlet.ObservationBatch.from_frames([oc.scene_observations(c, s)[o] for s in range(len(c.shapes))], band0=b0)
             for o, (b0, _) in enumerate(c.bands)]
    b = scarlet.BlendBatch.from_observations(lists, [cen for _, cen in oc.scenes(c)], mse_capacity=16)
    b.init_combined(_bg(c.bands))
    b.fit(3, e_rel=0)
    ref = _make(scarlet, c)
    ref.fit(3, e_rel=0)
    _assert_identical(_state(ref), _state(b), "from_frames against the padded block")
    assert b.n_components is None and tuple(b.frame_shapes.shape) == (7, 2) and b.frame_shapes.dtype == torch.int32


# ------------------------------------------------------------------ 2. the initialisation alone
@pytest.mark.parametrize("name", ["wave", "tile"])
def test_init_combined_on_each_scenes_own_frame(env, name):
    scarlet, _ = env
    c = oc.CASES[name]
    _, shapes, _, n = oc.padded(c)
    b = _make(scarlet, c)
    st = _state(b)
    assert not st["status"].any() and not st["it"].any()
    for i in range(len(c.shapes)):
        h, w = shapes[i]
        sed, morph, cen = oc.oracle_start(c, i)
        cur = st["cur"][i]
        e = dict(sed=rel_err(st["sed"][cur][i][:n[i]], sed), morph=rel_err(st["morph"][cur][i][:n[i], :h, :w], morph))
        print("init_combined %s scene %d %s: %s" % (name, i, tuple(shapes[i]), {k: "%.2e" % v for k, v in e.items()}))
        assert max(e.values()) <= TOL, (name, i, e)
        assert np.array_equal((st["morph"][cur][i][:n[i], :h, :w] == 0), (morph == 0)), (name, i)
        np.testing.assert_array_equal(st["cen"][i][:n[i]], cen)
        np.testing.assert_array_equal(st["flags"][i][:n[i]], np.full(n[i], 3))       # both NOT_CONVERGED bits, as a new Source
        assert np.isnan(st["shifts"][i]).all()                                       # no update() ran
    _assert_outside_zero(b, shapes, "init_combined " + name)


# ------------------------------------------------------------------ 3. outside stays zero
@pytest.mark.parametrize("name", ["wave", "psf"])
def test_outside_pixels_stay_zero(env, name):
    scarlet, _ = env
    c = oc.CASES[name]
    _, shapes, _, _ = oc.padded(c)
    b = _make(scarlet, c, fill=7.0)              # padding that is not zero: the batch masks data and weights itself
    _assert_outside_zero(b, shapes, "init_combined")
    b.fit(3, e_rel=0)
    _assert_outside_zero(b, shapes, "fit")
    b.step(e_rel=0)
    _assert_outside_zero(b, shapes, "step")
    ref = _make(scarlet, c)
    ref.fit(3, e_rel=0)
    ref.step(e_rel=0)
    _assert_identical(_state(ref), _state(b), name + ": dirty padding against zero padding")
    rng = np.random.default_rng(11)
    b.set_state(rng.uniform(0.5, 1.5, size=(b.S, b.K, b.B)).astype(np.float32),
                rng.uniform(0.1, 1.0, size=(b.S, b.K, b.H, b.W)).astype(np.float32))
    _assert_outside_zero(b, shapes, "set_state")
    b.fit(2, e_rel=0)
    _assert_outside_zero(b, shapes, "set_state + fit")
    assert np.isfinite(b.morph_current.cpu().numpy()).all()


# ------------------------------------------------------------------ 4. full-size shapes change nothing
@pytest.mark.parametrize("name", ["wave", "psf"])
def test_full_size_shapes_give_the_bits_of_the_uniform_batch(env, name):
    """the padded block read as S full-size scenes: frame_shapes all (H, W) against no frame_shapes"""
    scarlet, _ = env
    c = oc.CASES[name]
    obs, shapes, centers, n = oc.padded(c)
    full = np.tile(np.array([[c.H, c.W]], np.int32), (len(shapes), 1))
    out = []
    for sh in (None, full):
        b = _build(scarlet, c, obs, sh, centers, n, mse_capacity=8)
        assert (b.frame_shapes is None) == (sh is None)
        b.init_combined(_bg(c.bands))
        b.fit(5, e_rel=0, check_every=3)
        out.append(_state(b))
        del b
    _assert_identical(out[0], out[1], name + ": full-size frame_shapes")     # sed, morph, mse, centres, it, flags, lipschitz
    assert (out[0]["it"] == 5).all() and not out[0]["status"].any()


# ------------------------------------------------------------------ 5. isolation
def test_copies_of_a_scene_agree_wherever_they_sit(env):
    scarlet, _ = env
    c = oc.CASES["wave"]
    obs, shapes, centers, n = oc.padded(c)
    S = 40
    order = np.random.default_rng(1).permutation(S) % len(shapes)
    tiled = [dict(o, images=o["images"][order]) for o in obs]
    b = _build(scarlet, c, tiled, shapes[order], centers[order], n[order])
    b.init_combined(_bg(c.bands))
    b.fit(6, e_rel=0)
    st = _state(b)
    assert not st["status"].any() and (st["it"] == 6).all()
    small = _make(scarlet, c)
    small.fit(6, e_rel=0)
    ss = _state(small)
    for i, src in enumerate(order):
        for key in ("sed", "morph"):
            assert np.array_equal(st[key][st["cur"][i]][i], ss[key][ss["cur"][src]][src]), (key, i, src)
        for key in ("cen", "shifts", "flags", "mse", "it", "lip"):
            assert np.array_equal(st[key][i], ss[key][src], equal_nan=True), (key, i, src)


# ------------------------------------------------------------------ 6. a bad shape on the device
def test_bad_shape_on_device(env):
    """the device check runs before any kernel of the fit reads a plane: the scene is refused and never touched"""
    scarlet, _ = env
    from scarlet_amd import _lib
    c = oc.CASES["psf"]
    S = len(c.shapes)
    out = []
    for corrupt in (False, True):
        b = _make(scarlet, c)
        if corrupt:
            b.frame_shapes[1, 1] = c.W + 1
        st0 = _state(b)
        b.fit(4, e_rel=0, check_every=3)
        b.step(e_rel=0)
        out.append((st0, _state(b)))
        if corrupt:
            with pytest.raises(ValueError, match=r"scenes \[1\]"):
                b.raise_on_status()
    (_, good), (st0, bad) = out
    assert bad["status"][1] == _lib.STATUS_BAD_FRAME and bad["active"][1] == 0 and bad["it"][1] == 0
    for key in ("sed", "morph"):
        for j in range(2):
            assert np.array_equal(bad[key][j][1], st0[key][j][1]), key
    for key in ("cen", "shifts", "flags", "mse", "cur", "lip"):
        assert np.array_equal(bad[key][1], st0[key][1], equal_nan=True), key
    keep = np.ones(S, bool)
    keep[1] = False
    assert not good["status"].any() and (good["it"] == 5).all()
    _assert_identical(good, bad, "the other scenes", keep=keep)


# ------------------------------------------------------------------ 7. products against their definition
@pytest.mark.parametrize("name", ["wave", "psf"])
def test_products_per_observation(env, name):
    """after two iterations: rendered, residual and loss of every observation and the state's model against the float64
    evaluation of each scene's cropped factors and data (tests/products_common.py); zero outside the frames; the loss is
    what the next iteration records; the call changes no bit of the state nor of the fit that follows"""
    import products_common as prc
    scarlet, _ = env
    c = oc.CASES[name]
    _, shapes, _, n = oc.padded(c)
    b = _make(scarlet, c, fill=7.0)
    b.fit(2, e_rel=0)
    before = _state(b)
    p = b.products()
    loss = b.get_loss()
    torch.cuda.synchronize()
    _assert_identical(before, _state(b), name + ": products() is read-only")
    out = _outside(shapes, c.H, c.W)
    model = p.model.cpu().numpy()
    assert not np.any(model[np.broadcast_to(out, model.shape)])
    diffs = oc.diff_kernels(c)
    for o, (b0, nb) in enumerate(c.bands):
        for key in ("rendered", "residual"):
            x = getattr(p, key)[o].cpu().numpy()
            assert x.shape == (len(shapes), nb, c.H, c.W) and np.isfinite(x).all()
            assert not np.any(x[np.broadcast_to(out, x.shape)]), "%s: observation %d %s is not zero outside the frames" % (name, o, key)
        for i in range(len(shapes)):
            h, w = shapes[i]
            sed, morph = (x.cpu().numpy() for x in b.scene(i))
            ref = prc.reference(sed[:, b0:b0 + nb], morph, oc.scene_observations(c, i)[o], 1.0, diffs[o])
            got = dict(rendered=p.rendered[o][:, :, :h, :w], residual=p.residual[o][:, :, :h, :w], loss=p.loss[o])
            prc.check_scene(got, i, ref, ("rendered", "residual", "loss"), where="ragged observations %s obs %d" % (name, o))
    for i in range(len(shapes)):
        h, w = shapes[i]
        sed, morph = (x.cpu().numpy() for x in b.scene(i))
        ref = prc.reference(sed, morph, np.zeros((c.C, h, w)))
        prc.check_scene(dict(model=p.model[:, :, :h, :w]), i, ref, ("model",), where="ragged observations %s state" % name)
    assert torch.equal(loss, sum(v.sum(dim=1) for v in p.loss))
    b.fit(1, e_rel=0)
    twin = _make(scarlet, c, fill=7.0)
    twin.fit(2, e_rel=0)
    twin.fit(1, e_rel=0)
    after = _state(b)
    _assert_identical(_state(twin), after, name + ": the fit continued after products()")
    e = rel_err(loss.cpu().numpy(), after["mse"][:, 2])
    print("%s: get_loss() against the next iteration's mse: %.2e" % (name, e))
    assert e <= TOL


# ------------------------------------------------------------------ 8. a converged run
def test_converged_run_matches_the_oracle(env):
    st = _vs_oracle(env, "wave", "ragged observations wave converged", iters=200, e_rel=1e-3)
    assert (st["active"] == 0).any(), "no scene converged within 200 iterations: the run tests nothing"
    assert (st["it"][st["active"] == 0] < 200).all()


# ------------------------------------------------------------------ 9. the refusals that need a batch
def test_refusals_on_a_ragged_joint_batch(env):
    import lowres_common as lc
    scarlet, _ = env
    from scarlet_amd import prior as sp
    c = oc.CASES["wave"]
    obs, shapes, centers, n = oc.padded(c)
    b = _make(scarlet, c)
    assert b.frame_shapes.dtype == torch.int32 and tuple(b.frame_shapes.shape) == (len(shapes), 2)
    out = _outside(shapes, c.H, c.W)
    for o, (_, ob) in zip(obs, b._observations):         # every gradient batch: masked weights, zeroed images
        assert not np.any(ob.weights.cpu().numpy()[np.broadcast_to(out, o["images"].shape)])
        assert not np.any(ob.images.cpu().numpy()[np.broadcast_to(out, o["images"].shape)])
    for call in (lambda: b.fit(1, prior=sp.QuadraticPrior(morph_weight=0.1)),
                 lambda: b.step(prior=sp.QuadraticPrior(morph_weight=0.1))):
        with pytest.raises(NotImplementedError, match="prior"):
            call()
    batches = [scarlet.ObservationBatch(o["images"], band0=o["band0"], frame_shapes=shapes) for o in obs]
    with pytest.raises(NotImplementedError, match="group"):
        scarlet.BlendBatch.from_observations(batches, centers, group=np.full((len(shapes), c.K), -1))
    with pytest.raises(NotImplementedError, match="from_observations"):
        scarlet.BlendBatch.from_observations(batches, centers, frame_shapes=shapes)
    geom, _ = lc.geometry(lc.fixture(), "a")
    lo = scarlet.LowResObservationBatch(np.zeros((2, 2, 16, 16), np.float32), band0=3, geometry=geom)
    hi = scarlet.ObservationBatch(np.zeros((2, 3, 32, 32), np.float32), frame_shapes=np.array([[32, 32], [30, 25]]))
    with pytest.raises(NotImplementedError, match="low-resolution"):
        scarlet.BlendBatch.from_observations([hi, lo], np.array([[[10, 10]], [[8, 9]]], np.int32))
    with pytest.raises(ValueError):
        b.set_state(b.sed_current, b.morph_current, centers=np.full((b.S, b.K, 2), 39, np.int32))      # outside 17 x 23
    # a ragged batch NOT made by from_observations keeps refusing init_combined
    single = scarlet.BlendBatch(np.concatenate([o["images"] for o in obs], axis=1), centers, frame_shapes=shapes)
    with pytest.raises(NotImplementedError):
        single.init_combined([np.ones(c.C) * oc.BG])
