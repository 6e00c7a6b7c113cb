"""-m gpu: catalogue batches -- BlendBatch.from_catalog / init_catalog / fit on ragged-frame scenes that hold point
sources, extended sources and multi-component sources (scarlet_init_sources_frames_mixed, scarlet_fit_frames_grouped).

Every scene must come out as the reference starts and fits the (B, h_s, w_s) scene alone.  The cases are those of
tests/catalog_cases.py; the oracle runs (each scene alone on its own frame, from the oracle's own start) are computed once
per module.  Checked here:
  1. the start: SEDs, morphologies, centres and flags of every scene against the oracle's constructors;
  2. the fit: 6 iterations at e_rel = 0 against the oracle's fit, with no exemption;
  3. identities, bit for bit: uniform cut-outs are the existing route, the _grouped entry points with full-size frames are
     the plain grouped calls, an extended-only catalogue is today's ragged route;
  4. isolation: a bad bg_rms row and a frame shape corrupted on the device leave their scene untouched and the others as
     they were;
  5. source(s, i), scene(s), products() and the other batch operations on such a batch.
Tolerance: parity_common.TOL (1e-5 relative max-norm) per scene; centres, flags, iteration counts and the shifts' NaN
pattern exact; pixels outside a frame exactly 0.0f."""
import ctypes
import multiprocessing as mp
import os

import numpy as np
import pytest

from conftest import rel_err
import catalog_cases as cc
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


@pytest.fixture(scope="module")
def oracle(env):
    """{case: [(start, fit) per scene]}: every scene alone on its own frame; computed once, read-only"""
    _, pool = env
    jobs = [(name, s, cc.ITERS, "own") for name, c in cc.CASES.items() for s in range(len(c.shapes))]
    out = {}
    for (name, s, _, _), r in zip(jobs, pool.map(cc.oracle_run, jobs)):
        out.setdefault(name, []).append(r)
    return out


def _specs(scarlet, c):
    return [[scarlet.SourceSpec(px, kind=kind, flux_percentiles=None if perc is None else list(perc)) for px, kind, perc in cat]
            for cat in cc.catalog(c)]


def _make(scarlet, c, mse_capacity=16):
    kw = {}
    if c.psf:
        kw["centroid_weight"] = cc.psfs(c)[1].astype(np.float32)
    b = scarlet.BlendBatch.from_catalog([np.array(im) for im, _ in cc.scenes(c)], _specs(scarlet, c), mse_capacity=mse_capacity, **kw)
    if c.psf:
        b.set_diff_kernel(cc.psfs(c)[2])
    return b


def _init(b, c, bg=None):
    kw = {}
    if c.psf:
        obs, model, _, _ = cc.psfs(c)
        kw = dict(obs_psfs=obs.astype(np.float32), model_psf=model.astype(np.float32))
    return b.init_catalog(np.ones(c.B) * cc.BG if bg is None else bg, **kw)


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


def _assert_outside_zero(arrays, shapes, what):
    """every array (S, n, H, W): exactly 0.0f outside each scene's own frame"""
    for i, m in enumerate(arrays):
        H, W = m.shape[-2:]
        for s, (h, w) in enumerate(shapes):
            out = np.ones((H, W), bool)
            out[:h, :w] = False
            x = m[s][..., out]
            assert np.array_equal(x, np.zeros(x.shape, np.float32)), "%s: array %d, scene %d is not zero outside its frame" % (what, i, s)


def _compare(c, st, ref, which, what):
    """the device state against the oracle snapshots `which` (0 = start, 1 = fit) of every scene"""
    assert not st["status"].any(), (what, st["status"])
    for s, (h, w) in enumerate(c.shapes):
        r = ref[s][which]
        n = cc.n_components(c, s)
        cur = st["cur"][s]
        sed, morph = st["sed"][cur][s][:n], st["morph"][cur][s][:n, :h, :w]
        e = dict(sed=rel_err(sed, r["sed"]), morph=rel_err(morph, r["morph"]))
        if which == 1:
            e["mse"] = rel_err(st["mse"][s][:st["it"][s]], r["mse"])
        print("%s scene %d %s: %s" % (what, s, (h, w), e))
        np.testing.assert_array_equal(st["cen"][s][:n], r["centers"], err_msg="%s scene %d centres" % (what, s))
        np.testing.assert_array_equal(st["flags"][s][:n], r["flags"], err_msg="%s scene %d flags" % (what, s))
        np.testing.assert_array_equal(np.isnan(st["shifts"][s][:n]).all(axis=1), r["shift_none"], err_msg="%s scene %d shifts" % (what, s))
        np.testing.assert_array_equal(np.isnan(st["shifts"][s][:n]).any(axis=1), r["shift_none"], err_msg="%s scene %d shifts" % (what, s))
        assert st["it"][s] == r["it"], (what, s, st["it"][s], r["it"])
        assert (st["flags"][s][n:] == 0).all() and not st["sed"][cur][s][n:].any() and not st["morph"][cur][s][n:].any()
        assert max(e.values()) <= TOL, "%s scene %d %s: %s" % (what, s, (h, w), e)


# ------------------------------------------------------------------ 1. the start, 2. the fit
@pytest.mark.parametrize("name", list(cc.CASES))
def test_start_and_fit_match_the_oracle_on_each_scenes_own_frame(env, oracle, name):
    scarlet, _ = env
    c = cc.CASES[name]
    b = _make(scarlet, c)
    assert (b.H, b.W) == cc.padded_shape(c) and b.frame_shapes.cpu().numpy().tolist() == [list(x) for x in c.shapes]
    _init(b, c)
    st = _state(b)
    _assert_outside_zero(st["morph"], c.shapes, name + " after init_catalog")
    _compare(c, st, oracle[name], 0, "catalogue %s start" % name)
    assert b.fit(cc.ITERS, e_rel=0) is not None
    st = _state(b)
    _assert_outside_zero(st["morph"], c.shapes, name + " after fit")
    _compare(c, st, oracle[name], 1, "catalogue %s fit" % name)
    assert (st["it"] == cc.ITERS).all()
    b.raise_on_status()


# ------------------------------------------------------------------ 3. identities
def _uniform_wave(name, catalog=None, shapes=None):
    c = cc.CASES["wave"]
    return c._replace(name=name, shapes=((40, 40),) * len(c.shapes) if shapes is None else shapes,
                      catalog=c.catalog if catalog is None else catalog)


def _existing_route(scarlet, c, images):
    """BlendBatch(images, centers, group=, n_components=) + init_sources(kind=, flux_percentiles=): the route that uniform
    frames have always had, from the arrays a user would write down for the catalogue"""
    from scarlet_amd.batch import catalog_arrays
    t = catalog_arrays(np.array(c.shapes), _specs(scarlet, c))
    b = scarlet.BlendBatch(images, t["centers"], group=t["group"], n_components=t["n_components"], mse_capacity=16)
    kind = np.where(t["kind"] == scarlet._lib.INIT_POINT, "point", "extended")
    return b, kind, t["percentiles"]


def test_uniform_cutouts_are_the_existing_route_bit_for_bit(env):
    scarlet, _ = env
    c = _uniform_wave("wave_uniform")
    images = np.stack([np.array(im) for im, _ in cc.scenes(c)])
    bg = np.ones(c.B) * cc.BG
    runs = []
    for cutouts in (images, list(images)):           # a block, and a list of equal shapes
        b = scarlet.BlendBatch.from_catalog(cutouts, _specs(scarlet, c), mse_capacity=16)
        assert b.frame_shapes is None
        b.init_catalog(bg)
        b.fit(cc.ITERS, e_rel=0)
        runs.append(_state(b))
    b, kind, perc = _existing_route(scarlet, c, images)
    b.init_sources(bg, kind=kind, flux_percentiles=perc)
    b.fit(cc.ITERS, e_rel=0)
    ref = _state(b)
    assert (ref["it"] == cc.ITERS).all() and not ref["status"].any()
    _assert_identical(ref, runs[0], "from_catalog(block) against the existing route")
    _assert_identical(ref, runs[1], "from_catalog(list of equal shapes) against the existing route")


def test_grouped_entry_points_with_full_size_frames_are_the_plain_grouped_calls(env):
    scarlet, _ = env
    _lib = scarlet._lib
    c = _uniform_wave("wave_uniform")
    images = np.stack([np.array(im) for im, _ in cc.scenes(c)])
    bg = np.ones(c.B) * cc.BG
    out = []
    for grouped in (False, True):
        b, kind, perc = _existing_route(scarlet, c, images)
        b.init_sources(bg, kind=kind, flux_percentiles=perc, run_update=False)
        hw = torch.tensor([[b.H, b.W]] * b.S, dtype=torch.int32, device=b.device).contiguous()
        f = _lib.ScarletFrames()
        f.frame_hw = hw.data_ptr()
        if grouped:
            _lib.check(_lib.lib.scarlet_source_update_frames_grouped(ctypes.byref(b._c), ctypes.byref(f), ctypes.byref(b._cons), 0,
                                                                     _lib.stream_ptr()))
        else:
            b.update_sources()
        st0 = _state(b)
        if grouped:
            _lib.check(_lib.lib.scarlet_fit_frames_grouped(ctypes.byref(b._c), ctypes.byref(f), ctypes.byref(b._cons), cc.ITERS, 0.0,
                                                           0, 10, _lib.stream_ptr()))
        else:
            b.fit(cc.ITERS, e_rel=0)
        out.append((st0, _state(b)))
        del hw
    assert (out[0][1]["it"] == cc.ITERS).all() and not out[0][1]["status"].any()
    _assert_identical(out[0][0], out[1][0], "scarlet_source_update_frames_grouped with H x W frames")
    _assert_identical(out[0][1], out[1][1], "scarlet_fit_frames_grouped with H x W frames")


def test_extended_only_catalogue_is_todays_ragged_route(env):
    scarlet, _ = env
    E = cc.E
    w = cc.CASES["wave"]
    c = _uniform_wave("wave_extended", catalog=((E, E), (E, E), (E, E), (E,), (E,), (E, E)), shapes=w.shapes)
    cutouts = [np.array(im) for im, _ in cc.scenes(c)]
    bg = np.ones(c.B) * cc.BG
    b = scarlet.BlendBatch.from_catalog(cutouts, _specs(scarlet, c), mse_capacity=16)
    assert b.group is None and b.frame_shapes is not None
    b.init_catalog(bg)
    b.fit(cc.ITERS, e_rel=0)
    got = _state(b)
    ref_b = scarlet.BlendBatch(cutouts, [cen for _, cen in cc.scenes(c)], mse_capacity=16)
    ref_b.init_extended(bg)
    ref_b.fit(cc.ITERS, e_rel=0)
    ref = _state(ref_b)
    assert (ref["it"] == cc.ITERS).all() and not ref["status"].any()
    _assert_identical(ref, got, "extended-only catalogue against BlendBatch(list) + init_extended + fit")


# ------------------------------------------------------------------ 4. isolation
def test_a_bad_scene_leaves_the_others_as_they_were(env):
    scarlet, _ = env
    _lib = scarlet._lib
    c = cc.CASES["wave"]
    S = len(c.shapes)
    bg = np.full((S, c.B), cc.BG, np.float32)

    def run(bad_bg=None, bad_frame=None):
        b = _make(scarlet, c)
        rows = bg.copy()
        if bad_bg is not None:
            rows[bad_bg, 1] = 0
        if bad_frame is not None:
            b.frame_shapes[bad_frame, 1] = b.W + 1            # corrupted on the device, after the host checks
        st0 = _state(b)
        _init(b, c, rows)
        st1 = _state(b)
        b.fit(cc.ITERS, e_rel=0)
        return b, st0, st1, _state(b)

    _, _, good1, good = run()
    assert not good["status"].any() and (good["it"] == cc.ITERS).all()
    for kw, bit, word in ((dict(bad_bg=0), _lib.STATUS_BAD_INIT, "init_sources"), (dict(bad_frame=2), _lib.STATUS_BAD_FRAME, "frame_shapes")):
        bad = list(kw.values())[0]
        b, st0, st1, st = run(**kw)
        keep = np.arange(S) != bad
        assert ((st["status"] & bit) != 0).tolist() == [s == bad for s in range(S)], st["status"]
        assert st["active"][bad] == 0 and st["it"][bad] == 0
        for key in ("sed", "morph", "cen", "shifts", "flags", "mse", "lip"):       # the scene was not touched
            xs, ys = (st0[key], st[key]) if isinstance(st[key], list) else ([st0[key]], [st[key]])
            for x, y in zip(xs, ys):
                assert np.array_equal(x[bad], y[bad], equal_nan=True), (kw, key)
        for a, r, when in ((st1, good1, "after init_catalog"), (st, good, "after fit")):
            for key in ("sed", "morph", "cen", "shifts", "flags", "mse", "it", "cur", "lip"):
                xs, ys = (a[key], r[key]) if isinstance(a[key], list) else ([a[key]], [r[key]])
                for x, y in zip(xs, ys):
                    assert np.array_equal(x[keep], y[keep], equal_nan=True), (kw, key, when)
        with pytest.raises(ValueError, match=r"%s.*\[%d\]" % (word, bad)):
            b.raise_on_status()
        frames = [tuple(x) for x in c.shapes]
        _assert_outside_zero(st["morph"], frames, "isolation %s" % kw)


# ------------------------------------------------------------------ 5. the batch's other operations
def test_source_scene_products_and_the_other_operations(env):
    scarlet, _ = env
    c = cc.CASES["wave"]
    b = _make(scarlet, c)
    _init(b, c)
    b.fit(cc.ITERS - 1, e_rel=0)
    b.step(e_rel=0)
    torch.cuda.synchronize()
    assert b.it.cpu().numpy().tolist() == [cc.ITERS] * b.S and not b.status.cpu().numpy().any()
    p = b.products()
    for s, (h, w) in enumerate(c.shapes):
        n = cc.n_components(c, s)
        sed, morph = b.scene(s)
        assert tuple(sed.shape) == (n, c.B) and tuple(morph.shape) == (n, h, w)
        k = 0
        for i, (_, kind, perc) in enumerate(cc.catalog(c)[s]):
            layers = 1 if perc is None else len(perc) + 1
            ssed, smorph = b.source(s, i)
            assert tuple(ssed.shape) == (layers, c.B) and tuple(smorph.shape) == (layers, h, w)
            assert torch.equal(ssed, sed[k:k + layers]) and torch.equal(smorph, morph[k:k + layers])
            k += layers
        assert k == n and len(b.sources[s]) == len(c.catalog[s])
        model = torch.einsum("kb,kyx->byx", sed.double(), morph.double()).cpu().numpy()
        # float32 products summed over at most 4 components: 4 roundings of 2^-24 each
        assert rel_err(p.model[s, :, :h, :w].cpu().numpy(), model) <= 4 * 2.0 ** -24 * 2
    for name in ("model", "rendered", "residual"):
        _assert_outside_zero([getattr(p, name).cpu().numpy()], c.shapes, "products " + name)
    assert torch.equal(b.get_model(), p.model) and torch.isfinite(p.loss).all() and torch.isfinite(p.flux).all()
    # the state can be loaded back, sources frozen, and the fit goes on with the approximate Lipschitz constants
    sed, morph = b.sed_current.clone(), b.morph_current.clone()
    b2 = _make(scarlet, c)
    b2.set_state(sed, morph, centers=b.centers.cpu().numpy(), shifts=b.shifts.cpu().numpy())
    b2.fix_sed = torch.zeros((b2.S, b2.K), dtype=torch.uint8, device=b2.device)
    b2.fix_sed[:, 0] = 1
    b2._fill_struct()
    b2.fit(2, e_rel=0, approximate_L=True)
    torch.cuda.synchronize()
    assert b2.it.cpu().numpy().tolist() == [2] * b2.S and not b2.status.cpu().numpy().any()
    assert torch.isfinite(b2.sed_current).all() and torch.isfinite(b2.morph_current).all()
    _assert_outside_zero([t.cpu().numpy() for t in b2.morph], c.shapes, "after set_state + fit")
    # what stays refused
    with pytest.raises(NotImplementedError):
        b.fit(1, prior={})
