"""-m gpu: catalogue batches whose sources carry the stock update functions' options -- BlendBatch.from_catalog with
SourceSpec options or update=, init_catalog, fit, step on ragged-frame scenes with point, extended and multi-component
sources (scarlet_fit_frames_options, scarlet_source_update_frames_options: the RAGGED x OPTIONS instances of the constraint
kernels).

Every scene must come out as the composed oracle of tests/catalog_option_cases.py runs it alone on its own frame.
  (a) every case x option set: init_catalog, 6 iterations at e_rel = 0 against the oracle from the batch's own start; one
      converged run (wave, soft, e_rel = 1e-3);
  (b) init_catalog alone against the oracle's constructors plus the composed update at it = 0;
  (c) update=UpdateOptions() gives the bits of the same catalogue without options, on every form, both on the general path;
  (d) batches without the new route give the bits the parent commit gave (tests/golden/catalog_options_parent_bits.json);
  (e) copies of one ragged scene with different option rows, tiled to 64 scenes, agree per row wherever they sit;
  (f) options corrupted on the device: STATUS_BAD_OPTION, the scene untouched, the others as in the clean run; a scene with a
      bad frame entry and a bad option carries both bits;
  (g) the nearest-neighbour sweep and sdss symmetry alone on ragged frames through scarlet_source_update_frames_options,
      bit-exact against the oracle's operators on the cropped scene;
  (h) pixels outside each frame are exactly zero in both morphology buffers after init and after every fit (asserted in
      (a), (b), (f)), and in products();
  (i) uniform cut-outs with a multi source and options against the composed oracle.
Tolerance: parity_common.TOL (1e-5 relative max-norm) per scene for SEDs, morphologies and the loss history; centres,
iteration counts, flags and the shifts' NaN pattern exact; no exemption."""
import ctypes
import json
import multiprocessing as mp
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import rel_err
import catalog_option_cases as oc
import frame_cases as fc
import parity_common as pc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
TOL = pc.TOL
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTSETS = list(oc.OPTION_SETS)


@pytest.fixture(scope="module")
def env():
    import scarlet_amd
    scarlet_amd._lib.require_gpu()
    from oracle import build as obuild
    obuild.build()
    pool = mp.get_context("spawn").Pool(min(16, os.cpu_count() or 1))
    yield scarlet_amd, pool
    pool.close(); pool.join()


def _specs(scarlet, c, optset):
    return [[scarlet.SourceSpec(px, kind=kind, flux_percentiles=None if perc is None else list(perc), **oc.spec_kwargs(optset, i))
             for i, (px, kind, perc) in enumerate(cat)] for cat in oc.catalog(c)]


def _make(scarlet, c, optset, mse_capacity=16, specs=None, cutouts=None, **kw):
    if c.psf:
        kw["centroid_weight"] = oc.psfs(c)[1].astype(np.float32)
    b = scarlet.BlendBatch.from_catalog([np.array(im) for im, _ in oc.scenes(c)] if cutouts is None else cutouts,
                                        _specs(scarlet, c, optset) if specs is None else specs, mse_capacity=mse_capacity, **kw)
    if c.psf:
        b.set_diff_kernel(oc.psfs(c)[2])
    return b


def _init(b, c):
    kw = {}
    if c.psf:
        obs, model, _, _ = oc.psfs(c)
        kw = dict(obs_psfs=obs.astype(np.float32), model_psf=model.astype(np.float32))
    return b.init_catalog(np.ones(c.B) * oc.BG, **kw)


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
            assert x.tobytes() == y.tobytes(), "%s: %s[%d] differs" % (what, key, i)


def _assert_outside_zero(arrays, shapes, what):
    """every array (S, n, H, W): exactly 0.0f outside each scene's own frame"""
    for i, m in enumerate(arrays):
        H, W = m.shape[-2:]
        for s, (h, w) in enumerate(shapes):
            out = np.ones((H, W), bool)
            out[:h, :w] = False
            x = m[s][..., out]
            assert x.tobytes() == np.zeros(x.shape, np.float32).tobytes(), "%s: array %d, scene %d is not zero outside its frame" % (what, i, s)


def _scene_state(c, st, s):
    """the current factors of scene s on its own frame, as the oracle takes them"""
    h, w = c.shapes[s]
    n = oc.n_components(c, s)
    cur = st["cur"][s]
    return dict(sed=st["sed"][cur][s][:n].copy(), morph=st["morph"][cur][s][:n, :h, :w].copy(), cen=st["cen"][s][:n].copy(),
                shifts=st["shifts"][s][:n].copy())


def _compare(c, st, refs, what, fit=True):
    """the device state against the oracle results `refs` (one per scene)"""
    assert not st["status"].any(), (what, st["status"])
    for s, (h, w) in enumerate(c.shapes):
        r = refs[s]
        n = oc.n_components(c, s)
        g = _scene_state(c, st, s)
        e = dict(sed=rel_err(g["sed"], r["sed"]), morph=rel_err(g["morph"], r["morph"]))
        if fit:
            e["mse"] = rel_err(st["mse"][s][:st["it"][s]], r["mse"])
        print("%s scene %d %s: %s" % (what, s, (h, w), {k: "%.2e" % v for k, v in e.items()}))
        np.testing.assert_array_equal(g["cen"], r["cen"], err_msg="%s scene %d centres" % (what, s))
        np.testing.assert_array_equal(np.isnan(g["shifts"]), np.isnan(r["shifts"]), err_msg="%s scene %d shifts" % (what, s))
        if fit:
            np.testing.assert_array_equal(st["flags"][s][:n], r["flags"], err_msg="%s scene %d flags" % (what, s))
            assert st["it"][s] == r["it"], (what, s, st["it"][s], r["it"])
        else:
            np.testing.assert_allclose(np.nan_to_num(g["shifts"]), np.nan_to_num(r["shifts"]), rtol=0, atol=1e-5)
        cur = st["cur"][s]
        assert (st["flags"][s][n:] == 0).all() and not st["sed"][cur][s][n:].any() and not st["morph"][cur][s][n:].any()
        assert max(e.values()) <= TOL, "%s scene %d %s: %s" % (what, s, (h, w), e)


def _oracle_fit(pool, key, c, optset, st0, iters=oc.ITERS, e_rel=0.0):
    jobs = [(key, s, optset, _scene_state(c, st0, s), iters, e_rel, "float32", "own") for s in range(len(c.shapes))]
    return [r for _, r in pool.map(oc.oracle_job, jobs)]


# ------------------------------------------------------------------ (a), (h)
@pytest.mark.parametrize("optset", OPTSETS)
@pytest.mark.parametrize("key", list(oc.CASES))
def test_fit_matches_the_composed_oracle_on_each_scenes_own_frame(env, key, optset):
    scarlet, pool = env
    c = oc.CASES[key]
    b = _make(scarlet, c, optset)
    assert b._catalog_options and b.frame_shapes is not None and b.group is not None
    assert (b.H, b.W) == oc.padded_shape(c) and fc.update_form(b.H, b.W) == ("wave" if key == "psf" else key)
    _init(b, c)
    st0 = _state(b)
    _assert_outside_zero(st0["morph"], c.shapes, "%s / %s after init_catalog" % (key, optset))
    assert b.fit(oc.ITERS, e_rel=0) is not None
    st = _state(b)
    _assert_outside_zero(st["morph"], c.shapes, "%s / %s after fit" % (key, optset))
    _compare(c, st, _oracle_fit(pool, key, c, optset, st0), "%s / %s fit" % (key, optset))
    assert (st["it"] == oc.ITERS).all()
    b.raise_on_status()


def test_converged_run(env):
    """wave, soft, e_rel = 1e-3: every scene stops where the oracle stops; the scene of one component cycles with period 2
    and reaches the cap in the oracle too (tests/test_catalog_option_cases.py test_converged_run_is_admissible)"""
    scarlet, pool = env
    c = oc.CASES["wave"]
    b = _make(scarlet, c, "soft", mse_capacity=oc.CONVERGED_CAP + 1)
    _init(b, c)
    st0 = _state(b)
    b.fit(oc.CONVERGED_CAP, e_rel=1e-3, check_every=10)
    st = _state(b)
    for s in range(len(c.shapes)):
        if oc.one_component(c, s):
            assert st["it"][s] == oc.CONVERGED_CAP and st["active"][s] == 1
        else:
            assert st["active"][s] == 0 and 2 < st["it"][s] < oc.CONVERGED_CAP and (st["flags"][s] == 0).all()
    _assert_outside_zero(st["morph"], c.shapes, "converged run")
    _compare(c, st, _oracle_fit(pool, "wave", c, "soft", st0, oc.CONVERGED_CAP, 1e-3), "wave / soft converged")


# ------------------------------------------------------------------ (b)
@pytest.mark.parametrize("optset", OPTSETS)
@pytest.mark.parametrize("key", list(oc.CASES))
def test_init_catalog_runs_the_constructors_update_with_the_options(env, key, optset):
    scarlet, pool = env
    c = oc.CASES[key]
    b = _make(scarlet, c, optset)
    _init(b, c)
    st = _state(b)
    assert (st["it"] == 0).all() and (st["cur"] == 0).all()
    _assert_outside_zero(st["morph"], c.shapes, "%s / %s start" % (key, optset))
    refs = pool.starmap(oc.oracle_start, [(c, s, optset) for s in range(len(c.shapes))])
    _compare(c, st, refs, "%s / %s start" % (key, optset), fit=False)


# ------------------------------------------------------------------ (c)
PROFILE_CLASSES = ["k_grad", "k_step", "k_source_update", "k_converge", "k_iterate", "psf_convolution", "k_prior_step"]


def _general_path(b):
    """scarlet_debug_fused_plan for the batch's struct, frames and constraints: no one-launch iteration.  (The query has no
    options argument: for a batch with options it says what the batch would take WITHOUT them; with them fit_call takes its
    options branch, the general step, before it looks at the plan -- `_fit_counting_launches` shows that on the device.)"""
    from scarlet_amd import _lib
    plan = (ctypes.c_int32 * 8)()
    assert _lib.lib.scarlet_debug_fused_plan(ctypes.byref(b._c), ctypes.byref(b._frames), ctypes.byref(b._cons), 0, 5,
                                             ctypes.cast(plan, ctypes.c_void_p)) == 0
    return plan[0] == 0


def _fit_counting_launches(b, iters):
    """fit(iters) between scarlet_profile_begin / _end: {kernel class: launches}"""
    from scarlet_amd import _lib
    _lib.check(_lib.lib.scarlet_profile_begin(iters + 1))
    b.fit(iters, e_rel=0)
    torch.cuda.synchronize()
    tot, cnt = (ctypes.c_double * 8)(), (ctypes.c_int64 * 8)()
    _lib.check(_lib.lib.scarlet_profile_end(tot, cnt))
    return {name: int(cnt[i]) for i, name in enumerate(PROFILE_CLASSES) if cnt[i]}


@pytest.mark.parametrize("key", list(oc.CASES))
def test_default_options_give_the_bits_of_no_options(env, key):
    scarlet, _ = env
    c = oc.CASES[key]
    plain = _make(scarlet, c, None)
    assert not plain._catalog_options and plain._upd is None and plain.group is not None
    opts = _make(scarlet, c, None, update=scarlet.UpdateOptions())
    assert opts._catalog_options and all(getattr(opts._upd, f) for f in scarlet.UpdateOptions.FIELDS)
    assert _general_path(plain) and _general_path(opts), "both batches must take the general path"
    _init(plain, c)
    _init(opts, c)
    _assert_identical(_state(plain), _state(opts), "%s after init_catalog" % key)
    launches = [_fit_counting_launches(plain, 5), _fit_counting_launches(opts, 5)]
    print("%s: launches of 5 iterations without / with options: %s" % (key, launches))
    for n in launches:           # the general path on the device: a constraint launch per iteration, no one-launch iteration
        assert "k_iterate" not in n and n.get("k_source_update", 0) >= 5, n
    a, b = _state(plain), _state(opts)
    assert (a["it"] == 5).all() and not a["status"].any()
    _assert_identical(a, b, "%s after 5 iterations" % key)


def test_step_is_one_iteration_of_fit_and_the_other_operations(env):
    scarlet, _ = env
    c = oc.CASES["wave"]
    a, b = _make(scarlet, c, "mixed"), _make(scarlet, c, "mixed")
    _init(a, c)
    _init(b, c)
    a.fit(2, e_rel=0)
    b.step(e_rel=0)
    b.step(e_rel=0)
    _assert_identical(_state(a), _state(b), "two steps against fit(2)")
    # (h) products of such a batch: the model of the current factors, zero outside every frame
    p = b.products()
    for s, (h, w) in enumerate(c.shapes):
        sed, morph = b.scene(s)
        assert tuple(morph.shape) == (oc.n_components(c, s), h, w)
        ssed, smorph = b.source(s, 0)
        assert torch.equal(smorph, morph[:smorph.shape[0]]) and torch.equal(ssed, sed[:ssed.shape[0]])
        model = torch.einsum("kb,kyx->byx", sed.double(), morph.double()).cpu().numpy()
        assert rel_err(p.model[s, :, :h, :w].cpu().numpy(), model) <= 4 * 2.0 ** -24 * 2
    for name in ("model", "rendered", "residual"):
        _assert_outside_zero([getattr(p, name).cpu().numpy()], c.shapes, "products " + name)
    assert torch.equal(b.get_model(), p.model) and torch.isfinite(p.loss).all() and torch.isfinite(p.flux).all()
    # the state can be loaded back, a SED frozen, and the fit goes on with the approximate Lipschitz constants
    b2 = _make(scarlet, c, "mixed")
    b2.set_state(b.sed_current.clone(), b.morph_current.clone(), centers=b.centers.cpu().numpy(), shifts=b.shifts.cpu().numpy())
    b2.fix_sed = torch.zeros((b2.S, b2.K), dtype=torch.uint8, device=b2.device)
    b2.fix_sed[:, 0] = 1
    b2._fill_struct()
    b2.fit(2, e_rel=0, approximate_L=True)
    torch.cuda.synchronize()
    assert b2.it.cpu().numpy().tolist() == [2] * b2.S and not b2.status.cpu().numpy().any()
    assert torch.isfinite(b2.sed_current).all() and torch.isfinite(b2.morph_current).all()
    _assert_outside_zero([t.cpu().numpy() for t in b2.morph], c.shapes, "after set_state + fit")
    # what stays refused
    prior = scarlet.QuadraticPrior(morph_weight=0.1)
    for call in (lambda: b.fit(1, prior=prior), lambda: b.step(prior=prior)):
        with pytest.raises(NotImplementedError):
            call()


# ------------------------------------------------------------------ (d)
_HASH_SCRIPT = r"""
import hashlib, sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import torch
import scarlet_amd as scarlet
import catalog_cases as cc, frame_cases as fc, update_option_cases as uc

def digest(b):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in (b.sed[0], b.sed[1], b.morph[0], b.morph[1], b.cur, b.centers, b.shifts, b.mse_buf, b.flags, b.it, b.status):
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()

out = []
c = cc.CASES["wave"]                       # a grouped ragged catalogue
specs = [[scarlet.SourceSpec(px, kind=kind, flux_percentiles=None if perc is None else list(perc)) for px, kind, perc in cat]
         for cat in cc.catalog(c)]
b = scarlet.BlendBatch.from_catalog([np.array(im) for im, _ in cc.scenes(c)], specs, mse_capacity=16)
b.init_catalog(np.ones(c.B) * cc.BG)
b.fit(6, e_rel=0)
out.append(digest(b))
for name in ("tile", "plane"):             # a ragged BlendBatch on the tile and plane forms
    c = fc.CASES[name]
    images, shapes, centers, counts = fc.padded(c)
    b = scarlet.BlendBatch(images, centers, frame_shapes=shapes, n_components=None if (counts == c.K).all() else counts, mse_capacity=16)
    b.init_extended(np.ones(c.B) * fc.BG)
    b.fit(6, e_rel=0)
    out.append(digest(b))
c = uc.CASES["tile"]                       # a uniform options batch
images, centers = uc.stacked(c)
b = scarlet.BlendBatch(images, centers, update=scarlet.UpdateOptions(**uc.update_kwargs("mixed", c.K)), mse_capacity=16)
b.init_extended(np.ones(c.B) * uc.BG)
b.fit(6, e_rel=0)
out.append(digest(b))
print("HASHES " + " ".join(out))
"""


def _hashes(root=ROOT):
    """the digests of the script above, run in a fresh process against the package under `root` (the cases come from this
    tree's tests/: the three case files are unchanged since the parent)"""
    env_ = dict(os.environ)
    env_.pop("SCARLET_LIB_PATH", None)
    out = subprocess.check_output([sys.executable, "-c", _HASH_SCRIPT % (os.path.join(ROOT, "tests"), root)], env=env_, timeout=300).decode()
    return [ln for ln in out.splitlines() if ln.startswith("HASHES ")][0].split()[1:]


def test_batches_without_the_new_route_keep_their_bits(env):
    """a grouped ragged catalogue, a ragged BlendBatch on the tile and plane forms and a uniform options batch, 6 iterations
    in a fresh process: the digests of the whole state (both buffers) equal those the parent commit gave
    (tests/golden/catalog_options_parent_bits.json, recorded on an MI355X by running the same script against the parent's
    tree and library)"""
    with open(os.path.join(ROOT, "tests", "golden", "catalog_options_parent_bits.json")) as f:
        want = json.load(f)["sha256"]
    assert _hashes() == want


# ------------------------------------------------------------------ (e)
def test_option_rows_travel_with_their_scenes(env):
    """scene 0 of the wave case (40 x 40) in front of 63 copies of its 40 x 27 scene (a multi and a point source), each copy
    with the options of one set: the padded frame is 40 x 40, the copies are ragged"""
    scarlet, _ = env
    c = oc.CASES["wave"]
    sc, cat = oc.scenes(c), oc.catalog(c)
    assert c.shapes[0] == (40, 40) and c.shapes[2] == (40, 27)
    S, names = 64, [None] + OPTSETS
    row = np.array([(7 * s + s // 8) % len(names) for s in range(S)])          # every set, at scattered places
    row[0] = 0
    assert set(row[1:]) == set(range(len(names)))

    def spec(s, optset):
        return [scarlet.SourceSpec(px, kind=kind, flux_percentiles=None if perc is None else list(perc), **oc.spec_kwargs(optset, i))
                for i, (px, kind, perc) in enumerate(cat[s])]

    cutouts = [np.array(sc[0][0])] + [np.array(sc[2][0])] * (S - 1)
    b = _make(scarlet, c, None, specs=[spec(0, None)] + [spec(2, names[r]) for r in row[1:]], cutouts=cutouts)
    assert b._catalog_options and b.frame_shapes is not None and (b.H, b.W) == (40, 40)
    _init(b, c)
    b.fit(oc.ITERS, e_rel=0)
    g = _state(b)
    assert not g["status"].any() and (g["it"] == oc.ITERS).all()
    _assert_outside_zero(g["morph"], [(40, 40)] + [(40, 27)] * (S - 1), "tiled")
    firsts = []
    for r in range(len(names)):
        idx = np.nonzero(row[1:] == r)[0] + 1
        assert len(idx) >= 2
        for s in idx[1:]:
            for k in ("sed", "morph"):
                for i in range(2):
                    assert g[k][i][s].tobytes() == g[k][i][idx[0]].tobytes(), (names[r], int(s), k)
            for k in ("cen", "shifts", "flags", "mse", "lip", "cur"):
                assert g[k][s].tobytes() == g[k][idx[0]].tobytes(), (names[r], int(s), k)
        firsts.append(idx[0])
    for i in range(len(firsts)):             # ... and the rows differ from each other
        for j in range(i):
            assert g["morph"][0][firsts[i]].tobytes() != g["morph"][0][firsts[j]].tobytes(), (names[i], names[j])


# ------------------------------------------------------------------ (f)
def test_corrupted_options_mark_the_scene_and_nothing_else(env):
    scarlet, _ = env
    _lib = scarlet._lib
    c = oc.CASES["wave"]
    S = len(c.shapes)

    def run(corrupt):
        b = _make(scarlet, c, "mixed")
        if corrupt:              # on the device, after the host checks: scene 4 before anything ran ...
            b.update_options["mono_thresh"][4, 1] = 1.5
            b.frame_shapes[4, 1] = b.W + 1
        st0 = _state(b)
        _init(b, c)
        if corrupt:              # ... scene 1 between init_catalog and the fit
            b.update_options["sym_algorithm"][1, 0] = 7
        st1 = _state(b)
        b.fit(5, e_rel=0)
        return b, st0, st1, _state(b)

    _, _, good1, good = run(False)
    assert not good["status"].any() and (good["it"] == 5).all()
    b, st0, st1, st = run(True)
    both = _lib.STATUS_BAD_OPTION | _lib.STATUS_BAD_FRAME
    assert st1["status"].tolist() == [both if s == 4 else 0 for s in range(S)], st1["status"]      # both bits from the first call on
    assert st["status"].tolist() == [{1: _lib.STATUS_BAD_OPTION, 4: both}.get(s, 0) for s in range(S)], st["status"]
    for bad, before in ((1, st1), (4, st0)):
        assert st["active"][bad] == 0 and st["it"][bad] == 0
        for key in ("sed", "morph", "cen", "shifts", "flags", "mse", "lip", "cur"):       # the scene was not touched, padding included
            xs, ys = (before[key], st[key]) if isinstance(st[key], list) else ([before[key]], [st[key]])
            for x, y in zip(xs, ys):
                assert x[bad].tobytes() == y[bad].tobytes(), (bad, key)
    for a, r, when, keep in ((st1, good1, "after init_catalog", [0, 1, 2, 3, 5]), (st, good, "after fit", [0, 2, 3, 5])):
        for key in ("sed", "morph", "cen", "shifts", "flags", "mse", "it", "cur", "lip", "active"):
            xs, ys = (a[key], r[key]) if isinstance(a[key], list) else ([a[key]], [r[key]])
            for x, y in zip(xs, ys):
                assert x[keep].tobytes() == y[keep].tobytes(), (key, when)
    _assert_outside_zero(st["morph"], c.shapes, "isolation")
    with pytest.raises(ValueError, match=r"update options of scenes \[1, 4\].*BAD_OPTION"):
        b.raise_on_status()


# ------------------------------------------------------------------ (g)
def _ragged_operator_batch(scarlet, shape, n, symmetric, monotonic, fields):
    """n one-component scenes of random own frames inside `shape`, random planes with the largest value on the centre, and
    a scarlet_update_options with `fields`; returns (batch, planes, frames, centres, keep-alive)"""
    H, W = shape
    rng = np.random.Generator(np.random.PCG64(H * 1000 + W + 7))
    frames = np.stack([rng.integers(H // 2, H + 1, size=n), rng.integers(W // 2, W + 1, size=n)], axis=1).astype(np.int32)
    frames[0] = (H, W)
    frames[1] = (H - 3, (W - 4) // 4 * 4)                                          # w % 4 == 0, w < W
    frames[2] = (H - 1, W - 5)
    cen = np.stack([rng.integers(0, frames[:, 0]), rng.integers(0, frames[:, 1])], axis=1).astype(np.int32)
    for i in range(3, min(n, 9)):           # the own frame's last row and column, its corners and edges
        h, w = frames[i]
        cen[i] = [(h - 1, w - 1), (0, 0), (0, w - 1), (h - 1, 0), (h - 1, 3), (5, w - 1)][i - 3]
    planes = np.zeros((n, 1, H, W), np.float32)
    for i, ((h, w), (cy, cx)) in enumerate(zip(frames, cen)):
        planes[i, 0, :h, :w] = rng.normal(0.3, 1.0, size=(h, w)).astype(np.float32)
        planes[i, 0, cy, cx] = 10.0 + i
    b = scarlet.BlendBatch(np.zeros((n, 1, H, W), np.float32), cen[:, None, :], frame_shapes=frames, symmetric=symmetric,
                           monotonic=monotonic)
    b.set_state(np.ones((n, 1, 1), np.float32), planes)
    upd = scarlet._lib.ScarletUpdateOptions()
    keep = []
    for name, (value, dtype) in fields.items():
        t = torch.full((n, 1), value, dtype=dtype, device=b.device).contiguous()
        keep.append(t)
        setattr(upd, name, t.data_ptr())
    return b, planes, frames, cen, upd, keep


SHAPES_G = [((40, 40), 32), ((72, 80), 24), ((96, 96), 16), ((oc.PLANE_SIDE, oc.PLANE_SIDE), 16)]


@pytest.mark.parametrize("shape, n", SHAPES_G)
def test_nearest_sweep_alone_on_ragged_frames_is_bit_exact(env, shape, n):
    """everything else of the pipeline off (no symmetry, no positivity, no normalisation); max_pixel keeps the centre"""
    from oracle import pgm
    scarlet, _ = env
    _lib = scarlet._lib
    b, planes, frames, cen, upd, keep = _ragged_operator_batch(
        scarlet, shape, n, False, True, dict(mono_nearest=(1, torch.uint8), positive=(0, torch.uint8), normalize=(_lib.NORM_NONE, torch.uint8)))
    _lib.check(_lib.lib.scarlet_source_update_frames_options(ctypes.byref(b._c), ctypes.byref(b._frames), ctypes.byref(b._cons),
                                                             ctypes.byref(upd), 0, _lib.stream_ptr()))
    g = _state(b)
    assert (g["status"] & ~_lib.STATUS_CENTER_AT_EDGE == 0).all()
    np.testing.assert_array_equal(g["cen"][:, 0], cen)
    assert (g["sed"][0] == 1).all()
    _assert_outside_zero([g["morph"][0]], [tuple(f) for f in frames], "nearest sweep")
    for i, (h, w) in enumerate(frames):
        want = pgm.prox_nearest_monotonic(planes[i, 0, :h, :w].astype(np.float64), cen[i]).astype(np.float32)
        assert g["morph"][0][i, 0, :h, :w].tobytes() == want.tobytes(), (i, (h, w), cen[i])


@pytest.mark.parametrize("shape, n", SHAPES_G)
def test_sdss_symmetry_alone_on_ragged_frames_is_bit_exact(env, shape, n):
    """symmetric, not monotonic, no positivity, no normalisation: max_pixel, the centroid (it = 0) and the sdss symmetry about
    the centre it gives, on the scene's own window"""
    from oracle import pgm
    scarlet, _ = env
    _lib = scarlet._lib
    b, planes, frames, cen, upd, keep = _ragged_operator_batch(
        scarlet, shape, n, True, False, dict(sym_algorithm=(_lib.SYM_SDSS, torch.uint8), positive=(0, torch.uint8),
                                             normalize=(_lib.NORM_NONE, torch.uint8)))
    _lib.check(_lib.lib.scarlet_source_update_frames_options(ctypes.byref(b._c), ctypes.byref(b._frames), ctypes.byref(b._cons),
                                                             ctypes.byref(upd), 0, _lib.stream_ptr()))
    g = _state(b)
    assert (g["status"] & ~_lib.STATUS_CENTER_AT_EDGE == 0).all()
    _assert_outside_zero([g["morph"][0]], [tuple(f) for f in frames], "sdss symmetry")
    cw = pgm.default_centroid_weight()
    for i, (h, w) in enumerate(frames):
        m = planes[i, 0, :h, :w].copy()
        edge = cen[i][0] < 2 or cen[i][1] < 2          # max_pixel's window starts before the frame: the reference fails, the device flags
        assert bool(g["status"][i] & _lib.STATUS_CENTER_AT_EDGE) == edge, (i, cen[i])
        c0 = tuple(int(v) for v in cen[i]) if edge else pgm.max_pixel(m, cen[i])
        c1, _ = pgm.psf_weighted_centroid(m, cw, c0)
        pgm.update_symmetric(m, c1, None, algorithm="sdss")
        np.testing.assert_array_equal(g["cen"][i, 0], c1)
        assert g["morph"][0][i, 0, :h, :w].tobytes() == m.tobytes(), (i, (h, w), cen[i], c1)


# ------------------------------------------------------------------ (i)
@pytest.mark.parametrize("optset", ["sdss", "norm_sed", "mixed"])
def test_uniform_cutouts_with_a_multi_source_and_options(env, optset):
    scarlet, pool = env
    c = oc.UNIFORM
    for cutouts in (np.stack([np.array(im) for im, _ in oc.scenes(c)]), None):          # a block, and a list of equal shapes
        b = _make(scarlet, c, optset, cutouts=cutouts)
        assert b._catalog_options and b.frame_shapes is None and b.group is not None and b._frames.frame_hw is None
        _init(b, c)
        st0 = _state(b)
        refs = pool.starmap(oc.oracle_start, [(c, s, optset) for s in range(len(c.shapes))])
        _compare(c, st0, refs, "uniform / %s start" % optset, fit=False)
        b.fit(oc.ITERS, e_rel=0)
        st = _state(b)
        _compare(c, st, _oracle_fit(pool, "uniform", c, optset, st0), "uniform / %s fit" % optset)
        assert (st["it"] == oc.ITERS).all()
