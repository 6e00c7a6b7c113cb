"""-m gpu: batches with update options (BlendBatch(update=UpdateOptions(...)), scarlet_update_options) against the composed
oracle of tests/update_option_cases.py.

(a) every case x option set: 6 iterations from the batch's own start; SED, morphology and loss history within
    parity_common.TOL, centres, iteration counts and flags equal, no exemptions (tests/test_update_option_cases.py chose the
    scenes so that the reference alone is decided); one converged run (wave, soft symmetry, e_rel = 1e-3)
(b) init_extended alone: the oracle's constructor followed by the composed update at it = 0
(c) UpdateOptions() with every default: the bits of update=None after init and 5 iterations on the general path, for
    every form of the constraint kernels (the box stage of update=None switched off: options batches run none)
(d) a batch without options: the bits the parent commit gave (its recorded digests, tests/golden)
(e) copies of one scene with different option rows, tiled to 64 scenes, agree per option row wherever they sit
(f) options corrupted on the device: BAD_OPTION, the scene untouched, the others bit-identical to the clean run
(g) the nearest-neighbour sweep alone through scarlet_source_update_options, bit-exact against the oracle
(h) the refusals that need a batch
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import rel_err
import parity_common
import update_option_cases as uc

pytestmark = pytest.mark.gpu
TOL = parity_common.TOL
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = ["wave", "tile", "tile_gscratch", "plane", "psf"]        # the single-observation cases, one per form (+ the PSF)


@pytest.fixture(scope="module")
def scarlet():
    import scarlet_amd
    scarlet_amd._lib.require_gpu()
    from oracle import build as obuild
    obuild.build()
    return scarlet_amd


def make_batch(scarlet, c, optset, update="case", run_update=True, images=None, centers=None):
    """the case's batch, started (init_extended; the joint case: init_combined).  update: "case" = the option set's
    UpdateOptions (None for optset None), or what to pass as update="""
    if images is None:
        images, centers = uc.stacked(c)
    if update == "case":
        update = None if optset is None else scarlet.UpdateOptions(**uc.update_kwargs(optset, c.K))
    if c.joint:
        obs = [scarlet.ObservationBatch(images[:, :uc.JOINT_SPLIT], band0=0),
               scarlet.ObservationBatch(images[:, uc.JOINT_SPLIT:], band0=uc.JOINT_SPLIT)]
        b = scarlet.BlendBatch.from_observations(obs, centers, update=update, mse_capacity=uc.CONVERGED_CAP + 1)
        b.init_combined([np.ones(uc.JOINT_SPLIT) * uc.BG, np.ones(c.B - uc.JOINT_SPLIT) * uc.BG])
        return b
    kw = dict(update=update, mse_capacity=uc.CONVERGED_CAP + 1)
    scale = None
    if c.psf:
        _, model, diff, scale = uc.psfs(c)
        kw["centroid_weight"] = model.astype(np.float32)
    b = scarlet.BlendBatch(images, centers, **kw)
    if c.psf:
        b.set_diff_kernel(diff)
    b.init_extended(np.ones(c.B) * uc.BG, sed_scale=scale, run_update=run_update)
    return b


def state(b):
    import torch
    torch.cuda.synchronize()
    return dict(sed=b.sed_current.cpu().numpy(), morph=b.morph_current.cpu().numpy(), cen=b.centers.cpu().numpy(),
                sh=b.shifts.cpu().numpy(), it=b.it.cpu().numpy(), flags=b.flags.cpu().numpy(), mse=b.mse_buf.cpu().numpy(),
                status=b.status.cpu().numpy(), active=b.active.cpu().numpy())


def assert_same_bits(a, b, keys=("sed", "morph", "cen", "sh", "it", "flags", "mse", "status", "active"), scenes=None):
    for k in keys:
        x, y = (a[k], b[k]) if scenes is None else (a[k][scenes], b[k][scenes])
        assert x.tobytes() == y.tobytes(), k


def compare(c, optset, st0, g, iters, e_rel=0.0, fixed=True):
    worst = dict(sed=0.0, morph=0.0, mse=0.0)
    assert int(np.abs(g["status"]).sum()) == 0, g["status"]
    for s in range(len(g["it"])):
        ref = uc.oracle_run(c, s, optset, (st0["sed"][s], st0["morph"][s], st0["cen"][s], st0["sh"][s]), iters=iters, e_rel=e_rel)
        n = ref["it"]
        assert g["it"][s] == n and (not fixed or n == iters), (s, g["it"][s], n)
        np.testing.assert_array_equal(g["cen"][s], ref["cen"])
        np.testing.assert_array_equal(g["flags"][s], ref["flags"])
        e = dict(sed=rel_err(g["sed"][s], ref["sed"]), morph=rel_err(g["morph"][s], ref["morph"]),
                 mse=rel_err(g["mse"][s][:n], ref["mse"]))
        print("%s / %s scene %d: %s" % (c.name, optset, s, {k: "%.2e" % v for k, v in e.items()}))
        for k in worst:
            worst[k] = max(worst[k], e[k])
    assert max(worst.values()) <= TOL, worst
    return worst


# ---- (a)
@pytest.mark.parametrize("optset", list(uc.OPTION_SETS))
@pytest.mark.parametrize("name", list(uc.CASES))
def test_fit_matches_the_composed_oracle(scarlet, name, optset):
    c = uc.CASES[name]
    b = make_batch(scarlet, c, optset)
    st0 = state(b)
    assert b.fit(uc.ITERS, e_rel=0) == uc.ITERS
    compare(c, optset, st0, state(b), uc.ITERS)


def test_converged_run(scarlet):
    c = uc.CASES["wave"]
    b = make_batch(scarlet, c, "soft")
    st0 = state(b)
    b.fit(uc.CONVERGED_CAP, e_rel=1e-3, check_every=10)
    g = state(b)
    assert (g["active"] == 0).all() and (g["it"] < uc.CONVERGED_CAP).all() and (g["flags"] == 0).all()
    compare(c, "soft", st0, g, uc.CONVERGED_CAP, e_rel=1e-3, fixed=False)


# ---- (b)
@pytest.mark.parametrize("optset", list(uc.OPTION_SETS))
@pytest.mark.parametrize("name", FORMS)
def test_init_extended_runs_the_options(scarlet, name, optset):
    c = uc.CASES[name]
    g = state(make_batch(scarlet, c, optset))
    assert int(np.abs(g["status"]).sum()) == 0
    for s in range(len(g["it"])):
        sed, morph, cen, sh = uc.oracle_start(c, s, optset)
        np.testing.assert_array_equal(g["cen"][s], cen)
        assert rel_err(g["sed"][s], sed) <= TOL and rel_err(g["morph"][s], morph) <= TOL
        np.testing.assert_array_equal(np.isnan(g["sh"][s]), np.isnan(sh))
        np.testing.assert_allclose(np.nan_to_num(g["sh"][s]), np.nan_to_num(sh), rtol=0, atol=1e-5)


# ---- (c)
@pytest.mark.parametrize("name", ["wave_k12", "tile", "tile_gscratch", "plane", "psf", "joint"])
def test_default_options_give_the_bits_of_no_options(scarlet, name):
    from scarlet_amd import _lib
    c = uc.CASES[name]
    old = _lib.set_option("NO_BOX", 1)           # (update=None beyond 64 pixels: the full-frame forms for every component)
    try:
        plain = make_batch(scarlet, c, None)
        plan = (ctypes.c_int32 * 8)()
        assert _lib.lib.scarlet_debug_fused_plan(ctypes.byref(plain._c), None, None, 0, 5, ctypes.cast(plan, ctypes.c_void_p)) == 0
        assert c.joint or plan[0] == 0, "the case must take the general path without options as well"
        opts = make_batch(scarlet, c, None, update=scarlet.UpdateOptions())
        assert opts._upd is not None and all(getattr(opts._upd, f) for f in scarlet.UpdateOptions.FIELDS)
        assert_same_bits(state(plain), state(opts))
        plain.fit(5, e_rel=0)
        opts.fit(5, e_rel=0)
        a, b = state(plain), state(opts)
        assert (a["it"] == 5).all()
        assert_same_bits(a, b)
    finally:
        _lib.set_option("NO_BOX", old)


def test_step_is_one_iteration_of_fit(scarlet):
    c = uc.CASES["wave"]
    a, b = make_batch(scarlet, c, "mixed"), make_batch(scarlet, c, "mixed")
    a.fit(2, e_rel=0)
    b.step(e_rel=0)
    b.step(e_rel=0)
    assert_same_bits(state(a), state(b))
    m = b.get_model().cpu().numpy()               # products of such a batch: the model of the current factors
    want = np.einsum("skb,skhw->sbhw", b.sed_current.cpu().numpy().astype(np.float64), b.morph_current.cpu().numpy().astype(np.float64))
    assert rel_err(m, want) <= TOL


# ---- (d)
_HASH_SCRIPT = r"""
import hashlib, sys
import numpy as np
sys.path.insert(0, %r)
import torch
import scarlet_amd as scarlet
from scarlet_amd import synth
out = []
for K, n, psf in ((4, 8, False), (4, 3, True), (12, 2, False)):
    sc = [synth.make_scene(4200 + i, B=5, H=64, W=64, K=K, min_sep=4 if K == 4 else 3) for i in range(n)]
    b = scarlet.BlendBatch(np.stack([s["images"] for s in sc]), np.stack([s["centers"] for s in sc]))
    if psf:
        k = np.zeros((5, 5, 5), np.float32); k[:, 2, 2] = 0.6; k[:, 2, 1] = k[:, 2, 3] = k[:, 1, 2] = k[:, 3, 2] = 0.1
        b.set_diff_kernel(k)
    b.init_extended(np.ones(5) * 0.1)
    b.fit(5, e_rel=0)
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in (b.sed_current, b.morph_current, b.centers, b.shifts, b.mse_buf, b.flags, b.it, b.status):
        h.update(t.cpu().numpy().tobytes())
    out.append(h.hexdigest())
print("HASHES " + " ".join(out))
"""


def _hashes(root=ROOT):
    """the digests of the script above, run in a fresh process against the package under `root`"""
    env = dict(os.environ)
    env.pop("SCARLET_LIB_PATH", None)
    out = subprocess.check_output([sys.executable, "-c", _HASH_SCRIPT % root], env=env, timeout=300).decode()
    return [ln for ln in out.splitlines() if ln.startswith("HASHES ")][0].split()[1:]


def test_batches_without_options_keep_their_bits(scarlet):
    """5 x 64 x 64, K = 4 (the one-launch iteration), the same with a PSF and K = 12 (general path), 5 iterations in a
    fresh process: the digests of the whole state equal those the parent commit gave (tests/golden/
    update_options_parent_bits.json, recorded on an MI355X by running the same script against the parent's tree and
    library: the new binding cannot load a library without the new entry points, so the comparison is with its record)."""
    with open(os.path.join(ROOT, "tests", "golden", "update_options_parent_bits.json")) as f:
        want = json.load(f)["sha256"]
    assert _hashes() == want


# ---- (e)
def test_option_rows_travel_with_their_scenes(scarlet):
    c = uc.CASES["wave"]
    images, centers = uc.scenes(c)[0]
    S, names = 64, list(uc.OPTION_SETS)
    row = np.array([(7 * s + s // 8) % len(names) for s in range(S)])          # every set, at scattered places
    assert set(row) == set(range(len(names)))
    per = [[uc.component_options(names[r], k) for k in range(c.K)] for r in row]
    kw = {f: [[p[f] for p in scene] for scene in per] for f in uc.DEFAULTS}
    b = make_batch(scarlet, c, None, update=scarlet.UpdateOptions(**kw), images=np.repeat(images[None], S, 0),
                   centers=np.repeat(centers[None], S, 0))
    b.fit(uc.ITERS, e_rel=0)
    g = state(b)
    assert int(np.abs(g["status"]).sum()) == 0 and (g["it"] == uc.ITERS).all()
    firsts = []
    for r in range(len(names)):
        idx = np.nonzero(row == r)[0]
        assert len(idx) >= 2
        for s in idx[1:]:
            for k in ("sed", "morph", "cen", "sh", "flags", "mse"):
                assert g[k][s].tobytes() == g[k][idx[0]].tobytes(), (names[r], int(s), k)
        firsts.append(idx[0])
    for i in range(len(firsts)):             # ... and the rows differ from each other
        for j in range(i):
            assert g["morph"][firsts[i]].tobytes() != g["morph"][firsts[j]].tobytes(), (names[i], names[j])


# ---- (f)
def test_corrupted_options_mark_the_scene_and_nothing_else(scarlet):
    from scarlet_amd import _lib
    c = uc.CASES["wave"]
    images, centers = uc.stacked(c)
    images, centers = np.concatenate([images, images[:2]]), np.concatenate([centers, centers[:2]])      # 5 scenes
    runs = []
    for corrupt in (False, True):
        b = make_batch(scarlet, c, "mixed", run_update=False, images=images, centers=centers)
        if corrupt:
            b.update_options["sym_algorithm"][1, 0] = 7
            b.update_options["mono_thresh"][3, 1] = 1.5
        before = state(b)
        b.update_sources()
        b.fit(5, e_rel=0)
        runs.append((b, before, state(b)))
    (_, _, clean), (bad, before, g) = runs
    assert (clean["status"] == 0).all() and (clean["it"] == 5).all()
    for s in (1, 3):
        assert g["status"][s] == _lib.STATUS_BAD_OPTION and g["active"][s] == 0 and g["it"][s] == 0
        assert_same_bits(before, g, keys=("sed", "morph", "cen", "sh", "flags", "mse"), scenes=s)
    for s in (0, 2, 4):
        assert_same_bits(clean, g, scenes=s)
    with pytest.raises(ValueError) as e:
        bad.raise_on_status()
    assert "[1, 3]" in str(e.value) and "BAD_OPTION" in str(e.value)


# ---- (g)
@pytest.mark.parametrize("shape, n", [((40, 40), 256), ((72, 80), 256), ((96, 96), 24), ((uc.PLANE_SIDE, uc.PLANE_SIDE), 24)])
def test_nearest_sweep_alone_is_bit_exact(scarlet, shape, n):
    """random planes, random centres with the edges and the four corners among them, everything else of the pipeline off
    (no symmetry, no positivity, no normalisation); max_pixel keeps the centre (the plane's largest value sits there)"""
    from oracle import pgm
    from scarlet_amd import _lib
    H, W = shape
    rng = np.random.Generator(np.random.PCG64(H * 1000 + W))
    planes = rng.normal(0.3, 1.0, size=(n, 1, H, W)).astype(np.float32)
    cen = np.stack([rng.integers(0, H, size=n), rng.integers(0, W, size=n)], axis=1).astype(np.int32)
    cen[:8] = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H // 2, 0), (H - 1, 3), (5, W - 1)]
    for i, (cy, cx) in enumerate(cen):
        planes[i, 0, cy, cx] = 10.0 + i
    b = scarlet.BlendBatch(np.zeros((n, 1, H, W), np.float32), cen[:, None, :], symmetric=False, monotonic=True,
                           update=scarlet.UpdateOptions(use_nearest=True, positive="none", normalization="none"))
    b.set_state(np.ones((n, 1, 1), np.float32), planes)
    b.update_sources()
    g = state(b)
    assert (g["status"] & ~_lib.STATUS_CENTER_AT_EDGE == 0).all()
    np.testing.assert_array_equal(g["cen"][:, 0], cen)
    assert (g["sed"] == 1).all()
    for i in range(n):
        want = pgm.prox_nearest_monotonic(planes[i, 0].astype(np.float64), cen[i]).astype(np.float32)
        assert g["morph"][i, 0].tobytes() == want.tobytes(), (i, cen[i])


# ---- (h)
def test_refusals_that_need_a_batch(scarlet):
    c = uc.CASES["wave"]
    images, centers = uc.stacked(c)
    upd = scarlet.UpdateOptions(symmetry="soft")
    with pytest.raises(NotImplementedError, match="group"):
        scarlet.BlendBatch(images, centers, update=upd, group=np.zeros(centers.shape[:2], np.int32))
    with pytest.raises(NotImplementedError, match="frame_shapes"):
        scarlet.BlendBatch(images, centers, update=upd, frame_shapes=np.full((len(images), 2), 40, np.int32))
    with pytest.raises(NotImplementedError, match="frame"):
        scarlet.BlendBatch([im for im in images], centers, update=upd)
    with pytest.raises(ValueError, match="UpdateOptions"):
        scarlet.BlendBatch(images, centers, update=dict(symmetry="soft"))
    with pytest.raises(ValueError, match="strength"):
        scarlet.BlendBatch(images, centers, update=scarlet.UpdateOptions(symmetry="soft", strength=2))
    b = make_batch(scarlet, c, "soft")
    prior = scarlet.QuadraticPrior(morph_weight=0.1)
    for call in (lambda: b.fit(1, prior=prior), lambda: b.step(prior=prior)):
        with pytest.raises(NotImplementedError, match="prior"):
            call()
    j = uc.CASES["joint"]
    im, cen = uc.stacked(j)
    obs = [scarlet.ObservationBatch(im[:, :3], band0=0), scarlet.ObservationBatch(im[:, 3:], band0=3)]
    with pytest.raises(NotImplementedError, match="wide"):
        scarlet.BlendBatch.from_observations(obs, cen, update=upd, wide=True)
    ragged = [scarlet.ObservationBatch(im[:, :3], band0=0, frame_shapes=np.full((len(im), 2), 40, np.int32)),
              scarlet.ObservationBatch(im[:, 3:], band0=3, frame_shapes=np.full((len(im), 2), 40, np.int32))]
    with pytest.raises(NotImplementedError, match="frame"):
        scarlet.BlendBatch.from_observations(ragged, cen, update=upd)
    low = scarlet.LowResObservationBatch.__new__(scarlet.LowResObservationBatch)      # (never looked at: the refusal comes first)
    with pytest.raises(NotImplementedError, match="low-resolution"):
        scarlet.BlendBatch.from_observations([obs[0], low], cen, update=upd)
