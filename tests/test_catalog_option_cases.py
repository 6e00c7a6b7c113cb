"""CPU: the cases of tests/catalog_option_cases.py and the host side of catalogue batches with update options.

1. every case x option set x scene is admissible: the composed oracle runs to finite results and its float32 and float64
   runs (from the same float32 start) agree to parity_common.TOL, on the centres and on the flags, and no factor's last
   change lies in (0, 1e-6) (the DECIDED rule of tests/test_update_option_cases.py) -- a scene that fails was re-seeded in
   the cases file, so that tests/test_gpu_catalog_options.py needs no exemption;
2. every option set moves some scene of its case by more than 100 x TOL against the stock pipeline (printed);
3. the own-frame result is not what zero-weight padding gives, with options (printed);
4. SourceSpec / catalog_option_arrays / from_catalog: host checks and precedence, before the device is asked for;
5. the C ABI: the two entry points in the header, the library and the binding, their refusals before any launch (fake
   pointers, no device), and the pinned refusals of the other routes.
"""
import ctypes
import multiprocessing as mp
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import rel_err
import catalog_option_cases as oc
import frame_cases as fc
import parity_common

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scarlet_hip.h")
ENTRY_POINTS = ["scarlet_fit_frames_options", "scarlet_source_update_frames_options"]
FAKE = 0x1000          # a non-NULL pointer that is never dereferenced (every call below returns before a launch)
TOL = parity_common.TOL
DECIDED = 1e-6         # ~ 16 float32 last bits of a factor's norm
OPTSETS = [None] + list(oc.OPTION_SETS)


@pytest.fixture(scope="module")
def pool():
    from oracle import build as obuild
    obuild.build()
    p = mp.get_context("spawn").Pool(min(16, os.cpu_count() or 1))
    yield p
    p.close(); p.join()


@pytest.fixture(scope="module")
def runs(pool):
    """{(case, option set, scene): (start, float32 fit)} from the oracle's own start -- computed once, read-only"""
    jobs = [(key, s, optset, None, oc.ITERS, 0.0, "float32", "own")
            for key, c in oc.ALL_CASES.items() for optset in OPTSETS for s in range(len(c.shapes))]
    return {(j[0], j[2], j[1]): r for j, r in zip(jobs, pool.map(oc.oracle_job, jobs))}


def test_cases_cover_the_forms_the_row_tails_and_the_source_types():
    forms = {key: fc.update_form(*oc.padded_shape(c)) for key, c in oc.CASES.items()}
    assert forms == dict(wave="wave", tile="tile", tile_gscratch="tile_gscratch", plane="plane", psf="wave")
    assert oc.padded_shape(oc.CASES["tile_gscratch"]) == (96, 96) and oc.padded_shape(oc.CASES["tile"]) == (72, 80)
    for key, c in oc.CASES.items():
        H, W = oc.padded_shape(c)
        ws = [w for _, w in c.shapes]
        assert any(w % 4 for w in ws), key
        assert any(w % 4 == 0 and w < W for w in ws), key
        assert c.B == 3 and len(c.catalog) == len(c.shapes), key
        for s, (im, cen) in enumerate(oc.scenes(c)):
            assert im.shape == (c.B,) + tuple(c.shapes[s]) and len(cen) == len(c.catalog[s])
            assert im[-1].mean() < -0.25           # the over-subtracted last band
        if key in ("plane", "tile_gscratch"):
            assert all(len(cat) >= 2 for cat in c.catalog), key
        assert any(kind == "multi" for cat in c.catalog for kind, _ in cat), key
    # under "mixed" every source leaves the defaults, the multi sources (the first source of their catalogues) included
    for c in oc.CASES.values():
        for cat in c.catalog:
            assert [i for i, (kind, _) in enumerate(cat) if kind == "multi"] in ([0], [])
            for i in range(len(cat)):
                assert oc.spec_kwargs("mixed", i) != {} and oc.source_options("mixed", i) != oc.source_options(None, i)


# ---- 1. admissible
@pytest.mark.parametrize("optset", OPTSETS)
@pytest.mark.parametrize("key", list(oc.ALL_CASES))
def test_case_is_admissible(pool, runs, key, optset):
    c = oc.ALL_CASES[key]
    S = len(c.shapes)
    jobs = [(key, s, optset, runs[(key, optset, s)][0], oc.ITERS, 0.0, "float64", "own") for s in range(S)]
    for s, (_, r64) in enumerate(pool.map(oc.oracle_job, jobs)):
        start, r32 = runs[(key, optset, s)]
        h, w = c.shapes[s]
        n = oc.n_components(c, s)
        assert r32["it"] == r64["it"] == oc.ITERS
        assert r32["morph"].shape == (n, h, w) and r32["sed"].shape == (n, c.B)
        assert np.isfinite(start["sed"]).all() and np.isfinite(start["morph"]).all(), s
        for k in ("sed", "morph", "mse"):
            assert np.isfinite(r32[k]).all(), (s, k)
            e = rel_err(r32[k], r64[k])
            assert e <= TOL, "scene %d sits on a threshold (%s: float32 and float64 differ by %.2e): re-seed it" % (s, k, e)
        np.testing.assert_array_equal(r32["cen"], r64["cen"])
        np.testing.assert_array_equal(r32["flags"], r64["flags"])
        assert ((r32["cen"] >= 0) & (r32["cen"] < np.array([h, w]))).all(), s
        ch = r64["change"]
        assert ((ch == 0) | (ch >= DECIDED)).all(), "scene %d: a factor's last change %.1e is float32 noise: re-seed it" % (
            s, ch[(ch > 0) & (ch < DECIDED)].min())
        assert (r32["morph"].reshape(n, -1).max(axis=1) > 0).all()


def test_converged_run_is_admissible(pool):
    """the one converged run of the GPU tests (wave, soft, e_rel = 1e-3): both precisions stop at the same iteration.  The
    scene of one component never stops -- it cycles with period 2 (catalog_option_cases.make_scene) -- so for it both
    precisions must reach the cap with equal flags, its SED flag still set.  No one-component scene that is both decided after
    6 iterations and converges was found: 80 seeds without a neighbour, then 100 seeds for each of 16 neighbour settings
    (offsets 2..5 px, peaks 15..60)."""
    c = oc.CASES["wave"]
    S = len(c.shapes)
    first = pool.map(oc.oracle_job, [("wave", s, "soft", None, oc.CONVERGED_CAP, 1e-3, "float32", "own") for s in range(S)])
    second = pool.map(oc.oracle_job, [("wave", s, "soft", first[s][0], oc.CONVERGED_CAP, 1e-3, "float64", "own") for s in range(S)])
    assert [oc.one_component(c, s) for s in range(S)].count(True) == 1
    for s in range(S):
        r32, r64 = first[s][1], second[s][1]
        print("\nwave / soft converged run, scene %d: it %d / %d, flags %s" % (s, r32["it"], r64["it"], r32["flags"]))
        if oc.one_component(c, s):
            assert r32["it"] == r64["it"] == oc.CONVERGED_CAP and r32["flags"].tolist() == r64["flags"].tolist() != [0]
        else:
            assert 2 < r32["it"] == r64["it"] < oc.CONVERGED_CAP, (s, r32["it"], r64["it"])
            assert (r32["flags"] == 0).all() and (r64["flags"] == 0).all()
        assert max(rel_err(r32[k], r64[k]) for k in ("sed", "morph", "mse")) <= TOL


# ---- 2. every option set matters
@pytest.mark.parametrize("optset", list(oc.OPTION_SETS))
@pytest.mark.parametrize("key", list(oc.ALL_CASES))
def test_option_set_moves_the_result(runs, key, optset):
    c = oc.ALL_CASES[key]
    moves = [max(rel_err(runs[(key, optset, s)][1][k], runs[(key, None, s)][1][k]) for k in ("sed", "morph"))
             for s in range(len(c.shapes))]
    print("\n%s / %s: moved by %s relative to the stock pipeline" % (key, optset, ["%.2e" % m for m in moves]))
    assert max(moves) > 100 * TOL


# ---- 3. zero-weight padding is another result
def test_zero_weight_padding_is_not_the_own_frame_result_with_options(pool, runs):
    """For every case, under "mixed", at least one component's morphology after 6 iterations differs between the own-frame
    run and the zero-weight-padded run by more than 1e-4 relative max-norm (10 x the GPU tolerance): a kernel that took
    the padded bounds could not pass tests/test_gpu_catalog_options.py."""
    for key, c in oc.CASES.items():
        S = len(c.shapes)
        pad = pool.map(oc.oracle_job, [(key, s, "mixed", None, oc.ITERS, 0.0, "float32", "padded") for s in range(S)])
        diffs = []
        for s, (h, w) in enumerate(c.shapes):
            own = runs[(key, "mixed", s)][1]["morph"]
            diffs.append(max(rel_err(pad[s][1]["morph"][k][:h, :w], own[k]) for k in range(len(own))))
        print("\n%s / mixed: zero-weight padding vs own frame, morphologies: %s"
              % (key, ["%s %.1e" % (c.shapes[s], d) for s, d in enumerate(diffs)]))
        assert any(d > 1e-4 for d in diffs), (key, diffs)


# ---- 4. host logic
@pytest.fixture()
def no_gpu(monkeypatch):
    """the device is never asked for: every check below is made on the host first"""
    from scarlet_amd import _lib

    def refuse():
        raise AssertionError("the device was asked for before the host checks were done")
    monkeypatch.setattr(_lib, "require_gpu", refuse)


def _cut(shapes, B=3):
    return [np.zeros((B, h, w), np.float32) for h, w in shapes]


def test_catalog_option_arrays_and_precedence():
    import scarlet_amd as scarlet
    from scarlet_amd import _lib
    from scarlet_amd.batch import catalog_arrays, catalog_option_arrays
    S_ = scarlet.SourceSpec
    plain = [[S_((10, 11), kind="multi"), S_((20, 5), kind="point")], [S_((8, 9))]]
    assert catalog_option_arrays(plain) is None and catalog_option_arrays(plain, None) is None
    assert not S_((1, 1)).has_options() and S_((1, 1), strength=0.5).has_options()
    # an explicit default is options already
    a = catalog_option_arrays(plain, scarlet.UpdateOptions())
    assert list(a) == list(scarlet.UpdateOptions.FIELDS) and all(v.shape == (2, 3) for v in a.values())
    ref = scarlet.UpdateOptions().arrays(2, 3)
    assert all(np.array_equal(a[f], ref[f]) for f in ref)
    # the catalogue's fields override the batch default; layers share their source's options; absent rows keep the defaults
    cat = [[S_((10, 11), kind="multi", flux_percentiles=[20, 60], symmetry="sdss", use_nearest=True),
            S_((20, 5), kind="point", normalization="sed", positive="morph")],
           [S_((8, 9), strength=0.25, monotonic_thresh=0.05)]]
    a = catalog_option_arrays(cat, scarlet.UpdateOptions(symmetry="soft", strength=0.75, positive="sed"))
    t = catalog_arrays([(30, 30), (16, 12)], cat)
    assert t["n_components"].tolist() == [4, 1] and all(v.shape == (2, 4) for v in a.values())
    assert a["sym_algorithm"].tolist() == [[_lib.SYM_SDSS] * 3 + [_lib.SYM_SOFT], [_lib.SYM_SOFT] + [_lib.SYM_KSPACE] * 3]
    assert a["sym_strength"].tolist() == [[0.75] * 4, [0.25, 0.5, 0.5, 0.5]]
    assert a["mono_nearest"].tolist() == [[1, 1, 1, 0], [0, 0, 0, 0]]
    assert np.allclose(a["mono_thresh"], [[0, 0, 0, 0], [0.05, 0, 0, 0]])
    assert a["positive"].tolist() == [[1, 1, 1, 2], [1, 3, 3, 3]]
    assert a["normalize"].tolist() == [[_lib.NORM_MORPH_MAX] * 3 + [_lib.NORM_SED], [_lib.NORM_MORPH_MAX] * 4]
    # without update= the stock pipeline's values are the default
    a = catalog_option_arrays(cat)
    assert a["sym_algorithm"].tolist() == [[_lib.SYM_SDSS] * 3 + [_lib.SYM_KSPACE], [_lib.SYM_KSPACE] * 4]
    assert a["positive"].tolist() == [[3, 3, 3, 2], [3, 3, 3, 3]]
    # the names may be the library's integers
    assert catalog_option_arrays([[S_((1, 1), symmetry=_lib.SYM_SDSS)]])["sym_algorithm"].tolist() == [[_lib.SYM_SDSS]]


def test_from_catalog_option_errors_come_before_the_device(no_gpu):
    import scarlet_amd as scarlet
    S_ = scarlet.SourceSpec
    shapes = [(20, 24), (12, 30)]

    def raises(match, cat, **kw):
        with pytest.raises(ValueError, match=match):
            scarlet.BlendBatch.from_catalog(_cut(shapes), cat, **kw)

    good = [S_((5, 5))]
    raises(r"scene 1, source 0: symmetry: unknown value 'fourier'", [good, [S_((6, 7), symmetry="fourier")]])
    raises(r"scene 0, source 1: positive: unknown value 'all'", [[S_((5, 5)), S_((9, 9), kind="multi", positive="all")], good])
    raises(r"scene 1, source 0: normalization: unknown value 'max'", [good, [S_((6, 7), normalization="max")]])
    raises(r"scene 1, source 0: strength = 1.5 lies outside \[0, 1\]", [good, [S_((6, 7), strength=1.5)]])
    raises(r"scene 0, source 0: strength = -0.1 lies outside", [[S_((5, 5), kind="point", strength=-0.1)], good])
    raises(r"scene 1, source 0: monotonic_thresh = 1.0 lies outside \[0, 1\)", [good, [S_((6, 7), monotonic_thresh=1.0)]])
    raises(r"scene 1, source 0: use_nearest with monotonic_thresh", [good, [S_((6, 7), use_nearest=True, monotonic_thresh=0.1)]])
    # ... also where the thresh is the batch's default and the sweep the source's
    raises(r"scene 0, source 0: use_nearest with monotonic_thresh", [[S_((5, 5), use_nearest=True)], good],
           update=scarlet.UpdateOptions(monotonic_thresh=0.2))
    raises(r"comes from the catalogue", [good, good], update=scarlet.UpdateOptions(symmetry=["soft", "sdss"]))
    raises(r"comes from the catalogue", [good, good], update=scarlet.UpdateOptions(strength=np.full((2, 1), 0.5)))
    raises(r"update must be an UpdateOptions", [good, good], update=dict(symmetry="soft"))
    raises(r"strength = 2.0 lies outside", [good, good], update=scarlet.UpdateOptions(strength=2.0))
    # the other catalogue checks still come first, and a good catalogue with options reaches the device request
    raises(r"scene 1, source 0: unknown source kind 'galaxy'", [good, [S_((6, 7), kind="galaxy", symmetry="soft")]])
    for kw, cat in ((dict(update=scarlet.UpdateOptions()), [good, good]), ({}, [good, [S_((6, 7), kind="multi", symmetry="sdss")]])):
        with pytest.raises(AssertionError, match="the device was asked for"):
            scarlet.BlendBatch.from_catalog(_cut(shapes), cat, **kw)
    # uniform cut-outs go the same way
    with pytest.raises(ValueError, match=r"scene 0, source 0: strength"):
        scarlet.BlendBatch.from_catalog(np.zeros((2, 3, 20, 24), np.float32), [[S_((5, 5), strength=7)], good])


def test_pinned_refusals_still_refuse(no_gpu):
    """BlendBatch(update=, group=), BlendBatch(update=) with ragged frames and a ragged BlendBatch with group= still refuse
    on the host.  (The other pins -- from_observations with update= and ragged frames, wide=True or a low-resolution
    observation, the priors, scarlet_fit_observations_options and the _frames init calls with b->group -- are held by the
    existing tests that set them, tests/test_gpu_update_options.py, test_update_option_cases.py, test_catalog_cases.py and
    test_gpu_frames.py, which this change leaves as they are; they are not repeated here.)"""
    import scarlet_amd as scarlet
    upd = scarlet.UpdateOptions(symmetry="soft")
    cen = np.full((2, 2, 2), 5, np.int32)
    with pytest.raises(NotImplementedError, match="group"):
        scarlet.BlendBatch(np.zeros((2, 3, 20, 24), np.float32), cen, update=upd, group=np.zeros((2, 2), np.int32))
    with pytest.raises(NotImplementedError, match="ragged"):
        scarlet.BlendBatch(np.zeros((2, 3, 20, 24), np.float32), cen, update=upd, frame_shapes=[(20, 24), (12, 20)])
    with pytest.raises(NotImplementedError, match="ragged"):
        scarlet.BlendBatch(_cut([(20, 24), (12, 30)]), cen, update=upd)
    with pytest.raises(NotImplementedError):
        scarlet.BlendBatch(_cut([(20, 24), (12, 30)]), cen, group=np.zeros((2, 2), np.int32))


# ---- 5. the C ABI
def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_entry_points():
    text = _header()
    for fn in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(\s*scarlet_batch \*b,\s*const scarlet_frames \*f,\s*const scarlet_constraints \*c\s*,\s*"
                         r"const scarlet_update_options \*o," % fn, text), fn
    assert re.search(r"scarlet_fit_frames_options\([^;]*int max_iter, double e_rel, int approximate_L,\s*int check_every, void \*stream\);", text)
    assert re.search(r"scarlet_source_update_frames_options\([^;]*int in_iteration, void \*stream\);", text)


def test_library_exports_and_binding():
    from scarlet_amd import _lib
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(ln.split()[-1] for ln in out.splitlines() if ln.strip())
    for fn in ENTRY_POINTS:
        assert fn in exported and fn in _lib.EXPORTS, fn
        f = getattr(_lib.lib, fn)
        assert f.restype is ctypes.c_int
        assert [t._type_ for t in f.argtypes[:4]] == [_lib.ScarletBatch, _lib.ScarletFrames, _lib.ScarletConstraints,
                                                      _lib.ScarletUpdateOptions]
    assert len(_lib.lib.scarlet_fit_frames_options.argtypes) == 9 and len(_lib.lib.scarlet_source_update_frames_options.argtypes) == 6
    assert ctypes.sizeof(_lib.ScarletUpdateOptions) == 48 and ctypes.sizeof(_lib.ScarletBatch) == 256      # unchanged


def _batch(S=4, K=3, B=5, H=32, W=32, pointers=True):
    from scarlet_amd import _lib
    b = _lib.ScarletBatch()
    b.S, b.K, b.B, b.H, b.W = S, K, B, H, W
    if pointers:
        for f in ("images", "cur", "centers", "shifts", "flags", "lipschitz", "mse", "it", "active", "status", "workspace"):
            setattr(b, f, FAKE)
        for i in range(2):
            b.sed[i] = FAKE
            b.morph[i] = FAKE
        b.mse_capacity = 8
    return b


def _calls():
    from scarlet_amd import _lib
    L = _lib.lib
    return [lambda b, f, c, o: L.scarlet_fit_frames_options(b, f, c, o, 1, 0.0, 0, 0, None),
            lambda b, f, c, o: L.scarlet_source_update_frames_options(b, f, c, o, 1, None)]


@pytest.mark.parametrize("which", range(2))
def test_refusals_before_any_launch(which):
    from scarlet_amd import _lib
    call = _calls()[which]
    o = _lib.ScarletUpdateOptions()
    o.mono_nearest = FAKE
    f = _lib.ScarletFrames()
    f.frame_hw = FAKE
    g = _batch()
    g.group = FAKE                                  # a group is allowed: none of the refusals below is about it
    for b in (_batch(), g):
        assert call(ctypes.byref(b), None, None, ctypes.byref(o)) == _lib.E_ARG
        assert "frames is NULL" in _lib.last_error()
        assert call(ctypes.byref(b), ctypes.byref(f), None, None) == _lib.E_ARG
        assert "options is NULL" in _lib.last_error()
    # the batch's own errors, whatever the structs hold; c may be NULL or given
    c = _lib.ScarletConstraints()
    for cp in (None, ctypes.byref(c)):
        assert call(ctypes.byref(_batch(pointers=False)), ctypes.byref(f), cp, ctypes.byref(o)) == _lib.E_ARG
        assert "null pointer in batch" in _lib.last_error()
    assert call(ctypes.byref(_batch(K=257)), ctypes.byref(f), None, ctypes.byref(o)) == _lib.E_NOTIMPL
    assert call(ctypes.byref(_batch(H=2048)), ctypes.byref(f), None, ctypes.byref(o)) == _lib.E_TOO_LARGE
    assert call(None, ctypes.byref(f), None, ctypes.byref(o)) == _lib.E_ARG
    c.symmetric = FAKE             # a symmetric array needs the centroid PSF, as in the _constrained entry points
    assert call(ctypes.byref(g), ctypes.byref(f), ctypes.byref(c), ctypes.byref(o)) == _lib.E_ARG
    assert "centroid_psf" in _lib.last_error()
    if which == 0:
        assert _lib.lib.scarlet_fit_frames_options(ctypes.byref(g), ctypes.byref(f), None, ctypes.byref(o), -1, 0.0, 0, 0, None) == _lib.E_ARG
        assert "max_iter" in _lib.last_error()


def test_pinned_entry_points_still_refuse_group():
    """scarlet_fit_options / scarlet_source_update_options with b->group, and the plain _frames calls with frame_hw and
    b->group: E_NOTIMPL before any launch, as before"""
    from scarlet_amd import _lib
    L = _lib.lib
    o = _lib.ScarletUpdateOptions()
    o.normalize = FAKE
    f = _lib.ScarletFrames()
    f.frame_hw = FAKE
    g = _batch()
    g.group = FAKE
    assert L.scarlet_fit_options(ctypes.byref(g), None, ctypes.byref(o), 1, 0.0, 0, 0, None) == _lib.E_NOTIMPL
    assert "group" in _lib.last_error()
    assert L.scarlet_source_update_options(ctypes.byref(g), None, ctypes.byref(o), 1, None) == _lib.E_NOTIMPL
    assert "group" in _lib.last_error()
    assert L.scarlet_fit_frames(ctypes.byref(g), ctypes.byref(f), None, 1, 0.0, 0, 0, None) == _lib.E_NOTIMPL
    assert "group" in _lib.last_error()
    assert L.scarlet_source_update_frames(ctypes.byref(g), ctypes.byref(f), None, 1, None) == _lib.E_NOTIMPL
    assert "group" in _lib.last_error()
