"""CPU: the cases of tests/update_option_cases.py and the host side of update options.

1. every case x option set is admissible: the composed oracle runs to finite results and its float32 and float64 runs
   (from the same float32 start) agree to parity_common.TOL, on the centres and on the flags, and no factor's last change
   is float32 noise (the flags at e_rel = 0) -- a scene where they do not sits on a threshold and was re-seeded here, so
   that tests/test_gpu_update_options.py needs no exemption;
2. the nearest-neighbour sweep's ring property: for every centre of small frames each pixel's reference (the oracle's
   table) is the closed form the device uses and lies on the previous Chebyshev ring, and the ring-by-ring sweep gives the
   bits of the oracle's sweep in distance order;
3. every option set moves the result away from the stock pipeline's by more than 100 x TOL on its case (printed): a device
   that ignores an option cannot pass the GPU tests;
4. UpdateOptions' host checks and broadcasting, and the C ABI: the struct's layout against the header, the three entry
   points, and their refusals before any launch (fake pointers, no device).
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import rel_err
import parity_common
import update_option_cases as uc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scarlet_hip.h")
FIELDS = ["sym_algorithm", "sym_strength", "mono_nearest", "mono_thresh", "positive", "normalize"]
ENTRY_POINTS = ["scarlet_fit_options", "scarlet_source_update_options", "scarlet_fit_observations_options"]
FAKE = 0x1000          # a non-NULL pointer that is never dereferenced (every call below returns before a launch)
TOL = parity_common.TOL
DECIDED = 1e-6         # ~ 16 float32 last bits of a factor's norm

_runs = {}


def _run(name, optset, s):
    """the composed oracle's float32 result of scene s (from the oracle's own start), cached"""
    key = (name, optset, s)
    if key not in _runs:
        c = uc.CASES[name]
        start = uc.oracle_start(c, s, optset, np.float32)
        _runs[key] = (start, uc.oracle_run(c, s, optset, start, dt=np.float32))
    return _runs[key]


# ---- 1. admissible
@pytest.mark.parametrize("optset", list(uc.OPTION_SETS))
@pytest.mark.parametrize("name", list(uc.CASES))
def test_case_is_admissible(name, optset):
    c = uc.CASES[name]
    for s in range(len(uc.scenes(c))):
        start, r32 = _run(name, optset, s)
        r64 = uc.oracle_run(c, s, optset, start, dt=np.float64)
        assert r32["it"] == r64["it"] == uc.ITERS
        for k in ("sed", "morph", "mse"):
            assert np.isfinite(r32[k]).all(), (s, k)
            e = rel_err(r32[k], r64[k])
            assert e <= TOL, "scene %d sits on a threshold (%s: float32 and float64 differ by %.2e): re-seed it" % (s, k, e)
        np.testing.assert_array_equal(r32["cen"], r64["cen"])
        np.testing.assert_array_equal(r32["flags"], r64["flags"])
        # the flags at e_rel = 0 ask whether a factor moved at all: decided only where the last iteration's relative change
        # (float64) is exactly zero or far above float32's resolution
        ch = r64["change"]
        assert ((ch == 0) | (ch >= DECIDED)).all(), "scene %d: a factor's last change %.1e is float32 noise: re-seed it" % (
            s, ch[(ch > 0) & (ch < DECIDED)].min())
        assert (r32["morph"].reshape(len(r32["morph"]), -1).max(axis=1) > 0).all()


def test_converged_run_is_admissible():
    """the one converged run of the GPU tests (wave, soft, e_rel = 1e-3): both precisions stop at the same iteration"""
    c = uc.CASES["wave"]
    for s in range(len(uc.scenes(c))):
        start = uc.oracle_start(c, s, "soft", np.float32)
        r32 = uc.oracle_run(c, s, "soft", start, iters=uc.CONVERGED_CAP, e_rel=1e-3, dt=np.float32)
        r64 = uc.oracle_run(c, s, "soft", start, iters=uc.CONVERGED_CAP, e_rel=1e-3, dt=np.float64)
        assert 2 < r32["it"] == r64["it"] < uc.CONVERGED_CAP
        assert (r32["flags"] == 0).all() and (r64["flags"] == 0).all()
        assert max(rel_err(r32[k], r64[k]) for k in ("sed", "morph", "mse")) <= TOL


# ---- 2. the ring property
@pytest.mark.parametrize("shape", [(5, 7), (8, 8), (9, 4)])
def test_nearest_reference_lies_on_the_previous_ring(shape):
    from oracle import pgm
    H, W = shape
    rng = np.random.Generator(np.random.PCG64(H * 100 + W))
    for cy in range(H):
        for cx in range(W):
            ref = pgm.nearest_reference(shape, (cy, cx))
            np.testing.assert_array_equal(ref, uc.nearest_ring_reference(shape, (cy, cx)))
            Y, X = np.mgrid[:H, :W]
            ring = np.maximum(np.abs(Y - cy), np.abs(X - cx)).reshape(-1)
            off = np.arange(H * W) != cy * W + cx
            np.testing.assert_array_equal(ring[ref][off], ring[off] - 1)
            assert ref[cy * W + cx] == cy * W + cx
            for _ in range(2):
                x = rng.normal(0.5, 1.0, size=shape)
                want = pgm.prox_nearest_monotonic(x.copy(), (cy, cx))
                got = uc.ring_sweep(x.copy(), (cy, cx))
                assert got.tobytes() == want.tobytes()
                # float32: cast up, sweep, cast down == the ring sweep on the float32 values
                x32 = x.astype(np.float32)
                want32 = pgm.prox_nearest_monotonic(x32.astype(np.float64), (cy, cx)).astype(np.float32)
                assert uc.ring_sweep(x32.copy(), (cy, cx)).tobytes() == want32.tobytes()


# ---- 3. every option set matters
@pytest.mark.parametrize("optset", list(uc.OPTION_SETS))
@pytest.mark.parametrize("name", list(uc.CASES))
def test_option_set_moves_the_result(name, optset):
    c = uc.CASES[name]
    moves = []
    for s in range(len(uc.scenes(c))):
        base, got = _run(name, None, s)[1], _run(name, optset, s)[1]
        moves.append(max(rel_err(got[k], base[k]) for k in ("sed", "morph")))
    print("\n%s / %s: moved by %s relative to the stock pipeline" % (name, optset, ["%.2e" % m for m in moves]))
    assert max(moves) > 100 * TOL


def test_mixed_set_keeps_component_zero_at_the_defaults():
    for K in (2, 3, 12):
        kw = uc.update_kwargs("mixed", K)
        assert all(kw[f][0] == uc.DEFAULTS[f] for f in uc.DEFAULTS)
        assert all(any(kw[f][k] != uc.DEFAULTS[f] for f in uc.DEFAULTS) for k in range(1, K))


# ---- 4. host checks of UpdateOptions
def test_update_options_arrays_and_broadcasting():
    import scarlet_amd as scarlet
    from scarlet_amd import _lib
    a = scarlet.UpdateOptions().arrays(3, 2)
    assert list(a) == FIELDS
    assert [a[f].dtype for f in FIELDS] == [np.uint8, np.float32, np.uint8, np.float32, np.uint8, np.uint8]
    assert all(a[f].shape == (3, 2) for f in FIELDS)
    assert (a["sym_algorithm"] == _lib.SYM_KSPACE).all() and (a["sym_strength"] == 0.5).all()
    assert not a["mono_nearest"].any() and not a["mono_thresh"].any()
    assert (a["positive"] == 3).all() and (a["normalize"] == _lib.NORM_MORPH_MAX).all()
    a = scarlet.UpdateOptions(symmetry=["soft", "sdss"], strength=0.25, use_nearest=[[0, 1], [1, 0], [0, 0]],
                              positive=np.array(["sed", "none"]), normalization=[["sed"], ["morph", "none"], []]).arrays(3, 2)
    assert a["sym_algorithm"].tolist() == [[1, 2]] * 3 and (a["sym_strength"] == 0.25).all()
    assert a["mono_nearest"].tolist() == [[0, 1], [1, 0], [0, 0]]
    assert a["positive"].tolist() == [[1, 0]] * 3
    assert a["normalize"].tolist() == [[_lib.NORM_SED, _lib.NORM_MORPH_MAX], [_lib.NORM_MORPH, _lib.NORM_NONE],
                                       [_lib.NORM_MORPH_MAX, _lib.NORM_MORPH_MAX]]
    assert scarlet.UpdateOptions(symmetry=_lib.SYM_SDSS).arrays(1, 1)["sym_algorithm"][0, 0] == _lib.SYM_SDSS
    kw = uc.update_kwargs("mixed", 3)
    a = scarlet.UpdateOptions(**kw).arrays(2, 3)
    assert a["sym_algorithm"].tolist() == [[0, 2, 1]] * 2 and a["mono_nearest"].tolist() == [[0, 1, 0]] * 2
    assert a["positive"].tolist() == [[3, 3, 2]] * 2 and np.allclose(a["mono_thresh"], [[0, 0, 0.05]] * 2)


@pytest.mark.parametrize("kwargs, word", [
    (dict(symmetry="fourier"), "symmetry"), (dict(symmetry=7), "symmetry"), (dict(symmetry=None), "symmetry"),
    (dict(strength=1.5), "strength"), (dict(strength=-0.1), "strength"), (dict(strength=float("nan")), "strength"),
    (dict(monotonic_thresh=1.0), "monotonic_thresh"), (dict(monotonic_thresh=-0.5), "monotonic_thresh"),
    (dict(use_nearest=True, monotonic_thresh=0.1), "nearest"), (dict(use_nearest=[0, 1], monotonic_thresh=[0.0, 0.2]), "nearest"),
    (dict(use_nearest="yes"), "use_nearest"),
    (dict(positive="all"), "positive"), (dict(positive=4), "positive"),
    (dict(normalization="max"), "normalization"), (dict(normalization=9), "normalization"),
    (dict(symmetry=["soft", "sdss", "kspace"]), "symmetry"), (dict(strength=[[0.5, 0.5]]), "strength"),
])
def test_update_options_refuses_bad_values(kwargs, word):
    import scarlet_amd as scarlet
    with pytest.raises(ValueError) as e:
        scarlet.UpdateOptions(**kwargs).arrays(3, 2)
    assert word in str(e.value)


# ---- 4. the C ABI
def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_struct_and_entry_points():
    text = _header()
    m = re.search(r"typedef struct scarlet_update_options \{(.*?)\} scarlet_update_options;", text, flags=re.S)
    assert m, "scarlet_update_options is not declared"
    assert re.findall(r"\*\s*(\w+)\s*;", m.group(1)) == FIELDS
    for f, ty in zip(FIELDS, ("uint8_t", "float", "uint8_t", "float", "uint8_t", "uint8_t")):
        assert re.search(r"const %s\s*\*\s*%s\s*;" % (ty, f), m.group(1)), f
    for fn in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(\s*scarlet_batch \*\w+,\s*const scarlet_constraints \*c\s*,\s*const scarlet_update_options \*o,"
                         % fn, text), fn
    for name, value in (("SCARLET_STATUS_BAD_OPTION", 32), ("SCARLET_NORM_NONE", 3), ("SCARLET_POSITIVE_SED", 1),
                        ("SCARLET_POSITIVE_MORPH", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), text), name


def test_library_exports_and_binding():
    from scarlet_amd import _lib
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(ln.split()[-1] for ln in out.splitlines() if ln.strip())
    for fn in ENTRY_POINTS:
        assert fn in exported and fn in _lib.EXPORTS, fn
        f = getattr(_lib.lib, fn)
        assert f.restype is ctypes.c_int
        assert [t._type_ for t in f.argtypes[:3]] == [_lib.ScarletBatch, _lib.ScarletConstraints, _lib.ScarletUpdateOptions]
    assert [f for f, _ in _lib.ScarletUpdateOptions._fields_] == FIELDS
    assert (_lib.STATUS_BAD_OPTION, _lib.NORM_NONE, _lib.POSITIVE_SED, _lib.POSITIVE_MORPH) == (32, 3, 1, 2)


def test_struct_offsets_match_the_c_compiler(tmp_path):
    from scarlet_amd import _lib
    src = tmp_path / "probe.c"
    body = "\n".join('printf("%s %%zu\\n", offsetof(scarlet_update_options, %s));' % (f, f) for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scarlet_hip.h"\n'
                   'int main(void){ printf("sizeof %zu\\n", sizeof(scarlet_update_options));\n'
                   'printf("batch %zu\\n", sizeof(scarlet_batch));\n' + body + '\nreturn 0;}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = {k: int(v) for k, v in (ln.split() for ln in subprocess.check_output([str(exe)]).decode().splitlines())}
    for i, f in enumerate(FIELDS):
        assert out[f] == 8 * i == getattr(_lib.ScarletUpdateOptions, f).offset, f
    assert out["sizeof"] == 48 == ctypes.sizeof(_lib.ScarletUpdateOptions)
    assert out["batch"] == 256 == ctypes.sizeof(_lib.ScarletBatch)          # scarlet_batch did not change


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
    band0 = (ctypes.c_int32 * 1)(0)

    def fit_obs(b, c, o):
        obs = (ctypes.POINTER(_lib.ScarletBatch) * 1)(ctypes.pointer(_batch()))
        return L.scarlet_fit_observations_options(b, c, o, obs, ctypes.cast(band0, ctypes.c_void_p), 1, 1, 0.0, 0, 0, None)

    return [
        ("scarlet_fit_options", lambda b, c, o: L.scarlet_fit_options(b, c, o, 1, 0.0, 0, 0, None)),
        ("scarlet_source_update_options", lambda b, c, o: L.scarlet_source_update_options(b, c, o, 1, None)),
        ("scarlet_fit_observations_options", fit_obs),
    ]


@pytest.mark.parametrize("which", range(3))
def test_refusals_before_any_launch(which):
    from scarlet_amd import _lib
    name, call = _calls()[which]
    o = _lib.ScarletUpdateOptions()
    o.mono_nearest = FAKE
    # NULL options
    assert call(ctypes.byref(_batch()), None, None) == _lib.E_ARG
    assert "options is NULL" in _lib.last_error()
    # group: layers are tied to soft symmetry
    g = _batch()
    g.group = FAKE
    assert call(ctypes.byref(g), None, ctypes.byref(o)) == _lib.E_NOTIMPL
    assert "group" in _lib.last_error()
    # the batch's own errors, whatever the struct holds; c may be NULL or given
    c = _lib.ScarletConstraints()
    for cp in (None, ctypes.byref(c)):
        assert call(ctypes.byref(_batch(pointers=False)), cp, ctypes.byref(o)) == _lib.E_ARG
        assert "null pointer in batch" in _lib.last_error()
    assert call(ctypes.byref(_batch(K=257)), None, ctypes.byref(o)) == _lib.E_NOTIMPL
    assert call(ctypes.byref(_batch(H=2048)), None, ctypes.byref(o)) == _lib.E_TOO_LARGE
    assert call(None, None, ctypes.byref(o)) == _lib.E_ARG
    c.symmetric = FAKE             # a symmetric array needs the centroid PSF, as in the _constrained entry points
    assert call(ctypes.byref(_batch()), ctypes.byref(c), ctypes.byref(o)) == _lib.E_ARG
    assert "centroid_psf" in _lib.last_error()


def test_wide_state_and_negative_iteration_count():
    from scarlet_amd import _lib
    o = _lib.ScarletUpdateOptions()
    o.normalize = FAKE
    fit_obs = _calls()[2][1]
    assert fit_obs(ctypes.byref(_batch(B=12)), None, ctypes.byref(o)) == _lib.E_NOTIMPL
    assert "wide" in _lib.last_error()
    assert _lib.lib.scarlet_fit_options(ctypes.byref(_batch()), None, ctypes.byref(o), -1, 0.0, 0, 0, None) == _lib.E_ARG
    assert "max_iter" in _lib.last_error()
