"""CPU: low-resolution observations of scenes with their own frames at the C ABI (struct scarlet_lowres_frames,
scarlet_fit_observations_frames_lowres, scarlet_observations_products_frames_lowres) and in the host layer
(LowResObservationBatch.from_frames(geometry=), BlendBatch.from_observations).  Every C call below returns before a
launch; every Python refusal is raised before a device is asked for (on a host without a GPU a refusal that came late
would be a RuntimeError instead)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import lowres_frame_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scarlet_hip.h")
FAKE = 0x1000          # a non-NULL pointer that is never dereferenced
NAMES = ("scarlet_fit_observations_frames_lowres", "scarlet_observations_products_frames_lowres")


def _batch(S=4, K=3, B=5, H=32, W=32, pointers=True):
    from scarlet_amd import _lib
    b = _lib.ScarletBatch()
    b.S, b.K, b.B, b.H, b.W = S, K, B, H, W
    if pointers:
        for f in ("images", "cur", "centers", "shifts", "flags", "lipschitz", "mse", "it", "active", "status", "workspace"):
            setattr(b, f, FAKE)
        b.sed[0] = b.sed[1] = b.morph[0] = b.morph[1] = FAKE
        b.mse_capacity = 1
    return b


def _frames(ptr=FAKE):
    from scarlet_amd import _lib
    f = _lib.ScarletFrames()
    f.frame_hw = ptr
    return f


def _lowres(per_scene=1, **kw):
    from scarlet_amd import _lib
    lr = _lib.ScarletLowres()
    lr.h, lr.w, lr.nfy, lr.nfx, lr.B = 16, 16, 9, 17, 2
    for f in ("uy", "ux", "vy", "vx", "dhat", "workspace"):
        setattr(lr, f, FAKE)
    lr.v_per_scene = lr.dhat_per_scene = per_scene
    for k, v in kw.items():
        setattr(lr, k, v)
    return lr


def _tables(**kw):
    from scarlet_amd import _lib
    lf = _lib.ScarletLowresFrames()
    lf.dims = lf.uy = lf.ux = FAKE
    for k, v in kw.items():
        setattr(lf, k, v)
    return lf


def _lists(obs, lows, tables, band0):
    from scarlet_amd import _lib
    arr = (ctypes.POINTER(_lib.ScarletBatch) * len(obs))(*[ctypes.pointer(o) for o in obs])
    lo = (ctypes.POINTER(_lib.ScarletLowres) * len(obs))(*[ctypes.POINTER(_lib.ScarletLowres)() if x is None else ctypes.pointer(x)
                                                            for x in lows])
    tb = (ctypes.POINTER(_lib.ScarletLowresFrames) * len(obs))(
        *[ctypes.POINTER(_lib.ScarletLowresFrames)() if x is None else ctypes.pointer(x) for x in tables])
    return arr, lo, tb, np.asarray(band0, dtype=np.int32)


def _fit(state, f, obs, lows, tables, band0, null_lists=()):
    from scarlet_amd import _lib
    arr, lo, tb, b0 = _lists(obs, lows, tables, band0)
    return _lib.lib.scarlet_fit_observations_frames_lowres(
        ctypes.byref(state), None if f is None else ctypes.byref(f), None, arr, None if "lowres" in null_lists else lo,
        None if "tables" in null_lists else tb, b0.ctypes.data_as(ctypes.c_void_p), len(obs), 1, 0.0, 0, 0, None)


def _products(state, f, obs, lows, tables, band0, null_lists=()):
    from scarlet_amd import _lib
    arr, lo, tb, b0 = _lists(obs, lows, tables, band0)
    outs = (_lib.ScarletProducts * len(obs))()
    for o in outs:
        o.rendered = FAKE
    return _lib.lib.scarlet_observations_products_frames_lowres(
        ctypes.byref(state), None if f is None else ctypes.byref(f), arr, None if "lowres" in null_lists else lo,
        None if "tables" in null_lists else tb, b0.ctypes.data_as(ctypes.c_void_p), len(obs), None, outs, None, 0, None)


def test_symbols_header_and_ctypes_agree(tmp_path):
    from scarlet_amd import _lib
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S))
    assert ("int scarlet_fit_observations_frames_lowres(scarlet_batch *state, const scarlet_frames *f, const scarlet_constraints *c , "
            "scarlet_batch *const *obs, const scarlet_lowres *const *lowres, const scarlet_lowres_frames *const *lowres_frames, "
            "const int32_t *band0, int n_obs, int max_iter, double e_rel, int approximate_L, int check_every, void *stream);") in flat
    assert ("int scarlet_observations_products_frames_lowres(const scarlet_batch *state, const scarlet_frames *f, "
            "scarlet_batch *const *obs, const scarlet_lowres *const *lowres, const scarlet_lowres_frames *const *lowres_frames, "
            "const int32_t *band0, int n_obs, const scarlet_products *state_out, const scarlet_products *out, void *scratch, "
            "int64_t scratch_bytes, void *stream);") in flat
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name), name
        assert getattr(_lib.lib, name).restype is ctypes.c_int
    # the arguments of the same-grid frames entry points with the two lists after the observations
    lists = [ctypes.POINTER(ctypes.POINTER(_lib.ScarletLowres)), ctypes.POINTER(ctypes.POINTER(_lib.ScarletLowresFrames))]
    fit, plain = _lib.lib.scarlet_fit_observations_frames_lowres.argtypes, _lib.lib.scarlet_fit_observations_frames.argtypes
    assert list(fit) == list(plain[:4]) + lists + list(plain[4:])
    prod, plain = _lib.lib.scarlet_observations_products_frames_lowres.argtypes, _lib.lib.scarlet_observations_products_frames.argtypes
    assert list(prod) == list(plain[:3]) + lists + list(plain[3:])
    # the struct as the C compiler lays it out; scarlet_lowres and scarlet_frames are as they were
    fields = [f for f, _ in _lib.ScarletLowresFrames._fields_]
    assert fields == ["dims", "uy", "ux"]
    src = tmp_path / "probe.c"
    body = "\n".join('printf("%s %%zu\\n", offsetof(scarlet_lowres_frames, %s));' % (f, f) for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scarlet_hip.h"\n'
                   'int main(void){ printf("sizeof %zu\\n", sizeof(scarlet_lowres_frames));\n'
                   'printf("lowres %zu\\n", sizeof(scarlet_lowres));\nprintf("frames %zu\\n", sizeof(scarlet_frames));\n'
                   + body + '\nreturn 0;}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = {k: int(v) for k, v in (ln.split() for ln in subprocess.check_output([str(exe)]).decode().splitlines())}
    assert out["sizeof"] == 24 == ctypes.sizeof(_lib.ScarletLowresFrames)
    for f in fields:
        assert out[f] == getattr(_lib.ScarletLowresFrames, f).offset, f
    assert out["lowres"] == 80 == ctypes.sizeof(_lib.ScarletLowres)
    assert out["frames"] == 8 == ctypes.sizeof(_lib.ScarletFrames)


@pytest.mark.parametrize("call", [_fit, _products], ids=["fit", "products"])
def test_c_refusals_before_any_launch(call):
    from scarlet_amd import _lib
    st, f = _batch(), _frames()
    hi, lo = _batch(B=3), _batch(B=2, H=16, W=16)
    lr, tb = _lowres(), _tables()
    args = ([hi, lo], [None, lr], [None, tb], [0, 3])
    assert call(st, None, *args) == _lib.E_ARG and "frames" in _lib.last_error()
    # null lists, null tables
    assert call(st, f, *args, null_lists=("lowres",)) == _lib.E_ARG and "low-resolution list" in _lib.last_error()
    assert call(st, f, *args, null_lists=("tables",)) == _lib.E_ARG and "low-resolution list" in _lib.last_error()
    for field in ("dims", "uy", "ux"):
        assert call(st, f, [hi, lo], [None, lr], [None, _tables(**{field: None})], [0, 3]) == _lib.E_ARG
        assert "null table" in _lib.last_error()
    # tables without the operator they belong to (here: beside a same-grid observation), and without frame_hw
    assert call(st, f, [hi, _batch(B=2)], [None, None], [None, tb], [0, 3]) == _lib.E_ARG
    assert "no scarlet_lowres" in _lib.last_error()
    assert call(st, _frames(None), *args) == _lib.E_ARG and "without frame_hw" in _lib.last_error()
    # the per-scene flags
    for flag in ("v_per_scene", "dhat_per_scene"):
        assert call(st, f, [hi, lo], [None, _lowres(**{flag: 0})], [None, tb], [0, 3]) == _lib.E_ARG
        assert "v_per_scene = dhat_per_scene = 1" in _lib.last_error()
    # frame_hw with a low-resolution observation that brings no tables: the operator of the padded frame
    assert call(st, f, [hi, lo], [None, lr], [None, None], [0, 3]) == _lib.E_NOTIMPL
    assert "scarlet_lowres_frames" in _lib.last_error()
    # group
    g = _batch()
    g.group = FAKE
    assert call(g, f, *args) == _lib.E_NOTIMPL and "group" in _lib.last_error()
    # the checks of the uniform low-resolution entry points stay: a null factor matrix, a shape that does not fit
    assert call(st, f, [hi, lo], [None, _lowres(vy=None)], [None, tb], [0, 3]) == _lib.E_ARG
    assert "null factor matrix" in _lib.last_error()
    assert call(st, f, [hi, _batch(B=2, H=16, W=12)], [None, lr], [None, tb], [0, 3]) == _lib.E_ARG
    assert "does not fit" in _lib.last_error()


def _small(B=2, band0=3):
    geos = list(fc.geometries("small", band0=band0))
    images = [np.zeros((B,) + tuple(g.frame.shape[1:]), np.float32) for g in geos]
    return geos, images


def test_host_value_errors_before_a_device_is_asked_for():
    from scarlet_amd import LowResObservation, LowResObservationBatch
    geos, images = _small()
    ok = LowResObservationBatch.from_frames(images, band0=3, geometry=geos)
    assert ok.dims.shape == (5, 6)
    with pytest.raises(ValueError, match="list of"):
        LowResObservationBatch.from_frames(np.zeros((5, 2, 16, 16), np.float32), geometry=geos)
    with pytest.raises(ValueError, match="4 geometries for S = 5"):
        LowResObservationBatch.from_frames(images, geometry=geos[:4])
    with pytest.raises(ValueError, match="list of S geometries"):
        LowResObservationBatch(ok.images, 3, geometry=geos[0], frame_shapes=ok.frame_shapes)
    with pytest.raises(ValueError, match="from_frames takes a list"):
        LowResObservationBatch(images, 3, geometry=geos, frame_shapes=ok.frame_shapes)
    # a geometry that is not matched, and one that does not cover its observation
    g = geos[1]
    raw = LowResObservation(np.zeros(g.frame.shape, np.float32), wcs=g.frame.wcs, psfs=np.asarray(g.frame.psfs.image))
    with pytest.raises(ValueError, match="after match"):
        LowResObservationBatch.from_frames(images, geometry=[geos[0], raw] + geos[2:])
    m, o, r, org = fc.CASES["small"][1][1]
    outside = fc.geometry(m, o, r, (org[0] + 3.0, org[1]), 2)
    assert not outside.covers
    with pytest.raises(ValueError, match="lie inside the model frame"):
        LowResObservationBatch.from_frames(images, geometry=[geos[0], outside] + geos[2:])
    # a geometry whose observation shape is not the image's
    with pytest.raises(ValueError, match="scene 1's images are .* its geometry describes"):
        LowResObservationBatch.from_frames(images, geometry=[geos[0], geos[0]] + geos[2:])
    # another band count, another model PSF
    three = fc.geometry(*fc.CASES["small"][1][2], 3, band0=2)
    with pytest.raises(ValueError, match="scene 2's images are"):
        LowResObservationBatch.from_frames(images, geometry=geos[:2] + [three] + geos[3:])
    import lowres_common as lc
    import scarlet_amd as scarlet
    wm, wl = lc.wcs_pair(m, o, r, org)
    frame = scarlet.Frame((5,) + m, wcs=wm, psfs=lc.gauss(11, 1.1)[None].astype(np.float32), channels=["c%d" % c for c in range(5)])
    other = LowResObservation(np.zeros((2,) + o, np.float32), wcs=wl, psfs=lc.limit_psfs(fc.PSF_PX, 2)[1],
                              channels=["c3", "c4"]).match(frame)
    with pytest.raises(ValueError, match="share the model PSF"):
        LowResObservationBatch.from_frames(images, geometry=[geos[0], other] + geos[2:])


def _hi(geos, shapes=None):
    from scarlet_amd import ObservationBatch
    shapes = [tuple(g.model_shape) for g in geos] if shapes is None else shapes
    return ObservationBatch.from_frames([np.zeros((3,) + s, np.float32) for s in shapes])


def test_from_observations_refusals_before_a_device_is_asked_for():
    from scarlet_amd import BlendBatch, LowResObservationBatch
    geos, images = _small()
    lo = LowResObservationBatch.from_frames(images, band0=3, geometry=geos)
    centers = [np.array([[5, 5]])] * 5
    # the geometries must be matched to the same-grid observations' frames: observation and first such scene are named
    shapes = [tuple(g.model_shape) for g in geos]
    shapes[2] = (18, 23)
    with pytest.raises(ValueError, match=r"low-resolution observation 1 was matched to a 17 x 23 model frame in scene 2, "
                                         r"observation 0 has that scene at 18 x 23"):
        BlendBatch.from_observations([_hi(geos, shapes), lo], centers)
    # a centre outside its scene's own model frame
    with pytest.raises(ValueError, match="scene 2"):
        BlendBatch.from_observations([_hi(geos), lo], centers[:2] + [np.array([[17, 3]])] + centers[3:])
    # low-resolution observations only: nothing carries the model frames
    with pytest.raises(NotImplementedError, match="low-resolution observations only"):
        BlendBatch.from_observations([lo], centers)
    # beside same-grid observations without frame shapes
    from scarlet_amd import ObservationBatch
    with pytest.raises(ValueError, match="carries frame shapes"):
        BlendBatch.from_observations([ObservationBatch(np.zeros((5, 3, 32, 32), np.float32)), lo], centers)
    # the refusals of ragged joint batches stay
    with pytest.raises(NotImplementedError, match="group"):
        BlendBatch.from_observations([_hi(geos), lo], centers, group=np.full((5, 1), -1))
    with pytest.raises(NotImplementedError, match="host-gradient"):
        BlendBatch.from_observations([_hi(geos), lo], centers, _host_gradients=True)
    with pytest.raises(NotImplementedError, match="frame_shapes"):
        BlendBatch.from_observations([_hi(geos), lo], centers, frame_shapes=np.array(shapes))
    with pytest.raises(NotImplementedError):
        LowResObservationBatch.from_frames(images)
    # a low-resolution observation without frame shapes of its own: one geometry, or a list matched to one frame
    full = fc.geometry((32, 32), (16, 16), 2.0, (0.0, 0.0), 2)
    for geometry in (full, [full] * 5):
        uniform = LowResObservationBatch(np.zeros((5, 2, 16, 16), np.float32), band0=3, geometry=geometry)
        with pytest.raises(NotImplementedError, match="low-resolution observation \\(observation 1\\)"):
            BlendBatch.from_observations([_hi(geos), uniform], centers)


def test_valid_input_passes_the_host_checks():
    """... and then needs the device, as a uniform joint batch does"""
    import torch
    from scarlet_amd import BlendBatch, LowResObservationBatch
    geos, images = _small()
    lo = LowResObservationBatch.from_frames(images, band0=3, geometry=geos, weights=[np.ones_like(a) for a in images])
    centers = [np.array([[5, 5]])] * 5
    if torch.cuda.is_available():
        b = BlendBatch.from_observations([_hi(geos), lo], centers, lowres_products=True)
        assert b.frame_shapes is not None and b._lowres[1] is not None and "frames" in b._lowres[1][1]
    else:
        with pytest.raises(RuntimeError, match="ROCm device"):
            BlendBatch.from_observations([_hi(geos), lo], centers)
