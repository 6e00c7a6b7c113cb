"""CPU: ragged frames (scenes of different frame sizes in one batch) at the C ABI and in the host layer.

scarlet_batch does not change: the shapes travel in struct scarlet_frames through the _frames entry points.  Checked
here: the struct mirror against the header (gcc offsetof), the status bit, the exports, and every refusal that is found on
the host before a launch."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scarlet_hip.h")
FAKE = 0x1000          # a non-NULL pointer that is never dereferenced (every call below returns before a launch)
ENTRY_POINTS = ("scarlet_fit_frames", "scarlet_source_update_frames", "scarlet_check_frames", "scarlet_init_extended_frames",
                "scarlet_init_sources_frames", "scarlet_batch_products_frames")


def test_struct_mirror_matches_header(tmp_path):
    from scarlet_amd import _lib
    src = tmp_path / "probe.c"
    fields = [f[0] for f in _lib.ScarletFrames._fields_]
    body = "\n".join('printf("%s %%zu\\n", offsetof(scarlet_frames, %s));' % (f, f) for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scarlet_hip.h"\n'
                   'int main(void){ printf("sizeof %zu\\n", sizeof(scarlet_frames));\n'
                   'printf("batch %zu\\n", sizeof(scarlet_batch));\n' + body + '\nreturn 0;}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert fields == ["frame_hw"]
    assert int(out["sizeof"]) == ctypes.sizeof(_lib.ScarletFrames) == 8
    assert int(out["frame_hw"]) == _lib.ScarletFrames.frame_hw.offset == 0
    assert int(out["batch"]) == ctypes.sizeof(_lib.ScarletBatch)          # scarlet_batch is as it was
    assert "frame_hw" not in [f for f, _ in _lib.ScarletBatch._fields_]


def test_status_bit_and_exports():
    from scarlet_amd import _lib
    text = open(HEADER).read()
    assert re.search(r"#define\s+SCARLET_STATUS_BAD_FRAME\s+16\b", text)
    assert _lib.STATUS_BAD_FRAME == 16
    assert not _lib.STATUS_BAD_FRAME & (_lib.STATUS_CENTER_AT_EDGE | _lib.STATUS_NONFINITE | _lib.STATUS_BAD_COUNT | _lib.STATUS_BAD_INIT)
    for name in ENTRY_POINTS:
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name), name


def _batch(S=4, K=3, B=5, H=32, W=32):
    from scarlet_amd import _lib
    b = _lib.ScarletBatch()
    b.S, b.K, b.B, b.H, b.W = S, K, B, H, W
    for f in ("images", "cur", "centers", "shifts", "flags", "lipschitz", "mse", "it", "active", "status", "workspace"):
        setattr(b, f, FAKE)
    for i in range(2):
        b.sed[i] = FAKE
        b.morph[i] = FAKE
    b.mse_capacity = 8
    return b


def test_c_abi_refusals_before_any_launch():
    from scarlet_amd import _lib
    lib = _lib.lib
    b, f = _batch(), _lib.ScarletFrames()
    f.frame_hw = FAKE
    bg = (ctypes.c_float * 5)(*([0.1] * 5))
    spec = _lib.ScarletInitSpec()
    spec.bg_rms = FAKE
    out = _lib.ScarletProducts()
    out.model = FAKE
    # a NULL struct
    for rc in (lib.scarlet_fit_frames(ctypes.byref(b), None, None, 1, 0.0, 0, 0, None),
               lib.scarlet_source_update_frames(ctypes.byref(b), None, None, 0, None),
               lib.scarlet_check_frames(ctypes.byref(b), None, None),
               lib.scarlet_init_extended_frames(ctypes.byref(b), None, bg, 1.0, None, 1, 1, 0, None),
               lib.scarlet_init_sources_frames(ctypes.byref(b), None, ctypes.byref(spec), None),
               lib.scarlet_batch_products_frames(ctypes.byref(b), None, ctypes.byref(out), None, 0, None)):
        assert rc == _lib.E_ARG and "frames" in _lib.last_error()
    # a NULL batch, a bad shape
    assert lib.scarlet_fit_frames(None, ctypes.byref(f), None, 1, 0.0, 0, 0, None) == _lib.E_ARG
    big = _batch(H=2048)
    assert lib.scarlet_fit_frames(ctypes.byref(big), ctypes.byref(f), None, 1, 0.0, 0, 0, None) == _lib.E_TOO_LARGE
    # group
    g = _batch()
    g.group = FAKE
    for rc in (lib.scarlet_fit_frames(ctypes.byref(g), ctypes.byref(f), None, 1, 0.0, 0, 0, None),
               lib.scarlet_source_update_frames(ctypes.byref(g), ctypes.byref(f), None, 0, None),
               lib.scarlet_check_frames(ctypes.byref(g), ctypes.byref(f), None),
               lib.scarlet_init_extended_frames(ctypes.byref(g), ctypes.byref(f), bg, 1.0, None, 1, 1, 0, None),
               lib.scarlet_init_sources_frames(ctypes.byref(g), ctypes.byref(f), ctypes.byref(spec), None)):
        assert rc == _lib.E_NOTIMPL and "group" in _lib.last_error()
    with pytest.raises(NotImplementedError):
        _lib.check(_lib.E_NOTIMPL)
    # init_sources: extended sources only
    spec.kind = FAKE
    rc = lib.scarlet_init_sources_frames(ctypes.byref(b), ctypes.byref(f), ctypes.byref(spec), None)
    assert rc == _lib.E_NOTIMPL and "kind" in _lib.last_error()
    # max_iter < 0 is still an argument error
    assert lib.scarlet_fit_frames(ctypes.byref(b), ctypes.byref(f), None, -1, 0.0, 0, 0, None) == _lib.E_ARG


def _scenes():
    rng = np.random.default_rng(3)
    return [rng.normal(size=(3, 20, 24)).astype(np.float32), rng.normal(size=(3, 17, 23)).astype(np.float32)]


def test_host_refusals_need_no_device():
    """ValueError / NotImplementedError of BlendBatch for a ragged-frame batch are raised before the device is asked for"""
    import scarlet_amd as sc
    from scarlet_amd.batch import pad_frames
    ims = _scenes()
    cen = np.array([[[10, 10]], [[8, 9]]], np.int32)
    block, shapes = pad_frames(ims)
    with pytest.raises(ValueError, match="frame_shapes"):
        sc.BlendBatch(ims, cen, frame_shapes=shapes)                            # a list carries its own shapes
    with pytest.raises(ValueError, match="bands"):
        sc.BlendBatch([ims[0], ims[1][:2]], cen)                                # differing B
    for bad in ([[0, 24], [17, 23]], [[20, 24], [21, 23]], [[20, 24], [17, 25]], [[20, 24], [17, -1]]):
        with pytest.raises(ValueError, match="lies outside 1.."):
            sc.BlendBatch(block, cen, frame_shapes=np.array(bad))
    with pytest.raises(ValueError, match="frame_shapes must be"):
        sc.BlendBatch(block, cen, frame_shapes=np.array([20, 24]))
    with pytest.raises(ValueError, match="frame_shapes must be"):
        sc.BlendBatch(block, cen, frame_shapes=np.array([[20.0, 24.0], [17.0, 23.0]]))
    # a centre inside the padded plane but outside its scene's own frame
    for c in ([[17, 9]], [[8, 23]]):
        with pytest.raises(ValueError, match="outside the scene's 17 x 23 frame"):
            sc.BlendBatch(ims, np.array([[[10, 10]], c], np.int32))
    # ... of any present component
    with pytest.raises(ValueError, match="outside the scene's 17 x 23 frame"):
        sc.BlendBatch(ims, np.array([[[10, 10], [5, 5]], [[16, 22], [19, 23]]], np.int32), n_components=np.array([2, 2]))
    with pytest.raises(ValueError, match="weights"):
        sc.BlendBatch(ims, cen, weights=[np.ones((3, 20, 24)), np.ones((3, 17, 22))])
    with pytest.raises(NotImplementedError, match="group"):
        sc.BlendBatch(ims, cen, group=np.array([[-1], [-1]]))
    with pytest.raises(NotImplementedError, match="group"):
        sc.BlendBatch(block, cen, frame_shapes=shapes, group=np.array([[-1], [-1]]))
    with pytest.raises(NotImplementedError, match="from_observations"):
        sc.BlendBatch.from_observations([sc.ObservationBatch(block)], cen, frame_shapes=shapes)


def test_uniform_batch_is_untouched_by_the_keyword():
    """frame_shapes=None: the constructor goes straight to the device check, as it always did"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import scarlet_amd as sc
    with pytest.raises(RuntimeError):
        sc.BlendBatch(np.zeros((1, 5, 16, 16), np.float32), np.zeros((1, 1, 2), np.int32) + 8, frame_shapes=None)
    # a valid ragged-frame batch passes the host checks and then needs the device
    with pytest.raises(RuntimeError):
        sc.BlendBatch(_scenes(), np.array([[[10, 10]], [[8, 9]]], np.int32))
