"""CPU: the C ABI of catalogue batches -- ragged frames with multi-component sources (b->group) and point sources.

Three entry points beside the ragged-frames block: scarlet_fit_frames_grouped, scarlet_source_update_frames_grouped and
scarlet_init_sources_frames_mixed.  Checked here: the exports and their signatures, that no struct changed size, and
every refusal that is found on the host before a launch (the pointers are never dereferenced).  The pinned entry points
keep refusing frame_hw with group: tests/test_frames_abi.py."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scarlet_hip.h")
FAKE = 0x1000          # a non-NULL pointer that is never dereferenced (every call below returns before a launch)
NEW = ("scarlet_fit_frames_grouped", "scarlet_source_update_frames_grouped", "scarlet_init_sources_frames_mixed")


def _batch(S=4, K=3, B=5, H=32, W=32, group=True):
    from scarlet_amd import _lib
    b = _lib.ScarletBatch()
    b.S, b.K, b.B, b.H, b.W = S, K, B, H, W
    for f in ("images", "cur", "centers", "shifts", "flags", "lipschitz", "mse", "it", "active", "status", "workspace"):
        setattr(b, f, FAKE)
    for i in range(2):
        b.sed[i] = FAKE
        b.morph[i] = FAKE
    b.mse_capacity = 8
    if group:
        b.group = FAKE
    return b


def test_exports_signatures_and_header():
    from scarlet_amd import _lib
    text = open(HEADER).read()
    P, c_int = ctypes.POINTER, ctypes.c_int
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert getattr(_lib.lib, name).restype is c_int
    head = [P(_lib.ScarletBatch), P(_lib.ScarletFrames)]
    assert _lib.lib.scarlet_fit_frames_grouped.argtypes == _lib.lib.scarlet_fit_frames.argtypes
    assert _lib.lib.scarlet_fit_frames_grouped.argtypes[:3] == head + [P(_lib.ScarletConstraints)]
    assert _lib.lib.scarlet_source_update_frames_grouped.argtypes == _lib.lib.scarlet_source_update_frames.argtypes
    assert _lib.lib.scarlet_init_sources_frames_mixed.argtypes == _lib.lib.scarlet_init_sources_frames.argtypes
    assert _lib.lib.scarlet_init_sources_frames_mixed.argtypes[:3] == head + [P(_lib.ScarletInitSpec)]
    # the sentence that lists what ragged batches do not take names the new route
    assert "scarlet_fit_frames_grouped, scarlet_source_update_frames_grouped" in text


def test_null_frames_is_an_argument_error():
    from scarlet_amd import _lib
    lib = _lib.lib
    spec = _lib.ScarletInitSpec()
    spec.bg_rms = FAKE
    for group in (True, False):
        b = _batch(group=group)
        for rc in (lib.scarlet_fit_frames_grouped(ctypes.byref(b), None, None, 1, 0.0, 0, 0, None),
                   lib.scarlet_source_update_frames_grouped(ctypes.byref(b), None, None, 0, None),
                   lib.scarlet_init_sources_frames_mixed(ctypes.byref(b), None, ctypes.byref(spec), None)):
            assert rc == _lib.E_ARG and "frames is NULL" in _lib.last_error()


def test_host_checks_run_before_any_launch():
    from scarlet_amd import _lib
    lib = _lib.lib
    f = _lib.ScarletFrames()
    f.frame_hw = FAKE
    b = _batch()
    spec = _lib.ScarletInitSpec()
    spec.bg_rms = FAKE
    # a NULL batch
    assert lib.scarlet_fit_frames_grouped(None, ctypes.byref(f), None, 1, 0.0, 0, 0, None) == _lib.E_ARG
    assert lib.scarlet_source_update_frames_grouped(None, ctypes.byref(f), None, 0, None) == _lib.E_ARG
    assert lib.scarlet_init_sources_frames_mixed(None, ctypes.byref(f), ctypes.byref(spec), None) == _lib.E_ARG
    # a frame beyond the engine's largest side
    big = _batch(H=2048)
    assert lib.scarlet_fit_frames_grouped(ctypes.byref(big), ctypes.byref(f), None, 1, 0.0, 0, 0, None) == _lib.E_TOO_LARGE
    assert lib.scarlet_source_update_frames_grouped(ctypes.byref(big), ctypes.byref(f), None, 0, None) == _lib.E_TOO_LARGE
    assert lib.scarlet_init_sources_frames_mixed(ctypes.byref(big), ctypes.byref(f), ctypes.byref(spec), None) == _lib.E_TOO_LARGE
    # max_iter < 0
    assert lib.scarlet_fit_frames_grouped(ctypes.byref(b), ctypes.byref(f), None, -1, 0.0, 0, 0, None) == _lib.E_ARG
    assert "max_iter" in _lib.last_error()
    # per-component symmetry needs the centroid PSF (the batch here has none)
    c = _lib.ScarletConstraints()
    c.symmetric = FAKE
    assert lib.scarlet_fit_frames_grouped(ctypes.byref(b), ctypes.byref(f), ctypes.byref(c), 1, 0.0, 0, 0, None) == _lib.E_ARG
    assert "centroid_psf" in _lib.last_error()
    assert lib.scarlet_source_update_frames_grouped(ctypes.byref(b), ctypes.byref(f), ctypes.byref(c), 0, None) == _lib.E_ARG
    # the init spec: NULL, no bg_rms, a model PSF without a centre pixel -- with frame_hw and without
    for fr in (f, _lib.ScarletFrames()):
        assert lib.scarlet_init_sources_frames_mixed(ctypes.byref(b), ctypes.byref(fr), None, None) == _lib.E_ARG
        assert "spec" in _lib.last_error()
        empty = _lib.ScarletInitSpec()
        assert lib.scarlet_init_sources_frames_mixed(ctypes.byref(b), ctypes.byref(fr), ctypes.byref(empty), None) == _lib.E_ARG
        assert "bg_rms" in _lib.last_error()
        even = _lib.ScarletInitSpec()
        even.bg_rms, even.model_psf, even.model_psf_P, even.kind = FAKE, FAKE, 4, FAKE
        assert lib.scarlet_init_sources_frames_mixed(ctypes.byref(b), ctypes.byref(fr), ctypes.byref(even), None) == _lib.E_ARG
        assert "model_psf" in _lib.last_error()


def test_structs_keep_their_sizes(tmp_path):
    """no struct of the header grew: the new entry points take the existing ones"""
    import subprocess
    from scarlet_amd import _lib
    names = dict(scarlet_batch=_lib.ScarletBatch, scarlet_frames=_lib.ScarletFrames, scarlet_init_spec=_lib.ScarletInitSpec,
                 scarlet_constraints=_lib.ScarletConstraints, scarlet_products=_lib.ScarletProducts)
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "scarlet_hip.h"\nint main(void){\n'
                   + "\n".join('printf("%s %%zu\\n", sizeof(%s));' % (n, n) for n in names) + "\nreturn 0;}\n")
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    for n, mirror in names.items():
        assert int(out[n]) == ctypes.sizeof(mirror), n
    assert int(out["scarlet_frames"]) == 8
