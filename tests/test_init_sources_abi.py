"""CPU: the C ABI of scarlet_init_sources (mixed source types, per-scene noise and PSF peaks).

The header declares the entry point and its spec struct, the ctypes mirror matches the C compiler's layout, the
constants agree, argument errors come back as SCARLET_E_ARG before anything is launched, and scarlet_batch keeps
its size."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scarlet_hip.h")
FAKE = 0x1000          # a non-NULL pointer that is never dereferenced (every call below returns before a launch)


def _header():
    return open(HEADER).read()


def test_header_declares_init_sources():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"int\s+scarlet_init_sources\s*\(\s*scarlet_batch\s*\*\s*b\s*,\s*const\s+scarlet_init_spec\s*\*",
                     text)
    from scarlet_amd import _lib
    assert "scarlet_init_sources" in _lib.EXPORTS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "scarlet_init_sources")


def test_constants_match_header():
    from scarlet_amd import _lib
    text = _header()
    for name, value in (("SCARLET_INIT_EXTENDED", _lib.INIT_EXTENDED), ("SCARLET_INIT_POINT", _lib.INIT_POINT),
                        ("SCARLET_MAX_LAYERS", _lib.MAX_LAYERS), ("SCARLET_STATUS_BAD_INIT", _lib.STATUS_BAD_INIT)):
        m = re.search(r"#define\s+%s\s+(\d+)\b" % name, text)
        assert m and int(m.group(1)) == value, name
    assert (_lib.INIT_EXTENDED, _lib.INIT_POINT, _lib.MAX_LAYERS, _lib.STATUS_BAD_INIT) == (0, 1, 8, 8)
    # a status bit of its own
    assert _lib.STATUS_BAD_INIT not in (_lib.STATUS_CENTER_AT_EDGE, _lib.STATUS_NONFINITE, _lib.STATUS_BAD_COUNT)


def test_spec_layout_matches_header(tmp_path):
    """sizeof/offsetof of scarlet_init_spec compiled as C == the ctypes mirror; scarlet_batch is still 256 bytes"""
    from scarlet_amd import _lib
    fields = [f[0] for f in _lib.ScarletInitSpec._fields_]
    src = tmp_path / "probe.c"
    body = "\n".join('printf("%s %%zu\\n", offsetof(scarlet_init_spec, %s));' % (f, f) for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scarlet_hip.h"\n'
                   'int main(void){ printf("sizeof %zu\\n", sizeof(scarlet_init_spec));\n'
                   'printf("batch %zu\\n", sizeof(scarlet_batch));\n' + body + '\nreturn 0;}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = {k: int(v) for k, v in (ln.split() for ln in subprocess.check_output([str(exe)]).decode().splitlines())}
    assert out["sizeof"] == ctypes.sizeof(_lib.ScarletInitSpec)
    for f in fields:
        assert out[f] == getattr(_lib.ScarletInitSpec, f).offset, f
    assert out["batch"] == 256 == ctypes.sizeof(_lib.ScarletBatch)


def _fake_batch():
    from scarlet_amd import _lib
    b = _lib.ScarletBatch()
    b.S, b.K, b.B, b.H, b.W = 2, 3, 5, 32, 32
    for f in ("images", "cur", "centers", "shifts", "flags", "lipschitz", "mse", "it", "active", "status", "workspace"):
        setattr(b, f, FAKE)
    b.sed[0] = b.sed[1] = b.morph[0] = b.morph[1] = FAKE
    b.symmetric = 0
    return b


@pytest.mark.parametrize("case", ["null_batch", "null_spec", "null_bg", "even_psf", "bad_shape", "null_images"])
def test_bad_arguments_return_e_arg(case):
    from scarlet_amd import _lib
    b = _fake_batch()
    spec = _lib.ScarletInitSpec()
    spec.bg_rms = FAKE
    bp, sp = ctypes.byref(b), ctypes.byref(spec)
    if case == "null_batch":
        bp = None
    elif case == "null_spec":
        sp = None
    elif case == "null_bg":
        spec.bg_rms = None
    elif case == "even_psf":
        spec.model_psf, spec.model_psf_P = FAKE, 4
    elif case == "bad_shape":
        b.H = 0
    elif case == "null_images":
        b.images = None
    rc = _lib.lib.scarlet_init_sources(bp, sp, None)
    assert rc == _lib.E_ARG and _lib.last_error()
    with pytest.raises(ValueError):
        _lib.check(rc)
