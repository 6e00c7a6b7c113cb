"""CPU: the products entry points of include/scarlet_hip.h -- exported, mirrored by ctypes as gcc lays the struct out, and
every argument error answered with SCARLET_E_ARG and a message on the host (there is no device here: a call that went
past its checks would come back with SCARLET_E_HIP instead)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("scarlet_products_scratch_bytes", "scarlet_batch_products", "scarlet_observations_products")
FAKE = 0x1000         # a non-NULL "device pointer": the checks compare against NULL and never dereference


@pytest.fixture(scope="module")
def _lib():
    from scarlet_amd import _lib
    return _lib


def fake_batch(_lib, S=3, K=2, B=3, H=21, W=25, psf=0):
    b = _lib.ScarletBatch()
    b.S, b.K, b.B, b.H, b.W = S, K, B, H, W
    b.images = b.cur = b.workspace = FAKE
    b.sed[0] = b.sed[1] = b.morph[0] = b.morph[1] = FAKE
    b.weight_scalar = 1.0
    if psf:
        b.diff_kernel, b.psf_h, b.psf_w = FAKE, psf, psf
    return b


def products(_lib, **fields):
    p = _lib.ScarletProducts()
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def test_library_exports_the_products_symbols(_lib):
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in _lib.EXPORTS


def test_products_struct_layout_matches_header(_lib, tmp_path):
    src = tmp_path / "probe.c"
    fields = [f[0] for f in _lib.ScarletProducts._fields_]
    body = "\n".join('printf("%s %%zu\\n", offsetof(scarlet_products, %s));' % (f, f) for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scarlet_hip.h"\n'
                   'int main(void){ printf("sizeof %zu\\n", sizeof(scarlet_products));\n' + body + '\nreturn 0;}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out["sizeof"]) == ctypes.sizeof(_lib.ScarletProducts) == 64
    for f in fields:
        assert int(out[f]) == getattr(_lib.ScarletProducts, f).offset, f


def test_scratch_query(_lib):
    q = _lib.lib.scarlet_products_scratch_bytes
    b = fake_batch(_lib)
    p = products(_lib, loss=FAKE)
    assert q(None, ctypes.byref(p)) == 0 and q(ctypes.byref(b), None) == 0 and q(None, None) == 0
    # the loss leaves the one-pass kernel as float64 tile partials [S][T][B]
    assert q(ctypes.byref(b), ctypes.byref(p)) >= 8 * 3 * 1 * 3
    assert q(ctypes.byref(b), ctypes.byref(products(_lib, model=FAKE))) == 0
    # a PSF batch without a `model` output stages the unconvolved planes in chunks of scenes: never more than 256 MiB
    # of them, whatever the batch (BASELINE config 3 would need 1.3 GB)
    big = fake_batch(_lib, S=4096, K=8, B=5, H=128, W=128, psf=41)
    staged = q(ctypes.byref(big), ctypes.byref(products(_lib, rendered=FAKE)))
    assert 128 * 128 * 4 * 5 <= staged <= (256 << 20) + 4096
    assert q(ctypes.byref(big), ctypes.byref(products(_lib, rendered=FAKE, model=FAKE))) == 0


def test_argument_errors_come_back_before_any_device_call(_lib):
    call = _lib.lib.scarlet_batch_products
    b = fake_batch(_lib)
    ok = products(_lib, loss=FAKE)
    nbytes = _lib.lib.scarlet_products_scratch_bytes(ctypes.byref(b), ctypes.byref(ok))
    sel = np.array([0, 2], dtype=np.int32)           # K = 2: index 2 is outside

    def refused(batch, out, scratch=FAKE, scratch_bytes=1 << 30):
        rc = call(None if batch is None else ctypes.byref(batch), None if out is None else ctypes.byref(out), scratch,
                  scratch_bytes, None)
        assert rc == _lib.E_ARG, (rc, _lib.last_error())
        assert _lib.last_error()
        with pytest.raises(ValueError):
            _lib.check(rc)
        return _lib.last_error()

    refused(None, ok)
    refused(b, None)
    assert "every output" in refused(b, products(_lib))
    assert "n_select" in refused(b, products(_lib, loss=FAKE, n_select=-1))
    assert "outside" in refused(b, products(_lib, component_models=FAKE, components=sel.ctypes.data, n_select=2))
    assert "outside" in refused(b, products(_lib, component_models=FAKE, n_select=3))      # NULL: 0 .. n_select - 1
    assert "selection" in refused(b, products(_lib, component_models=FAKE))
    assert "scratch" in refused(b, ok, scratch=FAKE, scratch_bytes=nbytes - 1)
    assert "scratch" in refused(b, ok, scratch=None, scratch_bytes=nbytes)
    noimg = fake_batch(_lib)
    noimg.images = None
    assert "images" in refused(noimg, ok)


def test_observations_argument_errors(_lib):
    call = _lib.lib.scarlet_observations_products
    state, ob = fake_batch(_lib, B=5), fake_batch(_lib, B=3)
    ptrs = (ctypes.POINTER(_lib.ScarletBatch) * 1)(ctypes.pointer(ob))
    band0 = np.array([3], dtype=np.int32)            # channels 3 .. 5 of a 5-channel state
    outs = (_lib.ScarletProducts * 1)()
    outs[0].loss = FAKE
    args = (ptrs, band0.ctypes.data, 1)
    assert call(None, *args, None, outs, FAKE, 1 << 30, None) == _lib.E_ARG
    assert call(ctypes.byref(state), *args, None, outs, FAKE, 1 << 30, None) == _lib.E_ARG and "fit" in _lib.last_error()
    band0[0] = 0
    assert call(ctypes.byref(state), *args, ctypes.byref(products(_lib, rendered=FAKE)), outs, FAKE, 1 << 30, None) == _lib.E_ARG
    outs[0].model = FAKE
    assert call(ctypes.byref(state), *args, None, outs, FAKE, 1 << 30, None) == _lib.E_ARG and "state" in _lib.last_error()
    outs[0].model = outs[0].loss = None
    assert call(ctypes.byref(state), *args, None, outs, FAKE, 1 << 30, None) == _lib.E_ARG and "every output" in _lib.last_error()
