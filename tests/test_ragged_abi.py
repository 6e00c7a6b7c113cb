"""CPU: ragged batches (scenes with different numbers of components) at the C ABI and in the host layer.

scarlet_batch gains one field at its end, n_components; every earlier field keeps its offset.  The workspace does not
depend on the counts, scarlet_fit_multi refuses them before it looks at pointers, and the padding helper of
BlendBatch works without a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scarlet_hip.h")

# offsetof(scarlet_batch, field) on x86-64 / gfx950 hosts before n_components existed (sizeof was 248)
OLD_OFFSETS = [
    ("S", 0), ("K", 4), ("B", 8), ("H", 12), ("W", 16), ("images", 24), ("weights", 32), ("weight_scalar", 40),
    ("sed", 48), ("morph", 64), ("cur", 80), ("centers", 88), ("shifts", 96), ("flags", 104), ("fix_sed", 112),
    ("fix_morph", 120), ("lipschitz", 128), ("mse", 136), ("mse_capacity", 144), ("it", 152), ("active", 160),
    ("status", 168), ("symmetric", 176), ("monotonic", 180), ("l0_thresh", 184), ("l1_thresh", 188),
    ("centroid_psf", 192), ("centroid_P", 200), ("diff_kernel", 208), ("psf_h", 216), ("psf_w", 220),
    ("diff_kernel_per_scene", 224), ("workspace", 232), ("group", 240),
]
FAKE = 0x1000          # a non-NULL pointer that is never dereferenced (every call below returns before a launch)


def _header_struct_body():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"typedef struct scarlet_batch \{(.*?)\} scarlet_batch;", text, flags=re.S)
    assert m
    return m.group(1)


def test_header_appends_n_components_and_status_bit():
    body = [ln.strip() for ln in _header_struct_body().splitlines() if ln.strip()]
    assert body[-1] == "const int32_t *n_components;"
    assert body[-2] == "const int32_t *group;"
    assert re.search(r"#define\s+SCARLET_STATUS_BAD_COUNT\s+4\b", open(HEADER).read())
    from scarlet_amd import _lib
    assert _lib.STATUS_BAD_COUNT == 4
    assert _lib.ScarletBatch._fields_[-1][0] == "n_components"


def test_earlier_offsets_unchanged(tmp_path):
    """the change is append-only: the C compiler places every earlier field where it was"""
    from scarlet_amd import _lib
    src = tmp_path / "probe.c"
    names = [f for f, _ in OLD_OFFSETS] + ["n_components"]
    body = "\n".join('printf("%s %%zu\\n", offsetof(scarlet_batch, %s));' % (f, f) for f in names)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scarlet_hip.h"\n'
                   'int main(void){ printf("sizeof %zu\\n", sizeof(scarlet_batch));\n' + body + '\nreturn 0;}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = {k: int(v) for k, v in (ln.split() for ln in subprocess.check_output([str(exe)]).decode().splitlines())}
    for f, off in OLD_OFFSETS:
        assert out[f] == off == getattr(_lib.ScarletBatch, f).offset, f
    assert out["n_components"] == 248 == _lib.ScarletBatch.n_components.offset
    assert out["sizeof"] == 256 == ctypes.sizeof(_lib.ScarletBatch)


def _batch(S, K, B, H, W):
    from scarlet_amd import _lib
    b = _lib.ScarletBatch()
    b.S, b.K, b.B, b.H, b.W = S, K, B, H, W
    return b


def _pointers(b):
    for f in ("images", "cur", "centers", "shifts", "flags", "lipschitz", "mse", "it", "active", "status", "workspace"):
        setattr(b, f, FAKE)
    for i in range(2):
        b.sed[i] = FAKE
        b.morph[i] = FAKE
    b.mse_capacity = 8
    return b


@pytest.mark.parametrize("psf", [None, (11, 11), (41, 41)])
def test_workspace_does_not_depend_on_counts(psf):
    from scarlet_amd import _lib
    assert "n_components" in [f for f, _ in _lib.ScarletBatch._fields_]     # (else the library never sees the field)
    ws = lambda b: _lib.lib.scarlet_batch_workspace_bytes(ctypes.byref(b))
    for S in (1, 7, 1024, 1600):
        for K in (1, 4, 8, 12, 30, 40, 64):
            for B in (1, 5, 6):
                for H, W in ((32, 32), (64, 64), (128, 96), (256, 256)):
                    b = _batch(S, K, B, H, W)
                    if psf:
                        b.diff_kernel, (b.psf_h, b.psf_w) = FAKE, psf
                    plain = ws(b)
                    b.n_components = FAKE
                    assert ws(b) == plain > 0, (S, K, B, H, W, psf)


def test_fit_multi_refuses_counts():
    """E_NOTIMPL naming the field, after the shape checks and before the null-pointer checks"""
    from scarlet_amd import _lib
    assert "n_components" in [f for f, _ in _lib.ScarletBatch._fields_]
    state = _batch(4, 3, 5, 32, 32)
    state.n_components = FAKE
    band0 = (ctypes.c_int32 * 1)(0)
    obs = (ctypes.POINTER(_lib.ScarletBatch) * 1)(ctypes.pointer(_batch(4, 3, 5, 32, 32)))
    rc = _lib.lib.scarlet_fit_multi(ctypes.byref(state), obs, band0, 1, 1, 0.0, 0, 0, None)
    assert rc == _lib.E_NOTIMPL and "n_components" in _lib.last_error()
    # shape errors still come first
    big = _batch(4, 257, 5, 32, 32)
    big.n_components = FAKE
    assert _lib.lib.scarlet_fit_multi(ctypes.byref(big), obs, band0, 1, 1, 0.0, 0, 0, None) == _lib.E_NOTIMPL
    assert "256" in _lib.last_error()
    # an observation batch with counts (the state is complete)
    state = _pointers(_batch(4, 3, 5, 32, 32))
    ob = _batch(4, 3, 5, 32, 32)
    ob.n_components = FAKE
    obs = (ctypes.POINTER(_lib.ScarletBatch) * 1)(ctypes.pointer(ob))
    rc = _lib.lib.scarlet_fit_multi(ctypes.byref(state), obs, band0, 1, 1, 0.0, 0, 0, None)
    assert rc == _lib.E_NOTIMPL and "n_components" in _lib.last_error()


def test_pad_centers():
    from scarlet_amd.batch import pad_centers
    cen, n = pad_centers([[(3, 4)], np.array([[1, 2], [5, 6], [7, 8]]), [(9, 9), (10, 11)]])
    assert cen.dtype == np.int32 and n.dtype == np.int32
    assert cen.shape == (3, 3, 2) and n.tolist() == [1, 3, 2]
    assert cen[0].tolist() == [[3, 4], [0, 0], [0, 0]]
    assert cen[1].tolist() == [[1, 2], [5, 6], [7, 8]]
    assert cen[2].tolist() == [[9, 9], [10, 11], [0, 0]]
    cen, n = pad_centers([[(3, 4)], [(1, 1), (2, 2)]], K=4)
    assert cen.shape == (2, 4, 2) and n.tolist() == [1, 2]


def test_pad_centers_rejects_empty_and_overlong():
    from scarlet_amd import _lib
    from scarlet_amd.batch import pad_centers
    with pytest.raises(ValueError):
        pad_centers([])
    with pytest.raises(ValueError):
        pad_centers([[(1, 1)], np.zeros((0, 2))])
    with pytest.raises(ValueError):
        pad_centers([[(1, 1), (2, 2), (3, 3)]], K=2)
    with pytest.raises(ValueError):
        pad_centers([np.ones((_lib.MAX_COMPONENTS + 1, 2))])
