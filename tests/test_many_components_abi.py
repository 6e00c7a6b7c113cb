"""CPU: the component limit of the engine is SCARLET_MAX_COMPONENTS = 256 (was 32).  Shape checks come before the null
pointer checks in check_batch, so a batch with null data pointers shows which limit a shape meets without a device."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scarlet_hip.h")


def _batch(S, K, B, H, W):
    from scarlet_amd import _lib
    b = _lib.ScarletBatch()
    b.S, b.K, b.B, b.H, b.W = S, K, B, H, W
    return b


def _fit(b):
    from scarlet_amd import _lib
    return _lib.lib.scarlet_fit(ctypes.byref(b), 1, 0.0, 0, 0, None)


def test_header_constant_matches_binding():
    from scarlet_amd import _lib
    m = re.search(r"#define\s+SCARLET_MAX_COMPONENTS\s+(\d+)", open(HEADER).read())
    assert m and int(m.group(1)) == _lib.MAX_COMPONENTS == 256


def test_many_components_pass_the_shape_check():
    """K = 33, 64 and 256 reach the null-pointer check (E_ARG) instead of E_NOTIMPL"""
    from scarlet_amd import _lib
    for K in (33, 64, 256):
        assert _fit(_batch(1, K, 5, 64, 64)) == _lib.E_ARG, (K, _lib.last_error())
        assert "null pointer" in _lib.last_error()


def test_limits_name_themselves():
    from scarlet_amd import _lib
    assert _fit(_batch(1, 257, 5, 64, 64)) == _lib.E_NOTIMPL
    assert "256" in _lib.last_error() and "B > 8" not in _lib.last_error()
    assert _fit(_batch(1, 64, 9, 64, 64)) == _lib.E_NOTIMPL
    assert "B > 8" in _lib.last_error() and "256" not in _lib.last_error()
    assert _fit(_batch(1, 256, 5, 1025, 64)) == _lib.E_TOO_LARGE


def _old_workspace_bytes(S, K, B, H, W):
    """the workspace formula of the K <= 32 path (partials with the packed Gram, convergence sums, flags, G planes)"""
    a256 = lambda v: (v + 255) & ~255
    T = (H * W + 4095) // 4096
    P = 1 + K * B + K * (K + 1) // 2
    resid = a256(4 * S * B * H * W) if K > 8 else 0
    return a256(8 * (S * T * P + S * K * 4) + 4 * (2 * S * K + 64)) + resid + 256


def test_workspace_unchanged_up_to_32_and_int64_beyond():
    """K <= 32 keeps its layout to the byte; K > 32 drops the Gram from the per-tile partials and adds the float64 Gram
    area of hugek.h, sized in int64 (no overflow at many scenes x 256 components x 1024^2)"""
    from scarlet_amd import _lib
    ws = lambda b: _lib.lib.scarlet_batch_workspace_bytes(ctypes.byref(b))
    for K in (9, 30, 32):
        assert ws(_batch(3, K, 5, 64, 64)) == _old_workspace_bytes(3, K, 5, 64, 64)
    small = ws(_batch(1, 256, 6, 1024, 1024))
    T, P = 256, 1 + 256 * 6
    gram = 8 * (36 * 16 * 1024 + 3 * 256 * 256)        # 36 block pairs x 16 chunks x 32 x 32, three 256 x 256 matrices
    assert small > 8 * T * P + 4 * 6 * 1024 * 1024 + gram
    assert small - ws(_batch(1, 32, 6, 1024, 1024)) < 8 * T * P + gram + 2 * 1024 * 1024 * 1024
    big = ws(_batch(4096, 256, 8, 1024, 1024))
    assert big > 2 ** 40 and big > 4096 * (small - 4096)
