"""CPU: the entry points of include/scarlet_hip.h for the products of a low-resolution observation
(scarlet_observations_products_lowres, scarlet_lowres_products_scratch_bytes): declared, exported and mirrored by ctypes;
every argument error answered with SCARLET_E_ARG and a message on the host (there is no device here: a call that went
past its checks would come back with SCARLET_E_HIP instead); and the form and scratch size that launch_plan.h's
lowres_products_plan chooses for the LIMITS and LARGE shapes, read through the scratch query."""
import ctypes
import os
import re

import numpy as np
import pytest

import lowres_common as lc
import lowres_large_common as ll

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000          # a non-NULL "device pointer": the checks compare against NULL and never dereference
LDS_LIMIT = 160 * 1024 - 1024
SCRATCH_CAP = 256 << 20
LOSS_BLOCKS = 64


@pytest.fixture(scope="module")
def _lib():
    from scarlet_amd import _lib
    return _lib


def batch(_lib, S, K, B, H, W):
    b = _lib.ScarletBatch()
    b.S, b.K, b.B, b.H, b.W = S, K, B, H, W
    b.images = b.cur = b.workspace = FAKE
    b.sed[0] = b.sed[1] = b.morph[0] = b.morph[1] = FAKE
    b.weight_scalar = 1.0
    return b


def lowres(_lib, h=16, w=16, nfy=9, nfx=17, B=2, **kw):
    lr = _lib.ScarletLowres()
    lr.h, lr.w, lr.nfy, lr.nfx, lr.B = h, w, nfy, nfx, B
    for f in ("uy", "ux", "vy", "vx", "dhat"):
        setattr(lr, f, FAKE)                     # (no workspace: the products do not use it)
    for k, v in kw.items():
        setattr(lr, k, v)
    return lr


def products(_lib, **fields):
    p = _lib.ScarletProducts()
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def call(_lib, state, obs, lows, band0, outs, state_out=None, scratch=FAKE, scratch_bytes=1 << 40, with_list=True):
    n = len(obs)
    arr = (ctypes.POINTER(_lib.ScarletBatch) * n)(*[ctypes.pointer(o) for o in obs])
    low = (ctypes.POINTER(_lib.ScarletLowres) * n)(*[ctypes.pointer(x) if x is not None else
                                                     ctypes.POINTER(_lib.ScarletLowres)() for x in lows])
    b0 = np.asarray(band0, dtype=np.int32)
    out = (_lib.ScarletProducts * n)(*outs)
    return _lib.lib.scarlet_observations_products_lowres(
        None if state is None else ctypes.byref(state), arr, low if with_list else None, b0.ctypes.data_as(ctypes.c_void_p), n,
        None if state_out is None else ctypes.byref(state_out), out, scratch, scratch_bytes, None)


def test_symbols_are_declared_exported_and_mirrored(_lib):
    header = open(os.path.join(ROOT, "include", "scarlet_hip.h")).read()
    flat = re.sub(r"\s+", " ", header)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for fn in ("scarlet_observations_products_lowres", "scarlet_lowres_products_scratch_bytes"):
        assert hasattr(lib, fn) and fn in _lib.EXPORTS
    assert ("int64_t scarlet_lowres_products_scratch_bytes(const scarlet_batch *state, const scarlet_batch *obs, "
            "const scarlet_lowres *lr, const scarlet_products *out);") in flat
    assert ("int scarlet_observations_products_lowres(const scarlet_batch *state, scarlet_batch *const *obs, "
            "const scarlet_lowres *const *lowres, const int32_t *band0, int n_obs, const scarlet_products *state_out, "
            "const scarlet_products *out, void *scratch, int64_t scratch_bytes, void *stream);") in flat
    P, B, L, R = ctypes.c_void_p, ctypes.POINTER(_lib.ScarletBatch), ctypes.POINTER(_lib.ScarletLowres), ctypes.POINTER(_lib.ScarletProducts)
    f = _lib.lib.scarlet_observations_products_lowres
    assert f.restype is ctypes.c_int
    assert list(f.argtypes) == [B, ctypes.POINTER(B), ctypes.POINTER(L), P, ctypes.c_int, R, R, P, ctypes.c_int64, P]
    q = _lib.lib.scarlet_lowres_products_scratch_bytes
    assert q.restype is ctypes.c_int64 and list(q.argtypes) == [B, B, L, R]


def test_argument_errors_come_back_before_any_launch(_lib):
    st, hi, lo = batch(_lib, 3, 2, 5, 32, 32), batch(_lib, 3, 2, 3, 32, 32), batch(_lib, 3, 2, 2, 16, 16)
    want = products(_lib, rendered=FAKE, residual=FAKE, loss=FAKE)
    none = products(_lib)

    def refused(*args, **kw):
        rc = call(_lib, *args, **kw)
        assert rc == _lib.E_ARG, (rc, _lib.last_error())
        assert _lib.last_error()
        with pytest.raises(ValueError):
            _lib.check(rc)
        return _lib.last_error()

    assert "low-resolution list" in refused(st, [hi, lo], [None, lowres(_lib)], [0, 3], [none, want], with_list=False)
    refused(None, [hi, lo], [None, lowres(_lib)], [0, 3], [none, want])
    assert "every output" in refused(st, [hi, lo], [None, lowres(_lib)], [0, 3], [none, none])
    # shapes
    for bad_lo, lr, b0 in ((batch(_lib, 3, 2, 2, 16, 12), lowres(_lib), 3), (batch(_lib, 3, 2, 2, 16, 16), lowres(_lib, h=12), 3),
                           (batch(_lib, 2, 2, 2, 16, 16), lowres(_lib), 3), (batch(_lib, 3, 3, 2, 16, 16), lowres(_lib), 3),
                           (batch(_lib, 3, 2, 2, 16, 16), lowres(_lib), 4), (batch(_lib, 3, 2, 2, 16, 16), lowres(_lib), -1)):
        assert "does not fit" in refused(st, [hi, bad_lo], [None, lr], [0, b0], [none, want])
    assert "bad shape" in refused(st, [hi, lo], [None, lowres(_lib, B=3)], [0, 3], [none, want])
    assert "bad shape" in refused(st, [hi, lo], [None, lowres(_lib, nfx=0)], [0, 3], [none, want])
    # null factor pointers, of the observation and of the state
    for name in ("uy", "ux", "vy", "vx", "dhat"):
        assert "null factor" in refused(st, [hi, lo], [None, lowres(_lib, **{name: None})], [0, 3], [none, want])
    nomorph = batch(_lib, 3, 2, 5, 32, 32)
    nomorph.morph[1] = None
    assert "null factor pointer" in refused(nomorph, [hi, lo], [None, lowres(_lib)], [0, 3], [none, want])
    # B <= 8
    st9, lo9 = batch(_lib, 3, 2, 8, 32, 32), batch(_lib, 3, 2, 9, 16, 16)
    assert "8 bands" in refused(st9, [lo9], [lowres(_lib, B=9)], [0], [want])
    # sides <= SCARLET_MAX_SIDE: the model frame, the observation, the retained frequencies
    assert "SCARLET_MAX_SIDE" in refused(batch(_lib, 3, 2, 5, 1025, 32), [lo], [lowres(_lib)], [3], [want])
    assert "SCARLET_MAX_SIDE" in refused(st, [batch(_lib, 3, 2, 2, 1025, 16)], [lowres(_lib, h=1025)], [3], [want])
    assert "SCARLET_MAX_SIDE" in refused(st, [lo], [lowres(_lib, nfy=1025)], [3], [want])
    assert "SCARLET_MAX_SIDE" in refused(st, [lo], [lowres(_lib, nfx=2049)], [3], [want])
    # a diff_kernel
    psf = batch(_lib, 3, 2, 2, 16, 16)
    psf.diff_kernel, psf.psf_h, psf.psf_w = FAKE, 5, 5
    assert "diff_kernel" in refused(st, [hi, psf], [None, lowres(_lib)], [0, 3], [none, want])
    # images NULL with residual or loss wanted (rendered alone needs none: see the scratch test below)
    noimg = batch(_lib, 3, 2, 2, 16, 16)
    noimg.images = None
    assert "images" in refused(st, [hi, noimg], [None, lowres(_lib)], [0, 3], [none, products(_lib, residual=FAKE)])
    assert "images" in refused(st, [hi, noimg], [None, lowres(_lib)], [0, 3], [none, products(_lib, loss=FAKE)])
    # what belongs to the state
    assert "state" in refused(st, [hi, lo], [None, lowres(_lib)], [0, 3], [none, products(_lib, rendered=FAKE, model=FAKE)])
    assert "observation" in refused(st, [hi, lo], [None, lowres(_lib)], [0, 3], [none, want], state_out=products(_lib, loss=FAKE))
    # the same-grid observation beside it keeps its own checks
    assert "fit the state" in refused(st, [batch(_lib, 3, 2, 3, 32, 30), lo], [None, lowres(_lib)], [0, 3], [want, want])


def test_scratch_that_is_too_small(_lib):
    big, big_lo = batch(_lib, 3, 2, 5, 256, 256), batch(_lib, 3, 2, 2, 64, 64)
    lr = lowres(_lib, h=64, w=64, nfy=66, nfx=131)
    want = products(_lib, loss=FAKE)
    need = _lib.lib.scarlet_lowres_products_scratch_bytes(ctypes.byref(big), ctypes.byref(big_lo), ctypes.byref(lr), ctypes.byref(want))
    assert need > 0
    for kw in (dict(scratch=FAKE, scratch_bytes=need - 1), dict(scratch=None, scratch_bytes=need)):
        assert call(_lib, big, [big_lo], [lr], [3], [want], **kw) == _lib.E_ARG
        assert "scratch" in _lib.last_error()
    # with the state's `model` wanted the need is the same: one layout whatever the call wants
    assert call(_lib, big, [big_lo], [lr], [3], [want], state_out=products(_lib, model=FAKE), scratch=FAKE,
                scratch_bytes=need - 1) == _lib.E_ARG
    # the LDS form needs none
    st, lo = batch(_lib, 3, 2, 5, 32, 32), batch(_lib, 3, 2, 2, 16, 16)
    with ll.options(LOWRES_STREAMED=0):
        assert _lib.lib.scarlet_lowres_products_scratch_bytes(ctypes.byref(st), ctypes.byref(lo), ctypes.byref(lowres(_lib)),
                                                              ctypes.byref(want)) == 0


def expected_scratch(S, B, H, W, h, w, nfy, nfx, streamed):
    """launch_plan.h lowres_products_plan restated: 0 where the factor matrices, the B spectra and one plane fit LDS;
    otherwise the chunk's planes times lowres_stream.h's per-plane bytes of a fit (M, A, B, Z, D, the loss partials)"""
    _, fixed = lc.scratch_terms(H, W, h, w, nfy, nfx)
    lds = fixed + 8 * B * nfy * nfx
    if not streamed and lds <= LDS_LIMIT:
        return 0
    ny2, nx2 = 2 * nfy, 2 * nfx
    a = max(H * nx2, ny2 * W, ny2 * w)
    per_plane = (H * W + a + 2 * ny2 * nx2 + h * w) * 4 + LOSS_BLOCKS * 8
    per_plane = (per_plane + 15) & ~15
    chunk = min(S * B, max(1, SCRATCH_CAP // per_plane), 65535)
    return chunk * per_plane


@pytest.mark.parametrize("name", ["j", "d", "g", "e", "p", "r"])
def test_form_and_scratch_of_the_limit_shapes(_lib, name):
    """LIMITS j, d, g, e fit LDS at their bands (no scratch) and one more band at e does not; LARGE p and r never do"""
    S, B = 3, ll.spec(name)[5]
    H, W, h, w, nfy, nfx = ll.dims(ll.geometry(name, B=1)[0])
    want = products(_lib, rendered=FAKE)

    def query(bands, s=S):
        st, lo = batch(_lib, s, 2, 8, H, W), batch(_lib, s, 2, bands, h, w)
        lo.images = None                                     # (rendered alone needs no images)
        lr = lowres(_lib, h=h, w=w, nfy=nfy, nfx=nfx, B=bands)
        return _lib.lib.scarlet_lowres_products_scratch_bytes(ctypes.byref(st), ctypes.byref(lo), ctypes.byref(lr), ctypes.byref(want))

    sizes = {}
    for streamed in (0, 1):
        with ll.options(LOWRES_STREAMED=streamed):
            sizes[streamed] = query(B)
            assert sizes[streamed] == expected_scratch(S, B, H, W, h, w, nfy, nfx, streamed)
            with ll.options(LOWRES_CHUNK=5):                 # lowers the chunk of the launches, never what is sized
                assert query(B) == sizes[streamed]
            assert _lib.lib.scarlet_lowres_products_scratch_bytes(None, None, None, ctypes.byref(products(_lib))) == 0
    print("%s: %d x %d / %d x %d, nfy, nfx = %d, %d, B = %d: scratch %d bytes, %d streamed" % (name, H, W, h, w, nfy, nfx, B,
                                                                                        sizes[0], sizes[1]))
    assert (sizes[0] == 0) == (name in "jdge") and sizes[1] > 0
    with ll.options(LOWRES_STREAMED=0):
        if name == "e":
            assert query(B + 1) == expected_scratch(S, B + 1, H, W, h, w, nfy, nfx, 0) > 0
        if name == "r":                                      # 4096 scenes: the chunk keeps the scratch within the cap
            many = query(B, 4096)
            assert many == expected_scratch(4096, B, H, W, h, w, nfy, nfx, 0) and SCRATCH_CAP // 2 < many <= SCRATCH_CAP
