"""CPU: the host set-up of a low-resolution observation at model frames past the LDS limit of the low-resolution kernels
(lowres_large_common.LARGE: 96 x 96, 104 x 104, 256 x 256, 100 x 90) against what the reference computed
(tests/golden/lowres_large.npz, tools/gen_lowres_large_golden.py), the float restatement of the joint fit against the
reference's fit at 96 x 96, and the C ABI of the *_large entry points with its argument checks.  Every library call
below returns before a launch."""
import ctypes

import numpy as np
import pytest

import lowres_common as lc
import lowres_large_common as ll
from conftest import load_golden, rel_err

FAKE = 0x1000          # a non-NULL pointer that is never dereferenced
HOST_TOL = 1.4e-6      # tests/test_lowres_host.py's; measured here: 0.7e-7 .. 1.6e-7 (profiles/lowres_rel_err.txt)


@pytest.fixture(scope="module")
def g():
    return load_golden("lowres_large")


def _channels(g, name):
    return ("r", "i")[:len(g[name + "_lr_psfs"])]


@pytest.mark.parametrize("name", ll.SQUARE)
def test_host_factors_reproduce_the_reference(g, name):
    from scarlet_amd import resampling as rs
    (H, W), (h, w), ratio, origin, psf_px, _ = ll.LARGE[name]
    assert (tuple(g[name + "_model_shape"]), tuple(g[name + "_lr_shape"])) == ((H, W), (h, w))
    assert float(g[name + "_ratio"]) == ratio and tuple(g[name + "_origin"]) == origin
    ch = _channels(g, name)
    obs, _ = lc.geometry(g, name, model_channels=ch, channels=ch)
    assert obs.covers and obs.lr_shape == (h, w)
    assert list(obs._fft_shape) == list(g[name + "_fft_shape"])
    model = g[name + "_models"][0]
    out = rs.apply_factors(obs.factors, model)
    err = rel_err(out, g[name + "_renders"][0])
    print("geometry %s (%d x %d): render rel err %.3e" % (name, H, W, err))
    assert err <= HOST_TOL
    wgt, img = g[name + "_weights_lr"].astype(np.float64), g[name + "_images_lr"].astype(np.float64)
    loss = 0.5 * np.sum((wgt * (out - img)) ** 2)
    assert abs(loss - g[name + "_losses"][0]) <= HOST_TOL * g[name + "_losses"][0]


def test_padded_planes_and_frequencies():
    """what the issue of the streamed form states: 100 x 100 with 25, 49; 108 x 108 with 27, 53; 270 x 270 with 68, 135"""
    want = {"p": ([100, 100], 25, 49), "q": ([108, 108], 27, 53), "r": ([270, 270], 68, 135)}
    for name, (F, nfy, nfx) in want.items():
        obs, _ = ll.geometry(name, B=1)
        assert list(obs._fft_shape) == F and ll.dims(obs)[4:] == (nfy, nfx)


def test_sandwich_is_the_reference_algorithm_at_100_x_90(g):
    """the non-square geometry n, which the reference refuses (its message is in the fixture): the factor sandwich
    against the reference's algorithm stated directly, and <T x, y> = <x, T^T y>, in float64"""
    from scarlet_amd import resampling as rs
    (H, W), (h, w) = ll.LARGE["n"][:2]
    obs, _ = ll.geometry("n", B=2)
    assert obs.covers and obs.small_axis == (w <= h)
    rng = np.random.default_rng(5)
    model = rng.random((2, H, W))
    out = rs.apply_factors(obs.factors, model)
    err = rel_err(out, lc.render_by_planes(obs, model))
    print("geometry n: sandwich vs planes %.3e" % err)
    assert err <= 1e-12
    y = rng.standard_normal(out.shape)
    lhs, rhs = np.sum(out * y), np.sum(model * rs.adjoint_factors(obs.factors, y))
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)
    assert str(g["n_reference_error"]).startswith("ValueError") and "broadcast" in str(g["n_reference_error"])


def test_matrix_products_are_the_three_operand_sums():
    """resampling.lowres_factors / apply_factors / adjoint_factors as matrix products against the einsum statements
    they replace (the factors may move by rounding only)"""
    from scarlet_amd import resampling as rs
    obs, _ = ll.geometry("j", B=3)
    f = obs.factors
    rng = np.random.default_rng(6)
    model, resid = rng.random((3,) + tuple(obs.model_shape)), rng.standard_normal((3,) + tuple(obs.frame.shape[1:]))
    spec = np.einsum("fy,byx,gx->bfg", f["uy"], model, f["ux"]) * f["dhat"]
    assert rel_err(rs.apply_factors(f, model), np.real(np.einsum("if,bfg,jg->bij", f["vy"], spec, f["vx"]))) <= 1e-13
    spec = np.einsum("if,bij,jg->bfg", f["vy"], resid, f["vx"]) * f["dhat"]
    assert rel_err(rs.adjoint_factors(f, resid), np.real(np.einsum("fy,bfg,gx->byx", f["uy"], spec, f["ux"]))) <= 1e-13


def test_float_restatement_of_the_joint_fit_reproduces_the_reference(g):
    obs, start, cw, _ = lc.fit_inputs(g, "p")
    sc = lc.fit(lc.scene_from(start, cw), obs, 5)
    tol = 2e-5                      # the float32 bound of tests/test_lowres_host.py's comparison at a and b
    errs = (rel_err(sc.mse, g["p_fit_mse"]), rel_err(np.array([c.sed for c in sc.sources]), g["p_fit_sed"]),
            rel_err(np.array([c.morph for c in sc.sources]), g["p_fit_morph"]))
    print("fit at 96 x 96 against the reference: mse %.3e sed %.3e morph %.3e" % errs)
    assert max(errs) <= tol
    np.testing.assert_array_equal(np.array([c.center for c in sc.sources]), g["p_fit_centers"])
    np.testing.assert_array_equal(np.array([c.flags for c in sc.sources]), g["p_fit_flags"])


# ---------------------------------------------------------------------------------------------- the C ABI
def _batch(S, K, B, H, W):
    from scarlet_amd import _lib
    b = _lib.ScarletBatch()
    b.S, b.K, b.B, b.H, b.W = S, K, B, H, W
    for f in ("images", "cur", "centers", "shifts", "flags", "lipschitz", "mse", "it", "active", "status", "workspace"):
        setattr(b, f, FAKE)
    b.sed[0] = b.sed[1] = b.morph[0] = b.morph[1] = FAKE
    b.mse_capacity = 1
    return b


def _lowres(h=16, w=16, nfy=9, nfx=17, B=2, **kw):
    from scarlet_amd import _lib
    lr = _lib.ScarletLowres()
    lr.h, lr.w, lr.nfy, lr.nfx, lr.B = h, w, nfy, nfx, B
    for f in ("uy", "ux", "vy", "vx", "dhat", "workspace"):
        setattr(lr, f, FAKE)
    for k, v in kw.items():
        setattr(lr, k, v)
    return lr


def _fit(fn, state, obs, lows, band0, with_list=True):
    from scarlet_amd import _lib
    n = len(obs)
    arr = (ctypes.POINTER(_lib.ScarletBatch) * n)(*[ctypes.pointer(o) for o in obs])
    low = (ctypes.POINTER(_lib.ScarletLowres) * n)(*[ctypes.pointer(x) if x is not None else
                                                     ctypes.POINTER(_lib.ScarletLowres)() for x in lows])
    b0 = np.asarray(band0, dtype=np.int32)
    cons = _lib.ScarletConstraints()
    return fn(ctypes.byref(state), ctypes.byref(cons), arr, low if with_list else None, b0.ctypes.data_as(ctypes.c_void_p),
              n, 1, 0.0, 0, 0, None)


def _big():
    """256 x 256 model planes with a 64 x 64 observation, as tests/test_lowres_host.py refuses them"""
    return _batch(3, 2, 5, 256, 256), _batch(3, 2, 3, 256, 256), _batch(3, 2, 2, 64, 64), dict(h=64, w=64, nfy=66, nfx=131)


def test_argument_errors_come_back_before_any_launch():
    from scarlet_amd import _lib
    fit = _lib.lib.scarlet_fit_observations_lowres_large
    st, hi, lo = _batch(3, 2, 5, 32, 32), _batch(3, 2, 3, 32, 32), _batch(3, 2, 2, 16, 16)
    assert _fit(fit, st, [hi, lo], [None, _lowres()], [0, 3], with_list=False) == _lib.E_ARG
    assert "low-resolution list" in _lib.last_error()
    for bad_lo, lr, b0 in ((_batch(3, 2, 2, 16, 12), _lowres(), 3), (_batch(3, 2, 2, 16, 16), _lowres(h=12), 3),
                           (_batch(2, 2, 2, 16, 16), _lowres(), 3), (_batch(3, 2, 2, 16, 16), _lowres(), 4)):
        assert _fit(fit, st, [hi, bad_lo], [None, lr], [0, b0]) == _lib.E_ARG
        assert "low-resolution observation does not fit" in _lib.last_error()
    assert _fit(fit, st, [hi, lo], [None, _lowres(B=3)], [0, 3]) == _lib.E_ARG and "bad shape" in _lib.last_error()
    assert _fit(fit, st, [hi, lo], [None, _lowres(nfx=0)], [0, 3]) == _lib.E_ARG and "bad shape" in _lib.last_error()
    for name in ("uy", "ux", "vy", "vx", "dhat"):
        assert _fit(fit, st, [hi, lo], [None, _lowres(**{name: None})], [0, 3]) == _lib.E_ARG
        assert "null factor" in _lib.last_error()
    assert _fit(fit, st, [hi, lo], [None, _lowres(workspace=None)], [0, 3]) == _lib.E_ARG and "workspace" in _lib.last_error()
    # past LDS the argument checks are the same ones
    big, big_hi, big_lo, shape = _big()
    assert _fit(fit, big, [big_hi, big_lo], [None, _lowres(workspace=None, **shape)], [0, 3]) == _lib.E_ARG
    assert "workspace" in _lib.last_error()
    assert _fit(fit, big, [big_hi, big_lo], [None, _lowres(dhat=None, **shape)], [0, 3]) == _lib.E_ARG
    # B <= 8 and sides <= SCARLET_MAX_SIDE
    assert _lib.lib.scarlet_lowres_op_scratch_bytes(1, 32, 32, ctypes.byref(_lowres(B=9))) == _lib.E_NOTIMPL
    assert "8 bands" in _lib.last_error()
    wide = _lowres(h=64, w=64, nfy=66, nfx=2049)
    assert _lib.lib.scarlet_lowres_op_scratch_bytes(1, 1024, 1024, ctypes.byref(wide)) == _lib.E_NOTIMPL
    assert "SCARLET_MAX_SIDE" in _lib.last_error()
    assert _lib.lib.scarlet_lowres_op_scratch_bytes(1, 1025, 1024, ctypes.byref(_lowres())) == _lib.E_NOTIMPL
    assert _lib.lib.scarlet_lowres_op_scratch_bytes(-1, 32, 32, ctypes.byref(_lowres())) == _lib.E_ARG
    assert _lib.lib.scarlet_lowres_op_scratch_bytes(1, 32, 32, None) == _lib.E_ARG
    # the plane operators
    lr = _lowres()
    for fn in (_lib.lib.scarlet_lowres_render_large, _lib.lib.scarlet_lowres_adjoint_large):
        assert fn(None, 1, 32, 32, ctypes.byref(lr), None, None, FAKE, None, 0, None) == _lib.E_ARG and "null plane" in _lib.last_error()
        assert fn(FAKE, -1, 32, 32, ctypes.byref(lr), None, None, FAKE, None, 0, None) == _lib.E_ARG
        assert fn(FAKE, 1, 32, 32, None, None, None, FAKE, None, 0, None) == _lib.E_ARG
        assert fn(FAKE, 1, 32, 32, ctypes.byref(_lowres(ux=None)), None, None, FAKE, None, 0, None) == _lib.E_ARG
        assert fn(FAKE, 0, 32, 32, ctypes.byref(lr), None, None, FAKE, None, 0, None) == 0
        assert fn(FAKE, 0, 256, 256, ctypes.byref(_lowres(**shape)), None, None, FAKE, None, 0, None) == 0


def test_old_entry_points_keep_their_limit_and_the_new_ones_size_past_it():
    from scarlet_amd import _lib
    big, big_hi, big_lo, shape = _big()
    lr = _lowres(**shape)
    assert _fit(_lib.lib.scarlet_fit_observations_lowres, big, [big_hi, big_lo], [None, lr], [0, 3]) == _lib.E_NOTIMPL
    assert "LDS" in _lib.last_error()
    args = (ctypes.byref(big), ctypes.byref(big_lo), ctypes.byref(lr))
    assert _lib.lib.scarlet_lowres_workspace_bytes(*args) == _lib.E_NOTIMPL
    for fn in (_lib.lib.scarlet_lowres_render, _lib.lib.scarlet_lowres_adjoint):
        assert fn(FAKE, 1, 256, 256, ctypes.byref(lr), None, None, FAKE, None) == _lib.E_NOTIMPL
    planes_and_losses = 3 * 2 * 256 * 256 * 4 + 3 * 2 * 8
    sizes = []
    for streamed in (0, 1):
        with ll.options(LOWRES_STREAMED=streamed):
            sizes.append(_lib.lib.scarlet_lowres_large_workspace_bytes(*args))
    assert sizes[0] == sizes[1] and sizes[0] > planes_and_losses
    # where LDS holds (geometry d) the scratch is part of the workspace all the same, whatever the switch says
    st8, lo8, lr8 = _batch(3, 2, 8, 64, 64), _batch(3, 2, 8, 32, 32), _lowres(h=32, w=32, nfy=19, nfx=37, B=8)
    sizes = []
    for streamed in (0, 1):
        with ll.options(LOWRES_STREAMED=streamed):
            sizes.append(_lib.lib.scarlet_lowres_large_workspace_bytes(ctypes.byref(st8), ctypes.byref(lo8), ctypes.byref(lr8)))
    assert sizes[0] == sizes[1] and sizes[0] > 3 * 8 * 64 * 64 * 4 + 3 * 8 * 8
    assert sizes[0] > _lib.lib.scarlet_lowres_workspace_bytes(ctypes.byref(st8), ctypes.byref(lo8), ctypes.byref(lr8))


def test_operator_scratch_and_its_check():
    from scarlet_amd import _lib
    lr8 = _lowres(h=32, w=32, nfy=19, nfx=37, B=8)
    with ll.options(LOWRES_STREAMED=0):
        assert _lib.lib.scarlet_lowres_op_scratch_bytes(24, 64, 64, ctypes.byref(lr8)) == 0
    _, _, _, shape = _big()
    lr = _lowres(**shape)
    need = _lib.lib.scarlet_lowres_op_scratch_bytes(4, 256, 256, ctypes.byref(lr))
    # per plane: A = max(H 2 nfx, 2 nfy W, 2 nfy w) floats, twice the 2 nfy x 2 nfx projection
    assert need >= 4 * 4 * (256 * 262 + 2 * 132 * 262)
    assert _lib.lib.scarlet_lowres_op_scratch_bytes(0, 256, 256, ctypes.byref(lr)) == 0
    for fn in (_lib.lib.scarlet_lowres_render_large, _lib.lib.scarlet_lowres_adjoint_large):
        assert fn(FAKE, 4, 256, 256, ctypes.byref(lr), None, None, FAKE, FAKE, need - 1, None) == _lib.E_ARG
        assert "scratch" in _lib.last_error()
        assert fn(FAKE, 4, 256, 256, ctypes.byref(lr), None, None, FAKE, None, need, None) == _lib.E_ARG
        assert fn(None, 4, 256, 256, ctypes.byref(lr), None, None, FAKE, FAKE, need, None) == _lib.E_ARG
    # LOWRES_CHUNK is a count (0 = automatic), refused when negative, and does not change what is sized
    old = _lib.set_option("LOWRES_CHUNK", 5)
    try:
        assert _lib.set_option("LOWRES_CHUNK", 3) == 5
        assert _lib.lib.scarlet_lowres_op_scratch_bytes(4, 256, 256, ctypes.byref(lr)) == need
        assert _lib.lib.scarlet_set_option(b"LOWRES_CHUNK", -1) == _lib.E_ARG
    finally:
        _lib.set_option("LOWRES_CHUNK", old)
