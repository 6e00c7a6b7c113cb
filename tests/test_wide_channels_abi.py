"""CPU: the C ABI and host checks of joint fits over more than 8 model channels (scarlet_fit_observations_wide and its
siblings, BlendBatch.from_observations(..., wide=True), launch_plan.h contract_plan).  Every call returns before a launch."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scarlet_hip.h")
FAKE = 0x1000          # a non-NULL pointer that is never dereferenced


def _batch(S, K, B, H, W, pointers=True):
    from scarlet_amd import _lib
    b = _lib.ScarletBatch()
    b.S, b.K, b.B, b.H, b.W = S, K, B, H, W
    if pointers:
        for f in ("images", "cur", "centers", "shifts", "flags", "lipschitz", "mse", "it", "active", "status",
                  "workspace"):
            setattr(b, f, FAKE)
        b.sed[0] = b.sed[1] = b.morph[0] = b.morph[1] = FAKE
        b.mse_capacity = 1
    return b


def _wide(state, obs, band0):
    from scarlet_amd import _lib
    arr = (ctypes.POINTER(_lib.ScarletBatch) * len(obs))(*[ctypes.pointer(o) for o in obs])
    b0 = np.asarray(band0, dtype=np.int32)
    return _lib.lib.scarlet_fit_observations_wide(ctypes.byref(state), None, None, arr, None,
                                                  b0.ctypes.data_as(ctypes.c_void_p), len(obs), 1, 0.0, 0, 0, None)


def _old(fn, state, obs, band0):
    from scarlet_amd import _lib
    arr = (ctypes.POINTER(_lib.ScarletBatch) * len(obs))(*[ctypes.pointer(o) for o in obs])
    b0 = np.asarray(band0, dtype=np.int32)
    return getattr(_lib.lib, fn)(ctypes.byref(state), arr, b0.ctypes.data_as(ctypes.c_void_p), len(obs), 1, 0.0, 0, 0, None)


def test_header_declares_the_wide_entry_points():
    text = open(HEADER).read()
    assert re.search(r"#define\s+SCARLET_MAX_CHANNELS\s+32\b", text)
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
    assert ("int scarlet_fit_observations_wide(scarlet_batch *state, const scarlet_constraints *c , const scarlet_prior *p , "
            "scarlet_batch *const *obs, const scarlet_lowres *const *lowres , const int32_t *band0, int n_obs, "
            "int max_iter, double e_rel, int approximate_L, int check_every, void *stream);") in flat
    assert ("int scarlet_observations_products_wide(const scarlet_batch *state, scarlet_batch *const *obs, "
            "const scarlet_lowres *const *lowres , const int32_t *band0, int n_obs, const scarlet_products *state_out, "
            "const scarlet_products *out, void *scratch, int64_t scratch_bytes, void *stream);") in flat
    for name in ("scarlet_init_combined_sed_wide", "scarlet_lowres_large_workspace_bytes_wide",
                 "scarlet_products_scratch_bytes_wide", "scarlet_lowres_products_scratch_bytes_wide",
                 "scarlet_debug_contract_plan"):
        assert re.search(r"\b%s\(" % name, flat), name
    from scarlet_amd import _lib
    assert _lib.MAX_CHANNELS == 32
    assert _lib.lib.scarlet_fit_observations_wide.argtypes == _lib.lib.scarlet_fit_observations_prior.argtypes
    assert _lib.lib.scarlet_observations_products_wide.argtypes == _lib.lib.scarlet_observations_products_lowres.argtypes
    for name in ("scarlet_fit_observations_wide", "scarlet_observations_products_wide", "scarlet_init_combined_sed_wide",
                 "scarlet_lowres_large_workspace_bytes_wide", "scarlet_products_scratch_bytes_wide",
                 "scarlet_lowres_products_scratch_bytes_wide", "scarlet_debug_contract_plan"):
        assert name in _lib.EXPORTS


@pytest.mark.parametrize("C", [9, 17, 32])
def test_wide_states_reach_the_pointer_check(C):
    """a state of up to 32 channels passes the shape checks: without its pointers it is E_ARG, not E_NOTIMPL"""
    from scarlet_amd import _lib
    ob = _batch(4, 3, 5, 32, 32)
    assert _wide(_batch(4, 3, C, 32, 32, pointers=False), [ob], [C - 5]) == _lib.E_ARG
    assert "null pointer" in _lib.last_error()
    # ... and with them, up to the observations' checks
    assert _wide(_batch(4, 3, C, 32, 32), [ob], [C - 4]) == _lib.E_ARG
    assert "does not fit" in _lib.last_error()


def test_wide_limits():
    from scarlet_amd import _lib
    ob = _batch(4, 3, 5, 32, 32)
    assert _wide(_batch(4, 3, 33, 32, 32), [ob], [0]) == _lib.E_NOTIMPL
    assert "32" in _lib.last_error() and "SCARLET_MAX_CHANNELS" in _lib.last_error()
    # an observation keeps at most 8 bands of its own
    assert _wide(_batch(4, 3, 17, 32, 32), [_batch(4, 3, 9, 32, 32)], [0]) == _lib.E_NOTIMPL
    assert "8 bands" in _lib.last_error()
    # band0 + B > C
    assert _wide(_batch(4, 3, 17, 32, 32), [ob, _batch(4, 3, 8, 32, 32)], [0, 10]) == _lib.E_ARG
    assert "does not fit" in _lib.last_error()
    assert _wide(_batch(4, 3, 17, 32, 32), [ob], [-1]) == _lib.E_ARG
    # a state of at most 8 channels goes through the same checks as before
    assert _wide(_batch(4, 3, 5, 32, 32, pointers=False), [ob], [0]) == _lib.E_ARG
    assert "null pointer" in _lib.last_error()


def test_old_entry_points_still_refuse_nine_bands():
    from scarlet_amd import _lib
    ob = _batch(4, 3, 5, 32, 32)
    st = _batch(4, 3, 9, 32, 32)
    for fn in ("scarlet_fit_observations", "scarlet_fit_multi"):
        assert _old(fn, st, [ob], [0]) == _lib.E_NOTIMPL
        assert "B > 8 bands" in _lib.last_error()
    assert _lib.lib.scarlet_fit(ctypes.byref(st), 1, 0.0, 0, 0, None) == _lib.E_NOTIMPL
    assert "B > 8 bands" in _lib.last_error()
    assert _lib.lib.scarlet_init_combined_sed(ctypes.byref(st), FAKE, 5, 0, None, 0, None, None) == _lib.E_NOTIMPL
    ps = _lib.ScarletProducts()
    ps.model = FAKE
    assert _lib.lib.scarlet_products_scratch_bytes(ctypes.byref(st), ctypes.byref(ps)) == 0
    assert _lib.lib.scarlet_batch_products(ctypes.byref(st), ctypes.byref(ps), None, 0, None) == _lib.E_NOTIMPL
    arr = (ctypes.POINTER(_lib.ScarletBatch) * 1)(ctypes.pointer(ob))
    b0 = np.zeros(1, np.int32)
    outs = (_lib.ScarletProducts * 1)()
    assert _lib.lib.scarlet_observations_products(ctypes.byref(st), arr, b0.ctypes.data_as(ctypes.c_void_p), 1, ctypes.byref(ps),
                                                  outs, None, 0, None) == _lib.E_NOTIMPL


def test_wide_products_checks():
    from scarlet_amd import _lib
    ob = _batch(4, 3, 5, 32, 32)
    arr = (ctypes.POINTER(_lib.ScarletBatch) * 1)(ctypes.pointer(ob))
    b0 = np.zeros(1, np.int32)
    outs = (_lib.ScarletProducts * 1)()
    ps = _lib.ScarletProducts()
    ps.flux = FAKE

    def call(st, scratch_bytes=0):
        return _lib.lib.scarlet_observations_products_wide(ctypes.byref(st), arr, None, b0.ctypes.data_as(ctypes.c_void_p), 1,
                                                           ctypes.byref(ps), outs, None, scratch_bytes, None)
    assert call(_batch(4, 3, 33, 32, 32)) == _lib.E_NOTIMPL
    assert "SCARLET_MAX_CHANNELS" in _lib.last_error()
    # 17 channels pass the shape check: the flux partials then ask for scratch
    st = _batch(4, 3, 17, 32, 32)
    need = _lib.lib.scarlet_products_scratch_bytes_wide(ctypes.byref(st), ctypes.byref(ps))
    assert need >= 8 * 4 * 3                      # [S][T = 1][K] float64
    assert call(st) == _lib.E_ARG
    assert "scratch" in _lib.last_error()
    assert _lib.lib.scarlet_products_scratch_bytes_wide(ctypes.byref(_batch(4, 3, 33, 32, 32)), ctypes.byref(ps)) == 0


def test_from_observations_wide_host_checks():
    from scarlet_amd import ObservationBatch, BlendBatch, _lib
    cen = np.zeros((2, 1, 2), np.int32)

    def obs(widths):
        out, at = [], 0
        for w in widths:
            out.append(ObservationBatch(np.zeros((2, w, 8, 8)), band0=at))
            at += w
        return out
    # without the keyword: as always
    with pytest.raises(ValueError, match="at most 8"):
        BlendBatch.from_observations(obs([5, 4]), cen)
    # with it: 33 channels and a 9-band observation are refused before a device is needed
    with pytest.raises(ValueError, match="33 model channels, at most 32"):
        BlendBatch.from_observations(obs([8, 8, 8, 8, 1]), cen, wide=True)
    with pytest.raises(ValueError, match="at most 8"):
        BlendBatch.from_observations(obs([9, 3]), cen, wide=True)
    with pytest.raises(ValueError, match="the model frame has 9"):
        BlendBatch.from_observations(obs([5, 5]), cen, wide=True, _channels=9)
    # 9 and 32 channels pass every host-side check: the next thing asked for is the device
    for widths in ([5, 4], [8, 8, 8, 8]):
        try:
            b = BlendBatch.from_observations(obs(widths), cen, wide=True)
        except RuntimeError as e:
            assert "ROCm device" in str(e)
        else:
            assert b.B == sum(widths) and b._wide and tuple(b.sed[0].shape) == (2, 1, sum(widths))


def test_the_oracle_has_no_channel_limit():
    """oracle.pgm.fit on one 17-channel scene seen through 6 + 4 + 7 band slices: it runs, the loss falls, and with
    one observation over all 17 channels it takes the same steps up to the factor n_obs in the constants"""
    import wide_channels_common as wc
    case = wc.case("oracle", 7000, (6, 4, 7), S=1, K=3, iters=4)
    sed, morph, mse, cen, it, flags, L = wc.oracle_fit((wc.spec_of(case, case.host_state(), 0), 4, 0.0, np.float64))
    assert sed.shape == (3, 17) and morph.shape == (3, 32, 32) and it == 4 and L.shape == (3, 2)
    assert np.isfinite(sed).all() and np.isfinite(morph).all() and mse[-1] < mse[0]
    whole = wc.case("oracle", 7000, (6, 4, 7), S=1, K=3, iters=1)
    whole.obs = [dict(images=np.concatenate([o["images"] for o in whole.obs], axis=1), band0=0)]
    one = wc.oracle_fit((wc.spec_of(whole, whole.host_state(), 0), 1, 0.0, np.float64))
    three = wc.oracle_fit((wc.spec_of(case, case.host_state(), 0), 1, 0.0, np.float64))
    assert abs(one[2][0] - three[2][0]) <= 1e-12 * abs(one[2][0])              # the same loss
    np.testing.assert_allclose(three[6], 3 * one[6], rtol=1e-12)               # L x n_obs


def _plan(K, C, prior=0):
    from scarlet_amd import _lib
    out = np.zeros(8, np.int32)
    rc = _lib.lib.scarlet_debug_contract_plan(K, C, prior, out.ctypes.data_as(ctypes.c_void_p))
    return rc, dict(zip(("kernel", "cw", "nw", "block", "lds", "limit", "prior"), out.tolist()))


@pytest.mark.parametrize("prior", [0, 1])
def test_contract_plan_grid(prior):
    limit = 160 * 1024 - 1024                     # LDS_LIMIT of launch_plan.h
    for K in (1, 4, 8, 9, 32, 33, 256):
        for C in (9, 16, 17, 32):
            rc, p = _plan(K, C, prior)
            assert rc == 0 and p["kernel"] == 3 and p["limit"] == limit and p["prior"] == prior, (K, C)
            assert p["cw"] == (16 if C <= 16 else 32) and p["cw"] >= C
            assert p["nw"] in (4, 2, 1) and p["block"] == 64 * p["nw"]
            # the waves' float64 slots [nw][K][C] and the padded SEDs [K][cw]
            assert p["lds"] == K * (p["nw"] * C * 8 + p["cw"] * 4) and p["lds"] <= limit, (K, C)
            # ... with the most waves that fit
            if p["nw"] < 4:
                assert K * (2 * p["nw"] * C * 8 + p["cw"] * 4) > limit, (K, C)
        for C in (1, 5, 8):
            rc, p = _plan(K, C, prior)
            assert rc == 0 and p["kernel"] == (1 if K <= 8 else 2) and p["block"] == 256, (K, C)
            assert p["lds"] == K * 8 * (4 * 8 + 4)            # obs_contract_lds(K): four waves' float64 slots, float SEDs
    # the shapes the GPU tests rely on for the two- and one-wave instances
    assert _plan(160, 32)[1]["nw"] == 2 and _plan(256, 32)[1]["nw"] == 1 and _plan(256, 17)[1]["nw"] == 2
    assert _plan(40, 32)[1]["nw"] == 4
    for K, C in ((4, 33), (257, 17), (0, 9), (4, 0)):
        assert _plan(K, C)[0] == -1
