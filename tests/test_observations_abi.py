"""CPU: the C ABI and host checks of fitting a batch against several observations (scarlet_fit_observations,
BlendBatch.from_observations / init_combined).  Every call below returns before a launch."""
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


def _call(fn, state, obs, band0, n=None):
    from scarlet_amd import _lib
    n = len(obs) if n is None else n
    arr = (ctypes.POINTER(_lib.ScarletBatch) * max(len(obs), 1))(*[ctypes.pointer(o) for o in obs])
    b0 = np.asarray(band0 if len(band0) else [0], dtype=np.int32)
    return getattr(_lib.lib, fn)(ctypes.byref(state), arr, b0.ctypes.data_as(ctypes.c_void_p), n, 1, 0.0, 0, 0, None)


def test_header_declares_fit_observations():
    text = open(HEADER).read()
    assert re.search(r"#define\s+SCARLET_MAX_OBSERVATIONS\s+8\b", text)
    flat = re.sub(r"\s+", " ", text)
    assert ("int scarlet_fit_observations(scarlet_batch *state, scarlet_batch *const *obs, const int32_t *band0, "
            "int n_obs, int max_iter, double e_rel, int approximate_L, int check_every, void *stream);") in flat
    from scarlet_amd import _lib
    assert _lib.MAX_OBSERVATIONS == 8
    fn = _lib.lib.scarlet_fit_observations
    assert fn.restype is ctypes.c_int
    assert fn.argtypes == _lib.lib.scarlet_fit_multi.argtypes
    assert len(fn.argtypes) == 9


def test_counts_on_the_state_reach_the_pointer_check():
    """the state's counts pass the shape checks of scarlet_fit_observations (null pointers then say E_ARG);
    scarlet_fit_multi still refuses them with E_NOTIMPL naming n_components"""
    from scarlet_amd import _lib
    st = _batch(4, 3, 5, 32, 32, pointers=False)
    st.n_components = FAKE
    ob = _batch(4, 3, 5, 32, 32)
    assert _call("scarlet_fit_observations", st, [ob], [0]) == _lib.E_ARG
    assert "null pointer" in _lib.last_error()
    assert _call("scarlet_fit_multi", st, [ob], [0]) == _lib.E_NOTIMPL
    assert "n_components" in _lib.last_error()
    # ... and with every pointer set the counts are accepted up to the observations' checks
    st = _batch(4, 3, 5, 32, 32)
    st.n_components = FAKE
    assert _call("scarlet_fit_observations", st, [ob], [1]) == _lib.E_ARG
    assert "does not fit" in _lib.last_error()


def test_observation_count_and_fit_errors():
    from scarlet_amd import _lib
    st = _batch(4, 3, 5, 32, 32)
    obs = [_batch(4, 3, 5, 32, 32) for _ in range(9)]
    for n in (0, 9):
        assert _call("scarlet_fit_observations", st, obs, [0] * 9, n=n) == _lib.E_ARG
        assert "1 to 8 observations" in _lib.last_error()
        assert _call("scarlet_fit_multi", st, obs, [0] * 9, n=n) == _lib.E_ARG
        assert "1 to 8 observations" in _lib.last_error()
    for bad, b0 in ((_batch(4, 3, 3, 32, 32), 3), (_batch(3, 3, 2, 32, 32), 0), (_batch(4, 2, 2, 32, 32), 0),
                    (_batch(4, 3, 2, 32, 16), 0), (_batch(4, 3, 2, 32, 32), -1)):
        assert _call("scarlet_fit_observations", st, [obs[0], bad], [0, b0]) == _lib.E_ARG
        assert "does not fit" in _lib.last_error()
    counted = _batch(4, 3, 2, 32, 32)
    counted.n_components = FAKE
    assert _call("scarlet_fit_observations", st, [obs[0], counted], [0, 3]) == _lib.E_ARG
    assert "n_components" in _lib.last_error()
    # shapes come first: a state of bad shape is E_ARG / E_NOTIMPL whatever its pointers
    assert _call("scarlet_fit_observations", _batch(4, 0, 5, 32, 32, pointers=False), [obs[0]], [0]) == _lib.E_ARG
    assert "shape" in _lib.last_error()
    assert _call("scarlet_fit_observations", _batch(4, 3, 9, 32, 32), [obs[0]], [0]) == _lib.E_NOTIMPL


def test_observation_batch_argument_errors():
    from scarlet_amd import ObservationBatch, BlendBatch
    with pytest.raises(ValueError):
        ObservationBatch(np.zeros((2, 3, 8)))
    with pytest.raises(ValueError):
        ObservationBatch(np.zeros((2, 3, 8, 8)), band0=-1)
    with pytest.raises(ValueError):
        ObservationBatch(np.zeros((2, 3, 8, 8)), weights=np.ones((2, 2, 8, 8)))
    with pytest.raises(ValueError):
        ObservationBatch(np.zeros((2, 3, 8, 8))).set_diff_kernel(np.zeros((2, 5, 5)))
    a = ObservationBatch(np.zeros((2, 3, 8, 8)))
    assert a.B == 3
    # from_observations refuses before it needs a device
    cen = np.zeros((2, 1, 2), np.int32)
    with pytest.raises(ValueError, match="1 to 8"):
        BlendBatch.from_observations([], cen)
    with pytest.raises(ValueError, match="1 to 8"):
        BlendBatch.from_observations([a] * 9, cen)
    with pytest.raises(ValueError, match="ObservationBatch"):
        BlendBatch.from_observations([np.zeros((2, 3, 8, 8))], cen)
    with pytest.raises(ValueError, match="scenes"):
        BlendBatch.from_observations([a, ObservationBatch(np.zeros((3, 2, 8, 8)), band0=3)], cen)
    with pytest.raises(ValueError, match="8"):
        BlendBatch.from_observations([a, ObservationBatch(np.zeros((2, 2, 8, 8)), band0=7)], cen)
    with pytest.raises(ValueError, match="the model frame has 2"):      # (the frame's channel count, as Blend passes it)
        BlendBatch.from_observations([a], cen, _channels=2)


def test_init_combined_argument_errors():
    """the checks of init_combined that need no device: a batch with its observation list attached but no tensors"""
    from scarlet_amd import ObservationBatch, BlendBatch
    b = BlendBatch.__new__(BlendBatch)
    b.torch, b.S, b.B = None, 2, 5
    b._observations = None
    with pytest.raises(ValueError, match="from_observations"):
        b.init_combined([np.ones(3), np.ones(2)])
    a, c = ObservationBatch(np.zeros((2, 3, 8, 8))), ObservationBatch(np.zeros((2, 2, 8, 8)), band0=3)
    b._observations = [(a, None), (c, None)]
    with pytest.raises(ValueError, match="tile"):
        BlendBatch.init_combined(_with(b, [(c, None), (a, None)]), [np.ones(2), np.ones(3)])
    with pytest.raises(ValueError, match="tile"):
        BlendBatch.init_combined(_with(b, [(a, None), (ObservationBatch(np.zeros((2, 2, 8, 8)), band0=2), None)]),
                                 [np.ones(3), np.ones(2)])
    with pytest.raises(ValueError, match="cover"):
        BlendBatch.init_combined(_with(b, [(a, None)]), [np.ones(3)])
    with pytest.raises(ValueError, match="obs_idx"):
        b.init_combined([np.ones(3), np.ones(2)], obs_idx=2)
    with pytest.raises(ValueError, match="one bg_rms"):
        b.init_combined([np.ones(3)])
    with pytest.raises(ValueError, match="bg_rms\\[1\\]"):
        b.init_combined([np.ones(3), np.ones(3)])
    with pytest.raises(ValueError, match="obs_psfs"):
        b.init_combined([np.ones(3), np.ones(2)], obs_psfs=[None])
    with pytest.raises(ValueError, match="obs_psfs\\[0\\]"):
        b.init_combined([np.ones(3), np.ones(2)], obs_psfs=[np.ones((2, 5, 5)), None])


def _with(b, obs):
    from scarlet_amd import BlendBatch
    c = BlendBatch.__new__(BlendBatch)
    c.__dict__.update(b.__dict__)
    c._observations = obs
    return c


def test_single_init_refused_on_an_observation_batch():
    from scarlet_amd import BlendBatch
    b = BlendBatch.__new__(BlendBatch)
    b._observations = [(None, None)]
    with pytest.raises(ValueError, match="init_combined"):
        b.init_extended(np.ones(5))
    with pytest.raises(ValueError, match="init_combined"):
        b.init_sources(np.ones(5))
