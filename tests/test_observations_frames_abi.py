"""CPU: joint fits of scenes with their own frames at the C ABI (scarlet_fit_observations_frames,
scarlet_observations_products_frames) and in the host layer (ObservationBatch(frame_shapes=...) / from_frames,
BlendBatch.from_observations).  Every C call below returns before a launch; every Python refusal is raised before a device
is asked for (on a host without a GPU a refusal that came late would be a RuntimeError instead)."""
import ctypes
import os
import re

import numpy as np
import pytest

import lowres_common as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scarlet_hip.h")
FAKE = 0x1000          # a non-NULL pointer that is never dereferenced
NAMES = ("scarlet_fit_observations_frames", "scarlet_observations_products_frames")


def _batch(S=4, K=3, B=5, H=32, W=32, pointers=True):
    from scarlet_amd import _lib
    b = _lib.ScarletBatch()
    b.S, b.K, b.B, b.H, b.W = S, K, B, H, W
    if pointers:
        for f in ("images", "cur", "centers", "shifts", "flags", "lipschitz", "mse", "it", "active", "status", "workspace"):
            setattr(b, f, FAKE)
        b.sed[0] = b.sed[1] = b.morph[0] = b.morph[1] = FAKE
        b.mse_capacity = 1
    return b


def _frames(ptr=FAKE):
    from scarlet_amd import _lib
    f = _lib.ScarletFrames()
    f.frame_hw = ptr
    return f


def _lists(obs, band0):
    from scarlet_amd import _lib
    arr = (ctypes.POINTER(_lib.ScarletBatch) * max(len(obs), 1))(*[ctypes.pointer(o) for o in obs])
    b0 = np.asarray(band0 if len(band0) else [0], dtype=np.int32)
    return arr, b0


def _fit(state, f, obs, band0, n=None, max_iter=1, cons=None):
    from scarlet_amd import _lib
    arr, b0 = _lists(obs, band0)
    return _lib.lib.scarlet_fit_observations_frames(
        None if state is None else ctypes.byref(state), None if f is None else ctypes.byref(f),
        None if cons is None else ctypes.byref(cons), arr, b0.ctypes.data_as(ctypes.c_void_p), len(obs) if n is None else n,
        max_iter, 0.0, 0, 0, None)


def _products(state, f, obs, band0, state_out=None, outs=None, n=None):
    from scarlet_amd import _lib
    arr, b0 = _lists(obs, band0)
    if outs is None:
        outs = (_lib.ScarletProducts * max(len(obs), 1))()
        for o in outs:
            o.rendered = FAKE
    return _lib.lib.scarlet_observations_products_frames(
        None if state is None else ctypes.byref(state), None if f is None else ctypes.byref(f), arr,
        b0.ctypes.data_as(ctypes.c_void_p), len(obs) if n is None else n, None if state_out is None else ctypes.byref(state_out),
        outs, None, 0, None)


def test_header_library_and_ctypes_agree():
    from scarlet_amd import _lib
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S))
    assert ("int scarlet_fit_observations_frames(scarlet_batch *state, const scarlet_frames *f, const scarlet_constraints *c , "
            "scarlet_batch *const *obs, const int32_t *band0, int n_obs, int max_iter, double e_rel, int approximate_L, "
            "int check_every, void *stream);") in flat
    assert ("int scarlet_observations_products_frames(const scarlet_batch *state, const scarlet_frames *f, "
            "scarlet_batch *const *obs, const int32_t *band0, int n_obs, const scarlet_products *state_out, "
            "const scarlet_products *out, void *scratch, int64_t scratch_bytes, void *stream);") in flat
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name), name
        assert getattr(_lib.lib, name).restype is ctypes.c_int
    # the arguments of the plain entry points with the frames struct after the state
    fit, plain = _lib.lib.scarlet_fit_observations_frames.argtypes, _lib.lib.scarlet_fit_observations_constrained.argtypes
    assert list(fit) == [plain[0], ctypes.POINTER(_lib.ScarletFrames)] + list(plain[1:])
    prod, plain = _lib.lib.scarlet_observations_products_frames.argtypes, _lib.lib.scarlet_observations_products.argtypes
    assert list(prod) == [plain[0], ctypes.POINTER(_lib.ScarletFrames)] + list(plain[1:])
    # scarlet_batch and scarlet_frames are as they were
    assert [f for f, _ in _lib.ScarletFrames._fields_] == ["frame_hw"] and ctypes.sizeof(_lib.ScarletFrames) == 8
    assert "frame_hw" not in [f for f, _ in _lib.ScarletBatch._fields_]


def test_fit_refusals_before_any_launch():
    from scarlet_amd import _lib
    st, f = _batch(), _frames()
    obs = [_batch(B=3), _batch(B=2)]
    # a NULL struct comes first, whatever else is wrong
    assert _fit(st, None, obs, [0, 3]) == _lib.E_ARG and "frames" in _lib.last_error()
    assert _fit(None, None, obs, [0, 3]) == _lib.E_ARG and "frames" in _lib.last_error()
    assert _fit(None, f, obs, [0, 3]) == _lib.E_ARG
    # group with frame_hw; without frame_hw the call is the plain one, which takes a group
    g = _batch()
    g.group = FAKE
    assert _fit(g, f, obs, [0, 3]) == _lib.E_NOTIMPL and "group" in _lib.last_error()
    # the argument errors of check_observations
    for n in (0, 9):
        assert _fit(st, f, [obs[0]] * 9, [0] * 9, n=n) == _lib.E_ARG and "1 to 8 observations" in _lib.last_error()
    for bad, b0 in ((_batch(B=3), 3), (_batch(S=3, B=2), 0), (_batch(K=2, B=2), 0), (_batch(B=2, W=16), 0), (_batch(B=2), -1)):
        assert _fit(st, f, [obs[0], bad], [0, b0]) == _lib.E_ARG and "does not fit" in _lib.last_error()
    counted = _batch(B=2)
    counted.n_components = FAKE
    assert _fit(st, f, [obs[0], counted], [0, 3]) == _lib.E_ARG and "n_components" in _lib.last_error()
    assert _fit(st, f, obs, [0, 3], max_iter=-1) == _lib.E_ARG and "max_iter" in _lib.last_error()
    assert _fit(_batch(pointers=False), f, obs, [0, 3]) == _lib.E_ARG and "null pointer" in _lib.last_error()
    assert _fit(_batch(K=0, pointers=False), f, obs, [0, 3]) == _lib.E_ARG and "shape" in _lib.last_error()
    assert _fit(_batch(H=2048), f, [_batch(B=3, H=2048)], [0]) == _lib.E_TOO_LARGE
    # a constraints struct with a symmetric array needs the centroid PSF, as in scarlet_fit_observations_constrained
    cons = _lib.ScarletConstraints()
    cons.symmetric = FAKE
    assert _fit(st, f, obs, [0, 3], cons=cons) == _lib.E_ARG and "centroid_psf" in _lib.last_error()
    # the state may span up to 32 channels (an observation keeps 8), not more
    wide = _batch(B=12)
    assert _fit(wide, f, [_batch(B=9)], [0]) == _lib.E_NOTIMPL and "8 bands" in _lib.last_error()
    assert _fit(wide, f, [_batch(B=8), _batch(B=8)], [0, 5]) == _lib.E_ARG and "does not fit" in _lib.last_error()
    assert _fit(_batch(B=33), f, [_batch(B=8)], [0]) == _lib.E_NOTIMPL and "32 channels" in _lib.last_error()


def test_products_refusals_before_any_launch():
    from scarlet_amd import _lib
    st, f = _batch(), _frames()
    obs = [_batch(B=3), _batch(B=2)]
    assert _products(st, None, obs, [0, 3]) == _lib.E_ARG and "frames" in _lib.last_error()
    assert _products(None, f, obs, [0, 3]) == _lib.E_ARG
    g = _batch()
    g.group = FAKE
    assert _products(g, f, obs, [0, 3]) == _lib.E_NOTIMPL and "group" in _lib.last_error()
    # those of scarlet_observations_products
    assert _products(st, f, obs, [0, 3], n=9) == _lib.E_ARG and "observation list" in _lib.last_error()
    empty = (_lib.ScarletProducts * 2)()
    assert _products(st, f, obs, [0, 3], outs=empty) == _lib.E_ARG and "every output is NULL" in _lib.last_error()
    assert _products(st, f, obs, [0, 4]) == _lib.E_ARG and "do not fit" in _lib.last_error()
    so = _lib.ScarletProducts()
    so.rendered = FAKE
    assert _products(st, f, obs, [0, 3], state_out=so) == _lib.E_ARG and "belong to an observation" in _lib.last_error()
    outs = (_lib.ScarletProducts * 2)()
    outs[1].model = FAKE
    assert _products(st, f, obs, [0, 3], outs=outs) == _lib.E_ARG and "belong to the state" in _lib.last_error()
    # (the loss leaves the kernels as float64 partials in the scratch, which _products does not pass)
    outs = (_lib.ScarletProducts * 2)()
    outs[0].loss = outs[1].loss = FAKE
    assert _products(st, f, obs, [0, 3], outs=outs) == _lib.E_ARG and "scratch" in _lib.last_error()


# ------------------------------------------------------------------ the host layer
def _scenes(B=3):
    rng = np.random.default_rng(3)
    return [rng.normal(size=(B, 20, 24)).astype(np.float32), rng.normal(size=(B, 17, 23)).astype(np.float32)]


CEN = np.array([[[10, 10]], [[8, 9]]], np.int32)


def test_observation_batch_with_frame_shapes():
    from scarlet_amd import ObservationBatch
    from scarlet_amd.batch import pad_frames
    ims = _scenes()
    block, shapes = pad_frames(ims)
    o = ObservationBatch(block, band0=2, frame_shapes=shapes)
    assert o.shape == (2, 3, 20, 24) and o.band0 == 2 and o.B == 3 and o.weights is None
    assert o.frame_shapes.dtype == np.int32 and o.frame_shapes.tolist() == [[20, 24], [17, 23]]
    p = ObservationBatch.from_frames(ims, band0=2)
    assert np.array_equal(p.images, block) and np.array_equal(p.frame_shapes, shapes) and p.band0 == 2
    assert p.shape[3] % 4 == 0 and p.shape[2:] == (20, 24)
    assert ObservationBatch.from_frames([np.zeros((2, 5, 9)), np.zeros((2, 7, 3))]).shape == (2, 2, 7, 12)
    # weights: a scalar, a block, or per-scene arrays (padded with zeros)
    assert ObservationBatch.from_frames(ims, weights=2.0).weights == 2.0
    w = ObservationBatch.from_frames(ims, weights=[np.ones((3, 20, 24)), np.full((3, 17, 23), 2.0)]).weights
    assert w.shape == (2, 3, 20, 24) and (w[1, :, :17, :23] == 2).all() and not w[1, :, 17:].any() and not w[1, :, :, 23:].any()
    assert ObservationBatch(block, weights=np.ones_like(block), frame_shapes=shapes).weights.shape == block.shape
    # shape, dtype and range of the entries
    for bad in ([[0, 24], [17, 23]], [[20, 24], [21, 23]], [[20, 24], [17, 25]], [[20, 24], [17, -1]]):
        with pytest.raises(ValueError, match="lies outside 1.."):
            ObservationBatch(block, frame_shapes=np.array(bad))
    for bad in (np.array([20, 24]), np.array([[20.0, 24.0], [17.0, 23.0]]), np.array([[20, 24]])):
        with pytest.raises(ValueError, match="frame_shapes must be"):
            ObservationBatch(block, frame_shapes=bad)
    with pytest.raises(ValueError):
        ObservationBatch(block[0], frame_shapes=shapes)
    with pytest.raises(ValueError, match="from_frames"):
        ObservationBatch(ims, frame_shapes=shapes)
    with pytest.raises(ValueError, match="list"):
        ObservationBatch.from_frames(block)
    with pytest.raises(ValueError, match="bands"):
        ObservationBatch.from_frames([ims[0], ims[1][:2]])
    # weights that do not match
    with pytest.raises(ValueError, match=r"weights\[1\]"):
        ObservationBatch.from_frames(ims, weights=[np.ones((3, 20, 24)), np.ones((3, 17, 22))])
    with pytest.raises(ValueError, match="weights"):
        ObservationBatch.from_frames(ims, weights=[np.ones((3, 20, 24))])
    with pytest.raises(ValueError, match="weights"):
        ObservationBatch(block, weights=np.ones((2, 3, 20, 20)), frame_shapes=shapes)


def test_observation_batch_without_frame_shapes_is_what_it_was():
    from scarlet_amd import ObservationBatch
    with pytest.raises(ValueError):
        ObservationBatch(np.zeros((2, 3, 8)))
    # a list of equally shaped arrays stays a uniform block
    a = ObservationBatch([np.zeros((3, 8, 8)), np.zeros((3, 8, 8))])
    assert a.shape == (2, 3, 8, 8) and a.frame_shapes is None
    b = ObservationBatch(np.zeros((2, 3, 8, 8)), band0=1, weights=2.0)
    assert b.frame_shapes is None
    assert sorted(vars(b)) == sorted(["images", "shape", "band0", "weights", "diff_kernel", "frame_shapes"])


def test_from_observations_host_refusals():
    """every one of these is raised before a device is asked for"""
    from scarlet_amd import BlendBatch, ObservationBatch, LowResObservationBatch
    from scarlet_amd.batch import pad_frames
    ims = _scenes()
    block, shapes = pad_frames(ims)
    a = ObservationBatch.from_frames([im[:2] for im in ims])
    b = ObservationBatch.from_frames([im[2:] for im in ims], band0=2)
    # shapes that differ between the observations: the observation and the first such scene are named
    other = shapes.copy()
    other[1] = (17, 20)
    with pytest.raises(ValueError, match=r"observation 1 has scene 1 at 17 x 20, observation 0 at 17 x 23"):
        BlendBatch.from_observations([a, ObservationBatch(block[:, 2:], band0=2, frame_shapes=other)], CEN)
    # a missing shape on one observation
    with pytest.raises(ValueError, match=r"observation 1 carries no frame_shapes.*scene 0"):
        BlendBatch.from_observations([a, ObservationBatch(block[:, 2:], band0=2)], CEN)
    with pytest.raises(ValueError, match=r"observation 0 carries no frame_shapes"):
        BlendBatch.from_observations([ObservationBatch(block[:, :2]), b], CEN)
    # lists of different maximum sizes give blocks of different sizes: the caller pads them to one
    small = ObservationBatch.from_frames([im[2:, :16, :20] for im in ims], band0=2)
    with pytest.raises(ValueError, match="one padded block"):
        BlendBatch.from_observations([a, small], CEN)
    # a centre outside its scene's own frame (inside the padded block)
    for c in ([[17, 9]], [[8, 23]]):
        with pytest.raises(ValueError, match="outside the scene's 17 x 23 frame"):
            BlendBatch.from_observations([a, b], np.array([[[10, 10]], c], np.int32))
    with pytest.raises(ValueError, match="outside the scene's 17 x 23 frame"):
        BlendBatch.from_observations([a, b], [np.array([[10, 10]]), np.array([[16, 22], [19, 23]])])
    # group=, the single-scene front end's host gradients, the old spelling
    with pytest.raises(NotImplementedError, match="group"):
        BlendBatch.from_observations([a, b], CEN, group=np.array([[-1], [-1]]))
    with pytest.raises(NotImplementedError, match="host-gradient"):
        BlendBatch.from_observations([a, b], CEN, _host_gradients=True)
    with pytest.raises(NotImplementedError, match="from_observations.*belong to the observations"):
        BlendBatch.from_observations([a, b], CEN, frame_shapes=shapes)
    # a low-resolution observation
    g = lc.fixture()
    geom, _ = lc.geometry(g, "a")
    lo = LowResObservationBatch(np.zeros((2, 2, 16, 16), np.float32), band0=3, geometry=geom)
    rng = np.random.default_rng(4)
    hi = ObservationBatch.from_frames([rng.normal(size=(3, 32, 32)).astype(np.float32), rng.normal(size=(3, 30, 25)).astype(np.float32)])
    with pytest.raises(NotImplementedError, match="low-resolution observation \\(observation 1\\)"):
        BlendBatch.from_observations([hi, lo], np.array([[[10, 10]], [[8, 9]]], np.int32))
    with pytest.raises(NotImplementedError):
        LowResObservationBatch.from_frames([np.zeros((2, 16, 16))])


def test_valid_ragged_observations_pass_the_host_checks():
    """... and then need the device, as a uniform joint batch does"""
    import torch
    from scarlet_amd import BlendBatch, ObservationBatch
    ims = _scenes()
    a = ObservationBatch.from_frames([im[:2] for im in ims])
    b = ObservationBatch.from_frames([im[2:] for im in ims], band0=2)
    uniform = [ObservationBatch(np.zeros((2, 3, 8, 8), np.float32))]
    if torch.cuda.is_available():
        assert BlendBatch.from_observations([a, b], CEN).frame_shapes.tolist() == [[20, 24], [17, 23]]
        assert BlendBatch.from_observations(uniform, np.zeros((2, 1, 2), np.int32)).frame_shapes is None
        return
    with pytest.raises(RuntimeError):
        BlendBatch.from_observations([a, b], CEN)
    with pytest.raises(RuntimeError):
        BlendBatch.from_observations(uniform, np.zeros((2, 1, 2), np.int32))


def test_init_combined_on_a_ragged_single_observation_batch_stays_refused():
    from scarlet_amd import BlendBatch
    b = BlendBatch.__new__(BlendBatch)
    b.frame_shapes, b._observations = object(), None
    with pytest.raises(NotImplementedError, match="not made by from_observations"):
        b.init_combined([np.ones(3)])
