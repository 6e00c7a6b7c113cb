"""Shared by the tests of the low-resolution operator past its LDS limit (csrc/lowres_stream.h): the geometries, in the
form lowres_common.limit_geometry takes as a tuple, and the new entry points called as the old ones are in
test_gpu_lowres_limits.py."""
import ctypes

import numpy as np

import lowres_common as lc

# name -> (model (H, W), observation (h, w), pixel ratio, model-frame position (y, x) of observation pixel (0, 0),
# (model PSF, observation PSF) side in pixels, the bands B the device tests run it with)
#   p  the first shape past LDS: padded plane 100 x 100, nfy, nfx = 25, 49
#   q  ratio 3 with an offset: 108 x 108; 27, 53
#   r  the multi-resolution tutorial's scale (ratio 5): 270 x 270; 68, 135
#   n  non-square (the reference refuses it): model 100 x 90, observation 30 x 27
LARGE = {
    "p": ((96, 96), (48, 48), 2.0, (0.0, 0.0), (11, 9), 3),
    "q": ((104, 104), (32, 32), 3.0, (1.2, 2.1), (11, 9), 2),
    "r": ((256, 256), (48, 48), 5.0, (3.3, 4.1), (15, 9), 2),
    "n": ((100, 90), (30, 27), 3.0, (1.5, 2.0), (11, 9), 3),
}
SQUARE = ("p", "q", "r")          # what tests/golden/lowres_large.npz holds the reference's answers to


def spec(name):
    """LARGE[name], or lowres_common.LIMITS[name] for the names of that table"""
    return LARGE[name] if name in LARGE else lc.LIMITS[name]


def geometry(name, B=None, **kw):
    """lowres_common.limit_geometry of LARGE[name] (or LIMITS[name]) at B bands (default: the table's)"""
    g = spec(name)
    return lc.limit_geometry(g, B=g[5] if B is None else B, **kw)


def dims(obs):
    """(H, W, h, w, nfy, nfx) of a matched LowResObservation"""
    f = obs.factors
    return tuple(obs.model_shape) + tuple(obs.frame.shape[1:]) + (f["uy"].shape[0], f["ux"].shape[0])


def operate(geo, S, B, x, y, band, scene, large=True):
    """render of the planes x and adjoint of the planes y as float64 arrays, by scarlet_lowres_render_large /
    _adjoint_large with a scratch of scarlet_lowres_op_scratch_bytes (large) or by the LDS-resident entry points"""
    import torch
    import scarlet_amd as scarlet
    from scarlet_amd import _lib
    n, H, W = x.shape
    h, w = y.shape[1:]
    lo = scarlet.LowResObservationBatch(np.zeros((S, B, h, w), np.float32), geometry=geo)
    lr, keep = lo.lowres_struct("cuda")
    bd, sd = torch.as_tensor(band.astype(np.int32)).cuda(), torch.as_tensor(scene.astype(np.int32)).cuda()
    xd, yd = torch.as_tensor(x).cuda(), torch.as_tensor(y).cuda()
    Tx = torch.empty((n, h, w), dtype=torch.float32, device="cuda")
    Ty = torch.empty((n, H, W), dtype=torch.float32, device="cuda")
    if large:
        nbytes = int(_lib.check(_lib.lib.scarlet_lowres_op_scratch_bytes(n, H, W, ctypes.byref(lr))))
        scratch = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device="cuda")
        _lib.check(_lib.lib.scarlet_lowres_render_large(xd.data_ptr(), n, H, W, ctypes.byref(lr), bd.data_ptr(), sd.data_ptr(),
                                                        Tx.data_ptr(), scratch.data_ptr(), nbytes, _lib.stream_ptr()))
        _lib.check(_lib.lib.scarlet_lowres_adjoint_large(yd.data_ptr(), n, H, W, ctypes.byref(lr), bd.data_ptr(), sd.data_ptr(),
                                                         Ty.data_ptr(), scratch.data_ptr(), nbytes, _lib.stream_ptr()))
    else:
        _lib.check(_lib.lib.scarlet_lowres_render(xd.data_ptr(), n, H, W, ctypes.byref(lr), bd.data_ptr(), sd.data_ptr(),
                                                  Tx.data_ptr(), _lib.stream_ptr()))
        _lib.check(_lib.lib.scarlet_lowres_adjoint(yd.data_ptr(), n, H, W, ctypes.byref(lr), bd.data_ptr(), sd.data_ptr(),
                                                   Ty.data_ptr(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return Tx.cpu().numpy().astype(np.float64), Ty.cpu().numpy().astype(np.float64)


def planes(geo, S, B, seed=7):
    """S x B planes in shuffled order: plane p carries band band[p] of scene scene[p]; every (scene, band) occurs once"""
    g0 = geo[0] if isinstance(geo, list) else geo
    (H, W), (h, w) = g0.model_shape, g0.frame.shape[1:]
    rng = np.random.default_rng(seed)
    order = rng.permutation(S * B)
    x = rng.random((S * B, H, W)).astype(np.float32)
    y = rng.standard_normal((S * B, h, w)).astype(np.float32)
    return x, y, order % B, order // B


class options(object):
    """with options(LOWRES_STREAMED=1, ...): the library's switches set, and put back afterwards"""

    def __init__(self, **values):
        self.values, self.old = values, {}

    def __enter__(self):
        from scarlet_amd import _lib
        for k, v in self.values.items():
            self.old[k] = _lib.set_option(k, v)

    def __exit__(self, *exc):
        from scarlet_amd import _lib
        for k, v in self.old.items():
            _lib.set_option(k, v)
