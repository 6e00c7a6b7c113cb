"""Joint fits of scenes with their own frame sizes against a LOW-RESOLUTION observation: the cases shared by
tests/test_lowres_frame_cases.py (CPU), tests/test_lowres_frames_abi.py (CPU) and tests/test_gpu_lowres_frames.py.

Every scene has its own model frame (H_s, W_s), its own observation (h_s, w_s), pixel ratio and origin, hence its own
periodic plane, (nfy_s, nfx_s) and five factor matrices: `LowResObservation.match(own frame)`, float64, once per scene.
The expected values of the device tests are the float restatement `lowres_common.fit` run on each scene alone, on its
cropped arrays, with that scene's own factors.  All cases use the 11 px model PSF and the 9 px observation PSFs of
lowres_common (`limit_psfs`)."""
import functools

import numpy as np

import lowres_common as lc
from oracle import pgm

PSF_PX = (11, 9)
HI_PSF_SIGMA = 1.3           # the same-grid observation's PSFs (11 px), wider than the model PSF's 0.9

# name -> (bands of the low-resolution observation, [(model frame, observation, pixel ratio, origin (y, x)), ...])
CASES = {
    # padded to 32 x 32 and 16 x 16; (nfy, nfx) all different, both orientations of w <= h
    "small": (2, [((32, 32), (16, 16), 2.0, (0.0, 0.0)),
                  ((24, 24), (12, 12), 2.0, (0.0, 0.0)),
                  ((17, 23), (5, 7), 3.0, (1.0, 1.0)),
                  ((28, 20), (11, 8), 2.5, (0.3, 0.1)),
                  ((20, 32), (8, 14), 2.2, (0.5, 0.4))]),
    # the maxima (64, 64, 36, 36, 19, 37) come from different scenes: 134.5 KiB of LDS at B = 8
    "lds_edge": (8, [((64, 64), (32, 32), 2.0, (0.0, 0.0)),
                     ((48, 64), (18, 26), 2.4, (1.3, 0.6)),
                     ((40, 40), (36, 36), 1.1, (0.2, 0.2))]),
    # the maxima take 196 KiB, above the 159 KiB limit: the streamed form as it comes
    "streamed": (2, [((96, 96), (48, 48), 2.0, (0.0, 0.0)),
                     ((80, 72), (32, 30), 2.4, (1.3, 0.6))]),
}
SMALL_NF = [(9, 17), (7, 15), (5, 15), (9, 13), (7, 17)]
SOURCES = {"small": [3, 1, 2, 2, 3], "lds_edge": [2, 1, 2], "streamed": [2, 2]}
LDS_LIMIT = 159 * 1024


def n_scenes(name):
    return len(CASES[name][1])


@functools.lru_cache(maxsize=None)
def geometries(name, band0=3, C=None, B=None):
    """The case's scenes as matched LowResObservations (a tuple), each on its own model frame; the observation covers
    the model channels band0 .. band0 + B - 1 of C (default: it ends the model frame)"""
    bands, scenes = CASES[name]
    B = bands if B is None else B
    return tuple(geometry(m, o, r, org, B, band0, C) for m, o, r, org in scenes)


def geometry(model_shape, lr_shape, ratio, origin, B, band0=3, C=None):
    """One matched LowResObservation of B bands (zero images) on a model frame of C channels (lowres_common's
    limit_geometry, for model frames of up to 32 channels)"""
    import scarlet_amd as scarlet
    wm, wl = lc.wcs_pair(model_shape, lr_shape, ratio, origin)
    model_psf, lr_psfs = lc.limit_psfs(PSF_PX, B)
    model_channels = ["c%d" % c for c in range(band0 + B if C is None else C)]
    channels = model_channels[band0:band0 + B]
    if channels == model_channels:
        channels = model_channels
    frame = scarlet.Frame((len(model_channels),) + tuple(model_shape), wcs=wm, psfs=model_psf, channels=model_channels)
    obs = scarlet.LowResObservation(np.zeros((B,) + tuple(lr_shape), np.float32), wcs=wl, psfs=lr_psfs, channels=channels)
    return obs.match(frame)


def maxima(name):
    """(H, W, h, w, nfy, nfx) per dimension over the case's scenes"""
    return tuple(int(v) for v in np.max([dims_of(g) for g in geometries(name)], axis=0))


def dims_of(g):
    f = g.factors
    return tuple(g.model_shape) + (f["vy"].shape[0], f["vx"].shape[0], f["uy"].shape[0], f["ux"].shape[0])


def lds_bytes(dims, B):
    """lowres.h's lowres_lds for the shape `dims` = (H, W, h, w, nfy, nfx) at B bands"""
    H, W, h, w, nfy, nfx = dims
    return lc.scratch_terms(H, W, h, w, nfy, nfx)[1] + 8 * B * nfy * nfx


def pad_factors(f, dims):
    """the factor dict `f` (any dtype) zero-padded to dims = (H, W, h, w, nfy, nfx)"""
    H, W, h, w, nfy, nfx = dims
    shapes = dict(uy=(nfy, H), ux=(nfx, W), vy=(h, nfy), vx=(w, nfx), dhat=(f["dhat"].shape[0], nfy, nfx))
    out = {}
    for k, shape in shapes.items():
        out[k] = np.zeros(shape + f[k].shape[len(shape):], f[k].dtype)          # ((re, im) pairs keep their last axis)
        out[k][tuple(slice(0, n) for n in f[k].shape)] = f[k]
    return out


def blob(shape, center, sigma):
    y, x = np.mgrid[:shape[0], :shape[1]]
    return np.exp(-((y - center[0]) ** 2 + (x - center[1]) ** 2) / (2 * sigma ** 2))


def hi_psfs(nb):
    return np.array([lc.gauss(PSF_PX[0], HI_PSF_SIGMA + 0.1 * b) for b in range(nb)]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def scene_data(name, hi_bands=3, lo_band0=None):
    """The case's data, one dict per scene (a tuple): images_hi (hi_bands, H_s, W_s), images_lo and weights_lo
    (B, h_s, w_s), start sed0 (n_s, C), morph0 (n_s, H_s, W_s), centres (n_s, 2), and `geo`, the matched geometry.
    The low-resolution observation covers the channels lo_band0 (default hi_bands) .. lo_band0 + B - 1 = C - 1."""
    B = CASES[name][0]
    lo_band0 = hi_bands if lo_band0 is None else lo_band0
    C = lo_band0 + B
    geos = geometries(name, band0=lo_band0, C=C)
    rng = np.random.default_rng(sum(map(ord, name)))
    out = []
    for s, (geo, n) in enumerate(zip(geos, SOURCES[name])):
        H, W = geo.model_shape
        h, w = geo.frame.shape[1:]
        # centres well inside the frame and apart from each other
        cen = np.array([(H // 2, W // 2), (H // 3 - 1, (2 * W) // 3), ((2 * H) // 3 + 1, W // 3 - 1)][:n], dtype=np.int32)
        true_morph = np.array([blob((H, W), c, 1.6 + 0.4 * k) for k, c in enumerate(cen)])
        true_sed = 1.0 + rng.random((n, C))
        model = np.einsum("kc,kyx->cyx", true_sed, true_morph)
        hi = pgm.convolve(model[:hi_bands], pgm.match_psfs(hi_psfs(hi_bands), lc.limit_psfs(PSF_PX, 1)[0]))
        lo = lc.apply_by_matmul(geo.factors, model[lo_band0:])
        out.append(dict(
            images_hi=(hi + 0.02 * rng.standard_normal(hi.shape)).astype(np.float32),
            images_lo=(lo + 0.02 * rng.standard_normal(lo.shape)).astype(np.float32),
            weights_lo=(0.75 + 0.5 * rng.random((B, h, w))).astype(np.float32),
            sed0=(true_sed * (1.1 + 0.05 * s)).astype(np.float32),
            morph0=np.array([blob((H, W), c, 2.0) for c in cen]).astype(np.float32),
            centers=cen, geo=geo, hi_bands=hi_bands, lo_band0=lo_band0, C=C))
    return tuple(out)


def model_psf():
    return lc.limit_psfs(PSF_PX, 1)[0]


def diff_kernel(hi_bands=3):
    return pgm.match_psfs(hi_psfs(hi_bands), model_psf()).astype(np.float32)


def oracle_fit(d, iters, e_rel=0.0, approximate_L=False, start=None, switches=None):
    """`lowres_common.fit` of the scene `d` (an entry of `scene_data`) alone, on its own frame with its own factors.
    start: (sed, morph, centres, shifts) instead of the data's own start; switches: per component (symmetric, monotonic)"""
    obs = [dict(images=d["images_hi"], band_slice=slice(0, d["hi_bands"]), weights=1, diff_kernel=diff_kernel(d["hi_bands"])),
           dict(images=d["images_lo"], band_slice=slice(d["lo_band0"], d["C"]), weights=d["weights_lo"], factors=d["geo"].factors)]
    sed0, morph0, cen0, shifts = (d["sed0"], d["morph0"], d["centers"], None) if start is None else start
    sc = lc.scene_from((sed0, morph0, cen0), model_psf()[0], shifts=shifts)
    for k, src in enumerate(sc.sources):
        if switches is not None:
            src.symmetric, src.monotonic = (bool(v) for v in switches[k])
    return lc.fit(sc, obs, iters, e_rel=e_rel, approximate_L=approximate_L)
