"""Shared by the low-resolution tests: the fixture's geometries rebuilt with scarlet_amd.LowResObservation, the float64
statement of the operator, and a float restatement of the joint fit of Blend(sources, [Observation, LowResObservation])
on top of the CPU oracle (oracle.pgm), which knows observations on the model's grid only."""
import numpy as np

from conftest import load_golden
from oracle import pgm

CH5 = ["g", "r", "i", "z", "y"]


def fixture():
    return load_golden("lowres")


def wcs_pair(model_shape, lr_shape, ratio, origin):
    """(model WCS, observation WCS): model pixels of size 1, observation pixels of size `ratio` whose pixel (0, 0) sits
    at model-frame position origin = (y, x)."""
    from scarlet_amd.resampling import AffineWCS
    return (AffineWCS(model_shape, 1.0),
            AffineWCS(lr_shape, ratio, crpix=(1 - origin[1] / ratio, 1 - origin[0] / ratio)))


def geometry(g, name, model_channels=("r", "i"), channels=("r", "i"), origin=None, images=None, weights="fixture"):
    """The fixture's geometry `name` as a matched scarlet_amd.LowResObservation (and its model frame)."""
    import scarlet_amd as scarlet
    H, W = (int(v) for v in g[name + "_model_shape"])
    h, w = (int(v) for v in g[name + "_lr_shape"])
    origin = tuple(g[name + "_origin"]) if origin is None else origin
    wm, wl = wcs_pair((H, W), (h, w), float(g[name + "_ratio"]), origin)
    model_channels, channels = list(model_channels), list(channels)
    if channels == model_channels:
        channels = model_channels
    frame = scarlet.Frame((len(model_channels), H, W), wcs=wm, psfs=g[name + "_model_psf"].copy(), channels=model_channels)
    obs = scarlet.LowResObservation(g[name + "_images_lr"].copy() if images is None else images, wcs=wl,
                                    psfs=g[name + "_lr_psfs"].copy(),
                                    weights=g[name + "_weights_lr"].copy() if isinstance(weights, str) else weights,
                                    channels=channels)
    return obs.match(frame), frame


# Geometries at the limits of the low-resolution kernels (tests/golden/lowres_limits.npz holds what the reference says
# to d .. h): name -> (model (H, W), observation (h, w), pixel ratio, model-frame position (y, x) of observation pixel
# (0, 0), (model PSF, observation PSF) side in pixels, the bands B the device tests run it with).
#   d, g, f, e  the shapes scarlet_hip.h promises, at their largest B: dynamic LDS of 133 - 158 KiB, the opt-in range
#   h           pixel ratio near 1: the only one whose scratch buffers are sized by h x ldw (`scratch_terms`)
#   i           non-square frame and observation past 48 KiB
#   j           every GEMM dimension off 16 and off 4 (H, W, h, w, 2 nfy, 2 nfx = 17, 23, 5, 7, 10, 30)
LIMITS = {
    "d": ((64, 64), (32, 32), 2.0, (0.0, 0.0), (11, 9), 8),
    "e": ((84, 84), (42, 42), 2.0, (0.0, 0.0), (11, 9), 2),
    "f": ((76, 76), (24, 24), 3.0, (1.2, 2.1), (11, 9), 6),
    "g": ((72, 72), (36, 36), 2.0, (0.0, 0.0), (11, 9), 8),
    "h": ((40, 40), (36, 36), 1.1, (0.2, 0.2), (11, 9), 2),
    "i": ((48, 64), (18, 26), 2.4, (1.3, 0.6), (11, 9), 3),
    "j": ((17, 23), (5, 7), 3.0, (1.0, 1.0), (5, 5), 3),
}
LIMIT_CHANNELS = ["c%d" % c for c in range(8)]


def gauss(n, sigma, dy=0.0, dx=0.0):
    y, x = np.mgrid[:n, :n] - (n // 2)
    g = np.exp(-((y - dy) ** 2 + (x - dx) ** 2) / (2 * sigma ** 2))
    return g / g.sum()


def limit_psfs(psf_px, B):
    """(model PSF (1, P, P), the observation's PSFs (B, p, p)) of a LIMITS geometry, the fixture's for B = 2"""
    return (gauss(psf_px[0], 0.9)[None].astype(np.float32),
            np.array([gauss(psf_px[1], 0.9 + 0.15 * b, 0.2, -0.1) for b in range(B)]).astype(np.float32))


def limit_geometry(name, B=2, origin=None, lr_shape=None, band0=0, C=None, weights=None):
    """Geometry `name` of LIMITS as a matched scarlet_amd.LowResObservation of B bands (zero images) that covers the
    model channels band0 .. band0 + B - 1 of C, and its model frame."""
    import scarlet_amd as scarlet
    (H, W), hw, ratio, org, psf_px, _ = LIMITS[name] if isinstance(name, str) else name       # (or such a tuple itself)
    h, w = hw if lr_shape is None else lr_shape
    wm, wl = wcs_pair((H, W), (h, w), ratio, org if origin is None else origin)
    model_psf, lr_psfs = limit_psfs(psf_px, B)
    model_channels = LIMIT_CHANNELS[:band0 + B if C is None else C]
    channels = model_channels[band0:band0 + B]
    if channels == model_channels:
        channels = model_channels
    frame = scarlet.Frame((len(model_channels), H, W), wcs=wm, psfs=model_psf, channels=model_channels)
    obs = scarlet.LowResObservation(np.zeros((B, h, w), np.float32), wcs=wl, psfs=lr_psfs, weights=weights, channels=channels)
    return obs.match(frame), frame


def scratch_terms(H, W, h, w, nfy, nfx):
    """lowres.h's lowres_lds restated: the four products whose largest sizes the scratch buffers X and Y (floats), and
    the footprint in bytes without the B band spectra, which take 8 nfy nfx bytes each."""
    odd = lambda n: n | 1
    ny2, nx2 = 2 * nfy, 2 * nfx
    terms = {"2nfy x ld2x": ny2 * odd(nx2), "2nfy x ldw": ny2 * odd(w), "h x ldw": h * odd(w), "2nfy x ldW": ny2 * odd(W)}
    sz = max(terms.values())
    proj = H * odd(W) + H * odd(nx2)
    fixed = ny2 * odd(H) + nx2 * odd(W) + h * odd(ny2) + w * odd(nx2) + sz + max(proj, sz)
    return terms, 4 * fixed


def apply_by_matmul(f, model):
    """resampling.apply_factors as four matrix products (float64; the fits call it every iteration, and the three-operand
    einsum there takes 0.1 s per call at 8 bands of 72 x 72); tests/test_lowres_host.py holds the two together"""
    spec = (f["uy"] @ np.asarray(model, dtype=np.float64) @ f["ux"].T) * f["dhat"]
    return np.real(f["vy"] @ spec @ f["vx"].T)


def adjoint_by_matmul(f, resid):
    """resampling.adjoint_factors likewise"""
    spec = (f["vy"].T @ np.asarray(resid, dtype=np.float64) @ f["vx"]) * f["dhat"]
    return np.real(f["uy"].T @ spec @ f["ux"])


def lowres_loss_and_gradients(seds, morphs, ob):
    """pgm.loss_and_gradients for a low-resolution observation: the operator and its adjoint in float64
    (resampling.apply_factors / adjoint_factors as matrix products), the gradients in the factors' dtype."""
    dt = seds[0].dtype
    images = np.asarray(ob["images"], dtype=np.float64)
    model = pgm.scene_model(seds, morphs, (len(seds[0]),) + morphs[0].shape, np.float64)
    w = ob.get("weights", 1)
    d = w * (apply_by_matmul(ob["factors"], model) - images)
    G = adjoint_by_matmul(ob["factors"], w * d)
    return (0.5 * np.sum(d ** 2), [(G * m[None]).sum(axis=(1, 2)).astype(dt) for m in morphs],
            [(G * s[:, None, None]).sum(axis=0).astype(dt) for s in seds])


def fit(scene, observations, max_iter, e_rel=0, approximate_L=False):
    """oracle.pgm.fit's loop over several observations, some of them low-resolution: dicts with images, band_slice,
    weights and either diff_kernel (model grid; may be None) or factors (low resolution)."""
    for _ in range(max_iter):
        seds = [c.sed for c in scene.sources]
        morphs = [c.morph for c in scene.sources]
        loss = 0
        gs = [np.zeros_like(sd) for sd in seds]
        gm = [np.zeros_like(m) for m in morphs]
        for ob in observations:
            sl = ob["band_slice"]
            sub = [sd[sl] for sd in seds]
            if "factors" in ob:
                l_, gs_, gm_ = lowres_loss_and_gradients(sub, morphs, ob)
            else:
                l_, gs_, gm_ = pgm.loss_and_gradients(sub, morphs, ob["images"], ob.get("weights", 1), ob.get("diff_kernel"))
            loss = loss + l_
            for k in range(len(seds)):
                gs[k][sl] += gs_[k]
                gm[k] = gm[k] + gm_[k]
        scene.mse.append(loss)
        L_sed, L_morph = pgm.lipschitz(seds, morphs, len(observations), approximate_L, scene.mse)
        for c, g_s, g_m in zip(scene.sources, gs, gm):
            c.L_sed, c.L_morph = L_sed, L_morph
            if not c.fix_sed:
                c.sed = c.sed - (1 / c.L_sed) * g_s
            if not c.fix_morph:
                c.morph = c.morph - (1 / c.L_morph) * g_m
        for c in scene.sources:
            pgm.source_update(c, scene.it)
        if pgm.check_convergence(scene, e_rel):
            break
    return scene


def fit_inputs(g, name):
    """The fixture's joint fit of geometry `name`: (the oracle's observation dicts, start (sed, morph, centres), the model
    PSF = the centroid weight, the matched LowResObservation)."""
    lo, _ = geometry(g, name, model_channels=CH5, channels=CH5[3:], images=g[name + "_fit_images_lr"].copy())
    model_psf = g[name + "_model_psf"]
    diff = pgm.match_psfs(g[name + "_hr_psfs"].astype(np.float32), model_psf.astype(np.float32)).astype(np.float32)
    obs = [dict(images=g[name + "_fit_images_hr"], band_slice=slice(0, 3), weights=1, diff_kernel=diff),
           dict(images=g[name + "_fit_images_lr"], band_slice=slice(3, 5), weights=g[name + "_weights_lr"], factors=lo.factors)]
    start = (g[name + "_fit_sed0"].copy(), g[name + "_fit_morph0"].copy(), g[name + "_fit_centers0"].copy())
    return obs, start, model_psf[0], lo


def scene_from(start, centroid_weight, shifts=None, n=None):
    sed0, morph0, cen0 = start
    n = len(sed0) if n is None else n
    H, W = morph0.shape[-2:]
    return pgm.scene_from_state(np.zeros((sed0.shape[1], H, W), np.float32), sed0[:n], morph0[:n], cen0[:n], shifts,
                                centroid_weight=centroid_weight)


def render_by_planes(obs, model):
    """The reference's algorithm stated directly (observation.py:345-403, 524-558) in float64, for checking the factor
    sandwich where the reference itself cannot run (non-square frames): pad model and difference kernels into the
    periodic plane; low-pass and shift the MODEL along the observation's shorter axis to every low-resolution position
    and the KERNEL along the other axis, by phases on a real transform of that axis; multiply plane by plane and sum;
    mirror the result along the model's axis."""
    from scarlet_amd import resampling as rs
    H, W = obs.model_shape
    h, w = obs.frame.shape[1:]
    F = obs._fft_shape
    y_at, x_at = obs._coord_hr
    sy = y_at - (y_at.max() - y_at.min() + 1) / 2
    sx = x_at - (x_at.max() - x_at.min() + 1) / 2
    a_obs, a_model = rs.affine(obs.frame.wcs), rs.affine(rs.AffineWCS((H, W), 1.0))
    D = rs.pad_center(np.asarray(obs._diff_kernels, dtype=np.float64), F) * (rs.pixel_scale(a_obs) / rs.pixel_scale(a_model)) ** 2
    M = rs.pad_center(np.asarray(model, dtype=np.float64), F)

    def shifted(planes, shifts, axis):
        n = planes.shape[axis]
        spec = np.fft.rfft(np.fft.ifftshift(planes, axes=axis), axis=axis)
        keep = np.zeros(n // 2 + 1)
        keep[rs.kept_frequencies(n)[0]] = 1
        phase = keep[None, :] * np.exp(-2j * np.pi * np.fft.rfftfreq(n)[None, :]) ** shifts[:, None]     # [shift][bin]
        shape = [1, len(shifts), 1, 1]
        shape[axis + 1] = n // 2 + 1
        moved = spec[:, None] * phase.reshape(shape)
        return np.fft.fftshift(np.fft.irfft(moved, n, axis=axis + 1), axes=axis + 1)               # [B][shift][Fy][Fx]

    if w <= h:
        out = np.einsum("bjyx,biyx->bij", shifted(M, sx, 2), shifted(D, sy, 1))
        return out[:, :, ::-1]
    out = np.einsum("biyx,bjyx->bij", shifted(M, sy, 1), shifted(D, sx, 2))
    return out[:, ::-1, :]
