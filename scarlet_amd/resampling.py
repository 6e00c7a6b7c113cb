"""Geometry of a coarser observation of the model frame (reference ``scarlet/resampling.py`` and the set-up half of
``LowResObservation``, observation.py:242-521), as float64 numpy.  It runs once per ``match`` and is not hot.

For frames that are not rotated against each other the reference's resample-and-convolve operator separates per axis.
Restricted to the frequencies its sinc cut keeps, it is a sandwich of five small complex matrices ("A
low-resolution observation"):

    out_c = Re( Vy . ( Dhat_c o (Uy . model_c . Ux^T) ) . Vx^T )

`lowres_factors` builds them; `apply_factors` / `adjoint_factors` are the float64 statements of the operator and of its
adjoint that the tests compare the device against.

Any WCS object serves that has ``.wcs.pc`` (or ``.cd``), ``.wcs.crpix``, ``.wcs.crval``, ``.naxis``, ``.array_shape``,
``deepcopy()``, ``all_pix2world`` and ``all_world2pix`` (astropy's does; it is not required).
"""
import numpy as np


class _Linear(object):
    """The ``.wcs`` member of `AffineWCS`: pc matrix, reference pixel (FITS, 1-based, (x, y)) and its sky position."""

    def __init__(self, pc, crpix, crval):
        self.pc = np.array(pc, dtype=np.float64).reshape(2, 2)
        self.crpix = tuple(float(v) for v in crpix)
        self.crval = tuple(float(v) for v in crval)


class AffineWCS(object):
    """A flat-sky WCS for callers without astropy: sky = crval + pc . (pixel + 1 - crpix), axes ordered (x, y) on the
    pixel side and (ra, dec) on the sky side, with the handful of astropy.wcs.WCS methods `LowResObservation` uses.

    shape : (Ny, Nx) of the image;  scale : pixel size (pc = scale * identity) unless `pc` is given
    crpix : FITS reference pixel (x, y), default (1, 1): pixel (0, 0) sits at crval"""

    naxis = 2

    def __init__(self, shape, scale=1.0, crpix=(1.0, 1.0), crval=(0.0, 0.0), pc=None):
        self.array_shape = (int(shape[-2]), int(shape[-1]))
        self.wcs = _Linear(np.eye(2) * float(scale) if pc is None else pc, crpix, crval)

    def deepcopy(self):
        return AffineWCS(self.array_shape, crpix=self.wcs.crpix, crval=self.wcs.crval, pc=self.wcs.pc.copy())

    def _separable(self):
        return self.wcs.pc[0, 1] == 0 and self.wcs.pc[1, 0] == 0

    def all_pix2world(self, x, y, origin, ra_dec_order=True):
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        pc, dx, dy = self.wcs.pc, x + (1 - origin) - self.wcs.crpix[0], y + (1 - origin) - self.wcs.crpix[1]
        if self._separable():                      # (the two axes may then come in different lengths)
            return [self.wcs.crval[0] + pc[0, 0] * dx, self.wcs.crval[1] + pc[1, 1] * dy]
        return [self.wcs.crval[0] + pc[0, 0] * dx + pc[0, 1] * dy, self.wcs.crval[1] + pc[1, 0] * dx + pc[1, 1] * dy]

    def all_world2pix(self, ra, dec, origin, ra_dec_order=True):
        ra, dec = np.asarray(ra, dtype=np.float64), np.asarray(dec, dtype=np.float64)
        pc, da, dd = self.wcs.pc, ra - self.wcs.crval[0], dec - self.wcs.crval[1]
        if self._separable():
            dx, dy = da / pc[0, 0], dd / pc[1, 1]
        else:
            inv = np.linalg.inv(pc)
            dx, dy = inv[0, 0] * da + inv[0, 1] * dd, inv[1, 0] * da + inv[1, 1] * dd
        return [dx + self.wcs.crpix[0] - (1 - origin), dy + self.wcs.crpix[1] - (1 - origin)]

    wcs_world2pix = all_world2pix


def next_fast_len(n):
    """Smallest 2^a 3^b 5^c >= n (scipy.fftpack.next_fast_len, as the reference's fft.py:99 uses it)."""
    n = int(n)
    if n <= 1:
        return 1
    best = None
    p5 = 1
    while p5 < 2 * n:
        p35 = p5
        while p35 < 2 * n:
            v = p35
            while v < n:
                v *= 2
            best = v if best is None or v < best else best
            p35 *= 3
        p5 *= 5
    return best


def fast_shape(sizes, padding=3):
    """Per axis next_fast_len(size + padding); the last axis is made even (a real transform runs along it)."""
    shape = [next_fast_len(int(s) + padding) for s in sizes]
    while shape[-1] % 2:
        shape[-1] = next_fast_len(shape[-1] + 1)
    return shape


def pad_start(n, n_padded):
    """First index of an n-long array centred in n_padded zeros: an odd array's centre lands right of the middle."""
    return (n_padded - n + 1) // 2


def pad_center(arr, shape):
    """Zero-pad the last two axes of `arr` to `shape`, centred as `pad_start` says."""
    out = np.zeros(arr.shape[:-2] + tuple(shape), dtype=arr.dtype)
    y0, x0 = pad_start(arr.shape[-2], shape[0]), pad_start(arr.shape[-1], shape[1])
    out[..., y0:y0 + arr.shape[-2], x0:x0 + arr.shape[-1]] = arr
    return out


def crop_center(arr, shape):
    """The centred `shape` part of the last two axes (the inverse of `pad_center`)."""
    y0, x0 = pad_start(shape[0], arr.shape[-2]), pad_start(shape[1], arr.shape[-1])
    return arr[..., y0:y0 + shape[0], x0:x0 + shape[1]]


def affine(wcs):
    """The 2 x 2 pixel-to-sky matrix of a WCS: ``wcs.wcs.pc``, or ``wcs.cd`` where there is none."""
    try:
        return np.asarray(wcs.wcs.pc, dtype=np.float64)
    except AttributeError:
        return np.asarray(wcs.cd, dtype=np.float64)


def pixel_scale(a):
    """Pixel size of an affine matrix as the reference measures it (observation.py:434-435)."""
    return np.sqrt(np.abs(a[0, 0]) * np.abs(a[1, 1] - a[0, 1] * a[1, 0]))


def rotation(a_obs, a_model):
    """(sin, cos, rotated?) of the angle between two frames: the normalised sums of the affine matrices' rows, their
    cross and dot products; rotated when sin^2 exceeds the float64 epsilon (observation.py:436-448)."""
    v_obs = np.sum(a_obs, axis=0)[:2] / pixel_scale(a_obs)
    v_mod = np.sum(a_model, axis=0)[:2] / pixel_scale(a_model)
    v_obs = v_obs / np.sqrt(np.sum(v_obs ** 2))
    v_mod = v_mod / np.sqrt(np.sum(v_mod ** 2))
    sin = float(v_obs[0] * v_mod[1] - v_obs[1] * v_mod[0])
    cos = float(np.dot(v_obs, v_mod))
    return sin, cos, bool(abs(sin) ** 2 > np.finfo(float).eps)


def _to_world(wcs, x, y):
    if np.size(wcs.array_shape) == 2:
        r = wcs.all_pix2world(x, y, 0, ra_dec_order=True)
    else:
        r = wcs.all_pix2world(x, y, 0, 0, ra_dec_order=True)
    return r[0], r[1]


def _to_pixel(wcs, ra, dec):
    if np.size(wcs.array_shape) == 2:
        r = wcs.all_world2pix(ra, dec, 0, ra_dec_order=True)
    else:
        r = wcs.all_world2pix(ra, dec, 0, 0, ra_dec_order=True)
    return r[0], r[1]


def axis_positions(wcs_from, shape_from, wcs_to):
    """Where the pixel rows and columns of one frame lie in the pixel coordinates of another, frames not rotated against
    each other: (y positions of the Ny rows, x positions of the Nx columns).  Rows are mapped along column 0 and columns
    along row 0, which for square frames is the reference's pairing of row i with column i up to the sky's curvature."""
    ny, nx = int(shape_from[-2]), int(shape_from[-1])
    rows, cols = np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64)
    ra, dec = _to_world(wcs_from, np.zeros(ny), rows)
    y = np.asarray(_to_pixel(wcs_to, ra, dec)[1], dtype=np.float64)
    ra, dec = _to_world(wcs_from, cols, np.zeros(nx))
    x = np.asarray(_to_pixel(wcs_to, ra, dec)[0], dtype=np.float64)
    return y, x


def match_patches(shape_hr, shape_lr, wcs_hr, wcs_lr):
    """Overlap of a fine and a coarse frame that are not rotated against each other (reference resampling.py:3-125 with
    isrot=False), per axis.  Returns a dict:

    lr_in, lr_at : per axis, the indices of the coarse pixels whose position p in the fine frame has 0 <= p < N + 1,
        and those positions
    hr_in : per axis, the indices of the fine pixels that lie inside the coarse frame by the same rule"""
    if wcs_hr is None or wcs_lr is None:
        raise ValueError("match_patches needs the WCS of both frames")
    ny_hr, nx_hr = int(shape_hr[-2]), int(shape_hr[-1])
    ny_lr, nx_lr = int(shape_lr[-2]), int(shape_lr[-1])
    y_at, x_at = axis_positions(wcs_lr, (ny_lr, nx_lr), wcs_hr)
    y_back, x_back = axis_positions(wcs_hr, (ny_hr, nx_hr), wcs_lr)
    my, mx = (y_at >= 0) & (y_at < ny_hr + 1), (x_at >= 0) & (x_at < nx_hr + 1)
    hy, hx = (y_back >= 0) & (y_back < ny_lr + 1), (x_back >= 0) & (x_back < nx_lr + 1)
    if not my.any() or not mx.any():
        raise ValueError("the two frames do not overlap: check the coordinates of the observations or the WCS")
    return dict(lr_in=(np.nonzero(my)[0], np.nonzero(mx)[0]), lr_at=(y_at[my], x_at[mx]),
                hr_in=(np.nonzero(hy)[0], np.nonzero(hx)[0]))


def _psf_wcs(wcs, shape):
    """A copy of `wcs` for a PSF image: sky origin at pixel (n / 2, n / 2) (FITS: n / 2 + 1), observation.py:281-296."""
    w = wcs.deepcopy()
    ny, nx = int(shape[-2]), int(shape[-1])
    if w.naxis == 2:
        w.wcs.crval = 0., 0.
        w.wcs.crpix = nx / 2. + 1, ny / 2. + 1
    else:
        w.wcs.crval = 0., 0., 0.
        w.wcs.crpix = nx / 2. + 1, ny / 2. + 1, 0.
    return w


def match_psfs(psf_hr, psfs_lr, wcs_hr, wcs_lr):
    """The model PSF and the observation's PSFs on one grid at the model's resolution (observation.py:252-315): the
    coarse PSFs are sinc-interpolated to the model pixels they overlap, the model PSF is cut to those pixels.
    Kept from the reference: the interpolation reads each coarse PSF transposed (square PSFs only), the model PSF cut
    sums to one and the coarse PSFs sum to one OVER ALL BANDS TOGETHER.
    Returns ((1, n, n), (B, n, n)) float64."""
    psf_hr = np.asarray(psf_hr, dtype=np.float64)
    psfs_lr = np.asarray(psfs_lr, dtype=np.float64)
    if psfs_lr.shape[-1] != psfs_lr.shape[-2] or psf_hr.shape[-1] != psf_hr.shape[-2]:
        raise NotImplementedError("LowResObservation: PSF images must be square (the reference's interpolation "
                                  "needs it)")
    m = match_patches(psf_hr.shape, psfs_lr.shape[1:], _psf_wcs(wcs_hr, psf_hr.shape), _psf_wcs(wcs_lr, psfs_lr.shape))
    (iy, ix), (py, px), (sy, sx) = m["lr_in"], m["lr_at"], m["hr_in"]
    valid = psfs_lr[:, iy.min():iy.max() + 1, ix.min():ix.max() + 1]
    step_y, step_x = abs(py[1] - py[0]), abs(px[1] - px[0])
    ky = np.sinc((py[None, :] - sy[:, None]) / step_y)             # [model rows][coarse rows]
    kx = np.sinc((px[:, None] - sx[None, :]) / step_x)             # [coarse columns][model columns]
    coarse = np.array([ky @ img.T @ kx for img in valid])
    fine = psf_hr[sy.min():sy.max() + 1, sx.min():sx.max() + 1].copy()
    if coarse.shape[1:] != fine.shape:
        raise ValueError("LowResObservation: the PSFs do not overlap on one patch of the model grid")
    return (fine / fine.sum())[None], coarse / coarse.sum()


def difference_kernel(psfs, target, padding=3):
    """The kernels that turn `target` (1, n, n) into `psfs` (B, n, n): the ratio of the spectra at the fast shape of
    2 n + padding, centred and cut back to n x n (reference fft.match_psfs, fft.py:264-301)."""
    n_y, n_x = psfs.shape[-2:]
    F = fast_shape((n_y + target.shape[-2], n_x + target.shape[-1]), padding)
    spec = lambda a: np.fft.rfftn(np.fft.ifftshift(pad_center(a, F), axes=(-2, -1)), axes=(-2, -1))
    ratio = spec(psfs) / spec(target)
    img = np.fft.fftshift(np.fft.irfftn(ratio, F, axes=(-2, -1)), axes=(-2, -1))
    return crop_center(img, (n_y, n_x))


def kept_frequencies(n):
    """The frequencies of an n-point periodic axis that survive the reference's sinc cut (observation.py:381-385): of the
    n // 2 + 1 bins k of the real transform those with k < q or k >= bins - ceil(bins / 4), q = bins // 4.
    Returns (k, weight) of the half spectrum -- weight 2 for a bin that stands for itself and its mirror, 1 for k = 0
    and for the Nyquist bin of an even n (numpy's inverse real transform drops their imaginary parts)."""
    bins = n // 2 + 1
    lo, hi = bins // 4, bins - (-(-bins // 4))
    k = np.array([i for i in range(bins) if i < lo or i >= hi], dtype=np.int64)
    w = np.where((k == 0) | ((n % 2 == 0) & (k == n // 2)), 1.0, 2.0)
    return k, w


def full_frequencies(n):
    """`kept_frequencies` written out over both signs: (f, weight) with the mirror of every bin listed separately, the
    Nyquist bin of an even n as +n/2 and -n/2 at weight 1/2 each (a shift by a fraction of a pixel tells them apart)."""
    k, _ = kept_frequencies(n)
    f, w = [], []
    for i in k:
        if i == 0:
            f.append(0); w.append(1.0)
        elif n % 2 == 0 and i == n // 2:
            f += [i, -i]; w += [0.5, 0.5]
        else:
            f += [i, -i]; w += [1.0, 1.0]
    return np.array(f, dtype=np.int64), np.array(w)


def lowres_factors(model_shape, lr_shape, psf_shape, diff_psf, y_at, x_at, area_ratio):
    """The five factor matrices of a matched low-resolution observation (complex128).

    model_shape : (H, W) of the model frame;  lr_shape : (h, w) of the observation;  psf_shape : of the model PSF
    diff_psf : (B, n, n) difference kernels at the model's resolution
    y_at, x_at : positions of the observation's rows / columns in model pixels
    area_ratio : (observation pixel / model pixel)^2

    The reference pads the model into a periodic plane of F = fast_shape(max(frame, PSF) + 3) with the frame at offset
    pad_start; along the observation's shorter axis (x when w <= h) it shifts the MODEL to every low-resolution column,
    along the other the KERNEL to every row, multiplies the two planes and sums.  That correlates along the first axis
    where a convolution is meant; it undoes this by mirroring the result along that axis.  Both are kept: the
    correlated axis carries the opposite sign in the model-side phases and its V rows come in reverse order.
    Returns dict(uy [nfy][H], ux [nfx][W], vy [h][nfy], vx [w][nfx], dhat [B][nfy][nfx], fft_shape)."""
    H, W = int(model_shape[0]), int(model_shape[1])
    h, w = int(lr_shape[0]), int(lr_shape[1])
    F = fast_shape((max(H, int(psf_shape[0])), max(W, int(psf_shape[1]))), 3)
    ny, nx = F
    cy, cx = ny // 2, nx // 2
    x_first = w <= h                                               # the reference's small_axis
    sgn_y, sgn_x = (1.0, -1.0) if x_first else (-1.0, 1.0)
    fy, wy = kept_frequencies(ny)                                  # half spectrum along y (the result's real part)
    fx, wx = full_frequencies(nx)
    # shifts: positions relative to half the extent they span (observation.py:470-471, 508-511)
    sy = np.asarray(y_at, dtype=np.float64) - (y_at.max() - y_at.min() + 1) / 2
    sx = np.asarray(x_at, dtype=np.float64) - (x_at.max() - x_at.min() + 1) / 2
    rows = np.arange(H) + pad_start(H, ny) - cy
    cols = np.arange(W) + pad_start(W, nx) - cx
    uy = np.exp(2j * np.pi * sgn_y * fy[:, None] * rows[None, :] / ny)
    ux = np.exp(2j * np.pi * sgn_x * fx[:, None] * cols[None, :] / nx)
    vy = wy[None, :] / ny * np.exp(-2j * np.pi * fy[None, :] * sy[:, None] / ny)
    vx = wx[None, :] / nx * np.exp(-2j * np.pi * fx[None, :] * sx[:, None] / nx)
    if x_first:
        vx = vx[::-1]
    else:
        vy = vy[::-1]
    # the spectra of the kernels padded into the plane (pad_center): only the kernels' own rows and columns are not zero,
    # so the two transforms run over those alone, as matrix products
    D = np.asarray(diff_psf, dtype=np.float64)
    py, px = np.arange(D.shape[-2]) + pad_start(D.shape[-2], ny), np.arange(D.shape[-1]) + pad_start(D.shape[-1], nx)
    ey = np.exp(-2j * np.pi * sgn_y * fy[:, None] * (py[None, :] - cy) / ny)
    ex = np.exp(-2j * np.pi * sgn_x * fx[:, None] * (px[None, :] - cx) / nx)
    dhat = area_ratio * (ey @ D @ ex.T)
    return dict(uy=uy, ux=ux, vy=np.ascontiguousarray(vy), vx=np.ascontiguousarray(vx), dhat=dhat, fft_shape=F)


def apply_factors(f, model):
    """The operator in float64: model (B, H, W) -> (B, h, w)."""
    spec = (f["uy"] @ np.asarray(model, dtype=np.float64) @ f["ux"].T) * f["dhat"]
    return np.real(f["vy"] @ spec @ f["vx"].T)


def adjoint_factors(f, resid):
    """Its adjoint in float64: (B, h, w) -> (B, H, W)."""
    spec = (f["vy"].T @ np.asarray(resid, dtype=np.float64) @ f["vx"]) * f["dhat"]
    return np.real(f["uy"].T @ spec @ f["ux"])
