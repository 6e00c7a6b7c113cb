"""Frame, Observation and LowResObservation (reference ``scarlet/observation.py`` API).

`Frame` describes the model (shape, PSF, channels, dtype); `Observation` holds the data
(images, weights, PSFs) and, after ``match(model_frame)``, the band slice and the PSF
difference kernel that map the model into the observed frame.  Data live on the device;
the engine computes in float32: a float64 DATA frame is cast to the model frame's dtype by ``match``
(as in the reference), a float64 MODEL frame is accepted with one warning -- the factors are stored in float32
(component._require_float32_frame; a strict opt-in refuses it).
"""
import ctypes
import logging

import numpy as np

from . import _lib
from . import fft

logger = logging.getLogger("scarlet_amd.observation")


class Frame(object):
    """Spatial and spectral characteristics of a model or of data
    (reference observation.py:13-99)."""

    def __init__(self, shape, wcs=None, psfs=None, channels=None, dtype=np.float32):
        assert len(shape) == 3
        self._shape = tuple(shape)
        self.wcs = wcs
        if psfs is None:
            logger.warning('No PSFs specified. Possible, but dangerous!')
        else:
            msg = 'PSFs need to have shape (1,Ny,Nx) for Blend and (B,Ny,Nx) for Observation'
            assert len(psfs) == 1 or len(psfs) == shape[0], msg
            if not isinstance(psfs, fft.Fourier):
                psfs = fft.Fourier(np.array(psfs))
            if not np.allclose(psfs.sum(axis=(1, 2)), 1):
                logger.warning('PSFs not normalized. Normalizing now..')
                psfs.normalize()
            if dtype != psfs.image.dtype:
                logger.warning("Dtypes of PSFs and Frame different. Casting PSFs to {}".format(dtype))
                psfs.update_dtype(dtype)
        self._psfs = psfs
        assert channels is None or len(channels) == shape[0]
        self.channels = channels
        self.dtype = dtype

    @property
    def C(self):
        return self._shape[0]

    @property
    def Ny(self):
        return self._shape[1]

    @property
    def Nx(self):
        return self._shape[2]

    @property
    def shape(self):
        return self._shape

    @property
    def psfs(self):
        return self._psfs

    def get_pixel(self, sky_coord):
        """Pixel (y, x) of a sky coordinate: integer truncation without a WCS
        (reference observation.py:84-99)."""
        if self.wcs is not None:
            if self.wcs.naxis == 3:
                coord = self.wcs.wcs_world2pix(sky_coord[0], sky_coord[1], 0, 0)
            elif self.wcs.naxis == 2:
                coord = self.wcs.wcs_world2pix(sky_coord[0], sky_coord[1], 0)
            else:
                raise ValueError("Invalid number of wcs dimensions: {0}".format(self.wcs.naxis))
            return (int(coord[0].item()), int(coord[1].item()))
        return tuple(int(coord) for coord in sky_coord)


def lowres_struct(factors, h, w, B, per_scene, device):
    """(struct scarlet_lowres without a workspace, the device tensors it points to) from the host factor matrices:
    `factors_f32()` of one geometry, or the dict whose vy / vx / dhat are stacked per scene (`per_scene`)."""
    torch = _lib.require_gpu()
    t = {k: torch.as_tensor(v).to(device).contiguous() for k, v in factors.items()}
    lr = _lib.ScarletLowres()
    lr.h, lr.w, lr.B = int(h), int(w), int(B)
    lr.nfy, lr.nfx = t["uy"].shape[0], t["ux"].shape[0]
    for k, v in t.items():
        setattr(lr, k, v.data_ptr())
    lr.v_per_scene = lr.dhat_per_scene = int(per_scene)
    return lr, t


def _match_dtype_and_bands(obs, model_frame):
    """What both `match` methods begin with (reference observation.py:155-180): the data cast to the model frame's
    dtype, and the band slice from the two frames' channels."""
    if obs.frame.dtype != model_frame.dtype:
        msg = "Dtypes of model and observation different. Casting observation to {}"
        logger.warning(msg.format(model_frame.dtype))
        obs.frame.dtype = model_frame.dtype
        obs.images = obs.images.astype(model_frame.dtype)
        if type(obs.weights) is np.ndarray:
            obs.weights = obs.weights.astype(model_frame.dtype)
        if obs.frame._psfs is not None:
            obs.frame.psfs.update_dtype(model_frame.dtype)
    obs._band_slice = slice(None)
    if obs.frame.channels is not model_frame.channels:
        assert obs.frame.channels is not None and model_frame.channels is not None
        bmin = list(model_frame.channels).index(obs.frame.channels[0])
        bmax = list(model_frame.channels).index(obs.frame.channels[-1])
        obs._band_slice = slice(bmin, bmax + 1)


def _weighted_loss(obs, d):
    """0.5 * sum (weights * d)^2 for the residual d on the device: array weights, a scalar other than 1, or none."""
    w = obs._weights_device()
    if w is not None:
        d = w * d
    elif obs.weights != 1:
        d = float(obs.weights) * d
    return 0.5 * (d.double() ** 2).sum()


class Observation(object):
    """Images, weights and PSFs of one data set (reference observation.py:102-239)."""

    def __init__(self, images, psfs=None, weights=None, wcs=None, channels=None, padding=10):
        images = np.asarray(images) if not hasattr(images, "detach") else images.detach().cpu().numpy()
        self.frame = Frame(images.shape, wcs=wcs, psfs=psfs, channels=channels, dtype=images.dtype)
        self.images = np.array(images)
        self.weights = np.array(weights) if weights is not None else 1
        self._padding = padding
        self._band_slice = slice(None)
        self._diff_kernels = None
        self._device = {}

    def match(self, model_frame):
        """Set up the mapping from the model frame to this observation: dtype, band slice and
        PSF difference kernel (reference observation.py:155-196)."""
        _match_dtype_and_bands(self, model_frame)
        self._diff_kernels = None
        if self.frame.psfs is not model_frame.psfs:
            assert self.frame.psfs is not None and model_frame.psfs is not None
            self._diff_kernels = fft.match_psfs(self.frame.psfs, model_frame.psfs)
        self._device = {}
        return self

    # ---- device copies used by the engine
    def _images_device(self):
        torch = _lib.require_gpu()
        if "images" not in self._device:
            self._device["images"] = torch.as_tensor(np.ascontiguousarray(self.images, dtype=np.float32)).cuda()
        return self._device["images"]

    def _weights_device(self):
        torch = _lib.require_gpu()
        if type(self.weights) is not np.ndarray:
            return None
        if "weights" not in self._device:
            w = np.broadcast_to(self.weights, self.images.shape)
            self._device["weights"] = torch.as_tensor(np.ascontiguousarray(w, dtype=np.float32)).cuda()
        return self._device["weights"]

    def render(self, model):
        """Map a model (bands, height, width) into the observed frame: band slice, then
        convolution with the difference kernel if there is one (reference observation.py:203-220)."""
        model_ = model[self._band_slice, :, :]
        if self._diff_kernels is not None:
            from .blend import render_with_kernel
            model_ = render_with_kernel(model_, self._diff_kernels.image)
        return model_

    def get_loss(self, model):
        """0.5 * sum (weights * (render(model) - images))^2 (reference observation.py:222-239)."""
        torch = _lib.require_gpu()
        m = self.render(model)
        m = m if torch.is_tensor(m) else torch.as_tensor(np.asarray(m)).cuda()
        return _weighted_loss(self, m.to(torch.float32) - self._images_device())

    def as_batch(self):
        """This observation as the one-scene `ObservationBatch` that `BlendBatch.from_observations` takes."""
        from .batch import ObservationBatch
        ob = ObservationBatch(self._images_device()[None], band0=self._band_slice.start or 0, weights=self._batch_weights())
        if self._diff_kernels is not None:
            ob.set_diff_kernel(np.asarray(self._diff_kernels.image, dtype=np.float32))
        return ob

    def _batch_weights(self):
        """the weights as a batch of one scene takes them: (1, B, H, W) on the device, or the Python scalar"""
        w = self._weights_device()
        return self.weights if w is None else w[None]


class LowResObservation(Observation):
    """A data set with coarser pixels than the model frame and its own PSFs, fitted jointly with the others
    (reference observation.py:242-599): ``Blend(sources, [obs_hr, obs_lr])``.

    images : (B, h, w);  wcs : required, any object `scarlet_amd.resampling` can read (astropy's WCS, or
    `resampling.AffineWCS`);  psfs : required, (B, p, p) on the observation's own pixel grid
    operator : 'exact', 'bilinear' or 'SVD' -- accepted and ignored, as in the reference

    Scope: frames that are not rotated against each other (a rotated pair raises NotImplementedError in `match`); pixel
    ratios need not be integers and the grids may be offset by fractions of a pixel.  The batch classes further need
    every low-resolution pixel inside the model frame (`covers`).
    """

    def __init__(self, images, wcs=None, psfs=None, weights=None, channels=None, padding=3, operator='exact'):
        assert wcs is not None, "WCS is necessary for LowResObservation"
        assert psfs is not None, "PSFs are necessary for LowResObservation"
        assert operator in ['exact', 'bilinear', 'SVD']
        Observation.__init__(self, images, psfs=psfs, weights=weights, wcs=wcs, channels=channels, padding=padding)
        self._factors = None

    def match(self, model_frame):
        """Dtype and band slice as `Observation.match`; then the geometry (reference observation.py:405-521): the
        overlap of the two grids, the PSFs matched at the model's resolution and their difference kernels, and from them
        the five factor matrices of the operator (`resampling.lowres_factors`).

        Sets ``lr_shape`` (the rows and columns of the observation that lie inside the model frame), ``covers`` (they
        are all of them), ``_band_slice``, ``origin`` / ``step`` (the model-frame position of pixel (0, 0) and the pixel
        ratio per axis), ``model_psf`` (the model frame's PSF image the kernels were matched to) and ``factors``
        (complex128; `factors_f32` and the device tensors derive from it)."""
        from . import resampling as rs
        _match_dtype_and_bands(self, model_frame)
        assert model_frame.wcs is not None and model_frame.psfs is not None, "the model frame needs a WCS and a PSF"
        a_obs, a_model = rs.affine(self.frame.wcs), rs.affine(model_frame.wcs)
        self.sin_rot, self.cos_rot, self.isrot = rs.rotation(a_obs, a_model)
        if self.isrot:
            raise NotImplementedError("LowResObservation: frames rotated against each other are not supported (the "
                                      "operator does not separate per axis)")
        self.sin_rot, self.cos_rot = 0, 1
        H, W = model_frame.Ny, model_frame.Nx
        h, w = self.frame.Ny, self.frame.Nx
        m = rs.match_patches((H, W), (h, w), model_frame.wcs, self.frame.wcs)
        (iy, ix), (y_at, x_at) = m["lr_in"], m["lr_at"]
        self._coord_lr, self._coord_hr = (iy, ix), (y_at, x_at)
        self.lr_shape = (int(iy.max() - iy.min() + 1), int(ix.max() - ix.min() + 1))
        self.covers = self.lr_shape == (h, w)
        self.small_axis = w <= h
        self.model_shape = (H, W)
        self.origin = (float(y_at[0]), float(x_at[0]))       # (of the first pixel inside: pixel (0, 0) when `covers`)
        self.step = (float(y_at[1] - y_at[0]) if len(y_at) > 1 else 1.0, float(x_at[1] - x_at[0]) if len(x_at) > 1 else 1.0)
        model_psf = np.asarray(model_frame.psfs.image)[0]
        self.model_psf = model_psf                       # (the batch classes check that the scenes of a batch share it)
        fine, coarse = rs.match_psfs(model_psf, np.asarray(self.frame.psfs.image), model_frame.wcs, self.frame.wcs)
        self._diff_kernels = rs.difference_kernel(coarse, fine)
        self._factors = None
        if self.covers:
            area = (rs.pixel_scale(a_obs) / rs.pixel_scale(a_model)) ** 2
            self._factors = rs.lowres_factors((H, W), (h, w), model_psf.shape, self._diff_kernels, y_at, x_at, area)
            self._fft_shape = self._factors["fft_shape"]
        self._device = {}
        return self

    @property
    def factors(self):
        """dict(uy, ux, vy, vx, dhat) complex128 of the matched geometry."""
        if self._factors is None:
            raise ValueError("LowResObservation: match() a model frame that contains every pixel of the observation first "
                             "(lr_shape = %s of %s)" % (getattr(self, "lr_shape", None), self.frame.shape[1:]))
        return self._factors

    def factors_f32(self):
        """The five matrices as float32 arrays whose last axis is (re, im): what the library reads."""
        f = self.factors
        return {k: np.ascontiguousarray(np.stack([f[k].real, f[k].imag], axis=-1), dtype=np.float32)
                for k in ("uy", "ux", "vy", "vx", "dhat")}

    def pixel_of(self, y, x):
        """The observation's pixel (row, column) under model-frame position (y, x), truncated as Frame.get_pixel does."""
        return int((y - self.origin[0]) / self.step[0]), int((x - self.origin[1]) / self.step[1])

    def _lowres_struct(self):
        """(struct scarlet_lowres without a workspace, the device tensors it points to)"""
        if "lowres" not in self._device:
            f = self.factors_f32()
            self._device["lowres"] = lowres_struct(f, self.frame.Ny, self.frame.Nx, f["dhat"].shape[0], False, "cuda")
        return self._device["lowres"]

    def _render(self, model):
        """The model's band slice resampled and convolved into the observation's pixels, on the device: (B, h, w)."""
        torch = _lib.require_gpu()
        lr, _keep = self._lowres_struct()
        m = model if torch.is_tensor(model) else torch.as_tensor(np.asarray(model))
        m = m[self._band_slice].to(device="cuda", dtype=torch.float32).contiguous()
        B, H, W = m.shape
        if (H, W) != tuple(self.model_shape) or B != lr.B:
            raise ValueError("LowResObservation.render: the model's band slice is %s, matched was %s"
                             % (tuple(m.shape), (lr.B,) + tuple(self.model_shape)))
        band = torch.arange(B, dtype=torch.int32, device="cuda")
        out = torch.empty((B, lr.h, lr.w), dtype=torch.float32, device="cuda")
        # (0 bytes where the model frame lets the LDS-resident kernel run)
        nbytes = int(_lib.check(_lib.lib.scarlet_lowres_op_scratch_bytes(B, H, W, ctypes.byref(lr))))
        scratch = torch.empty((nbytes,), dtype=torch.uint8, device="cuda") if nbytes else None
        _lib.check(_lib.lib.scarlet_lowres_render_large(m.data_ptr(), B, H, W, ctypes.byref(lr), band.data_ptr(), None,
                                                        out.data_ptr(), _lib.ptr(scratch), nbytes, _lib.stream_ptr()))
        return out

    def render(self, model):
        """The model as this observation sees it (reference observation.py:561-578; every pixel lies inside the model
        frame, so the rendered patch is the whole image)."""
        return self._render(model)

    def get_loss(self, model):
        """0.5 * sum (weights * (render(model) - images))^2 (reference observation.py:580-599)."""
        return _weighted_loss(self, self._render(model) - self._images_device())

    def as_batch(self):
        """This observation as the one-scene `LowResObservationBatch` that `BlendBatch.from_observations` takes (the
        difference kernels live in the factor matrices: the batch gets none)."""
        from .batch import LowResObservationBatch
        return LowResObservationBatch(self._images_device()[None], band0=self._band_slice.start or 0, geometry=self,
                                      weights=self._batch_weights())
