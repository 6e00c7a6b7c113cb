"""Batched Blend.fit() on one GPU: S independent scenes of identical shape.

This is the new, batched entry point the reference lacks (it fits one scene at a time in
Python).  `scarlet_amd.Blend` (single scene, reference API) is a thin view on a batch
of size 1.  State lives in PyTorch-ROCm tensors; all arithmetic is in the C-ABI HIP
library (`scarlet_amd/_lib.py`).  No CPU fallback.
"""
import ctypes

import numpy as np

from . import _lib
from . import prior as _prior


def default_centroid_weight():
    """Centroid weight used when the model frame has no PSF (reference source.py:483-490):
    41x41 integrated Gaussian, sigma=0.9, scaled to peak 1, float64."""
    from .psf import generate_psf_image, gaussian
    psf = generate_psf_image(gaussian, (41, 41), amplitude=1, sigma=.9, normalize=False).image
    return psf / psf.max()


def pad_centers(centers, K=None):
    """Ragged centre lists -> one padded array and the counts (no device needed).

    centers : list of S arrays of shape (n_s, 2), the integer pixel centres (y, x) of scene s's sources
    K : components per scene of the padded array; default max(n_s)
    Returns ((S, K, 2) int32 with zeros in the absent rows, (S,) int32 counts n_s)."""
    rows = [np.asarray(c, dtype=np.int64).reshape(-1, 2) if np.size(c) else np.zeros((0, 2), np.int64) for c in centers]
    if not rows:
        raise ValueError("pad_centers: no scenes")
    counts = np.array([len(r) for r in rows], dtype=np.int32)
    if (counts < 1).any():
        raise ValueError("pad_centers: scene %d has no sources" % int(np.argmin(counts)))
    K = int(counts.max()) if K is None else int(K)
    if K > _lib.MAX_COMPONENTS:
        raise ValueError("pad_centers: %d components per scene, at most %d are supported" % (K, _lib.MAX_COMPONENTS))
    if (counts > K).any():
        s = int(np.argmax(counts > K))
        raise ValueError("pad_centers: scene %d has %d sources, more than K = %d" % (s, counts[s], K))
    out = np.zeros((len(rows), K, 2), dtype=np.int32)
    for s, r in enumerate(rows):
        out[s, :len(r)] = r
    return out, counts


def pad_frames(images, fill=0):
    """Scenes of different frame sizes -> one padded block and the shapes (no device needed).

    images : list of S arrays of shape (B, h_s, w_s): every scene has its own height and width, all have B bands
    fill : value of the padding (the batch never reads it as data: its weights are zero there)
    Returns ((S, B, H, W) float32 with scene s in the top-left corner of its planes, where H = max h_s and W = max w_s
    rounded up to a multiple of 4 (the 16-byte paths of the kernels), and the (S, 2) int32 shapes (h_s, w_s))."""
    arrs = [np.asarray(a.detach().cpu() if hasattr(a, "detach") else a) for a in images]
    if not arrs:
        raise ValueError("pad_frames: no scenes")
    for s, a in enumerate(arrs):
        if a.ndim != 3 or min(a.shape) < 1:
            raise ValueError("pad_frames: scene %d must be (B, h, w) with every side >= 1, not %s" % (s, a.shape))
        if a.shape[0] != arrs[0].shape[0]:
            raise ValueError("pad_frames: scene %d has %d bands, scene 0 has %d" % (s, a.shape[0], arrs[0].shape[0]))
    shapes = np.array([a.shape[1:] for a in arrs], dtype=np.int32)
    H, W = int(shapes[:, 0].max()), -(-int(shapes[:, 1].max()) // 4) * 4
    out = np.full((len(arrs), arrs[0].shape[0], H, W), fill, dtype=np.float32)
    for s, a in enumerate(arrs):
        out[s, :, :a.shape[1], :a.shape[2]] = a
    return out, shapes


def _is_frame_list(images):
    """True for a list of per-scene (B, h_s, w_s) arrays (not one (S, B, H, W) block, nested lists included)."""
    return isinstance(images, (list, tuple)) and len(images) > 0 and all(np.ndim(a) == 3 for a in images)


def ragged_frame_inputs(images, centers, frame_shapes, weights, group, n_components):
    """The host-side checks and padding of a ragged-frame batch (no device needed): what BlendBatch does with `images`
    given as a list, or as a padded block with `frame_shapes`.  Returns (images block, (S, 2) int32 shapes, weights as None /
    scalar / (S, B, H, W) block, centres, n_components); ValueError for bad input, NotImplementedError for `group`."""
    if group is not None:
        raise NotImplementedError("a ragged-frame batch (frame_shapes / a list of images) does not take group=")
    if images is None:
        raise NotImplementedError("from_observations does not take frame_shapes")
    images, shapes, weights = ragged_frame_block(images, frame_shapes, weights)
    centers, n_components = ragged_frame_centers(centers, shapes, n_components)
    return images, shapes, weights, centers, n_components


def ragged_frame_block(images, frame_shapes, weights):
    """The image side of `ragged_frame_inputs`, which an `ObservationBatch` with frame shapes shares (no device needed):
    (images block, (S, 2) int32 shapes, weights as None / scalar / (S, B, H, W) block); ValueError for bad input."""
    if _is_frame_list(images):
        if frame_shapes is not None:
            raise ValueError("frame_shapes comes with a padded (S, B, H, W) block; a list of images carries its own shapes")
        images, shapes = pad_frames(images)
    else:
        if isinstance(images, (list, tuple)):
            images = np.asarray(images)
        if np.ndim(images) != 4:
            raise ValueError("images must be (S, B, H, W) or a list of (B, h, w) arrays")
        shapes = np.asarray(frame_shapes.cpu() if hasattr(frame_shapes, "cpu") else frame_shapes)
        if shapes.shape != (np.shape(images)[0], 2) or not np.issubdtype(shapes.dtype, np.integer):
            raise ValueError("frame_shapes must be (S, 2) = (%d, 2) integers (h, w)" % np.shape(images)[0])
        shapes = shapes.astype(np.int32)
    S, B, H, W = (int(v) for v in np.shape(images))
    bad = (shapes[:, 0] < 1) | (shapes[:, 0] > H) | (shapes[:, 1] < 1) | (shapes[:, 1] > W)
    if bad.any():
        s = int(np.argmax(bad))
        raise ValueError("frame_shapes[%d] = %s lies outside 1..%d x 1..%d" % (s, tuple(int(v) for v in shapes[s]), H, W))
    if isinstance(weights, (list, tuple)) and _is_frame_list(weights):
        if len(weights) != S:
            raise ValueError("weights: %d per-scene arrays for S = %d scenes" % (len(weights), S))
        for s, w in enumerate(weights):
            if tuple(np.shape(w)) != (B, int(shapes[s, 0]), int(shapes[s, 1])):
                raise ValueError("weights[%d] must be %s, not %s" % (s, (B, int(shapes[s, 0]), int(shapes[s, 1])), tuple(np.shape(w))))
        weights = pad_frames(weights)[0]
    return images, shapes, weights


def ragged_frame_centers(centers, shapes, n_components):
    """The centre side of `ragged_frame_inputs`: the centres of the present components lie inside their scene's own frame
    (ValueError otherwise).  Returns (centres, n_components), padded from ragged lists where they were given."""
    S = len(shapes)
    if isinstance(centers, (list, tuple)) and len(centers) and np.ndim(centers[0]) == 2 and \
            len(set(np.shape(c)[0] for c in centers)) > 1:
        centers, counts = pad_centers(centers)
        if n_components is not None and not np.array_equal(np.asarray(n_components).reshape(-1), counts):
            raise ValueError("n_components does not match the lengths of the centre lists")
        n_components = counts
    c = np.asarray(centers.cpu() if hasattr(centers, "cpu") else centers)
    if c.ndim != 3 or c.shape[0] != S or c.shape[2] != 2:
        raise ValueError("centers must be (S, K, 2) or a list of S (n_s, 2) arrays")
    out = (c[..., 0] < 0) | (c[..., 0] >= shapes[:, None, 0]) | (c[..., 1] < 0) | (c[..., 1] >= shapes[:, None, 1])
    if n_components is not None:
        n = np.asarray(n_components.cpu() if hasattr(n_components, "cpu") else n_components).reshape(-1)
        if n.shape == (S,):
            out &= np.arange(c.shape[1])[None, :] < n[:, None]
    if out.any():
        s, k = [int(v[0]) for v in np.nonzero(out)]
        raise ValueError("centre %s of scene %d, source %d lies outside the scene's %d x %d frame"
                         % (tuple(int(v) for v in c[s, k]), s, k, shapes[s, 0], shapes[s, 1]))
    return centers, n_components


_SWITCHES, _THRESHOLDS = ("symmetric", "monotonic"), ("l0_thresh", "l1_thresh")


def is_scalar_setting(value):
    """True for what BlendBatch has always taken for a constraint setting: None, a bool or a number."""
    if value is None or isinstance(value, (bool, int, float, np.generic)):
        return True
    return hasattr(value, "ndim") and value.ndim == 0        # 0-d array / tensor


def constraint_arrays(value, S, K, kind, group=None):
    """One constraint setting of a batch as an (S, K) host array, one entry per component (no device needed).

    value : a scalar (every component), a (K,) sequence (one row for all scenes), an (S, K) array, or a list of S
        per-scene lists of at most K entries each (ragged batches, padded like `pad_centers` pads the centres: the
        entries of absent components are "off" and never read)
    kind : "symmetric" / "monotonic" -> uint8 0 / 1;  "l0_thresh" / "l1_thresh" -> float32, where None or a negative
        number means off and is stored as -1
    group : None or (S, K) integers as BlendBatch takes them: the members of one multi-component source (equal
        group >= 0) must agree on a switch (ValueError otherwise); thresholds may differ between layers
    A wrong shape raises ValueError."""
    if kind not in _SWITCHES + _THRESHOLDS:
        raise ValueError("constraint_arrays: unknown kind %r" % (kind,))
    switch = kind in _SWITCHES
    S, K = int(S), int(K)

    def entry(v):
        if switch:
            if v is None:
                raise ValueError("%s: None is not a switch value" % kind)
            return 1 if bool(v) else 0
        if v is None:
            return -1.0
        v = float(v)
        if v != v:
            raise ValueError("%s: NaN is not a threshold" % kind)
        return -1.0 if v < 0 else v

    dtype, off = (np.uint8, 0) if switch else (np.float32, -1.0)
    out = np.full((S, K), off, dtype=dtype)
    if hasattr(value, "detach"):                       # a torch tensor
        value = value.detach().cpu().numpy()
    if is_scalar_setting(value):
        out[:] = entry(value if not hasattr(value, "ndim") else value.item())
    else:
        seq = list(value)
        rows = [hasattr(r, "__len__") and not isinstance(r, (str, bytes)) for r in seq]
        if any(rows):
            if not all(rows):
                raise ValueError("%s: a mix of per-scene rows and single entries" % kind)
            if len(seq) != S:
                raise ValueError("%s: %d per-scene rows for S = %d scenes" % (kind, len(seq), S))
            for s_, r in enumerate(seq):
                r = list(r)
                if len(r) > K:
                    raise ValueError("%s: scene %d has %d entries, more than K = %d" % (kind, s_, len(r), K))
                if any(hasattr(v, "__len__") for v in r):
                    raise ValueError("%s must be a scalar, (K,) = (%d,), (S, K) = (%d, %d) or S per-scene lists" % (kind, K, S, K))
                out[s_, :len(r)] = [entry(v) for v in r]
        else:
            if len(seq) != K:
                raise ValueError("%s: %d entries for K = %d components per scene" % (kind, len(seq), K))
            out[:] = np.array([entry(v) for v in seq], dtype=dtype)[None, :]
    if switch and group is not None:
        g = np.asarray(group).reshape(S, K)
        same = (g[:, 1:] == g[:, :-1]) & (g[:, 1:] >= 0)          # (members are adjacent components)
        bad = same & (out[:, 1:] != out[:, :-1])
        if bad.any():
            s_, k = [int(v[0]) for v in np.nonzero(bad)]
            raise ValueError("%s: components %d and %d of scene %d are layers of one multi-component source (group %d) "
                             "and must agree" % (kind, k, k + 1, s_, int(g[s_, k])))
    return out


_SYMMETRY_NAMES = {"kspace": _lib.SYM_KSPACE, "soft": _lib.SYM_SOFT, "sdss": _lib.SYM_SDSS}
_POSITIVE_NAMES = {"both": _lib.POSITIVE_SED | _lib.POSITIVE_MORPH, "sed": _lib.POSITIVE_SED, "morph": _lib.POSITIVE_MORPH,
                   "none": 0}
_NORMALIZATION_NAMES = {"morph_max": _lib.NORM_MORPH_MAX, "morph": _lib.NORM_MORPH, "sed": _lib.NORM_SED, "none": _lib.NORM_NONE}


def _setting_array(value, S, K, name, entry, dtype, default):
    """`value` as an (S, K) host array with the broadcasting of `constraint_arrays`: one value, a (K,) sequence, an (S, K)
    array or S per-scene lists of at most K entries (the rest keeps `default`).  `entry` maps one item to its stored value
    and raises ValueError for a bad one."""
    out = np.full((S, K), default, dtype=dtype)
    if hasattr(value, "detach"):
        value = value.detach().cpu().numpy()
    if isinstance(value, (str, bytes)) or is_scalar_setting(value):
        out[:] = entry(value.item() if hasattr(value, "ndim") else value)
        return out
    seq = list(value)
    rows = [hasattr(r, "__len__") and not isinstance(r, (str, bytes)) for r in seq]
    if any(rows):
        if not all(rows):
            raise ValueError("%s: a mix of per-scene rows and single entries" % name)
        if len(seq) != S:
            raise ValueError("%s: %d per-scene rows for S = %d scenes" % (name, len(seq), S))
        for s_, r in enumerate(seq):
            r = list(r)
            if len(r) > K:
                raise ValueError("%s: scene %d has %d entries, more than K = %d" % (name, s_, len(r), K))
            if any(hasattr(v, "__len__") and not isinstance(v, (str, bytes)) for v in r):
                raise ValueError("%s must be one value, (K,) = (%d,), (S, K) = (%d, %d) or S per-scene lists" % (name, K, S, K))
            out[s_, :len(r)] = [entry(v) for v in r]
    else:
        if len(seq) != K:
            raise ValueError("%s: %d entries for K = %d components per scene" % (name, len(seq), K))
        out[:] = np.array([entry(v) for v in seq], dtype=dtype)[None, :]
    return out


class UpdateOptions(object):
    """The options of the reference's stock update functions for the components of a batch: what a user who overrides
    PointSource / ExtendedSource.update (source.py:402-440) to call them with other arguments passes as
    `BlendBatch(..., update=UpdateOptions(...))`.  The pipeline's order stays the reference's.

    symmetry : "kspace" (default) | "soft" | "sdss" -- update.symmetric(algorithm=)
    strength : soft symmetry's strength in [0, 1], default 0.5 (update.py:170)
    use_nearest : update.monotonic(use_nearest=): the nearest-neighbour sweep instead of the weighted one
    monotonic_thresh : update.monotonic(thresh=) in [0, 1); must be 0 with use_nearest (the reference raises ValueError)
    positive : "both" (update.positive) | "sed" (positive_sed) | "morph" (positive_morph) | "none"
    normalization : "morph_max" (default) | "morph" | "sed" -- update.normalized(type=) -- | "none"

    Each is one value for the batch or one per component, broadcast like the constraint switches (`constraint_arrays`): a
    (K,) sequence, an (S, K) array, or S per-scene lists for ragged counts.  Names may be given as the library's integers.
    `arrays(S, K)` checks everything on the host (ValueError) and needs no device."""

    FIELDS = ("sym_algorithm", "sym_strength", "mono_nearest", "mono_thresh", "positive", "normalize")

    def __init__(self, symmetry="kspace", strength=0.5, use_nearest=False, monotonic_thresh=0, positive="both",
                 normalization="morph_max"):
        self.symmetry, self.strength, self.use_nearest = symmetry, strength, use_nearest
        self.monotonic_thresh, self.positive, self.normalization = monotonic_thresh, positive, normalization

    def arrays(self, S, K):
        """{member of scarlet_update_options: (S, K) host array}; ValueError for an unknown name, a number out of range or
        use_nearest with a thresh."""
        S, K = int(S), int(K)

        def named(table, what):
            def entry(v):
                if isinstance(v, bytes):
                    v = v.decode()
                if isinstance(v, str):
                    if v.lower() not in table:
                        raise ValueError("%s: unknown value %r (one of %s)" % (what, v, ", ".join(sorted(table))))
                    return table[v.lower()]
                if isinstance(v, (bool, float)) or v is None or int(v) not in table.values():
                    raise ValueError("%s: unknown value %r (one of %s)" % (what, v, ", ".join(sorted(table))))
                return int(v)
            return entry

        def number(what, lo, hi, closed):
            def entry(v):
                if v is None or isinstance(v, (str, bytes)):
                    raise ValueError("%s: %r is not a number" % (what, v))
                v = float(v)
                if not (lo <= v <= hi if closed else lo <= v < hi):
                    raise ValueError("%s = %r lies outside [%g, %g%s" % (what, v, lo, hi, "]" if closed else ")"))
                return v
            return entry

        def switch(v):
            if v is None or isinstance(v, (str, bytes)):
                raise ValueError("use_nearest: %r is not a switch value" % (v,))
            return 1 if bool(v) else 0

        out = {
            "sym_algorithm": _setting_array(self.symmetry, S, K, "symmetry", named(_SYMMETRY_NAMES, "symmetry"), np.uint8,
                                            _lib.SYM_KSPACE),
            "sym_strength": _setting_array(self.strength, S, K, "strength", number("strength", 0.0, 1.0, True), np.float32, 0.5),
            "mono_nearest": _setting_array(self.use_nearest, S, K, "use_nearest", switch, np.uint8, 0),
            "mono_thresh": _setting_array(self.monotonic_thresh, S, K, "monotonic_thresh",
                                          number("monotonic_thresh", 0.0, 1.0, False), np.float32, 0.0),
            "positive": _setting_array(self.positive, S, K, "positive", named(_POSITIVE_NAMES, "positive"), np.uint8,
                                       _POSITIVE_NAMES["both"]),
            "normalize": _setting_array(self.normalization, S, K, "normalization", named(_NORMALIZATION_NAMES, "normalization"),
                                        np.uint8, _lib.NORM_MORPH_MAX),
        }
        bad = (out["mono_nearest"] != 0) & (out["mono_thresh"] != 0)
        if bad.any():
            s, k = [int(v[0]) for v in np.nonzero(bad)]
            raise ValueError("use_nearest with monotonic_thresh = %g (scene %d, component %d): Thresholding does not work with "
                             "nearest neighbor monotonicity" % (float(out["mono_thresh"][s, k]), s, k))
        return out


def _check_obs_psfs(psfs, S, B, name, shapes="(B, P, P) or (S, B, P, P)"):
    """The observed PSFs are one set for every scene or one per scene."""
    if np.ndim(psfs) not in (3, 4) or tuple(np.shape(psfs)[:-2]) not in ((B,), (S, B)):
        raise ValueError("%s must be %s, not %s" % (name, shapes, tuple(np.shape(psfs))))


def _check_model_psf(psf, name):
    """The model PSF is one square image with a centre pixel."""
    shape = tuple(np.shape(psf))
    if len(shape) != 2 or shape[0] != shape[1] or shape[0] % 2 != 1:
        raise ValueError("%s must be (P, P) with P odd, not %s" % (name, shape))


class ObservationBatch(object):
    """One observation of S scenes for `BlendBatch.from_observations` (reference Observation, observation.py:101-224,
    as one element of Blend(sources, [obs_a, obs_b])): the images cover the model channels band0 .. band0 + B - 1.

    images : (S, B, H, W) array or tensor
    band0 : first model channel of the observation; observations may overlap in channels (several epochs of the same
        bands)
    weights : None (scalar 1), a Python scalar, or (S, B, H, W)
    frame_shapes : None (every scene is H x W), or (S, 2) integers (h_s, w_s): the images are the padded block of scenes
        with their own frame sizes, as `BlendBatch(frame_shapes=...)` takes them (`from_frames` pads a list).  The joint
        fit then runs every scene on its own frame; every same-grid observation of a batch must carry the same shapes.
        `weights` may then also be a list of per-scene (B, h_s, w_s) arrays.  Checked on the host (ValueError).
    """

    def __init__(self, images, band0=0, weights=None, frame_shapes=None):
        self.frame_shapes = None
        if frame_shapes is not None:
            if _is_frame_list(images):
                raise ValueError("ObservationBatch: frame_shapes comes with a padded (S, B, H, W) block; "
                                 "ObservationBatch.from_frames takes a list of images")
            images, self.frame_shapes, weights = ragged_frame_block(images, frame_shapes, weights)
        if np.ndim(images) != 4:
            raise ValueError("ObservationBatch: images must be (S, B, H, W), not %s" % (tuple(np.shape(images)),))
        self.images = images
        self.shape = tuple(int(v) for v in np.shape(images))
        self.band0 = int(band0)
        if self.band0 < 0:
            raise ValueError("ObservationBatch: band0 must be >= 0, not %d" % self.band0)
        if weights is not None and np.ndim(weights) != 0 and tuple(np.shape(weights)) != self.shape:
            raise ValueError("ObservationBatch: weights must be a scalar or %s, not %s" % (self.shape, tuple(np.shape(weights))))
        self.weights = weights
        self.diff_kernel = None

    @classmethod
    def from_frames(cls, images, band0=0, weights=None):
        """The observation of S scenes with their own frame sizes: `images` is a list of (B, h_s, w_s) arrays, padded by
        `pad_frames` (H = max h_s, W = max w_s rounded up to a multiple of 4); `weights` a scalar or a list of per-scene
        (B, h_s, w_s) arrays.  Two observations of one batch need one block size: lists of different maximum sizes are
        padded by the caller (`ObservationBatch(block, frame_shapes=...)`)."""
        if cls is not ObservationBatch:
            raise NotImplementedError("%s.from_frames: only same-grid observations take ragged frames" % cls.__name__)
        if not _is_frame_list(images):
            raise ValueError("ObservationBatch.from_frames: images must be a list of (B, h, w) arrays")
        block, shapes = pad_frames(images)
        return cls(block, band0=band0, weights=weights, frame_shapes=shapes)

    @property
    def B(self):
        return self.shape[1]

    def set_diff_kernel(self, kernel):
        """PSF difference kernel of this observation (Observation.match): (B, P, P) shared by all scenes or
        (S, B, P, P) one set per scene, as BlendBatch.set_diff_kernel."""
        S, B = self.shape[:2]
        if tuple(np.shape(kernel)[:-2]) not in ((B,), (S, B)) or np.ndim(kernel) not in (3, 4):
            raise ValueError("ObservationBatch: the kernel must be (B, P, P) or (S, B, P, P), not %s"
                             % (tuple(np.shape(kernel)),))
        self.diff_kernel = kernel
        return self


class LowResObservationBatch(ObservationBatch):
    """One LOW-RESOLUTION observation of S scenes for `BlendBatch.from_observations` (reference LowResObservation as one
    element of Blend(sources, [obs_hr, obs_lr])): images on a coarser pixel grid than the model frame, with their own
    PSFs, covering the model channels band0 .. band0 + B - 1.

    images : (S, B, h, w) array or tensor
    geometry : a `LowResObservation` matched to the model frame -- one for every scene -- or a list of S of them (scenes
        cut at different sub-pixel phases or observed with different PSFs; they must share the model frame, its PSF and
        the observation's shape).  Only its geometry is read (factor matrices, band count), not its images.
    weights : None (scalar 1), a Python scalar, or (S, B, h, w)

    frame_shapes : None, or (S, 2) integers (h_s, w_s): the images are the padded block of scenes whose observations have
        their own sizes (`from_frames(images, geometry=[...])` pads a list), beside same-grid observations that carry the
        scenes' model frames.  `geometry` is then a list of S `LowResObservation`s, each matched to its own scene's model
        frame (C, H_s, W_s) -- the reference builds the operator from the scene's own frame, so a geometry matched to the
        padded frame would fit another scene.  The batch keeps `model_shapes` (S, 2) = (H_s, W_s) read from the
        geometries, `dims` (S, 6) = (H_s, W_s, h_s, w_s, nfy_s, nfx_s), and every scene's five factor matrices
        zero-padded to the per-dimension maxima (exact: the padding only adds products with 0).  `weights` may also be a
        list of per-scene (B, h_s, w_s) arrays.  The geometries must share the model PSF and the band count.

    Every pixel of the observation must lie inside the model frame (ValueError otherwise); a geometry that was not
    matched raises ValueError too."""

    def __init__(self, images, band0=0, geometry=None, weights=None, frame_shapes=None):
        if frame_shapes is not None and _is_frame_list(images):
            raise ValueError("LowResObservationBatch: frame_shapes comes with a padded (S, B, h, w) block; "
                             "LowResObservationBatch.from_frames takes a list of images")
        ObservationBatch.__init__(self, images, band0=band0, weights=weights, frame_shapes=frame_shapes)
        S, B, h, w = self.shape
        geoms = list(geometry) if isinstance(geometry, (list, tuple)) else [geometry]
        if isinstance(geometry, (list, tuple)) and len(geoms) != S:
            raise ValueError("LowResObservationBatch: %d geometries for S = %d scenes" % (len(geoms), S))
        if frame_shapes is not None and not isinstance(geometry, (list, tuple)):
            raise ValueError("LowResObservationBatch: frame_shapes needs a list of S geometries, each matched to its own "
                             "scene's model frame")
        for g in geoms:
            if not hasattr(g, "factors_f32") or getattr(g, "model_shape", None) is None:
                raise ValueError("LowResObservationBatch: geometry must be a LowResObservation after match(model_frame)")
            if not g.covers:
                raise ValueError("LowResObservationBatch: only %s of the observation's %s pixels lie inside the model frame; "
                                 "every low-resolution pixel must" % (g.lr_shape, tuple(g.frame.shape[1:])))
        self.per_scene = isinstance(geometry, (list, tuple))
        self.geometries = geoms
        self.model_shape = tuple(geoms[0].model_shape)
        self.model_shapes = self.dims = None
        if frame_shapes is not None:
            self._pack_frames()
            return
        f0 = geoms[0].factors_f32()
        if f0["dhat"].shape[0] != B or (f0["vy"].shape[0], f0["vx"].shape[0]) != (h, w):
            raise ValueError("LowResObservationBatch: images are %s, the geometry describes %s"
                             % (self.shape[1:], (f0["dhat"].shape[0], f0["vy"].shape[0], f0["vx"].shape[0])))
        fs = [f0] + [g.factors_f32() for g in geoms[1:]]
        for f in fs[1:]:
            if tuple(g.model_shape) != self.model_shape or any(f[k].shape != f0[k].shape for k in f0) or \
                    not (np.array_equal(f["uy"], f0["uy"]) and np.array_equal(f["ux"], f0["ux"])):
                raise ValueError("LowResObservationBatch: the scenes' geometries must share the model frame, its PSF and "
                                 "the observation's shape")
        self.host_factors = dict(uy=f0["uy"], ux=f0["ux"])
        for k in ("vy", "vx", "dhat"):
            self.host_factors[k] = np.stack([f[k] for f in fs]) if self.per_scene else f0[k]

    def _pack_frames(self):
        """The per-scene tables of scenes with their own frames: `model_shapes`, `dims` and the zero-padded factors."""
        S, B, h, w = self.shape
        fs = [g.factors_f32() for g in self.geometries]
        for s, (g, f) in enumerate(zip(self.geometries, fs)):
            own = (f["dhat"].shape[0], f["vy"].shape[0], f["vx"].shape[0])
            want = (B, int(self.frame_shapes[s, 0]), int(self.frame_shapes[s, 1]))
            if own != want:
                raise ValueError("LowResObservationBatch: scene %d's images are %s, its geometry describes %s" % (s, want, own))
            if own[0] != fs[0]["dhat"].shape[0]:
                raise ValueError("LowResObservationBatch: the scenes' geometries must share the band count")
            if not np.array_equal(g.model_psf, self.geometries[0].model_psf):
                raise ValueError("LowResObservationBatch: scene %d's geometry was matched with another model PSF than scene "
                                 "0's; the scenes' geometries must share the model PSF" % s)
        self.model_shapes = np.array([g.model_shape for g in self.geometries], dtype=np.int32)
        self.dims = np.array([tuple(g.model_shape) + (f["vy"].shape[0], f["vx"].shape[0], f["uy"].shape[0], f["ux"].shape[0])
                              for g, f in zip(self.geometries, fs)], dtype=np.int32)
        self.model_shape = (int(self.dims[:, 0].max()), int(self.dims[:, 1].max()))
        H, W = self.model_shape
        nfy, nfx = int(self.dims[:, 4].max()), int(self.dims[:, 5].max())
        shapes = dict(uy=(nfy, H), ux=(nfx, W), vy=(h, nfy), vx=(w, nfx), dhat=(B, nfy, nfx))
        self.host_factors = {}
        for k, shape in shapes.items():
            out = np.zeros((S,) + shape + (2,), np.float32)
            for s, f in enumerate(fs):
                out[(s,) + tuple(slice(0, n) for n in f[k].shape)] = f[k]
            self.host_factors[k] = out

    @classmethod
    def from_frames(cls, images, band0=0, weights=None, geometry=None):
        """The low-resolution observation of S scenes with their own sizes: `images` is a list of (B, h_s, w_s) arrays,
        padded by `pad_frames`; `geometry` a list of S `LowResObservation`s, each matched to its own scene's model frame
        (C, H_s, W_s); `weights` a scalar or a list of per-scene (B, h_s, w_s) arrays.  The padded-block spelling is
        `LowResObservationBatch(block, band0, geometry=[...], weights=..., frame_shapes=...)`.  Without `geometry` there
        is nothing to build the scenes' operators from: NotImplementedError."""
        if geometry is None:
            raise NotImplementedError("%s.from_frames: only same-grid observations take ragged frames without geometry= "
                                      "(a list of per-scene LowResObservations)" % cls.__name__)
        if not _is_frame_list(images):
            raise ValueError("LowResObservationBatch.from_frames: images must be a list of (B, h, w) arrays")
        block, shapes = pad_frames(images)
        return cls(block, band0=band0, geometry=geometry, weights=weights, frame_shapes=shapes)

    def pixels_of(self, centers):
        """(..., 2) model-frame centres (torch, integer) -> the observation's pixels under them, truncated as
        Frame.get_pixel does; scene s uses its own geometry."""
        import torch
        t = centers.to(dtype=torch.float64)
        S = self.shape[0]
        geoms = self.geometries if self.per_scene else self.geometries * S
        org = t.new_tensor([g.origin for g in geoms]).view(S, 1, 2)
        stp = t.new_tensor([g.step for g in geoms]).view(S, 1, 2)
        return ((t - org) / stp).trunc().to(dtype=centers.dtype)

    def lowres_struct(self, device, model_block=None):
        """(struct scarlet_lowres without a workspace, the device tensors it points to).  With frame shapes: the struct
        holds the maxima, uy / ux are the per-scene tables padded on to the (H, W) of `model_block` -- the state's padded
        planes -- and the tensors include `dims` and the struct scarlet_lowres_frames ("frames") that points to them."""
        from .observation import lowres_struct
        if self.dims is None:
            return lowres_struct(self.host_factors, self.shape[2], self.shape[3], self.shape[1], self.per_scene, device)
        f = dict(self.host_factors)
        H, W = self.model_shape if model_block is None else (int(v) for v in model_block)
        for k, n in (("uy", H), ("ux", W)):
            if f[k].shape[2] != n:
                out = np.zeros(f[k].shape[:2] + (n, 2), np.float32)
                out[:, :, :f[k].shape[2]] = f[k]
                f[k] = out
        lr, keep = lowres_struct(f, self.shape[2], self.shape[3], self.shape[1], True, device)
        lr.nfy, lr.nfx = f["uy"].shape[1], f["ux"].shape[1]
        keep["dims"] = _lib.require_gpu().as_tensor(self.dims).to(device).contiguous()
        lf = _lib.ScarletLowresFrames()
        lf.dims, lf.uy, lf.ux = keep["dims"].data_ptr(), keep["uy"].data_ptr(), keep["ux"].data_ptr()
        keep["frames"] = lf
        return lr, keep


_SOURCE_KINDS = ("extended", "point", "multi")


class SourceSpec(object):
    """One source of a catalogue for `BlendBatch.from_catalog`: a small host object.

    center : (y, x) integer pixel centre in the scene's own coordinates
    kind : "extended" (ExtendedSource, the default) | "point" (PointSource) | "multi" (MultiComponentSource)
    flux_percentiles : multi only: the n boundaries between its n + 1 layers, ascending inside (0, 100); default [25]
    symmetric, monotonic, l0_thresh, l1_thresh : as the reference's sources carry them; the layers of a multi source
        share them by construction
    symmetry, strength, use_nearest, monotonic_thresh, positive, normalization : the stock update functions' options of
        this source, with the values `UpdateOptions` takes; None (the default) = the batch's default
        (`from_catalog(update=)`, else the stock pipeline's).  The layers of a multi source share them."""
    OPTION_FIELDS = ("symmetry", "strength", "use_nearest", "monotonic_thresh", "positive", "normalization")
    __slots__ = ("center", "kind", "flux_percentiles", "symmetric", "monotonic", "l0_thresh", "l1_thresh") + OPTION_FIELDS

    def __init__(self, center, kind="extended", flux_percentiles=None, symmetric=True, monotonic=True, l0_thresh=None,
                 l1_thresh=None, symmetry=None, strength=None, use_nearest=None, monotonic_thresh=None, positive=None,
                 normalization=None):
        self.center, self.kind, self.flux_percentiles = center, kind, flux_percentiles
        self.symmetric, self.monotonic, self.l0_thresh, self.l1_thresh = symmetric, monotonic, l0_thresh, l1_thresh
        self.symmetry, self.strength, self.use_nearest = symmetry, strength, use_nearest
        self.monotonic_thresh, self.positive, self.normalization = monotonic_thresh, positive, normalization

    def has_options(self):
        """True when the source sets one of the update options itself."""
        return any(getattr(self, name) is not None for name in self.OPTION_FIELDS)

    def layers(self, where="source"):
        """Number of components the source expands to; ValueError (naming `where`) for an unknown kind, percentiles on a
        source that is not multi, percentiles not ascending inside (0, 100) or more than MAX_LAYERS layers."""
        if self.kind not in _SOURCE_KINDS:
            raise ValueError("%s: unknown source kind %r (one of %s)" % (where, self.kind, ", ".join(_SOURCE_KINDS)))
        if self.kind != "multi":
            if self.flux_percentiles is not None:
                raise ValueError("%s: flux_percentiles belong to a multi source, not to kind %r" % (where, self.kind))
            return 1
        p = np.asarray([25] if self.flux_percentiles is None else self.flux_percentiles, dtype=np.float64).reshape(-1)
        if p.size < 1 or not (np.all(p > 0) and np.all(p < 100) and np.all(np.diff(p) > 0)):
            raise ValueError("%s: flux_percentiles %s must be ascending inside (0, 100)" % (where, p.tolist()))
        if p.size + 1 > _lib.MAX_LAYERS:
            raise ValueError("%s: %d flux_percentiles give %d layers, at most %d (SCARLET_MAX_LAYERS) are supported"
                             % (where, p.size, p.size + 1, _lib.MAX_LAYERS))
        return int(p.size) + 1


def catalog_arrays(shapes, catalog):
    """A catalogue -- one list of `SourceSpec`s per scene, lengths differ -- as the arrays a batch holds (no device needed).

    shapes : (S, 2) integers, every scene's own frame (h_s, w_s)
    Returns a dict: `centers` (S, K, 2) int32 padded to K = the largest number of components of a scene, `n_components`
    (S,) int32, `group` (S, K) int32 (a fresh id per multi source of its scene, -1 elsewhere), `kind` (S, K) int32 of
    INIT_EXTENDED / INIT_POINT (the layers of a multi source read as extended; ignored by the library), `percentiles`
    (S, K) float32 (at layer j >= 1 of a multi source the boundary below it, 0 elsewhere), `symmetric`, `monotonic`
    (S, K) uint8 and `l0_thresh`, `l1_thresh` (S, K) float32 (-1 = off) as `constraint_arrays` stores them, and `sources`,
    per scene the list of (first component, layers) of its sources.  ValueError, naming scene and source, for an unknown
    kind, bad percentiles, too many layers, percentiles on a source that is not multi, a centre outside its own frame, an
    empty scene, or too many components."""
    shapes = np.asarray(shapes).reshape(-1, 2)
    S = len(shapes)
    if len(catalog) != S:
        raise ValueError("from_catalog: %d catalogues for %d scenes" % (len(catalog), S))
    rows, sources = [], []
    for s, specs in enumerate(catalog):
        specs = list(specs)
        if not specs:
            raise ValueError("from_catalog: scene %d has no sources" % s)
        comps, table = [], []
        for i, sp in enumerate(specs):
            where = "from_catalog: scene %d, source %d" % (s, i)
            if not isinstance(sp, SourceSpec):
                raise ValueError("%s is not a SourceSpec" % where)
            n = sp.layers(where)
            c = np.asarray(sp.center).reshape(-1)
            if c.size != 2 or not np.all(c == np.round(c)):
                raise ValueError("%s: the centre must be two integers (y, x), not %r" % (where, sp.center))
            y, x = int(c[0]), int(c[1])
            if not (0 <= y < shapes[s, 0] and 0 <= x < shapes[s, 1]):
                raise ValueError("%s: centre (%d, %d) lies outside the scene's own %d x %d frame" % (where, y, x, shapes[s, 0], shapes[s, 1]))
            perc = [0.0] if sp.kind != "multi" else [0.0] + [float(v) for v in ([25] if sp.flux_percentiles is None else sp.flux_percentiles)]
            for v in (sp.l0_thresh, sp.l1_thresh):
                if v is not None and float(v) != float(v):
                    raise ValueError("%s: NaN is not a threshold" % where)
            table.append((len(comps), n))
            for j in range(n):
                comps.append(dict(center=(y, x), group=i if sp.kind == "multi" else -1,
                                  kind=_lib.INIT_POINT if sp.kind == "point" else _lib.INIT_EXTENDED, perc=perc[j],
                                  symmetric=1 if sp.symmetric else 0, monotonic=1 if sp.monotonic else 0,
                                  l0_thresh=-1.0 if sp.l0_thresh is None or sp.l0_thresh < 0 else float(sp.l0_thresh),
                                  l1_thresh=-1.0 if sp.l1_thresh is None or sp.l1_thresh < 0 else float(sp.l1_thresh)))
        if len(comps) > _lib.MAX_COMPONENTS:
            raise ValueError("from_catalog: scene %d expands to %d components, at most %d are supported" % (s, len(comps), _lib.MAX_COMPONENTS))
        rows.append(comps)
        sources.append(table)
    K = max(len(r) for r in rows)
    out = dict(centers=np.zeros((S, K, 2), np.int32), n_components=np.array([len(r) for r in rows], np.int32),
               group=np.full((S, K), -1, np.int32), kind=np.full((S, K), _lib.INIT_EXTENDED, np.int32),
               percentiles=np.zeros((S, K), np.float32), symmetric=np.zeros((S, K), np.uint8),
               monotonic=np.zeros((S, K), np.uint8), l0_thresh=np.full((S, K), -1.0, np.float32),
               l1_thresh=np.full((S, K), -1.0, np.float32), sources=sources)
    for s, r in enumerate(rows):
        for k, comp in enumerate(r):
            out["centers"][s, k] = comp["center"]
            for name in ("group", "kind", "symmetric", "monotonic", "l0_thresh", "l1_thresh"):
                out[name][s, k] = comp[name]
            out["percentiles"][s, k] = comp["perc"]
    return out


def catalog_option_arrays(catalog, update=None):
    """The update options of a catalogue as the (S, K) tables of `UpdateOptions.arrays`, one row per component in the
    layout of `catalog_arrays` (no device needed), or None where nothing asks for options.

    update : None, or an `UpdateOptions` whose fields are single values: the default of every source.  A `SourceSpec`
        field that is not None overrides it; the layers of a multi source share their source's options.
    Returns None when `update` is None and no source sets an option -- such a catalogue takes the route of a catalogue
    without options -- else {member of scarlet_update_options: (S, K) host array}; rows of absent components hold the
    stock pipeline's values and are never read.  ValueError, naming scene and source, for an unknown name, a strength
    outside [0, 1], a thresh outside [0, 1) or use_nearest with a thresh; ValueError for an `update` with per-component
    arrays (they come from the catalogue)."""
    if update is not None:
        if not isinstance(update, UpdateOptions):
            raise ValueError("from_catalog: update must be an UpdateOptions (or None), not %r" % type(update).__name__)
        for name in SourceSpec.OPTION_FIELDS:
            v = getattr(update, name)
            if not (isinstance(v, (str, bytes)) or is_scalar_setting(v)):
                raise ValueError("from_catalog: update.%s per component comes from the catalogue (SourceSpec(%s=...)); "
                                 "update= takes single values, the batch's defaults" % (name, name))
    if update is None and not any(isinstance(sp, SourceSpec) and sp.has_options() for specs in catalog for sp in specs):
        return None
    base = UpdateOptions() if update is None else update
    rows = []
    for s, specs in enumerate(catalog):
        comps = []
        for i, sp in enumerate(specs):
            kw = {name: getattr(base, name) if getattr(sp, name) is None else getattr(sp, name)
                  for name in SourceSpec.OPTION_FIELDS}
            try:
                one = UpdateOptions(**kw).arrays(1, 1)
            except ValueError as e:
                raise ValueError("from_catalog: scene %d, source %d: %s" % (s, i, e))
            comps += [one] * sp.layers("from_catalog: scene %d, source %d" % (s, i))
        rows.append(comps)
    S, K = len(rows), max(len(r) for r in rows)
    out = UpdateOptions().arrays(S, K)
    for s, r in enumerate(rows):
        for k, one in enumerate(r):
            for name in UpdateOptions.FIELDS:
                out[name][s, k] = one[name][0, 0]
    return out


def catalog_frames(cutouts):
    """The cut-outs of `from_catalog` as (list of per-scene arrays or the block, (S, 2) int32 shapes, uniform) -- no device
    needed.  ValueError for scenes of differing B or a wrong shape."""
    if _is_frame_list(cutouts):
        arrs = list(cutouts)
        for s, a in enumerate(arrs):
            if min(np.shape(a)) < 1:
                raise ValueError("from_catalog: scene %d must be (B, h, w) with every side >= 1, not %s" % (s, tuple(np.shape(a))))
            if np.shape(a)[0] != np.shape(arrs[0])[0]:
                raise ValueError("from_catalog: scene %d has B = %d bands, scene 0 has %d" % (s, np.shape(a)[0], np.shape(arrs[0])[0]))
        shapes = np.array([np.shape(a)[1:] for a in arrs], dtype=np.int32)
        return arrs, shapes, bool((shapes == shapes[0]).all())
    if isinstance(cutouts, (list, tuple)):
        raise ValueError("from_catalog: the cut-outs must be a list of (B, h, w) arrays or one (S, B, H, W) block")
    if np.ndim(cutouts) != 4:
        raise ValueError("from_catalog: the cut-outs must be a list of (B, h, w) arrays or one (S, B, H, W) block")
    S, _, H, W = (int(v) for v in np.shape(cutouts))
    return cutouts, np.tile(np.array([[H, W]], np.int32), (S, 1)), True


class BatchProducts(object):
    """What `BlendBatch.products` returns: device tensors, None for what was not asked for.  For a batch made by
    `from_observations`, `rendered`, `residual` and `loss` are lists with one entry per observation.  `components`
    holds the indices (host int32 array) that `component_models` was made for."""
    __slots__ = ("model", "rendered", "residual", "loss", "flux", "component_models", "components")

    def __init__(self):
        for name in self.__slots__:
            setattr(self, name, None)


class BlendBatch(object):
    """S scenes x K components x B bands x H x W pixels, all float32 on one device.

    Parameters
    ----------
    images : (S, B, H, W) array or tensor; or a list of S arrays (B, h_s, w_s) -- scenes with their own frame sizes,
        padded by `pad_frames`; or the padded block together with `frame_shapes`
    centers : (S, K, 2) integer pixel centres (y, x) of the sources, or a list of S arrays (n_s, 2): the scenes then
        have different numbers of sources, padded to K = max n_s (`pad_centers`), and n_components is derived
    weights : None (scalar 1, reference observation.py:148-151), a Python scalar, or (S, B, H, W); for a ragged-frame
        batch also a list of per-scene (B, h_s, w_s) arrays
    symmetric, monotonic : constraint switches of PointSource/ExtendedSource.update
    l0_thresh, l1_thresh : None or sparsity thresholds (update.sparse_l0 / sparse_l1)
        Each of the four is one value for the batch, or one per component (`constraint_arrays`): a (K,) sequence, an
        (S, K) array, or per-scene lists for ragged batches -- as the reference's sources each carry their own
        symmetric= / monotonic=.  With any of them per component the batch is `constrained` (its scarlet_constraints
        then carries that setting's array); `symmetric` / `monotonic` then read "any component is", `l0_thresh` /
        `l1_thresh` None.  The layers of one `group` must agree on the switches.  Initialisation switches stay per batch:
        `init_monotonic=None` means "any component is monotonic", and the layers of a group start with the batch's
        `symmetric`; a per-component start option is out of scope.
    centroid_weight : (P, P) float64 centroid PSF; default = reference default
    group : None, or (S, K) integers: -1 = the component is a source of its own, g >= 0 = it is a layer of
        multi-component source g of its scene (reference MultiComponentSource, source.py:538-641): the layers
        of a source (adjacent components) share one centre measured on their flux-weighted sum
    n_components : None (every scene has K components), or (S,) counts: scene s uses components 0 .. n[s] - 1, the
        others are absent -- zero in both buffers, flags 0, outside the model, the constraints and the convergence test
    frame_shapes : None (every scene is H x W), or (S, 2) integers (h_s, w_s): scene s lies in the top-left corner of its
        padded planes and is fitted as the reference fits the (B, h_s, w_s) scene alone -- pixels outside do not exist
        for the constraints, stay exactly zero in the morphologies and carry zero weight (the batch materialises
        (S, B, H, W) weights with the frame mask multiplied in).  Centres are in the scene's own coordinates.  Such a
        batch takes no `group` and no prior; `init_sources` starts extended sources only (`from_catalog` makes the
        ragged-frame batch that holds point and multi-component sources as well).  A joint fit gets its frames
        from its observations (`ObservationBatch(frame_shapes=...)`), not from this keyword.
    update : None (the stock pipeline of source.py:402-440), or an `UpdateOptions`: each component's symmetry algorithm and
        strength, sweep (weighted with a thresh, or nearest neighbour), positivity and normalisation, on the device
        (scarlet_update_options).  Such a batch takes the general path, and no `group`, prior, ragged frames, `wide=True` or
        low-resolution observation (NotImplementedError).  A scene whose options were corrupted on the device gets
        STATUS_BAD_OPTION and is left untouched and inactive (`raise_on_status` names it).
    """

    def __init__(self, images, centers, weights=None, symmetric=True, monotonic=True,
                 l0_thresh=None, l1_thresh=None, centroid_weight=None, mse_capacity=256,
                 device=None, group=None, n_components=None, _frame=None, _morph=True, frame_shapes=None,
                 _frames=None, update=None, _grouped_frames=False):
        frames = _frames             # (from_observations: the checked shapes of its observations, for the state)
        # (_grouped_frames: from_catalog -- a ragged-frame batch with group=, through the library's _grouped entry points)
        if update is not None:       # host-side refusals first: they need no device
            if not isinstance(update, UpdateOptions):
                raise ValueError("update must be an UpdateOptions (or None), not %r" % type(update).__name__)
            if group is not None:
                raise NotImplementedError("a batch with update= (UpdateOptions) does not take group=: the layers of a "
                                          "multi-component source are tied to soft symmetry")
            if frames is not None or frame_shapes is not None or _is_frame_list(images):
                raise NotImplementedError("a batch with update= (UpdateOptions) does not take frame_shapes / a list of frames "
                                          "(ragged frames)")
        if frame_shapes is not None or _is_frame_list(images):      # host-side checks first: they need no device
            images, frames, weights, centers, n_components = ragged_frame_inputs(
                images, centers, frame_shapes, weights, None if _grouped_frames else group, n_components)
        torch = _lib.require_gpu()
        self.torch = torch
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        f32 = dict(dtype=torch.float32, device=self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        f64 = dict(dtype=torch.float64, device=self.device)
        if images is None:
            # the model-frame state of several observations (from_observations): no data of its own, the library
            # does not read it
            S, B, H, W = _frame
            self.images = torch.zeros((1,), **f32)
        else:
            self.images = torch.as_tensor(images).to(**f32).contiguous()
            assert self.images.ndim == 4, "images must be (S, B, H, W)"
            S, B, H, W = self.images.shape
        if isinstance(centers, (list, tuple)) and len(centers) and np.ndim(centers[0]) == 2 and \
                len(set(np.shape(c)[0] for c in centers)) > 1:
            centers, counts = pad_centers(centers)
            if n_components is not None and not np.array_equal(np.asarray(n_components).reshape(-1), counts):
                raise ValueError("n_components does not match the lengths of the centre lists")
            n_components = counts
        self.centers = torch.as_tensor(np.asarray(centers) if not torch.is_tensor(centers) else centers).to(**i32).contiguous()
        assert self.centers.ndim == 3 and self.centers.shape[0] == S and self.centers.shape[2] == 2
        K = self.centers.shape[1]
        self.S, self.K, self.B, self.H, self.W = S, K, B, H, W
        self.frame_shapes = None if frames is None else torch.as_tensor(frames).to(**i32).contiguous()
        self.n_components = None
        if n_components is not None:
            n = np.asarray(n_components.cpu() if torch.is_tensor(n_components) else n_components).reshape(-1)
            if n.shape != (S,) or not np.issubdtype(n.dtype, np.integer):
                raise ValueError("n_components must be S = %d integers" % S)
            bad = (n < 1) | (n > K)
            if bad.any():
                s = int(np.argmax(bad))
                raise ValueError("n_components[%d] = %d lies outside 1..K = 1..%d" % (s, int(n[s]), K))
            self.n_components = torch.as_tensor(n.astype(np.int32)).to(**i32).contiguous()
        self._check_centers(self.centers)
        self.weight_scalar = 1.0
        if weights is not None and np.ndim(weights) == 0 and not torch.is_tensor(weights):
            self.weight_scalar, weights = float(weights), None
        self.weights = None if weights is None else torch.as_tensor(weights).to(**f32).contiguous()
        self._frame_mask = None
        self._frames = _lib.ScarletFrames()         # frame_hw NULL: the _frames entry points are their plain counterparts
        if frames is not None:
            # pixels outside a scene's frame do not exist: zero weight (and zero data, so that residuals vanish there)
            self._frames.frame_hw = self.frame_shapes.data_ptr()
            fh, fw = self.frame_shapes[:, 0].view(S, 1, 1, 1), self.frame_shapes[:, 1].view(S, 1, 1, 1)
            self._frame_mask = (torch.arange(H, device=self.device).view(1, 1, H, 1) < fh) & \
                               (torch.arange(W, device=self.device).view(1, 1, 1, W) < fw)            # (S, 1, H, W)
        if frames is not None and images is not None:       # (the state of a joint fit has no data to mask)
            zero = torch.zeros((), **f32)
            full = torch.full((S, B, H, W), self.weight_scalar, **f32) if self.weights is None else self.weights
            if tuple(full.shape) != (S, B, H, W):
                raise ValueError("weights must be a scalar, (S, B, H, W) = %s or per-scene arrays, not %s"
                                 % ((S, B, H, W), tuple(full.shape)))
            self.weights, self.weight_scalar = torch.where(self._frame_mask, full, zero).contiguous(), 1.0
            self.images = torch.where(self._frame_mask, self.images, zero).contiguous()
        self.sed = [torch.zeros((S, K, B), **f32) for _ in range(2)]
        # (_morph=False: a gradient batch of from_observations, whose fit reads the state's morphologies instead)
        self.morph = [torch.zeros((S, K, H, W) if _morph else (1,), **f32) for _ in range(2)]
        self.cur = torch.zeros((S,), **i32)
        self.shifts = torch.full((S, K, 2), float("nan"), **f64)      # NaN == reference's "no shift yet"
        self.flags = torch.full((S, K), _lib.FLAG_SED_NOT_CONVERGED | _lib.FLAG_MORPH_NOT_CONVERGED, **i32)
        if self.n_components is not None:
            self.flags.masked_fill_(~self._present(), 0)          # absent components keep flags 0
        self.lipschitz = torch.ones((S, 2), **f64)
        self.mse_capacity = int(mse_capacity)
        self.mse_buf = torch.zeros((S, self.mse_capacity), **f64)
        self.it = torch.zeros((S,), **i32)
        self.active = torch.ones((S,), **i32)
        self.status = torch.zeros((S,), **i32)
        self.fix_sed = None
        self.fix_morph = None
        self._init_checked = False    # init_sources ran: scenes may carry STATUS_BAD_INIT
        self._catalog = None          # from_catalog: the tables of catalog_arrays, for init_catalog and source()
        self._catalog_options = False  # from_catalog with update options (they go with frames and group there)
        self.group = None
        if group is not None:
            g = np.asarray(group, dtype=np.int32).reshape(S, K)
            for row in g:                    # the layers of a source are adjacent components
                seen = set()
                for k, v in enumerate(row):
                    if v >= 0 and v in seen and row[k - 1] != v:
                        raise ValueError("the components of a multi-component source must be adjacent")
                    seen.add(int(v))
            if self.n_components is not None:
                absent = ~self._present().cpu().numpy()
                if (g[absent] >= 0).any():
                    s, k = [int(v[0]) for v in np.nonzero(absent & (g >= 0))]
                    raise ValueError("group[%d][%d] = %d: an absent component must have group -1" % (s, k, g[s, k]))
            self.group = torch.as_tensor(g).to(**i32).contiguous()
        # the four settings: scalars (the entry points of old) or per component (scarlet_constraints)
        given = dict(symmetric=symmetric, monotonic=monotonic, l0_thresh=l0_thresh, l1_thresh=l1_thresh)
        self.constraints = {}         # name -> (S, K) device tensor, for the settings given per component
        g_host = None if self.group is None else self.group.cpu().numpy()
        for name, value in given.items():
            if is_scalar_setting(value):
                continue
            arr = constraint_arrays(value, S, K, name, group=g_host)
            if self.n_components is not None:          # rows of absent components: off (never read)
                arr[~self._present().cpu().numpy()] = 0 if name in _SWITCHES else -1.0
            self.constraints[name] = torch.as_tensor(arr).to(device=self.device).contiguous()
            given[name] = bool(arr.any()) if name in _SWITCHES else None
        self.symmetric, self.monotonic = bool(given["symmetric"]), bool(given["monotonic"])
        self.l0_thresh, self.l1_thresh = given["l0_thresh"], given["l1_thresh"]
        self._cons = _lib.ScarletConstraints()      # members NULL for the settings given as scalars
        for name, x in self.constraints.items():
            setattr(self._cons, name, x.data_ptr())
        # update options (scarlet_update_options): checked on the host, then one (S, K) device array per member
        self.update_options, self._upd = None, None
        if update is not None:
            host = update.arrays(S, K)
            self.update_options = {name: torch.as_tensor(a).to(device=self.device).contiguous() for name, a in host.items()}
            self._upd = _lib.ScarletUpdateOptions()
            for name, x in self.update_options.items():
                setattr(self._upd, name, x.data_ptr())
        cw = default_centroid_weight() if centroid_weight is None else np.asarray(centroid_weight, dtype=np.float64)
        assert cw.ndim == 2 and cw.shape[0] == cw.shape[1] and cw.shape[0] % 2 == 1
        self.centroid_weight = torch.as_tensor(cw).to(**f64).contiguous()
        self._observations = None     # from_observations: [(ObservationBatch, its gradient batch)]
        self._lowres = None           # ... and per observation None, or (scarlet_lowres, what it points to)
        self._lowres_products = False  # from_observations(lowres_products=True): `products` evaluates those too
        self._wide = False            # from_observations(wide=True): the library's _wide entry points (C <= 32)
        self.L_components = None      # (S, K, 2) float64 after a fit with a prior: the constants each component stepped with
        self._c = _lib.ScarletBatch()
        self._fill_struct()
        self._alloc_workspace()

    # ------------------------------------------------------------------ plumbing
    @property
    def constrained(self):
        """True when a constraint setting was given per component."""
        return bool(self.constraints)

    # Every call into the library's loops goes through one request (scarlet_fit_request): whatever the batch carries --
    # its constraints (a NULL member reads that setting from the batch's scalars), update options, frames, the
    # observations with their low-resolution structs and tables -- and the prior's struct `ps`.  The library refuses what
    # does not go together and copies the pointer arrays into its argument structs before it launches
    # anything; `keep` holds them until the call has returned.
    def _request(self, ps, max_iter=0, e_rel=0.0, approximate_L=False, check_every=0):
        r = _lib.ScarletFitRequest()
        r.constraints, r.frames = ctypes.pointer(self._cons), ctypes.pointer(self._frames)
        if self._upd is not None:
            r.options = ctypes.pointer(self._upd)
        if ps is not None:
            r.prior = ctypes.pointer(ps)
        r.max_iter, r.e_rel, r.approximate_L, r.check_every = int(max_iter), float(e_rel), int(bool(approximate_L)), int(check_every)
        keep = None
        if self._observations is not None:
            r.n_obs = n = len(self._observations)
            r.obs = (ctypes.POINTER(_lib.ScarletBatch) * n)(*[ctypes.pointer(ob._c) for _, ob in self._observations])
            keep = np.array([o.band0 for o, _ in self._observations], dtype=np.int32)
            r.band0 = keep.ctypes.data
            if any(x is not None for x in self._lowres):
                none = ctypes.POINTER(_lib.ScarletLowres)()
                r.lowres = (ctypes.POINTER(_lib.ScarletLowres) * n)(*[none if x is None else ctypes.pointer(x[0]) for x in self._lowres])
                if self.frame_shapes is not None:           # (each low-resolution observation with its own tables)
                    r.lowres_frames = self._lowres_frames()
        return r, keep

    def _lib_fit(self, ps, max_iter, e_rel, approximate_L, check_every):
        r, keep = self._request(ps, max_iter, e_rel, approximate_L, check_every)
        return _lib.check(_lib.lib.scarlet_fit_with(ctypes.byref(self._c), ctypes.byref(r), _lib.stream_ptr()))

    def _lib_update(self, ps, in_iteration):
        r, keep = self._request(ps)
        return _lib.check(_lib.lib.scarlet_source_update_with(ctypes.byref(self._c), ctypes.byref(r), int(in_iteration), _lib.stream_ptr()))

    def _alloc_workspace(self):
        """The workspace for the batch as its struct describes it now (it grows with a difference kernel); the library
        expects it zeroed."""
        nbytes = _lib.lib.scarlet_batch_workspace_bytes(ctypes.byref(self._c))
        self.workspace = self.torch.zeros((int(nbytes),), dtype=self.torch.uint8, device=self.device)
        self._c.workspace = self.workspace.data_ptr()

    def _present(self):
        """(S, K) bool device mask of the components each scene uses (all of them without n_components)."""
        k = self.torch.arange(self.K, device=self.device)
        if self.n_components is None:
            return self.torch.ones((self.S, self.K), dtype=self.torch.bool, device=self.device)
        return k.view(1, -1) < self.n_components.view(-1, 1)

    def _check_centers(self, centers):
        """Source centres index the frame directly (init, max_pixel window, sweeps): the reference raises
        IndexError for a source outside the image; here it is a ValueError before anything is launched.
        The centres of absent components are not read and not checked."""
        c = centers
        if self.frame_shapes is not None:
            hw = self.frame_shapes.view(self.S, 1, 2)
            if bool(((c < 0) | (c >= hw))[self._present()].any().item()):
                raise ValueError("a centre lies outside its scene's own frame (frame_shapes)")
        bad = (c[..., 0] < 0) | (c[..., 0] >= self.H) | (c[..., 1] < 0) | (c[..., 1] >= self.W)
        if self.n_components is not None:
            bad &= self._present()
        if bool(bad.any().item()):
            s, k = [int(v[0]) for v in self.torch.nonzero(bad, as_tuple=True)]
            raise ValueError("centre %s of scene %d, source %d lies outside the %d x %d frame"
                             % (tuple(int(v) for v in c[s, k].tolist()), s, k, self.H, self.W))

    def _fill_struct(self):
        c, p = self._c, (lambda t: None if t is None else t.data_ptr())
        c.S, c.K, c.B, c.H, c.W = self.S, self.K, self.B, self.H, self.W
        c.images, c.weights, c.weight_scalar = p(self.images), p(self.weights), float(self.weight_scalar)
        c.sed[0], c.sed[1] = p(self.sed[0]), p(self.sed[1])
        c.morph[0], c.morph[1] = p(self.morph[0]), p(self.morph[1])
        c.cur = p(self.cur)
        c.centers, c.shifts, c.flags = p(self.centers), p(self.shifts), p(self.flags)
        c.fix_sed, c.fix_morph = p(self.fix_sed), p(self.fix_morph)
        c.lipschitz, c.mse, c.mse_capacity = p(self.lipschitz), p(self.mse_buf), self.mse_capacity
        c.it, c.active, c.status = p(self.it), p(self.active), p(self.status)
        c.symmetric, c.monotonic = int(self.symmetric), int(self.monotonic)
        c.l0_thresh = -1.0 if self.l0_thresh is None else float(self.l0_thresh)
        c.l1_thresh = -1.0 if self.l1_thresh is None else float(self.l1_thresh)
        c.centroid_psf, c.centroid_P = p(self.centroid_weight), int(self.centroid_weight.shape[0])
        c.group = p(self.group)
        c.n_components = p(self.n_components)
        if getattr(self, "workspace", None) is not None:
            c.workspace = self.workspace.data_ptr()

    def _ensure_mse_capacity(self, extra):
        need = int(self.it.max().item()) + int(extra)
        if need > self.mse_capacity:
            new_cap = max(need, 2 * self.mse_capacity)
            buf = self.torch.zeros((self.S, new_cap), dtype=self.torch.float64, device=self.device)
            buf[:, :self.mse_capacity] = self.mse_buf
            self.mse_buf, self.mse_capacity = buf, new_cap
            self._fill_struct()

    def _pick(self, pair):
        """Current-buffer view per scene (scenes flip their buffer index independently)."""
        cur = self.cur.to(self.torch.bool)
        shape = (-1,) + (1,) * (pair[0].ndim - 1)
        return self.torch.where(cur.view(shape), pair[1], pair[0])

    # ------------------------------------------------------------------ state access
    def set_state(self, sed, morph, centers=None, shifts=None):
        """Load factors into the current buffers (e.g. a state produced elsewhere).  The rows of absent components
        are stored as zeros whatever they hold."""
        t = self.torch
        as_t = lambda a: a if t.is_tensor(a) else t.as_tensor(np.asarray(a))
        sed = as_t(sed).to(self.sed[0])
        morph = as_t(morph).to(self.morph[0])
        if self.n_components is not None:
            present = self._present()
            sed = t.where(present.view(self.S, self.K, 1), sed.expand_as(self.sed[0]), t.zeros((), dtype=sed.dtype, device=self.device))
            morph = t.where(present.view(self.S, self.K, 1, 1), morph.expand_as(self.morph[0]),
                            t.zeros((), dtype=morph.dtype, device=self.device))
        if self.frame_shapes is not None:                # pixels outside a scene's frame stay zero in both buffers
            morph = t.where(self._frame_mask, morph.expand_as(self.morph[0]), t.zeros((), dtype=morph.dtype, device=self.device))
        for b in range(2):
            self.sed[b].copy_(sed)
            self.morph[b].copy_(morph)
        if centers is not None:
            new = t.as_tensor(np.asarray(centers)).to(self.centers)
            self._check_centers(new)
            self.centers.copy_(new)
        if shifts is not None:
            self.shifts.copy_(t.as_tensor(np.asarray(shifts, dtype=np.float64)).to(self.shifts))

    def set_diff_kernel(self, kernel):
        """PSF difference kernel (what Observation.match computes, reference observation.py:191-194):
        (B, Py, Px) shared by all scenes, or (S, B, Py, Px) when every scene was observed with its own
        PSFs (`fft.match_psfs_device` makes them in one call).  Enables the FFT-convolution render
        (row a3b): grows the workspace by the FFT buffers and transforms the kernels once."""
        t = self.torch
        k = (kernel if t.is_tensor(kernel) else t.as_tensor(np.ascontiguousarray(kernel, dtype=np.float32)))
        self.diff_kernel = k.to(device=self.device, dtype=t.float32).contiguous()
        per_scene = self.diff_kernel.ndim == 4
        assert (self.diff_kernel.ndim == 3 and self.diff_kernel.shape[0] == self.B) or \
               (per_scene and tuple(self.diff_kernel.shape[:2]) == (self.S, self.B))
        self._c.diff_kernel = self.diff_kernel.data_ptr()
        self._c.diff_kernel_per_scene = int(per_scene)
        self._c.psf_h, self._c.psf_w = int(self.diff_kernel.shape[-2]), int(self.diff_kernel.shape[-1])
        self._alloc_workspace()
        _lib.check(_lib.lib.scarlet_batch_prepare_psf(ctypes.byref(self._c), _lib.stream_ptr()))
        return self

    @property
    def sed_current(self):
        return self._pick(self.sed)

    @property
    def morph_current(self):
        return self._pick(self.morph)

    def scene(self, s):
        """Current (sed, morph) of scene s: (n, B) and (n, H, W) tensors of its n = n_components[s] components; of a
        ragged-frame batch the morphologies on the scene's own frame, (n, h_s, w_s)."""
        n = self.K if self.n_components is None else int(self.n_components[s].item())
        c = int(self.cur[s].item())
        if self.frame_shapes is not None:
            h, w = (int(v) for v in self.frame_shapes[s].tolist())
            return self.sed[c][s, :n], self.morph[c][s, :n, :h, :w]
        return self.sed[c][s, :n], self.morph[c][s, :n]

    def mse(self, s=0):
        """List of losses of scene `s`, one per iteration (reference Blend.mse)."""
        n = int(self.it[s].item())
        return self.mse_buf[s, :n].cpu().numpy().tolist()

    def raise_on_status(self):
        st = self.status.cpu().numpy()
        if (st & _lib.STATUS_BAD_OPTION).any():
            bad = np.nonzero(st & _lib.STATUS_BAD_OPTION)[0]
            raise ValueError("update options of scenes {} hold an unknown or out-of-range value (BAD_OPTION); they were left "
                             "untouched and inactive".format(bad.tolist()))
        if (st & _lib.STATUS_BAD_FRAME).any():
            bad = np.nonzero(st & _lib.STATUS_BAD_FRAME)[0]
            raise ValueError("frame_shapes of scenes {} lie outside 1..{} x 1..{}; they were left untouched and "
                             "inactive".format(bad.tolist(), self.H, self.W))
        if (st & _lib.STATUS_CENTER_AT_EDGE).any():
            bad = np.nonzero(st & _lib.STATUS_CENTER_AT_EDGE)[0][:5]
            raise ValueError("max_pixel window left the image in scenes {} (the reference fails "
                             "there too: measurement.py:24-29)".format(bad.tolist()))
        if (st & _lib.STATUS_BAD_INIT).any():
            bad = np.nonzero(st & _lib.STATUS_BAD_INIT)[0]
            raise ValueError("init_sources: bad input in scenes {} (bg_rms <= 0 in a band, a group of more than {} "
                             "components, percentiles not ascending inside (0, 100), or an empty layer); they were "
                             "left inactive".format(bad.tolist(), _lib.MAX_LAYERS))

    # ------------------------------------------------------------------ products of the state
    def products(self, model=True, rendered=True, residual=True, loss=True, flux=True, components=None, out=None, obs=None):
        """What the reference reads off a fitted Blend, for every scene, from the current factors (read-only: the state,
        the fit's bookkeeping and the workspace stay as they are; scarlet_batch_products, or scarlet_observations_products
        / scarlet_observations_products_lowres / scarlet_observations_products_frames for a batch made by
        `from_observations`).  One call into the library on
        the current stream, no host synchronisation.  Returns a `BatchProducts` of device tensors (None for what was not
        asked for):

        model : (S, C, H, W) sum_k sed[k] morph[k] over the model frame's channels (blend.get_model())
        rendered : (S, B, H, W) the model as the data sees it, convolved with the difference kernel when there is one
            (observation.render(model))
        residual : (S, B, H, W) images - rendered
        loss : (S, B) float64, 0.5 sum (weights (rendered - images))^2 per band (its sum: observation.get_loss(model))
        flux : (S, K, C) float64 morph[k].sum() * sed[k] (component.get_flux()); zero rows for absent components
        components : None or component indices -> component_models (S, n, C, H, W) = sed[k] morph[k] (component.get_model())
        out : a BatchProducts of an earlier call, whose tensors are written again where their shapes fit
        obs : (from_observations) the observations to evaluate, default all

        With `from_observations`, rendered / residual / loss are lists with one entry per observation (None for those
        left out by `obs`).  A low-resolution observation's entries lie on its own pixel grid: rendered and residual are
        (S, B, h, w) -- the model through the observation's resampling and PSFs, LowResObservation.render(model) -- and
        loss is (S, B) (scarlet_observations_products_lowres).  They are evaluated for a batch made with
        `from_observations(..., lowres_products=True)`; a batch made without that keyword behaves as it always did and
        raises NotImplementedError for them (model, flux and the other observations' products are available)."""
        t = self.torch
        S, K, C, H, W = self.S, self.K, self.B, self.H, self.W
        res = BatchProducts() if out is None else out

        def buf(old, want, shape, dtype):
            if not want:
                return None
            if t.is_tensor(old) and tuple(old.shape) == shape and old.dtype == dtype and old.device == self.device \
                    and old.is_contiguous():
                return old
            return t.empty(shape, dtype=dtype, device=self.device)

        sel = None
        if components is not None:
            sel = np.ascontiguousarray(np.asarray(components, dtype=np.int32).reshape(-1))
            if sel.size == 0 or sel.min() < 0 or sel.max() >= K:
                raise ValueError("products: components must name 1 or more of the components 0 .. %d" % (K - 1))
        ps = _lib.ScarletProducts()
        res.model = buf(res.model, model, (S, C, H, W), t.float32)
        res.flux = buf(res.flux, flux, (S, K, C), t.float64)
        res.component_models = buf(res.component_models, sel is not None, (S, 0 if sel is None else sel.size, C, H, W), t.float32)
        res.components = None if sel is None else sel.copy()
        ps.model, ps.flux, ps.component_models = _lib.ptr(res.model), _lib.ptr(res.flux), _lib.ptr(res.component_models)
        if sel is not None:
            ps.components, ps.n_select = sel.ctypes.data, int(sel.size)
        wants = (("rendered", rendered, t.float32), ("residual", residual, t.float32), ("loss", loss, t.float64))
        if self._observations is None:
            if obs not in (None, 0, [0], (0,)):
                raise ValueError("products: this batch has one observation, obs = %r" % (obs,))
            for name, want, dtype in wants:
                x = buf(getattr(res, name), want, (S, C) if name == "loss" else (S, C, H, W), dtype)
                setattr(res, name, x)
                setattr(ps, name, _lib.ptr(x))
            nbytes = _lib.lib.scarlet_products_scratch_bytes(ctypes.byref(self._c), ctypes.byref(ps))
            scratch = self._products_scratch(nbytes)
            if self.frame_shapes is not None:       # nothing outside each scene's own frame
                c = self._c
                if self.group is not None:          # (from_catalog: the products do not depend on the groups)
                    c = _lib.ScarletBatch.from_buffer_copy(self._c)
                    c.group = None
                _lib.check(_lib.lib.scarlet_batch_products_frames(ctypes.byref(c), ctypes.byref(self._frames), ctypes.byref(ps),
                                                                  _lib.ptr(scratch), int(nbytes), _lib.stream_ptr()))
                return res
            _lib.check(_lib.lib.scarlet_batch_products(ctypes.byref(self._c), ctypes.byref(ps), _lib.ptr(scratch), int(nbytes),
                                                       _lib.stream_ptr()))
            return res
        n = len(self._observations)
        idx = list(range(n)) if obs is None else [int(i) for i in np.atleast_1d(obs)]
        if any(i < 0 or i >= n for i in idx):
            raise ValueError("products: obs = %r, there are %d observations" % (obs, n))
        if not (rendered or residual or loss):
            idx = []
        for i in idx:
            if self._lowres[i] is not None and not self._lowres_products:
                raise NotImplementedError("products: rendered, residual and loss of a low-resolution observation (observation "
                                          "%d) are evaluated for a batch made with from_observations(..., "
                                          "lowres_products=True); model and flux are available without it" % i)
        outs = (_lib.ScarletProducts * n)()
        for name, want, dtype in wants:
            old = getattr(res, name)
            old = old if isinstance(old, list) and len(old) == n else [None] * n
            new = [None] * n
            for i in idx:
                o = self._observations[i][0]
                # (a low-resolution observation's planes lie on its own pixel grid)
                new[i] = buf(old[i], want, (S, o.B) if name == "loss" else (S, o.B) + tuple(o.shape[2:]), dtype)
                setattr(outs[i], name, _lib.ptr(new[i]))
            setattr(res, name, new if want else None)
        any_state = model or flux or sel is not None
        state_bytes = _lib.lib.scarlet_products_scratch_bytes_wide if self._wide else _lib.lib.scarlet_products_scratch_bytes
        lowres_bytes = (_lib.lib.scarlet_lowres_products_scratch_bytes_wide if self._wide
                        else _lib.lib.scarlet_lowres_products_scratch_bytes)
        nbytes = state_bytes(ctypes.byref(self._c), ctypes.byref(ps)) if any_state else 0
        for i in idx:
            ob = self._observations[i][1]
            if self._lowres[i] is None:
                need = _lib.lib.scarlet_products_scratch_bytes(ctypes.byref(ob._c), ctypes.byref(outs[i]))
            else:
                need = _lib.check(lowres_bytes(
                    ctypes.byref(self._c), ctypes.byref(ob._c), ctypes.byref(self._lowres[i][0]), ctypes.byref(outs[i])))
            nbytes = max(nbytes, need)
        scratch = self._products_scratch(nbytes)
        ptrs = (ctypes.POINTER(_lib.ScarletBatch) * n)(*[ctypes.pointer(ob._c) for _, ob in self._observations])
        first = np.array([o.band0 for o, _ in self._observations], dtype=np.int32)
        tail = (first.ctypes.data_as(ctypes.c_void_p), n, ctypes.byref(ps) if any_state else None, outs, _lib.ptr(scratch),
                int(nbytes), _lib.stream_ptr())
        lows = None
        if any(x is not None for x in self._lowres):
            none = ctypes.POINTER(_lib.ScarletLowres)()
            lows = (ctypes.POINTER(_lib.ScarletLowres) * n)(*[none if x is None else ctypes.pointer(x[0]) for x in self._lowres])
        if self.frame_shapes is not None and lows is not None:
            _lib.check(_lib.lib.scarlet_observations_products_frames_lowres(
                ctypes.byref(self._c), ctypes.byref(self._frames), ptrs, lows, self._lowres_frames(), *tail))
        elif self.frame_shapes is not None:         # nothing outside each scene's own frame, in every observation
            _lib.check(_lib.lib.scarlet_observations_products_frames(ctypes.byref(self._c), ctypes.byref(self._frames), ptrs, *tail))
        elif self._wide:
            _lib.check(_lib.lib.scarlet_observations_products_wide(ctypes.byref(self._c), ptrs, lows, *tail))
        elif lows is not None:
            _lib.check(_lib.lib.scarlet_observations_products_lowres(ctypes.byref(self._c), ptrs, lows, *tail))
        else:
            _lib.check(_lib.lib.scarlet_observations_products(ctypes.byref(self._c), ptrs, *tail))
        return res

    def _products_scratch(self, nbytes):
        """Device scratch of `products`, kept between calls and grown when a call needs more."""
        old = getattr(self, "_scratch", None)
        if nbytes and (old is None or old.numel() < nbytes):
            self._scratch = old = self.torch.empty((int(nbytes),), dtype=self.torch.uint8, device=self.device)
        return old if nbytes else None

    def _one_product(self, name, obs=0, **kw):
        want = dict(model=False, rendered=False, residual=False, loss=False, flux=False)
        want[name] = True
        x = getattr(self.products(obs=None if name in ("model", "flux") or self._observations is None else [obs], **want, **kw), name)
        return x[obs] if isinstance(x, list) else x

    def get_model(self):
        """(S, C, H, W) model of every scene over the model frame's channels (reference blend.get_model())."""
        return self._one_product("model")

    def render(self, obs=0):
        """(S, B, H, W) the model as observation `obs` sees it (reference observation.render(blend.get_model()))."""
        return self._one_product("rendered", obs)

    def residual(self, obs=0):
        """(S, B, H, W) images - render of observation `obs`."""
        return self._one_product("residual", obs)

    def get_loss(self):
        """(S,) float64 loss of every scene, summed over bands and observations as Blend._loss does: what the next
        iteration records in `mse`."""
        x = self.products(model=False, rendered=False, residual=False, loss=True, flux=False).loss
        return sum(v.sum(dim=1) for v in x) if isinstance(x, list) else x.sum(dim=1)

    def get_flux(self):
        """(S, K, C) float64 flux of every component in every channel (reference component.get_flux())."""
        return self._one_product("flux")

    def component_models(self, ks):
        """(S, len(ks), C, H, W) models sed[k] morph[k] of the components `ks` (reference component.get_model())."""
        return self.products(model=False, rendered=False, residual=False, loss=False, flux=False, components=ks).component_models

    # ------------------------------------------------------------------ operations
    def init_extended(self, bg_rms, thresh=1.0, sed_scale=None, init_symmetric=True, init_monotonic=None,
                      run_update=True):
        """ExtendedSource initialisation for every component (reference source.py:139-180,
        444-492) followed by the constructor's update() call."""
        self._refuse_single_init()
        bg = np.ascontiguousarray(bg_rms, dtype=np.float32)
        assert bg.shape == (self.B,)
        sc = None if sed_scale is None else np.ascontiguousarray(sed_scale, dtype=np.float32)
        args = (bg.ctypes.data_as(ctypes.c_void_p), float(thresh),
                None if sc is None else sc.ctypes.data_as(ctypes.c_void_p), int(bool(init_symmetric)),
                int(self.monotonic if init_monotonic is None else bool(init_monotonic)),
                int(bool(run_update) and not self.constrained and self._upd is None), _lib.stream_ptr())
        if self.frame_shapes is not None:           # each scene's start on its own frame
            rc = _lib.lib.scarlet_init_extended_frames(ctypes.byref(self._c), ctypes.byref(self._frames), *args)
        else:
            rc = _lib.lib.scarlet_init_extended(ctypes.byref(self._c), *args)
        _lib.check(rc)
        if run_update and (self.constrained or self._upd is not None):
            # the constructors' update() with each component's own settings and update options
            self.update_sources()
        return self

    def init_sources(self, bg_rms, kind=None, flux_percentiles=None, obs_psfs=None, model_psf=None, thresh=1.0,
                     init_symmetric=True, init_monotonic=None, run_update=True):
        """Initialise every component as the source type the reference's constructors would make of it, on the
        device for the whole batch (scarlet_init_sources), then run their update() once.

        bg_rms : (B,) shared by all scenes, or (S, B) per scene
        kind : None (every component is an ExtendedSource), or (S, K) of "extended" / "point" or INIT_* integers;
            ignored for the layers of a multi-component source (`group` >= 0)
        flux_percentiles : the boundaries between the layers of a MultiComponentSource: None (the reference's
            default [25]), one list for every group (sorted, as the reference does: groups then have len + 1
            members), or an (S, K) array holding at member j >= 1 of each group the percentile of boundary j
        obs_psfs : None, (B, P, P) or (S, B, P, P): the observed PSFs; their peaks divide the pixel SEDs
        model_psf : None or (P, P), P odd: the model frame's PSF (frame.psfs[0]); point sources paste it, extended
            SEDs are multiplied by its max (get_psf_sed)
        init_symmetric, init_monotonic : the arguments of init_extended_source for the extended sources (the layers
            use the batch's `symmetric`, as MultiComponentSource does)

        Bad input of the whole call raises ValueError; bad input of single scenes (a bg_rms row with a value <= 0, a
        group of more than MAX_LAYERS members, percentiles not ascending inside (0, 100)) gives those scenes
        STATUS_BAD_INIT and leaves them untouched and inactive (`raise_on_status` names them).

        A ragged-frame batch (`frame_shapes`) starts extended sources only: `kind` raises NotImplementedError.  One made
        by `from_catalog` starts every kind on each scene's own frame (scarlet_init_sources_frames_mixed; `init_catalog`
        passes the catalogue's tables)."""
        self._refuse_single_init()
        mixed = self.frame_shapes is not None and self._catalog is not None       # (from_catalog: every stock source type)
        if self.frame_shapes is not None and kind is not None and not mixed:
            raise NotImplementedError("init_sources on a ragged-frame batch starts extended sources only (kind must be None)")
        t = self.torch
        S, K, B = self.S, self.K, self.B
        keep = []

        def dev(a, dtype):
            x = (a if t.is_tensor(a) else t.as_tensor(np.asarray(a))).to(device=self.device, dtype=dtype).contiguous()
            keep.append(x)
            return x

        bg = dev(bg_rms, t.float32)
        if tuple(bg.shape) not in ((B,), (S, B)):
            raise ValueError("bg_rms must have shape (B,) = (%d,) or (S, B) = (%d, %d), not %s" % (B, S, B, tuple(bg.shape)))
        if bg.ndim == 1 and not bool((bg > 0).all().item()):
            raise ValueError("bg_rms must be greater than zero in all channels")
        spec = _lib.ScarletInitSpec()
        spec.bg_rms, spec.bg_rms_per_scene = bg.data_ptr(), int(bg.ndim == 2)
        if kind is not None:
            kk = np.asarray(kind.cpu() if t.is_tensor(kind) else kind)
            if kk.shape != (S, K):
                raise ValueError("kind must have shape (S, K) = (%d, %d), not %s" % (S, K, kk.shape))
            if kk.dtype.kind in "US":
                names = {"extended": _lib.INIT_EXTENDED, "point": _lib.INIT_POINT}
                unknown = set(kk.ravel().tolist()) - set(names)
                if unknown:
                    raise ValueError("unknown source kind %r (extended or point)" % sorted(unknown)[0])
                kk = np.vectorize(names.get, otypes=[np.int32])(kk)
            elif not np.issubdtype(kk.dtype, np.integer) or not np.isin(kk, (_lib.INIT_EXTENDED, _lib.INIT_POINT)).all():
                raise ValueError("kind must hold INIT_EXTENDED or INIT_POINT")
            spec.kind = dev(kk.astype(np.int32), t.int32).data_ptr()
        if flux_percentiles is not None and np.ndim(flux_percentiles) == 2:
            perc = np.asarray(flux_percentiles.cpu() if t.is_tensor(flux_percentiles) else flux_percentiles)
            if perc.shape != (S, K):
                raise ValueError("flux_percentiles must be one list or (S, K) = (%d, %d), not %s" % (S, K, perc.shape))
            spec.flux_percentiles = dev(perc.astype(np.float32), t.float32).data_ptr()
        elif self.group is not None:
            # one list for every group (the reference sorts it): every group needs len + 1 members
            lst = np.sort(np.asarray([25] if flux_percentiles is None else flux_percentiles, dtype=np.float64).ravel())
            if ((lst <= 0) | (lst >= 100)).any():
                raise ValueError("flux_percentiles must lie inside (0, 100): %s" % lst.tolist())
            g = self.group.cpu().numpy()
            perc = np.zeros((S, K), np.float32)
            for s in range(S):
                k = 0
                while k < K:
                    if g[s, k] < 0:
                        k += 1
                        continue
                    n = 1
                    while k + n < K and g[s, k + n] == g[s, k]:
                        n += 1
                    if n != len(lst) + 1:
                        raise ValueError("scene %d, component %d: a group of %d components needs %d flux_percentiles, "
                                         "%d given" % (s, k, n, n - 1, len(lst)))
                    perc[s, k + 1:k + n] = lst
                    k += n
            spec.flux_percentiles = dev(perc, t.float32).data_ptr()
        if obs_psfs is not None:
            op = dev(obs_psfs, t.float32)
            _check_obs_psfs(op, S, B, "obs_psfs")
            peak = op.amax(dim=(-2, -1)).contiguous()
            keep.append(peak)
            spec.obs_psf_peak, spec.obs_psf_peak_per_scene = peak.data_ptr(), int(op.ndim == 4)
        if model_psf is not None:
            mp = dev(model_psf, t.float32)
            _check_model_psf(mp, "model_psf")
            spec.model_psf, spec.model_psf_P = mp.data_ptr(), int(mp.shape[0])
        spec.thresh = float(thresh)
        spec.init_symmetric = int(bool(init_symmetric))
        spec.init_monotonic = int(self.monotonic if init_monotonic is None else bool(init_monotonic))
        spec.run_update = int(bool(run_update) and not self.constrained and self._upd is None)
        if mixed:
            _lib.check(_lib.lib.scarlet_init_sources_frames_mixed(ctypes.byref(self._c), ctypes.byref(self._frames), ctypes.byref(spec),
                                                                  _lib.stream_ptr()))
        elif self.frame_shapes is not None:
            _lib.check(_lib.lib.scarlet_init_sources_frames(ctypes.byref(self._c), ctypes.byref(self._frames), ctypes.byref(spec),
                                                            _lib.stream_ptr()))
        else:
            _lib.check(_lib.lib.scarlet_init_sources(ctypes.byref(self._c), ctypes.byref(spec), _lib.stream_ptr()))
        self._init_checked = True
        if run_update and (self.constrained or self._upd is not None):
            # the constructors' update() with each component's own settings; scenes with STATUS_BAD_INIT stay untouched
            self.update_sources()
        return self

    # ------------------------------------------------------------------ catalogues
    @classmethod
    def from_catalog(cls, cutouts, catalog, weights=None, update=None, **kwargs):
        """A batch made from survey cut-outs and one catalogue per cut-out: stars, plain galaxies and multi-component
        galaxies in scenes with their own frame sizes.

        cutouts : a list of S arrays (B, h_s, w_s), or one (S, B, H, W) block
        catalog : S lists of `SourceSpec`, lengths differ; every source expands to its layers (adjacent components, one
            group per multi source: `catalog_arrays`)
        weights : as `BlendBatch` takes them (a list of per-scene arrays for ragged cut-outs)
        update : None, or an `UpdateOptions` of single values: the batch's default for the update options every
            `SourceSpec` may set itself (symmetry, strength, use_nearest, monotonic_thresh, positive, normalization;
            `catalog_option_arrays`).  Per-component arrays raise ValueError: they come from the catalogue.
        kwargs : centroid_weight, mse_capacity, device

        The batch keeps `sources` (per scene the (first component, layers) of its sources: `source(s, i)`) and the kind and
        percentile tables for `init_catalog`.  Uniform cut-outs (a block, or a list of equal shapes) give exactly
        `BlendBatch(images, centers, group=, n_components=, symmetric=, ...)`; ragged ones a ragged-frame batch that also
        takes `group` -- every scene is started and fitted on its own frame, as the reference does for the scene alone
        (scarlet_init_sources_frames_mixed, scarlet_fit_frames_grouped).  A catalogue in which nothing sets an update
        option, with `update=None`, is exactly that batch.  Anything else -- an explicit `update=UpdateOptions()` and
        uniform cut-outs included -- carries each component's options on the device and runs the constraint kernels'
        options instances on each scene's own frame (scarlet_fit_frames_options, scarlet_source_update_frames_options):
        the general path on one pipeline; `init_catalog` starts the sources and then runs the constructors' update with
        the options, and a scene whose options were corrupted on the device gets STATUS_BAD_OPTION and is left untouched.
        Priors, joint fits and the single-scene `Blend` stay out of scope for a catalogue batch.  Every check of the input
        is made on the host (ValueError naming scene and source) before the device is asked for."""
        for name in ("centers", "group", "n_components", "frame_shapes", "symmetric", "monotonic", "l0_thresh", "l1_thresh"):
            if name in kwargs:
                raise ValueError("from_catalog: %s comes from the catalogue" % name)
        images, shapes, uniform = catalog_frames(cutouts)
        t = catalog_arrays(shapes, catalog)
        options = catalog_option_arrays(catalog, update)
        S, K = t["group"].shape
        full = bool((t["n_components"] == K).all())
        present = np.arange(K)[None, :] < t["n_components"][:, None]
        settings = {}
        for name in _SWITCHES + _THRESHOLDS:       # one value for the batch where the catalogue agrees on it
            vals = np.unique(t[name][present])
            if vals.size == 1:
                v = vals[0]
                settings[name] = bool(v) if name in _SWITCHES else (None if v < 0 else float(v))
            else:
                settings[name] = t[name]
        group = t["group"] if (t["group"] >= 0).any() else None
        if uniform:
            block = np.stack([np.asarray(a) for a in images]) if isinstance(images, list) else images
            if isinstance(weights, (list, tuple)) and _is_frame_list(weights):      # per-scene weights of equal shapes
                weights = np.stack([np.asarray(w) for w in weights])
            b = cls(block, t["centers"], weights=weights, group=group, n_components=None if full else t["n_components"],
                    **settings, **kwargs)
        else:
            b = cls(images, t["centers"], weights=weights, group=group, n_components=None if full else t["n_components"],
                    _grouped_frames=True, **settings, **kwargs)
        b._catalog = t
        b.sources = t["sources"]
        if options is not None:
            b._set_catalog_options(options)
        return b

    def _set_catalog_options(self, host):
        """(from_catalog) the catalogue's update options on the device; from here on the batch calls the library's
        _frames_options entry points, which take its group and its frames (frame_hw NULL for uniform cut-outs)"""
        self.update_options = {name: self.torch.as_tensor(a).to(device=self.device).contiguous() for name, a in host.items()}
        self._upd = _lib.ScarletUpdateOptions()
        for name, x in self.update_options.items():
            setattr(self._upd, name, x.data_ptr())
        self._catalog_options = True

    def init_catalog(self, bg_rms, obs_psfs=None, model_psf=None, thresh=1.0):
        """Start every source of the catalogue by its own constructor (ExtendedSource, PointSource,
        MultiComponentSource), on its scene's own frame, and run the constructors' update() once: `init_sources` with
        the kind and percentile tables `from_catalog` kept.  Bad scenes follow `init_sources`: STATUS_BAD_INIT, left
        untouched and inactive, named by `raise_on_status`."""
        if self._catalog is None:
            raise ValueError("init_catalog: the batch was not made by from_catalog")
        t = self._catalog
        kind = t["kind"] if (t["kind"] == _lib.INIT_POINT).any() else None
        return self.init_sources(bg_rms, kind=kind, flux_percentiles=None if self.group is None else t["percentiles"],
                                 obs_psfs=obs_psfs, model_psf=model_psf, thresh=thresh)

    def source(self, s, i):
        """Current (sed, morph) of source i of scene s of a batch made by `from_catalog`: (n_layers, B) and
        (n_layers, h_s, w_s) tensors, the morphologies on the scene's own frame as `scene(s)` gives them."""
        if self._catalog is None:
            raise ValueError("source: the batch was not made by from_catalog")
        first, n = self.sources[s][i]
        sed, morph = self.scene(s)
        return sed[first:first + n], morph[first:first + n]

    def update_sources(self):
        """Run the constraint pipeline once with it=0 (what the source constructors do)."""
        self._lib_update(None, 0)
        return self

    def fit(self, max_iter=200, e_rel=1e-2, approximate_L=False, check_every=10, prior=None):
        """Blend.fit for every scene (reference blend.py:65-102).  Scenes that reach e_rel
        stop iterating individually.  Returns the number of iterations launched.  A batch made by
        `from_observations` fits all its observations jointly.  Every batch goes through scarlet_fit_with.

        prior : None, or what scarlet_amd.prior describes -- a QuadraticPrior and / or constant given tensors (one
            call into the library with the prior's struct), a callable evaluated once per iteration on the
            current stream (the host looks at `active` only every `check_every` iterations), or a list of these.
            `L_components` then holds the constants each component stepped with.  Shapes are those of this batch: for
            one made by `from_observations` the SEDs are (S, K, C) over the model frame's C channels."""
        self._refuse_frames_prior(prior)
        self._refuse_update_prior(prior)
        self._ensure_mse_capacity(max_iter)
        self.active.fill_(1)          # a new fit() call iterates again, like the reference
        if self._init_checked:        # ... except the scenes whose init_sources input was bad
            self.active.masked_fill_((self.status & _lib.STATUS_BAD_INIT) != 0, 0)
        if prior is not None:
            return self._fit_prior(prior, int(max_iter), float(e_rel), int(bool(approximate_L)), int(check_every))
        return self._lib_fit(None, max_iter, e_rel, approximate_L, check_every)

    def step(self, e_rel=1e-2, approximate_L=False, prior=None):
        """One iteration in three separately callable phases (used by tests and by the
        Python-level update() override path).  A batch made by `from_observations` runs one iteration
        of its joint fit.  `prior`: as in `fit`."""
        self._refuse_frames_prior(prior)
        self._refuse_update_prior(prior)
        self._ensure_mse_capacity(1)
        if self._upd is not None and self._observations is None:
            # one iteration of the library's loop: the device checks (counts, frames, options) come before the gradient step
            self._lib_fit(None, 1, e_rel, approximate_L, 0)
            return
        if self._observations is not None:
            if self._init_checked:
                self.active.masked_fill_((self.status & _lib.STATUS_BAD_INIT) != 0, 0)
            if prior is None:
                self._lib_fit(None, 1, e_rel, approximate_L, 0)
                return
        if prior is not None:
            quad, given, fns = _prior.split_priors(prior)
            self._prior_iteration(self._prior_struct(quad), given, fns, float(e_rel), int(bool(approximate_L)))
            return
        if self.frame_shapes is not None and self.group is not None:
            # (from_catalog) one iteration of the library's loop: its device check of the frames comes first
            self._lib_fit(None, 1, e_rel, approximate_L, 0)
            return
        s = _lib.stream_ptr()
        if self.frame_shapes is not None:           # the device check first: the gradient kernels skip the scenes it refuses
            _lib.check(_lib.lib.scarlet_check_frames(ctypes.byref(self._c), ctypes.byref(self._frames), s))
        _lib.check(_lib.lib.scarlet_backward_step(ctypes.byref(self._c), int(bool(approximate_L)), s))
        self._lib_update(None, 1)
        _lib.check(_lib.lib.scarlet_check_convergence(ctypes.byref(self._c), float(e_rel), s))

    def _refuse_frames_prior(self, prior):
        if prior is not None and self.frame_shapes is not None:
            raise NotImplementedError("a ragged-frame batch (frame_shapes) does not take a prior")

    # ------------------------------------------------------------------ priors
    def _refuse_update_prior(self, prior):
        if prior is not None and self._upd is not None:
            raise NotImplementedError("a batch with update= (UpdateOptions) does not take a prior")

    def _prior_struct(self, quad):
        """scarlet_prior with the quadratic part bound to this batch and L_comp = L_components."""
        t = self.torch
        if self.L_components is None:
            self.L_components = t.zeros((self.S, self.K, 2), dtype=t.float64, device=self.device)
        ps = _lib.ScarletPrior()
        self._prior_keep = bound = {} if quad is None else quad.bind(self)
        for name, x in bound.items():
            setattr(ps, name, None if x is None else x.data_ptr())
        ps.L_comp = self.L_components.data_ptr()
        return ps

    def _set_given(self, ps, dicts):
        """Sum the given values of `dicts` into full-shape float32 tensors and point the struct at them."""
        t = self.torch
        f32 = dict(dtype=t.float32, device=self.device)
        shapes = dict(grad_sed=(self.S, self.K, self.B), grad_morph=(self.S, self.K, self.H, self.W),
                      L_sed=(self.S, self.K), L_morph=(self.S, self.K))
        keep = {}
        for d in dicts:
            _prior.check_given_keys(d)
            for key, v in d.items():
                if v is None:
                    continue
                if not t.is_tensor(v):
                    v = t.full((), float(v), **f32) if np.ndim(v) == 0 else t.as_tensor(np.asarray(v, dtype=np.float32))
                v = v.to(**f32)
                _prior.check_target(v.shape, shapes[key], key)
                keep[key] = v.expand(shapes[key]) if key not in keep else keep[key] + v
        for key in _prior.GIVEN_KEYS:
            x = keep.get(key)
            if x is not None:
                keep[key] = x = x.contiguous()
            setattr(ps, key, None if x is None else x.data_ptr())
        self._given_keep = keep          # alive until the next iteration replaces them (same stream)

    def _prior_iteration(self, ps, given, fns, e_rel, approximate_L):
        dicts = list(given)
        if fns:
            sed, morph = self.sed_current, self.morph_current          # gathered copies: the callables cannot touch the state
            dicts += [fn(sed, morph) for fn in fns]
        self._set_given(ps, dicts)
        if self._observations is not None:                             # one iteration of the joint fit, no host look
            self._lib_fit(ps, 1, e_rel, approximate_L, 0)
            return
        s = _lib.stream_ptr()
        _lib.check(_lib.lib.scarlet_backward_step_prior(ctypes.byref(self._c), ctypes.byref(ps), approximate_L, s))
        self._lib_update(ps, 1)
        _lib.check(_lib.lib.scarlet_check_convergence(ctypes.byref(self._c), e_rel, s))

    def _fit_prior(self, prior, max_iter, e_rel, approximate_L, check_every):
        quad, given, fns = _prior.split_priors(prior)
        ps = self._prior_struct(quad)
        if not fns:
            # nothing changes between iterations: the library's own loop
            self._set_given(ps, given)
            return self._lib_fit(ps, max_iter, e_rel, approximate_L, check_every)
        launched = 0
        for i in range(max_iter):
            self._prior_iteration(ps, given, fns, e_rel, approximate_L)
            launched += 1
            if check_every > 0 and (i + 1) % check_every == 0 and i + 1 < max_iter and not bool(self.active.any().item()):
                break
        return launched

    # ------------------------------------------------------------------ several observations
    @classmethod
    def from_observations(cls, observations, centers, _host_gradients=False, _channels=None, lowres_products=False, wide=False,
                          **kwargs):
        """A batch fitted jointly against several observations of every scene (reference Blend(sources, [obs_a,
        obs_b]), blend.py:24-43, 120-139, 219-220).  The factors span the model frame's C = max(band0 + B) channels
        (C <= 8, with `wide=True` C <= 32); `centers` and the other keyword arguments are those of BlendBatch (ragged
        centre lists give n_components).  Start the sources with `init_combined` (or `set_state`), then `fit` / `step`.

        Observations that carry `frame_shapes` (all of them, with equal shapes) make the batch a ragged-frame one: every
        scene is fitted on its own (C, h_s, w_s) frame, as the reference fits it alone (scarlet_fit_observations_frames;
        see `BlendBatch`'s frame_shapes).  Centres are then in each scene's own coordinates.  A low-resolution
        observation joins such a batch with one geometry per scene, each matched to its own scene's model frame
        (`LowResObservationBatch.from_frames(images, geometry=[...])`; its `model_shapes` must be the same-grid
        observations' shapes: scarlet_fit_observations_frames_lowres); one without frame shapes of its own, a batch of
        low-resolution observations only, `group` and a prior raise NotImplementedError.

        wide : the model frame may span up to 32 channels (scarlet_fit_observations_wide and its siblings): instruments
            whose bands do not coincide, each still with at most 8 bands of its own.  SEDs, `flux` and `model` then
            have C channels.  With C <= 8 the batch is the one made without the keyword, bit for bit; without the
            keyword nothing changes, the ValueError above 8 channels included.

        lowres_products : `products`, `render`, `residual` and `get_loss` also evaluate the low-resolution observations
            (on their own pixel grids).  Off by default: a batch made without it raises NotImplementedError for those,
            as such batches always did.  The fit does not depend on it.
        _host_gradients : `Blend`'s Python pipeline calls scarlet_backward_gradients on the state and on every
            observation's batch itself, so the state gets real (zero) images and the observations' batches keep their
            own morphology planes; the joint fit reads neither.
        _channels : the model frame's channel count where the observations need not reach its last channel (`Blend`)."""
        if kwargs.get("frame_shapes") is not None:
            raise NotImplementedError("from_observations does not take frame_shapes (ragged frames): they belong to the "
                                      "observations, ObservationBatch(..., frame_shapes=...) or ObservationBatch.from_frames")
        obs = list(observations)
        if kwargs.get("update") is not None:        # update options: same-grid observations, at most 8 model channels
            if wide:
                raise NotImplementedError("from_observations: update= (UpdateOptions) with wide=True is not implemented")
            if any(isinstance(o, LowResObservationBatch) for o in obs):
                raise NotImplementedError("from_observations: update= (UpdateOptions) with a low-resolution observation is not "
                                          "implemented")
        if not 1 <= len(obs) <= _lib.MAX_OBSERVATIONS:
            raise ValueError("from_observations: 1 to %d observations, not %d" % (_lib.MAX_OBSERVATIONS, len(obs)))
        if not all(isinstance(o, ObservationBatch) for o in obs):      # (a LowResObservationBatch is one)
            raise ValueError("from_observations: every observation must be an ObservationBatch")
        same_grid = [o for o in obs if not isinstance(o, LowResObservationBatch)]
        S = obs[0].shape[0]
        H, W = same_grid[0].shape[2:] if same_grid else obs[0].model_shape
        # scenes with their own frames: the shapes travel with the same-grid observations, which must agree on them
        ragged = any(o.frame_shapes is not None for o in same_grid)
        low_frames = [i for i, o in enumerate(obs) if isinstance(o, LowResObservationBatch) and o.frame_shapes is not None]
        if low_frames and not same_grid:
            raise NotImplementedError("from_observations: a ragged-frame batch of low-resolution observations only (observation "
                                      "%d carries frame shapes): a same-grid observation must carry the model frames" % low_frames[0])
        if low_frames and not ragged:
            raise ValueError("from_observations: low-resolution observation %d carries frame shapes, the same-grid "
                             "observations carry none: every observation of a ragged-frame batch needs them" % low_frames[0])
        if ragged:
            for i, o in enumerate(obs):
                # (one geometry, or a list matched to one frame: its operator would be that of the padded frame)
                if isinstance(o, LowResObservationBatch) and o.frame_shapes is None:
                    raise NotImplementedError("from_observations: a low-resolution observation (observation %d) without frame "
                                              "shapes of its own in a batch whose observations carry frame_shapes (ragged "
                                              "frames): make it with LowResObservationBatch.from_frames(images, geometry=[...])"
                                              % i)
            if kwargs.get("group") is not None:
                raise NotImplementedError("from_observations: observations with frame_shapes (ragged frames) do not take group=")
            if _host_gradients:
                raise NotImplementedError("from_observations: observations with frame_shapes (ragged frames) have no "
                                          "host-gradient form")
        for i, o in enumerate(obs):
            if isinstance(o, LowResObservationBatch) and o.frame_shapes is not None:
                if o.shape[0] != S:
                    raise ValueError("from_observations: low-resolution observation %d has %d scenes, the batch has %d"
                                     % (i, o.shape[0], S))
                continue                    # (its model frames are checked against the same-grid observations' below)
            if isinstance(o, LowResObservationBatch):
                if o.shape[0] != S or o.model_shape != (H, W):
                    raise ValueError("from_observations: low-resolution observation %d has %d scenes and was matched to a "
                                     "%d x %d model frame, the batch has %d scenes of %d x %d"
                                     % ((i, o.shape[0]) + o.model_shape + (S, H, W)))
                continue
            if (o.shape[0], o.shape[2], o.shape[3]) != (S, H, W):
                raise ValueError("from_observations: observation %d has %d scenes of %d x %d, observation 0 %d of %d x %d%s"
                                 % (i, o.shape[0], o.shape[2], o.shape[3], S, H, W,
                                    " (observations with frame_shapes share one padded block size: pad lists of different "
                                    "maximum sizes to one (S, B, H, W) block and pass frame_shapes)" if ragged else ""))
        C = max(o.band0 + o.B for o in obs)
        if _channels is not None:
            if int(_channels) < C:
                raise ValueError("from_observations: the observations span %d model channels, the model frame has %d"
                                 % (C, _channels))
            C = int(_channels)
        for i, o in enumerate(obs):
            if wide and o.B > 8:
                raise ValueError("from_observations: observation %d has %d bands, an observation has at most 8 (split it "
                                 "into two observations on the same grid)" % (i, o.B))
        if wide and C > _lib.MAX_CHANNELS:
            raise ValueError("from_observations: the observations span %d model channels, at most %d are supported"
                             % (C, _lib.MAX_CHANNELS))
        if C > 8 and not wide:
            raise ValueError("from_observations: the observations span %d model channels, at most 8 are supported" % C)
        for k in ("weights", "images"):
            if k in kwargs:
                raise ValueError("from_observations: %s belong to the observations" % k)
        frames = None
        if ragged:
            first = next(i for i, o in enumerate(obs) if o.frame_shapes is not None and not isinstance(o, LowResObservationBatch))
            frames = obs[first].frame_shapes
            for i, o in enumerate(obs):
                if isinstance(o, LowResObservationBatch):
                    if not np.array_equal(o.model_shapes, frames):
                        s = int(np.argmax((o.model_shapes != frames).any(axis=1)))
                        raise ValueError("from_observations: low-resolution observation %d was matched to a %d x %d model frame "
                                         "in scene %d, observation %d has that scene at %d x %d: the geometries must be "
                                         "matched to the scenes' own frames"
                                         % (i, o.model_shapes[s, 0], o.model_shapes[s, 1], s, first, frames[s, 0], frames[s, 1]))
                    continue
                if o.frame_shapes is None:
                    raise ValueError("from_observations: observation %d carries no frame_shapes, observation %d does "
                                     "(scene 0 there is %d x %d): every observation of a ragged-frame batch needs them"
                                     % (i, first, frames[0, 0], frames[0, 1]))
                if not np.array_equal(o.frame_shapes, frames):
                    s = int(np.argmax((o.frame_shapes != frames).any(axis=1)))
                    raise ValueError("from_observations: observation %d has scene %d at %d x %d, observation %d at %d x %d: "
                                     "the observations must agree on every scene's frame"
                                     % (i, s, o.frame_shapes[s, 0], o.frame_shapes[s, 1], first, frames[s, 0], frames[s, 1]))
            # centres are in each scene's own coordinates (host check, as for BlendBatch; ragged lists are padded here)
            centers, kwargs["n_components"] = ragged_frame_centers(centers, frames, kwargs.get("n_components"))
        state = cls(None, centers, _frame=(S, C, H, W), _frames=frames, **kwargs)
        state._wide = bool(wide)
        torch, f32 = state.torch, dict(dtype=state.torch.float32, device=state.device)
        if _host_gradients:
            state.images = torch.zeros((S, C, H, W), **f32)
            state._fill_struct()
        batches = []
        state._lowres = [None] * len(obs)
        state._lowres_products = bool(lowres_products)
        for i, o in enumerate(obs):
            low = isinstance(o, LowResObservationBatch)
            # (a low-resolution batch lives on its own pixel grid: the model-frame centres mean nothing there)
            ob = cls(o.images, torch.zeros_like(state.centers) if low else state.centers, weights=o.weights, symmetric=False,
                     monotonic=False, mse_capacity=1, centroid_weight=state.centroid_weight.cpu().numpy(), device=state.device,
                     _morph=_host_gradients, frame_shapes=o.frame_shapes)
            if low:
                state._lowres[i] = state._attach_lowres(o, ob)
            elif o.diff_kernel is not None:
                ob.set_diff_kernel(o.diff_kernel)
            batches.append((o, ob))
        state._observations = batches
        return state

    def _init_lowres_sed(self, o, ob, peak, mmax):
        """The SED slice a low-resolution observation contributes to init_combined (get_psf_sed, source.py:41-71): its
        pixel under every present component's centre (the geometry's map, truncated as Frame.get_pixel does), divided by
        the observation's PSF peaks and multiplied by the model PSF's max.  Written to both buffers' channels of the
        scenes init_sources accepted; plain indexing, no kernel."""
        t = self.torch
        pix = o.pixels_of(self.centers).long()
        h, w = o.shape[2:]
        present = self._present() & ((self.status & _lib.STATUS_BAD_INIT) == 0).view(-1, 1)
        hs, ws = h, w
        if o.frame_shapes is not None:             # the scene's own pixels
            own = t.as_tensor(o.frame_shapes).to(device=self.device, dtype=pix.dtype)
            hs, ws = own[:, 0].view(-1, 1), own[:, 1].view(-1, 1)
        bad = present & ((pix[..., 0] < 0) | (pix[..., 0] >= hs) | (pix[..., 1] < 0) | (pix[..., 1] >= ws))
        if bool(bad.any().item()):
            s, k = [int(v[0]) for v in t.nonzero(bad, as_tuple=True)]
            raise ValueError("init_combined: source %d of scene %d lies outside the low-resolution observation" % (k, s))
        pix = pix.clamp(min=0)
        py, px = pix[..., 0].clamp(max=h - 1), pix[..., 1].clamp(max=w - 1)
        sidx = t.arange(self.S, device=self.device).view(-1, 1).expand(self.S, self.K)
        sed = ob.images[sidx, :, py, px]                                  # (S, K, B)
        if peak is not None:
            sed = sed / (peak.view(self.S, 1, o.B) if peak.ndim == 2 else peak.view(1, 1, o.B))
        if mmax is not None:
            sed = sed * mmax
        for b in range(2):
            dst = self.sed[b][:, :, o.band0:o.band0 + o.B]
            dst.copy_(t.where(present.view(self.S, self.K, 1), sed.to(dst.dtype), dst))

    def _refuse_single_init(self):
        if self._observations is not None:
            raise ValueError("a batch of several observations starts its sources with init_combined "
                             "(CombinedExtendedSource), not init_extended / init_sources")

    def _attach_lowres(self, o, ob):
        """(scarlet_lowres with its workspace, what it points to) of the low-resolution observation `o` with gradient
        batch `ob`, sized for this state batch"""
        lr, keep = o.lowres_struct(self.device) if o.dims is None else o.lowres_struct(self.device, (self.H, self.W))
        sizer = _lib.lib.scarlet_lowres_large_workspace_bytes_wide if self._wide else _lib.lib.scarlet_lowres_large_workspace_bytes
        nbytes = _lib.check(sizer(ctypes.byref(self._c), ctypes.byref(ob._c), ctypes.byref(lr)))
        keep["workspace"] = self.torch.empty((int(nbytes),), dtype=self.torch.uint8, device=self.device)
        lr.workspace = keep["workspace"].data_ptr()
        return lr, keep

    def _lowres_frames(self):
        """the array of scarlet_lowres_frames pointers beside `_lowres` (NULL for the same-grid observations)"""
        none = ctypes.POINTER(_lib.ScarletLowresFrames)()
        return (ctypes.POINTER(_lib.ScarletLowresFrames) * len(self._lowres))(
            *[none if x is None or "frames" not in x[1] else ctypes.pointer(x[1]["frames"]) for x in self._lowres])

    def init_combined(self, bg_rms, obs_idx=0, obs_psfs=None, model_psf=None, thresh=1.0, init_monotonic=None):
        """CombinedExtendedSource for every component (reference source.py:183-240, 495-536): the SED is the
        concatenation of every observation's pixel SED (divided by the observation's PSF peak and multiplied by the
        model PSF's max when PSFs are given, get_psf_sed), the morphology the extended start from observation
        `obs_idx` alone with its noise, always symmetric; no update() runs, as in the reference.

        bg_rms : one entry per observation, each (B_o,) or (S, B_o)
        obs_psfs : None, or one entry per observation: None, (B_o, P, P) or (S, B_o, P, P)
        model_psf : None or (P, P), P odd
        The observations' channel slices must tile 0 .. C - 1 in order (the reference's concatenation).  A scene
        whose bg_rms row of observation obs_idx has a value <= 0 gets STATUS_BAD_INIT and stays inactive.
        Where the observations carry frame shapes, every scene starts on its own frame (scarlet_init_sources_frames)."""
        if getattr(self, "frame_shapes", None) is not None and self._observations is None:
            raise NotImplementedError("init_combined on a ragged-frame batch (frame_shapes) that was not made by from_observations")
        if self._observations is None:
            raise ValueError("init_combined needs a batch made by BlendBatch.from_observations")
        t, obs = self.torch, self._observations
        n = len(obs)
        end = 0
        for o, _ in obs:
            if o.band0 != end:
                raise ValueError("init_combined: the observations' channels must tile 0 .. %d in order (observation "
                                 "at band0 = %d, expected %d)" % (self.B - 1, o.band0, end))
            end += o.B
        if end != self.B:
            raise ValueError("init_combined: the observations cover %d of the %d model channels" % (end, self.B))
        if not 0 <= int(obs_idx) < n:
            raise ValueError("init_combined: obs_idx = %d, there are %d observations" % (obs_idx, n))
        obs_idx = int(obs_idx)
        if isinstance(obs[obs_idx][0], LowResObservationBatch):
            raise ValueError("init_combined: obs_idx = %d names a low-resolution observation; the morphology starts from "
                             "an observation on the model's pixel grid" % obs_idx)
        if len(bg_rms) != n:
            raise ValueError("init_combined: one bg_rms per observation (%d), not %d" % (n, len(bg_rms)))
        if obs_psfs is not None and len(obs_psfs) != n:
            raise ValueError("init_combined: one obs_psfs entry per observation (%d), not %d" % (n, len(obs_psfs)))
        keep = []

        def dev(a):
            x = (a if t.is_tensor(a) else t.as_tensor(np.asarray(a))).to(device=self.device, dtype=t.float32).contiguous()
            keep.append(x)
            return x

        peaks = []
        for i, (o, _) in enumerate(obs):
            bg = np.shape(bg_rms[i])
            if tuple(bg) not in ((o.B,), (self.S, o.B)) and not (isinstance(o, LowResObservationBatch) and bg_rms[i] is None):
                raise ValueError("init_combined: bg_rms[%d] must be (%d,) or (%d, %d), not %s" % (i, o.B, self.S, o.B, tuple(bg)))
            p = None if obs_psfs is None else obs_psfs[i]
            if p is not None:
                _check_obs_psfs(p, self.S, o.B, "init_combined: obs_psfs[%d]" % i,
                                "(%d, P, P) or (%d, %d, P, P)" % (o.B, self.S, o.B))
                p = dev(p).amax(dim=(-2, -1)).contiguous()
                keep.append(p)
            peaks.append(p)
        mmax = None
        if model_psf is not None:
            mp = np.asarray(model_psf.cpu() if t.is_tensor(model_psf) else model_psf)
            _check_model_psf(mp, "init_combined: model_psf")
            mmax = dev(mp).amax().reshape(1).contiguous()
            keep.append(mmax)
        # the morphology: the extended start on observation obs_idx, written straight into the state's current buffers
        # (the observation batch's SEDs receive its own band slice, which the SED kernel below replaces)
        o, ob = obs[obs_idx]
        c = ob._c
        c.morph[0], c.morph[1] = self.morph[0].data_ptr(), self.morph[1].data_ptr()
        c.cur, c.flags, c.status, c.active = self.cur.data_ptr(), self.flags.data_ptr(), self.status.data_ptr(), self.active.data_ptr()
        c.n_components = None if self.n_components is None else self.n_components.data_ptr()
        c.centers = self.centers.data_ptr()
        try:
            ob.init_sources( bg_rms[obs_idx], obs_psfs=None if obs_psfs is None else obs_psfs[obs_idx],
                                    model_psf=model_psf, thresh=thresh, init_symmetric=True,
                                    init_monotonic=self.monotonic if init_monotonic is None else init_monotonic,
                                    run_update=False)
        finally:
            ob._fill_struct()
        for i, (o, ob) in enumerate(obs):
            p = peaks[i]
            if isinstance(o, LowResObservationBatch):
                self._init_lowres_sed(o, ob, p, mmax)
                continue
            combined_sed = _lib.lib.scarlet_init_combined_sed_wide if self._wide else _lib.lib.scarlet_init_combined_sed
            _lib.check(combined_sed(
                ctypes.byref(self._c), ob.images.data_ptr(), int(o.B), int(o.band0), None if p is None else p.data_ptr(),
                int(p is not None and p.ndim == 2), None if mmax is None else mmax.data_ptr(), _lib.stream_ptr()))
        self._init_checked = True
        return self
