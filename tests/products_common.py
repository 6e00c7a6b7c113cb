"""Shared by the products tests (tests/test_gpu_products.py): the float64 statement of what BlendBatch.products returns
-- oracle.pgm.scene_model / render on the state read back from the device, the reference's get_flux / get_loss formulas
(component.py:172-175, observation.py:222-239) -- and the comparison: the project's 1e-5 max-norm relative per scene and
per array (tests/parity_common.py), every element counted."""
import numpy as np

from conftest import rel_err
from oracle import pgm
from parity_common import TOL


# test_scenes_on_different_buffers: first scene of the eight (synth.make_scene seeds) and the e_rel at which they stop after
# different numbers of iterations, some on buffer 0 and some on buffer 1 (without PSF, with PSF, two observations)
MIXED_SEED = {False: 500, True: 600, "obs": 700}
MIXED_E_REL = 1e-2


def npy(t):
    return t.detach().cpu().numpy()


def reference(sed, morph, images, weights=1.0, diff=None):
    """float64 products of ONE scene: sed (K, B), morph (K, H, W), images / weights (B, H, W) (weights may be a scalar),
    diff None or (B, P, P).  Absent components are rows of zeros."""
    sed, morph = np.asarray(sed, np.float64), np.asarray(morph, np.float64)
    images = np.asarray(images, np.float64)
    model = pgm.scene_model(sed, morph, images.shape, np.float64)
    # (the kernel as the device holds it: float32)
    rendered = pgm.render(model, None if diff is None else np.asarray(diff, np.float32).astype(np.float64))
    d = np.asarray(weights, np.float64) * (rendered - images)
    return dict(model=model, rendered=rendered, residual=images - rendered, loss=0.5 * (d ** 2).sum(axis=(1, 2)),
                flux=morph.sum(axis=(1, 2))[:, None] * sed, component_models=sed[:, :, None, None] * morph[:, None])


def state(b):
    """(sed, morph) of the batch's current buffers, host float32"""
    return npy(b.sed_current), npy(b.morph_current)


def check_scene(got, s, ref, names, components=None, where=""):
    """scene s of the tensors `got` (a BatchProducts, or a dict name -> tensor) against the float64 `ref` of that scene;
    every figure is printed before anything is asserted"""
    worst = {}
    for name in names:
        x = npy((got[name] if isinstance(got, dict) else getattr(got, name))[s])
        want = ref[name][list(components)] if name == "component_models" else ref[name]
        assert x.shape == want.shape, (name, x.shape, want.shape)
        worst[name] = rel_err(x, want)
    print("%s scene %d: %s" % (where, s, {k: "%.2e" % v for k, v in worst.items()}))
    for name, e in worst.items():
        assert e <= TOL, "%s scene %d: %s differs from float64 by %.3e" % (where, s, name, e)
    return worst


def synthetic(seed, S, K, B, H, W, weights=None):
    """random non-negative factors and images near their model: (images, centers, sed, morph), float32 / int32"""
    rng = np.random.default_rng(seed)
    sed = (0.2 + rng.random((S, K, B))).astype(np.float32)
    morph = rng.random((S, K, H, W)).astype(np.float32)
    images = np.einsum("skb,skp->sbp", sed, morph.reshape(S, K, -1)).reshape(S, B, H, W)
    images = (images * (1 + 0.2 * rng.standard_normal(images.shape))).astype(np.float32)
    centers = np.stack([rng.integers(0, H, (S, K)), rng.integers(0, W, (S, K))], axis=-1).astype(np.int32)
    return images, centers, sed, morph


def kernels(seed, shape):
    """random positive difference kernels, each of unit sum: shape (..., P, P)"""
    k = np.random.default_rng(seed).random(shape) + 0.05
    return (k / k.sum(axis=(-2, -1), keepdims=True)).astype(np.float32)
