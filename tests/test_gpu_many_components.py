"""-m gpu: scenes with more than 32 components (up to SCARLET_MAX_COMPONENTS = 256).  Before, every entry point refused
them with NotImplementedError.

Engine runs follow tests/parity_common.py: the CPU oracle starts from the device's own initial state; sed / morph /
loss history <= 1e-5 max-norm relative, centres and iteration counts bit-exact, at most one scene per test through the
float64-anchored threshold exemption (logged).  Paths covered: the gradient step of hugek.h (float64 Gram on the matrix
cores, lambda_max by repeated squaring) without a PSF, with the LDS-resident and the hipFFT PSF convolution, per-pixel
weights, L0, approximate Lipschitz constants, grouped sources, the single-scene Blend, and a 1024^2 scene at K = 256.
"""
import multiprocessing as mp
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import rel_err
import parity_common as pc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
TOL = pc.TOL
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def env():
    import scarlet_amd
    scarlet_amd._lib.require_gpu()
    from oracle import build as obuild
    obuild.build()
    pool = mp.get_context("spawn").Pool(min(16, os.cpu_count() or 1))
    yield scarlet_amd, pool
    pool.close(); pool.join()


# ------------------------------------------------------------------ engine vs oracle, fixed iterations
@pytest.mark.parametrize("B,H,W,K,S,iters,psf,l0,first", [
    (5, 64, 64, 40, 2, 10, False, None, 8100),
    (5, 128, 128, 40, 2, 10, False, None, 8110),
    (6, 256, 256, 64, 1, 8, False, 0.05, 8120),         # L0
    (6, 512, 512, 128, 1, 5, False, None, 8130),
    (6, 256, 256, 256, 1, 4, False, None, 8140),        # 256 peaks at min_sep 4
    (5, 128, 128, 48, 2, 8, True, None, 8150),          # PSF: LDS-resident convolution
    (5, 320, 320, 48, 1, 5, True, None, 8160),          # PSF: hipFFT chain
])
def test_many_components_fixed_iterations_vs_oracle(env, B, H, W, K, S, iters, psf, l0, first):
    scarlet, pool = env
    wl = pc.Workload(B=B, H=H, W=W, K=K, psf=psf, l0=l0)
    images, centers = wl.scenes(first, S)
    pc.check_fixed_iterations(scarlet, wl, images, centers, pool, iters, 1,
                              "many components %dx%dx%d K=%d psf=%s l0=%s" % (B, H, W, K, psf, l0))


def _oracle_from_state(args):
    """worker: oracle fit with per-pixel weights and / or approximate Lipschitz constants"""
    from oracle import pgm
    images, sed0, morph0, cen0, sh0, weights, iters, approx = args
    sc = pgm.scene_from_state(images, sed0, morph0, cen0, sh0, weights=1 if weights is None else weights)
    pgm.fit(sc, iters, e_rel=0, approximate_L=approx)
    return (np.array([s.sed for s in sc.sources]), np.array([s.morph for s in sc.sources]), np.array(sc.mse),
            np.array([s.center for s in sc.sources]))


@pytest.mark.parametrize("weighted,approx", [(True, False), (False, True)])
def test_weights_and_approximate_L_vs_oracle(env, weighted, approx):
    """K = 64 on 128^2: per-pixel weights (zeros = masked pixels), and approximate_L (trace of the Gram, doubled when
    the loss rose)"""
    scarlet, pool = env
    from scarlet_amd import synth
    B, H, W, K, S, iters = 5, 128, 128, 64, 2, 8
    scenes = [synth.make_scene(8200 + 10 * approx + i, B=B, H=H, W=W, K=K) for i in range(S)]
    images = np.stack([s["images"] for s in scenes])
    weights = None
    if weighted:
        rng = np.random.RandomState(5)
        weights = rng.uniform(0.5, 1.5, size=images.shape).astype(np.float32)
        weights[rng.rand(*images.shape) < 0.03] = 0
    b = scarlet.BlendBatch(images, np.stack([s["centers"] for s in scenes]), weights=weights, mse_capacity=iters + 1)
    b.init_extended(np.ones(B) * 0.1)
    st0 = [t.cpu().numpy() for t in (b.sed_current, b.morph_current, b.centers, b.shifts)]
    b.fit(iters, e_rel=0, approximate_L=approx)
    torch.cuda.synchronize()
    assert int(b.status.abs().sum().item()) == 0
    ref = pool.map(_oracle_from_state, [(images[i], st0[0][i], st0[1][i], st0[2][i], st0[3][i],
                                         None if weights is None else weights[i], iters, approx) for i in range(S)])
    for i in range(S):
        np.testing.assert_array_equal(b.centers[i].cpu().numpy(), ref[i][3])
        assert rel_err(b.sed_current[i].cpu().numpy(), ref[i][0]) <= TOL
        assert rel_err(b.morph_current[i].cpu().numpy(), ref[i][1]) <= TOL
        assert rel_err(b.mse(i), ref[i][2]) <= TOL


def test_many_components_converged_run_vs_oracle(env):
    """K = 64 on 128^2 to e_rel = 1e-3 (a scene the oracle takes about 100 iterations for): the iteration count equals
    the oracle's and is below max_iter"""
    scarlet, pool = env
    wl = pc.Workload(B=5, H=128, W=128, K=64)
    images, centers = wl.scenes(8302, 1)
    st0, g = pc.gpu_fit(scarlet, wl, images, centers, 200, 1e-3)
    ref = pool.map(pc.oracle_fit, [(images[0], st0[0][0], st0[1][0], st0[2][0], st0[3][0], 200, 1e-3, np.float32,
                                    wl.oracle_kwargs())])[0]
    assert int(np.abs(g["status"]).sum()) == 0
    assert int(g["it"][0]) == ref[4] < 200
    np.testing.assert_array_equal(g["cen"][0], ref[3])
    np.testing.assert_array_equal(g["flags"][0], ref[5])
    assert rel_err(g["sed"][0], ref[0]) <= TOL
    assert rel_err(g["morph"][0], ref[1]) <= TOL
    assert rel_err(g["mse"][0][:ref[4]], ref[2]) <= TOL


# ------------------------------------------------------------------ the Lipschitz constant of the SED step
def identical_sources(K, H, B=5, sigma=2.0):
    """K identical, noise-free Gaussian sources on a grid with no overlap: a Gram matrix with a K-fold top eigenvalue"""
    n = int(np.ceil(np.sqrt(K)))
    step = H // n
    yy, xx = np.mgrid[:H, :H].astype(np.float64)
    centers = np.array([[step // 2 + step * (k // n), step // 2 + step * (k % n)] for k in range(K)], np.int32)
    sed = np.linspace(1.0, 2.0, B) * 30
    model = sum(np.exp(-0.5 * ((yy - cy) ** 2 + (xx - cx) ** 2) / sigma ** 2) for cy, cx in centers)
    return (sed[:, None, None] * model[None]).astype(np.float32)[None], centers[None]


@pytest.mark.parametrize("K,H,kind", [(64, 128, "synth"), (128, 256, "synth"), (256, 256, "synth"),
                                      (64, 256, "identical"), (256, 512, "identical")])
def test_lipschitz_equals_eigvalsh_of_the_device_gram(env, K, H, kind):
    """after one step, lipschitz[:, 0] = lambda_max of the float64 Gram of the morphologies the step started from, to
    1e-7 relative; also for a degenerate top eigenvalue (identical isolated sources)"""
    scarlet, _ = env
    from scarlet_amd import synth
    if kind == "synth":
        scenes = [synth.make_scene(8400 + K + i, B=6, H=H, W=H, K=K) for i in range(2)]
        images, centers = np.stack([s["images"] for s in scenes]), np.stack([s["centers"] for s in scenes])
    else:
        images, centers = identical_sources(K, H)
    b = scarlet.BlendBatch(images, centers, mse_capacity=4)
    b.init_extended(np.ones(images.shape[1]) * 0.1)
    morph0 = b.morph_current.cpu().numpy().astype(np.float64)
    b.step(e_rel=0)
    torch.cuda.synchronize()
    L = b.lipschitz[:, 0].cpu().numpy()
    for s in range(len(images)):
        M = morph0[s].reshape(K, -1)
        ev = np.linalg.eigvalsh(M @ M.T)
        if kind == "identical":
            assert ev[-1] - ev[-2] <= 1e-12 * ev[-1]          # the top eigenvalue is degenerate
        assert abs(L[s] - ev[-1]) <= 1e-7 * ev[-1], (s, L[s], ev[-1])


# ------------------------------------------------------------------ grouped sources, single-scene Blend
def test_grouped_sources_device_pipeline(env):
    """40 two-layer MultiComponentSources (K = 80) through the device pipeline against the Python pipeline"""
    scarlet, _ = env
    from scarlet_amd import synth
    scn = synth.make_scene(8500, B=5, H=192, W=192, K=40, min_sep=12)
    images = scn["images"]
    frame = scarlet.Frame(images.shape)
    obs = scarlet.Observation(images).match(frame)
    bg = np.ones(5) * 0.1
    cen = [tuple(int(v) for v in p) for p in scn["centers"]]

    def make(py):
        srcs = [scarlet.MultiComponentSource(frame, c, obs, bg, flux_percentiles=[30]) for c in cen]
        bl = scarlet.Blend(srcs, obs)
        bl.python_pipeline = py
        return bl
    bd, bp = make(False), make(True)
    assert len(bd.components) == 80 and bd._builtin_pipeline() and not bp._builtin_pipeline()
    bd.fit(6, e_rel=0); bp.fit(6, e_rel=0)
    npy = lambda t: t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    assert rel_err(bd.mse, bp.mse) <= TOL
    assert rel_err(np.array([npy(c.morph) for c in bd.components]), np.array([npy(c.morph) for c in bp.components])) <= TOL
    assert rel_err(np.array([npy(c.sed) for c in bd.components]), np.array([npy(c.sed) for c in bp.components])) <= TOL


def test_single_scene_blend_with_40_sources_equals_batch(env):
    """scarlet.Blend with 40 ExtendedSources fits without raising, and equals the BlendBatch run of the same scene"""
    scarlet, _ = env
    from scarlet_amd import synth
    scn = synth.make_scene(8600, B=5, H=96, W=96, K=40)
    images = scn["images"]
    frame = scarlet.Frame(images.shape)
    obs = scarlet.Observation(images).match(frame)
    bg = np.ones(5) * 0.1
    srcs = [scarlet.ExtendedSource(frame, tuple(int(v) for v in p), obs, bg) for p in scn["centers"]]
    blend = scarlet.Blend(srcs, obs)
    blend.fit(10, e_rel=0)
    b = scarlet.BlendBatch(images[None], scn["centers"][None], mse_capacity=11)
    b.init_extended(bg)
    b.fit(10, e_rel=0)
    torch.cuda.synchronize()
    npy = lambda t: t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    assert rel_err(np.array([npy(c.morph) for c in blend.components]), b.morph_current[0].cpu().numpy()) <= TOL
    assert rel_err(np.array([npy(c.sed) for c in blend.components]), b.sed_current[0].cpu().numpy()) <= TOL
    assert rel_err(np.asarray(blend.mse), b.mse(0)) <= TOL


# ------------------------------------------------------------------ K <= 32 is unchanged
CHILD = """
import sys, numpy as np, torch
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import scarlet_amd as scarlet
import parity_common as pc
K, psf, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
wl = pc.Workload(B=5, H=64, W=64, K=K, psf=bool(psf), min_sep=3)
images, centers = wl.scenes(8700 + K, 3)
b = wl.batch(scarlet, images, centers, 9)
b.fit(8, e_rel=0)
torch.cuda.synchronize()
np.savez(out, sed=b.sed_current.cpu().numpy(), morph=b.morph_current.cpu().numpy(), mse=b.mse_buf.cpu().numpy(),
         cen=b.centers.cpu().numpy(), lip=b.lipschitz.cpu().numpy())
""" % (ROOT, os.path.join(ROOT, "tests"))


def _child_run(tmp_path, K, psf, force):
    out = str(tmp_path / ("k%d_p%d_f%s.npz" % (K, psf, force)))
    env = dict(os.environ)
    env.pop("SCARLET_FORCE_HUGEK", None)
    if force is not None:
        env["SCARLET_FORCE_HUGEK"] = str(force)
    r = subprocess.run([sys.executable, "-c", CHILD, str(K), str(psf), out], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return dict(np.load(out))


@pytest.mark.parametrize("K", [30, 32])
def test_k_up_to_32_unchanged(env, tmp_path, K):
    """K = 30 and 32 take the kernels they always took: a default run and a run with the hugek.h switch explicitly
    off are bit-identical.  With FORCE_HUGEK = 1 the same K = 30 / 32 scenes run the gradient step of hugek.h
    instead (with and without a PSF): within 1e-5 of the K <= 32 kernels"""
    for psf in (0, 1):
        a, off = _child_run(tmp_path, K, psf, None), _child_run(tmp_path, K, psf, 0)
        for k in a:
            np.testing.assert_array_equal(a[k], off[k])
        f = _child_run(tmp_path, K, psf, 1)
        np.testing.assert_array_equal(a["cen"], f["cen"])
        for k in ("sed", "morph", "mse", "lip"):
            assert rel_err(f[k], a[k]) <= TOL, (k, psf, rel_err(f[k], a[k]))


# ------------------------------------------------------------------ 1024^2 at K = 256
def test_1024_frame_at_256_components(env):
    """one tiled 1024^2 scene with 256 components (2 x 1 GB of morphologies): two iterations, finite, status 0"""
    scarlet, _ = env
    from scarlet_amd import synth
    tile = synth.make_scene(8800, B=5, H=256, W=256, K=16, min_sep=12)
    images = np.tile(tile["images"], (1, 4, 4))
    centers = np.concatenate([tile["centers"] + np.array([256 * (j // 4), 256 * (j % 4)], np.int32) for j in range(16)])
    b = scarlet.BlendBatch(images[None], centers[None], mse_capacity=3)
    b.init_extended(np.ones(5) * 0.1)
    assert b.fit(2, e_rel=0, check_every=0) == 2
    torch.cuda.synchronize()
    assert int(b.status.abs().sum().item()) == 0
    assert int(b.it[0].item()) == 2
    assert torch.isfinite(b.morph_current).all() and torch.isfinite(b.sed_current).all()
    assert np.isfinite(b.lipschitz.cpu().numpy()).all() and np.isfinite(b.mse(0)).all()
