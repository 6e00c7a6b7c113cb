"""-m gpu: frames with a side over 256 px, up to SCARLET_MAX_SIDE = 1024 (square or not), in the batched engine, in
init_extended and in the standalone operators.  Before, every one of these shapes was refused with ValueError.

Engine runs follow tests/parity_common.py: the CPU oracle starts from the device's own initial state; sed / morph /
loss history <= 1e-5 max-norm relative, centres and iteration counts bit-exact, at most one scene per test through
the float64-anchored threshold exemption (logged).  Paths covered: the streamed box kernels (boxupdate.h, NB = 0),
the full-frame kernel in HBM (k_source_update<2>) for footprints that leave the 127 x 127 box and for
monotonic=False, the K > 8 gradient kernels, the hipFFT PSF chain, init_extended's float64 tile in HBM and
k_operator<true>.
"""
import ctypes
import multiprocessing as mp
import os

import numpy as np
import pytest

from conftest import rel_err
import parity_common as pc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
TOL = pc.TOL


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
    (5, 384, 384, 8, 2, 20, False, None, 7100),         # square: streamed box kernels + k_grad / k_step
    (5, 200, 520, 6, 2, 15, False, None, 7110),         # W > 256 with H <= 256
    (5, 520, 200, 6, 2, 15, False, None, 7120),         # H > 256 with W <= 256
    (6, 512, 512, 30, 2, 10, False, 0.05, 7130),        # K > 8 (k_bigk_*) + L0 + box kernels
    (5, 320, 320, 4, 2, 10, True, None, 7140),          # PSF: hipFFT chain
    (5, 300, 301, 4, 1, 10, True, None, 7150),          # PSF, odd width
])
def test_large_frames_fixed_iterations_vs_oracle(env, B, H, W, K, S, iters, psf, l0, first):
    scarlet, pool = env
    wl = pc.Workload(B=B, H=H, W=W, K=K, psf=psf, l0=l0)
    images, centers = wl.scenes(first, S)
    pc.check_fixed_iterations(scarlet, wl, images, centers, pool, iters, 1,
                              "large frames %dx%dx%d K=%d psf=%s l0=%s" % (B, H, W, K, psf, l0))


def test_large_frame_converged_run_vs_oracle(env):
    """one 384 x 384 scene to e_rel = 1e-3: the iteration count equals the oracle's"""
    scarlet, pool = env
    wl = pc.Workload(B=5, H=384, W=384, K=8)
    images, centers = wl.scenes(7160, 1)
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


def wide_scene(seed, B=5, H=384, W=384, K=3, sigma=45.0):
    """sources far wider than the 127 x 127 box; returns images, centres, and the true SEDs and morphologies"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[:H, :W].astype(np.float64)
    centers = np.array([[H // 2 + rng.randint(-60, 60), W // 2 + rng.randint(-60, 60)] for _ in range(K)], np.int32)
    morphs = np.array([np.exp(-0.5 * ((yy - cy) ** 2 + (xx - cx) ** 2) / sigma ** 2) for cy, cx in centers])
    seds = np.array([np.exp(rng.uniform(np.log(20.), np.log(60.))) * rng.uniform(0.3, 1.0, B) for _ in range(K)])
    model = np.einsum("kb,kyx->byx", seds, morphs)
    return ((model + rng.normal(0, 0.1, model.shape)).astype(np.float32), centers, seds.astype(np.float32),
            morphs.astype(np.float32))


def wide_state(scarlet, images, centers, seds, morphs, monotonic, mse_capacity):
    """a batch started from the given (true) factors; centres and shifts from init_extended"""
    b = scarlet.BlendBatch(images, centers, monotonic=monotonic, mse_capacity=mse_capacity)
    b.init_extended(np.ones(images.shape[1]) * 0.1)
    b.set_state(seds, morphs)
    return b


def oracle_from_state(images, st, iters, dt, monotonic, trace=False):
    """oracle fit of one scene from a device state; with `trace`: per iteration (morph after it, (stepped morph,
    morph before prox_plus)), as parity_common.oracle_trace, for a pipeline with or without monotonicity"""
    from oracle import pgm
    sc = pgm.scene_from_state(images.astype(dt), st[0].astype(dt), st[1].astype(dt), st[2], st[3])
    for src in sc.sources:
        src.monotonic = monotonic
        if trace:
            src.trace = dict(step=[], pre_plus=[])
    post = []
    pgm.fit(sc, iters, e_rel=0, callback=(lambda scn: post.append(np.array([x.morph.copy() for x in scn.sources])))
            if trace else None)
    if not trace:
        return sc
    pre = [(np.array([x.trace["step"][t] for x in sc.sources]), np.array([x.trace["pre_plus"][t] for x in sc.sources]))
           for t in range(iters)]
    return sc, post, pre


def straddles_threshold_from_state(scarlet, images, centers, seds, morphs, iters, monotonic):
    """parity_common.straddles_threshold for ONE scene started from given factors: re-run iteration by iteration on
    the GPU and in the float32 / float64 oracles; accepted only if the GPU and the float32 oracle agree within 1e-5
    until an iteration t0 at which they disagree about the support of the morphology in a pixel whose float64 value
    at one of the two threshold tests lies within 1e-5 x max|morph| of 0.  Returns (ok, message)."""
    b = wide_state(scarlet, images[None], centers[None], seds[None], morphs[None], monotonic, iters + 1)
    st = [t.cpu().numpy()[0] for t in (b.sed_current, b.morph_current, b.centers, b.shifts)]
    snaps = []
    for _ in range(iters):
        b.fit(1, e_rel=0)
        snaps.append(b.morph_current.cpu().numpy()[0].copy())
    _, o32, _ = oracle_from_state(images, st, iters, np.float32, monotonic, trace=True)
    _, o64, pre64 = oracle_from_state(images, st, iters, np.float64, monotonic, trace=True)
    for t in range(iters):
        gm = snaps[t]
        mismatch = (gm == 0) != (o32[t] == 0)
        if mismatch.any():
            scale = np.abs(o64[t]).max()
            near = np.minimum(np.abs(pre64[t][0][mismatch]), np.abs(pre64[t][1][mismatch]))
            on_threshold = near <= TOL * scale
            if on_threshold.any():
                k, y, x = (int(v[np.argmax(on_threshold)]) for v in np.nonzero(mismatch))
                return True, ("iteration %d, component %d pixel (%d, %d): float64 values at the threshold tests: stepped "
                              "%.3e, before prox_plus %.3e (tolerance 1e-5 x %.3g); gpu %.3e, float32 oracle %.3e" % (
                                  t + 1, k, y, x, pre64[t][0][k, y, x], pre64[t][1][k, y, x], scale, gm[k, y, x],
                                  o32[t][k, y, x]))
        if rel_err(gm, o32[t]) > TOL:
            return False, "iteration %d: gpu and float32 oracle differ by %.2e with no pixel on a threshold" % (
                t + 1, rel_err(gm, o32[t]))
    return False, "no divergence found when re-running the scene alone"


@pytest.mark.parametrize("monotonic", [True, False])
def test_full_frame_kernel_on_large_frames_vs_oracle(env, monotonic):
    """MODE 2 reached: the fit starts from the true, 384-pixel-wide profiles, so every monotonic envelope leaves the
    127 x 127 box and the full-frame kernel (k_source_update<2>) takes the component; monotonic=False sends every
    component there.  Against the float32 oracle as check_fixed_iterations does: sed / morph / loss <= 1e-5, centres,
    iteration counts and flags bit-exact, at most one scene through the float64-anchored threshold exemption."""
    scarlet, pool = env
    iters = 8
    ims, cens, seds, morphs = (np.stack(a) for a in zip(*[wide_scene(7170 + i) for i in range(2)]))
    b = wide_state(scarlet, ims, cens, seds, morphs, monotonic, iters + 1)
    st0 = [t.cpu().numpy() for t in (b.sed_current, b.morph_current, b.centers, b.shifts)]
    b.fit(iters, e_rel=0)
    torch.cuda.synchronize()
    assert int(b.status.abs().sum().item()) == 0
    assert (b.it.cpu().numpy() == iters).all()
    morph = b.morph_current.cpu().numpy()
    # rows with more than 127 non-zero pixels: output the box kernels cannot write
    assert (np.count_nonzero(morph > 0, axis=-1) > 127).any()
    exempt = []
    for i in range(len(ims)):
        o32 = oracle_from_state(ims[i], [a[i] for a in st0], iters, np.float32, monotonic)
        np.testing.assert_array_equal(b.centers[i].cpu().numpy(), np.array([s.center for s in o32.sources]))
        np.testing.assert_array_equal(b.flags[i].cpu().numpy(), np.array([int(s.flags) for s in o32.sources]))
        e = dict(sed=rel_err(b.sed_current[i].cpu().numpy(), np.array([s.sed for s in o32.sources])),
                 morph=rel_err(morph[i], np.array([s.morph for s in o32.sources])),
                 mse=rel_err(b.mse_buf[i].cpu().numpy()[:iters], np.array(o32.mse)))
        if max(e.values()) <= TOL:
            continue
        ok, msg = straddles_threshold_from_state(scarlet, ims[i], cens[i], seds[i], morphs[i], iters, monotonic)
        assert ok, "scene %d beyond 1e-5 (%s) and not a threshold straddle: %s" % (i, e, msg)
        exempt.append((i, e, msg))
    pc.log_exemptions("full-frame kernel 384x384 monotonic=%s" % monotonic, exempt, 1)
    assert len(exempt) <= 1, exempt


# ------------------------------------------------------------------ 32-bit index overflow
def test_no_index_overflow_at_1024(env):
    """2 distinct 6 x 1024 x 1024 scenes, K = 30, tiled to 72: S K H W > 2^31 floats per morphology buffer.  Two
    iterations; every copy bit-identical to the 2-scene run."""
    scarlet, _ = env
    from scarlet_amd import synth
    B, H, W, K, U, S, iters = 6, 1024, 1024, 30, 2, 72, 2
    assert S * K * H * W > 2 ** 31
    scenes = [synth.make_scene(7180 + i, B=B, H=H, W=W, K=K) for i in range(U)]
    images = torch.as_tensor(np.stack([s["images"] for s in scenes])).cuda()
    centers = torch.as_tensor(np.stack([s["centers"] for s in scenes])).cuda()
    small = scarlet.BlendBatch(images, centers, l0_thresh=0.05, mse_capacity=iters + 1)
    small.init_extended(np.ones(B) * 0.1)
    small.fit(iters, e_rel=0)
    torch.cuda.synchronize()
    assert int(small.status.abs().sum().item()) == 0
    big = scarlet.BlendBatch(images.repeat(S // U, 1, 1, 1), centers.repeat(S // U, 1, 1), l0_thresh=0.05,
                             mse_capacity=iters + 1)
    big.init_extended(np.ones(B) * 0.1)
    big.fit(iters, e_rel=0)
    torch.cuda.synchronize()
    assert int(big.status.abs().sum().item()) == 0
    for c in range(S):
        u = c % U
        assert torch.equal(big.morph_current[c], small.morph_current[u]), c
        assert torch.equal(big.sed_current[c], small.sed_current[u]), c
        assert torch.equal(big.centers[c], small.centers[u]), c
        assert torch.equal(big.mse_buf[c, :iters], small.mse_buf[u, :iters]), c
        assert int(big.it[c]) == int(small.it[u]) == iters


# ------------------------------------------------------------------ standalone operators vs oracle
def dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype).contiguous()


def run_op(L, name, x, centers, *args):
    xs = dev(x, torch.float32)
    cs = dev(np.asarray(centers).reshape(-1, 2), torch.int32)
    n, H, W = xs.shape
    L.check(getattr(L.lib, name)(L.ptr(xs), n, H, W, L.ptr(cs), *args, L.stream_ptr()))
    torch.cuda.synchronize()
    return xs.cpu().numpy()


def sym(L, X, c, shift, alg, strength=.5):
    xs = dev(np.asarray(X)[None], torch.float32)
    cs = dev(np.asarray(c).reshape(1, 2), torch.int32)
    sh = None if shift is None else dev(np.asarray(shift, dtype=np.float64).reshape(1, 2), torch.float64)
    H, W = xs.shape[1:]
    L.check(L.lib.scarlet_prox_symmetry(L.ptr(xs), 1, H, W, L.ptr(cs), L.ptr(sh), alg, ctypes.c_float(strength), 0,
                                        ctypes.c_float(0.0), L.stream_ptr()))
    torch.cuda.synchronize()
    return xs.cpu().numpy()[0]


@pytest.mark.parametrize("shape", [(300, 700), (1024, 1024)])
def test_operators_on_large_arrays_vs_oracle(env, shape):
    scarlet, _ = env
    L = scarlet._lib
    from oracle import pgm
    rng = np.random.RandomState(shape[1])
    H, W = shape
    yy, xx = np.mgrid[:H, :W]
    for c in ((H // 2 + 3, W // 2 - 5), (5, 7), (H - 6, W - 9), (H - 4, 3)):
        X = (np.exp(-((yy - c[0]) ** 2 + (xx - c[1]) ** 2) / 300.) + .02 * rng.randn(H, W)).astype(np.float32)
        # radial monotonicity: weighted (thresh 0 and 0.1) and strict (nearest neighbour)
        for th in (0.0, 0.1):
            Y = run_op(L, "scarlet_prox_weighted_monotonic", X[None], [c], ctypes.c_float(th))[0]
            ref = X.astype(np.float64).copy()
            pgm.prox_weighted_monotonic(ref, c, thresh=th)
            assert rel_err(Y, ref) <= TOL, (shape, c, th)
        Y = run_op(L, "scarlet_prox_nearest_monotonic", X[None], [c], ctypes.c_float(0.0))[0]
        ref = X.astype(np.float64).copy()
        pgm.prox_nearest_monotonic(ref, c)
        assert rel_err(Y, ref) <= TOL, (shape, c, "nearest")
        # prox_uncentered_symmetry: kspace (with a shift), soft, sdss; the window (the untouched pixels outside it)
        # is bit-exact
        sh = tuple(rng.uniform(-.5, .5, 2))
        for name, alg, shift in (("kspace", L.SYM_KSPACE, sh), ("soft", L.SYM_SOFT, None), ("sdss", L.SYM_SDSS, None)):
            Y = sym(L, X, c, shift, alg)
            ref = X.astype(np.float64)
            pgm.prox_symmetry(ref, c, name, None, shift, .5)
            win = pgm.symmetric_window(X.shape, c)
            outside = np.ones(X.shape, bool)
            outside[win] = False
            np.testing.assert_array_equal(Y[outside], X[outside])
            assert rel_err(Y, ref) <= TOL, (shape, c, name)
    # prox_kspace_symmetry on the whole array (padding 10)
    # (an even side whose FFT length next_fast_len(2 N + 10) is odd -- N = 300: 625 -- is outside the closed form of
    # prox_ops.h at every size: test_whole_array_kspace_symmetry_even_side_odd_fft_length; the non-square case takes
    # 301 rows)
    if H == 300:
        H = 301
    yy, xx = np.mgrid[:H, :W]
    X = (np.exp(-((yy - H // 2) ** 2 + (xx - W // 2) ** 2) / 500.) + .02 * rng.randn(H, W)).astype(np.float32)
    sh = (0.3, -0.2)
    Y = sym(L, X, (H // 2, W // 2), sh, L.SYM_KSPACE | L.SYM_FULL_WINDOW)
    ref = pgm.kspace_symmetry(X.astype(np.float64), sh)
    assert rel_err(Y, ref) <= TOL


@pytest.mark.xfail(strict=True, reason="known defect, independent of the frame size: the closed form of prox_ops.h "
                   "(kspace_vectors) does not reproduce the reference's rfft/irfft for an EVEN side whose FFT length "
                   "next_fast_len(2 N + 10) is ODD (N = 32: 75, N = 300: 625); the engine never meets it (its windows "
                   "are odd), only the whole-array operator does")
def test_whole_array_kspace_symmetry_even_side_odd_fft_length(env):
    scarlet, _ = env
    L = scarlet._lib
    from oracle import pgm
    H, W = 32, 40
    assert pgm.next_fast_len(2 * H + 10) % 2 == 1
    rng = np.random.RandomState(1)
    yy, xx = np.mgrid[:H, :W]
    X = (np.exp(-((yy - H // 2) ** 2 + (xx - W // 2) ** 2) / 50.) + .02 * rng.randn(H, W)).astype(np.float32)
    Y = sym(L, X, (H // 2, W // 2), (0.3, -0.2), L.SYM_KSPACE | L.SYM_FULL_WINDOW)
    assert rel_err(Y, pgm.kspace_symmetry(X.astype(np.float64), (0.3, -0.2))) <= TOL


def test_init_extended_600_vs_oracle(env):
    scarlet, _ = env
    from oracle import pgm
    from scarlet_amd import synth
    B, H, W, K = 5, 600, 600, 6
    sc = synth.make_scene(7190, B=B, H=H, W=W, K=K)
    b = scarlet.BlendBatch(sc["images"][None], sc["centers"][None])
    b.init_extended(np.ones(B) * 0.1, run_update=False)
    torch.cuda.synchronize()
    sed, morph = b.sed_current.cpu().numpy()[0], b.morph_current.cpu().numpy()[0]
    for k in range(K):
        rs, rm = pgm.init_extended_source(tuple(sc["centers"][k]), sc["images"], np.ones(B) * 0.1)
        assert rel_err(sed[k], rs) <= TOL, k
        assert rel_err(morph[k], rm) <= TOL, k


def test_frames_over_1024_are_refused(env):
    scarlet, _ = env
    L = scarlet._lib
    images = np.zeros((1, 2, 16, 1025), np.float32)
    with pytest.raises(ValueError, match="1024"):
        b = scarlet.BlendBatch(images, np.array([[[8, 500]]], np.int32))
        b.init_extended(np.ones(2) * 0.1)
    with pytest.raises(ValueError, match="1024"):
        run_op(L, "scarlet_prox_weighted_monotonic", np.zeros((1, 8, 1025), np.float32), [(4, 500)], ctypes.c_float(0.0))
