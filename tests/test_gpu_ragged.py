"""-m gpu: ragged batches -- scenes with different numbers of components in one BlendBatch (n_components).

Scene s uses components 0 .. n[s] - 1; the others are absent: zero in both buffers, flags 0, outside the model, the
constraints and the convergence test.  Checked here:
  1. counts all equal to K give the NULL run bit for bit on every path scarlet_fit can choose;
  2. each scene of a ragged batch matches the oracle run of that scene with its own n[s] sources (tests/parity_common.py
     tolerances, at most one logged threshold-straddle exemption per test);
  3. absent components stay exactly zero, flags 0, centres / shifts as given, and tiled copies of a scene agree bit for
     bit wherever they sit in the batch;
  4. init_extended is per source: present components equal those of a batch built with K = n[s], bit for bit;
  5. counts outside 1..K set SCARLET_STATUS_BAD_COUNT on the device and leave those scenes untouched.
"""
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


def _batch(scarlet, wl, images, centers, n=None, group=None, mse_capacity=64):
    kw = dict(mse_capacity=mse_capacity, l0_thresh=wl.l0, group=group)
    if n is not None:
        kw["n_components"] = n
    if wl.psf:
        kw["centroid_weight"] = wl.model_psf.astype(np.float32)
    b = scarlet.BlendBatch(images, centers, **kw)
    if wl.psf:
        b.set_diff_kernel(wl.diff)
    return b


def _state(b):
    torch.cuda.synchronize()
    return dict(sed=[t.cpu().numpy() for t in b.sed], morph=[t.cpu().numpy() for t in b.morph],
                cur=b.cur.cpu().numpy(), cen=b.centers.cpu().numpy(), shifts=b.shifts.cpu().numpy(),
                flags=b.flags.cpu().numpy(), mse=b.mse_buf.cpu().numpy(), it=b.it.cpu().numpy(),
                status=b.status.cpu().numpy(), active=b.active.cpu().numpy())


def _assert_identical(a, b, what):
    for key in a:
        x, y = a[key], b[key]
        if isinstance(x, list):
            for i in range(len(x)):
                assert np.array_equal(x[i], y[i], equal_nan=True), "%s: %s[%d] differs" % (what, key, i)
        else:
            assert np.array_equal(x, y, equal_nan=True), "%s: %s differs" % (what, key)


def _ragged_scenes(wl, first, counts):
    """S scenes of K = wl.K sources each, images made with n[s] sources only; returns images, (S, K, 2), counts"""
    from scarlet_amd import synth
    imgs, cens = [], []
    kw = dict(B=wl.B, H=wl.H, W=wl.W, min_sep=wl.min_sep)
    if wl.psf:
        kw["psfs"] = wl.obs_psfs
    for i, n in enumerate(counts):
        sc = synth.make_scene(first + i, K=int(n), **kw)
        c = np.zeros((wl.K, 2), np.int32)
        c[:n] = sc["centers"]
        imgs.append(sc["images"]); cens.append(c)
    return np.stack(imgs), np.stack(cens), np.asarray(counts, np.int32)


def _check_absent(st0, st, n, what):
    """absent components: zero in both buffers, flags 0, centres / shifts as given; no scene NONFINITE"""
    from scarlet_amd import _lib
    K = st["flags"].shape[1]
    absent = np.arange(K)[None, :] >= n[:, None]
    for key in ("sed", "morph"):
        for i in range(2):
            assert not np.any(st[key][i][absent]), "%s: absent %s[%d] not zero" % (what, key, i)
    assert not np.any(st["flags"][absent]), what
    assert np.array_equal(st["cen"][absent], st0["cen"][absent]), what
    assert np.array_equal(st["shifts"][absent], st0["shifts"][absent], equal_nan=True), what
    assert not np.any(st["status"] & _lib.STATUS_NONFINITE), what


# ------------------------------------------------------------------ 1. counts == K give the NULL run bit for bit
PATHS = [
    # (id, B, H, W, K, S, iters, psf, grouped)
    ("fit2x", 5, 64, 64, 4, 1600, 6, False, False),
    ("iterate2_generic", 5, 48, 48, 4, 8, 6, False, False),
    ("iterate_b6", 6, 64, 64, 4, 8, 6, False, False),
    ("general_k6", 5, 64, 64, 6, 8, 6, False, False),
    ("bigk12", 5, 64, 64, 12, 4, 5, False, False),
    ("bigk30", 6, 128, 128, 30, 2, 5, False, False),
    ("hugek40", 5, 64, 64, 40, 2, 5, False, False),
    ("psf_lds", 5, 64, 64, 4, 4, 5, True, False),
    ("psf_hipfft", 5, 320, 320, 4, 2, 4, True, False),       # (frames beyond the LDS-resident transform)
    ("box128", 5, 128, 128, 4, 4, 5, False, False),
    ("box256", 6, 256, 256, 8, 2, 5, False, False),
    ("streamed384", 5, 384, 384, 4, 1, 4, False, False),
    ("grouped", 5, 64, 64, 4, 4, 6, False, True),
]


@pytest.mark.parametrize("name,B,H,W,K,S,iters,psf,grouped", PATHS, ids=[p[0] for p in PATHS])
def test_full_counts_bit_identical_to_null(env, name, B, H, W, K, S, iters, psf, grouped):
    scarlet, _ = env
    wl = pc.Workload(B=B, H=H, W=W, K=K, psf=psf)
    distinct = min(S, 16)
    images, centers = wl.scenes(9000 + 37 * len(name), distinct)
    reps = (S + distinct - 1) // distinct
    images, centers = np.tile(images, (reps, 1, 1, 1))[:S], np.tile(centers, (reps, 1, 1))[:S]
    group = None
    if grouped:
        group = np.tile(np.array([[-1, 0, 0, -1]], np.int32), (S, 1))
    out = []
    for n in (None, np.full(S, K, np.int32)):
        b = _batch(scarlet, wl, images, centers, n=n, group=group)
        b.init_extended(np.ones(B) * 0.1, sed_scale=wl.scale)
        b.fit(iters, e_rel=0, check_every=3)
        out.append(_state(b))
        del b
    _assert_identical(out[0], out[1], name)
    assert (out[0]["it"] == iters).all()


# ------------------------------------------------------------------ 2. ragged batch vs the oracle, scene by scene
def _ragged_vs_oracle(scarlet, pool, wl, images, centers, n, iters, e_rel, test, max_exempt=1, distinct=None):
    b = _batch(scarlet, wl, images, centers, n=n, mse_capacity=iters + 1)
    b.init_extended(np.ones(wl.B) * 0.1, sed_scale=wl.scale)
    st0 = _state(b)
    b.fit(iters, e_rel=e_rel, check_every=10)
    st = _state(b)
    _check_absent(st0, st, n, test)
    S = len(images) if distinct is None else distinct
    pick = lambda d, i: d[st0["cur"][i]][i] if isinstance(d, list) else d[i]
    ref = pool.map(pc.oracle_fit, [(images[i], pick(st0["sed"], i)[:n[i]], pick(st0["morph"], i)[:n[i]],
                                    st0["cen"][i][:n[i]], st0["shifts"][i][:n[i]], iters, e_rel, np.float32,
                                    wl.oracle_kwargs()) for i in range(S)])
    assert not st["status"].any(), st["status"]
    exempt = []
    for i in range(S):
        c = st["cur"][i]
        sed, morph = st["sed"][c][i][:n[i]], st["morph"][c][i][:n[i]]
        np.testing.assert_array_equal(st["cen"][i][:n[i]], ref[i][3])
        assert st["it"][i] == ref[i][4], (i, st["it"][i], ref[i][4])
        if e_rel > 0:
            flags = st["flags"][i][:n[i]] & (scarlet._lib.FLAG_SED_NOT_CONVERGED | scarlet._lib.FLAG_MORPH_NOT_CONVERGED)
            ref_flags = np.array(ref[i][5]) & 3
            assert np.array_equal(flags, ref_flags), (i, flags, ref_flags)
        e = dict(sed=rel_err(sed, ref[i][0]), morph=rel_err(morph, ref[i][1]),
                 mse=rel_err(st["mse"][i][:st["it"][i]], ref[i][2]))
        if max(e.values()) <= TOL:
            continue
        assert e_rel == 0, "scene %d (n = %d) beyond 1e-5 in a converged run: %s" % (i, n[i], e)
        ok, msg = pc.straddles_threshold(scarlet, wl, images[i], centers[i][:n[i]], iters)
        assert ok, "scene %d (n = %d) beyond 1e-5 (%s) and not a threshold straddle: %s" % (i, n[i], e, msg)
        exempt.append((i, e, msg))
    pc.log_exemptions(test, exempt, max_exempt)
    assert len(exempt) <= max_exempt, exempt
    return st


def test_headline_ragged_vs_oracle_tiled(env):
    """5 x 64^2, K = 4, n in 1..4, 50 iterations; 32 distinct scenes tiled to 1664 so that k_fit2x's queue hands out
    ragged scenes; every copy of a scene comes out bit-identical to the first"""
    scarlet, pool = env
    wl = pc.Workload(B=5, H=64, W=64, K=4)
    counts = np.arange(32) % 4 + 1
    images, centers, n = _ragged_scenes(wl, 9400, counts)
    reps = 52
    images, centers, n = np.tile(images, (reps, 1, 1, 1)), np.tile(centers, (reps, 1, 1)), np.tile(n, reps)
    st = _ragged_vs_oracle(scarlet, pool, wl, images, centers, n, 50, 0.0, "ragged headline", distinct=32)
    for key in ("sed", "morph"):
        cur = np.stack([st[key][st["cur"][i]][i] for i in range(len(n))])
        first = cur[:32]
        for r in range(1, reps):
            assert np.array_equal(cur[32 * r:32 * (r + 1)], first), (key, r)
    assert np.array_equal(st["mse"].reshape(reps, 32, -1), np.broadcast_to(st["mse"][:32], (reps,) + st["mse"][:32].shape))


def test_config5_ragged_vs_oracle(env):
    scarlet, pool = env
    wl = pc.Workload(B=6, H=256, W=256, K=30)
    images, centers, n = _ragged_scenes(wl, 9500, [1, 7, 19, 30])
    _ragged_vs_oracle(scarlet, pool, wl, images, centers, n, 8, 0.0, "ragged config 5")


def test_k64_ragged_vs_oracle(env):
    scarlet, pool = env
    wl = pc.Workload(B=5, H=128, W=128, K=64)
    images, centers, n = _ragged_scenes(wl, 9600, [5, 33, 64])
    _ragged_vs_oracle(scarlet, pool, wl, images, centers, n, 6, 0.0, "ragged K = 64")


def test_k40_ragged_vs_oracle(env):
    """hugek.h (K > 32) with scenes of at most 32 components: their second 32-block of the Gram is neither formed, reduced
    nor squared, and the Lipschitz pass reads only their own rows"""
    scarlet, pool = env
    wl = pc.Workload(B=5, H=64, W=64, K=40)
    images, centers, n = _ragged_scenes(wl, 9650, [3, 20, 32, 33, 40])
    _ragged_vs_oracle(scarlet, pool, wl, images, centers, n, 6, 0.0, "ragged K = 40")


def _check_tiled(st, distinct, what):
    """copies of the first `distinct` scenes (scene s is a copy of scene s % distinct) came out bit-identical"""
    S = len(st["it"])
    for key in ("sed", "morph"):
        cur = np.stack([st[key][st["cur"][i]][i] for i in range(S)])
        for i in range(distinct, S):
            assert np.array_equal(cur[i], cur[i % distinct]), (what, key, i)
    for i in range(distinct, S):
        assert np.array_equal(st["mse"][i], st["mse"][i % distinct]), (what, i)


RAGGED_PATHS = [
    # (id, B, H, W, K, S, counts of the distinct scenes, iters, psf)
    ("bigk_gram_chunked", 5, 63, 63, 12, 5, [1, 5, 8, 9, 12], 6, False),    # HW % 4 != 0: k_bigk_gram, k_bigk_step
    ("iterate_b6", 6, 64, 64, 4, 8, [1, 2, 3, 4, 4, 3, 2, 1], 8, False),    # k_iterate<4, 6>
    ("iterate2_generic", 5, 48, 48, 4, 8, [1, 2, 3, 4, 4, 3, 2, 1], 8, False),
    ("box128", 5, 128, 128, 4, 4, [1, 2, 3, 4], 6, False),
    ("streamed384", 5, 384, 384, 4, 2, [1, 3], 4, False),
    ("psf_hipfft", 5, 320, 320, 4, 2, [2, 4], 4, True),
    ("psf_two_pipelines", 5, 64, 64, 4, 1024, [1, 2, 3, 4, 4, 3, 2, 1], 6, True),   # batch_view halves
]


@pytest.mark.parametrize("name,B,H,W,K,S,counts,iters,psf", RAGGED_PATHS, ids=[p[0] for p in RAGGED_PATHS])
def test_ragged_paths_vs_oracle(env, name, B, H, W, K, S, counts, iters, psf):
    """each path a ragged batch can take: absent components stay out, the distinct scenes match the oracle, and tiled
    copies (the two half-batch pipelines for >= 1024 PSF scenes) agree bit for bit"""
    import ctypes
    scarlet, pool = env
    wl = pc.Workload(B=B, H=H, W=W, K=K, psf=psf)
    images, centers, n = _ragged_scenes(wl, 9660 + 17 * len(name), counts)
    d = len(counts)
    reps = (S + d - 1) // d
    images, centers, n = (np.tile(images, (reps, 1, 1, 1))[:S], np.tile(centers, (reps, 1, 1))[:S],
                          np.tile(n, reps)[:S])
    if name == "psf_two_pipelines":
        b = _batch(scarlet, wl, images, centers, n=n)
        assert scarlet._lib.lib.scarlet_batch_pipelines(ctypes.byref(b._c)) == 2
        del b
    st = _ragged_vs_oracle(scarlet, pool, wl, images, centers, n, iters, 0.0, "ragged " + name, distinct=d)
    _check_tiled(st, d, name)


def test_psf_ragged_vs_oracle(env):
    scarlet, pool = env
    wl = pc.Workload(B=5, H=64, W=64, K=4, psf=True)
    images, centers, n = _ragged_scenes(wl, 9700, [1, 2, 3, 4, 2, 1])
    _ragged_vs_oracle(scarlet, pool, wl, images, centers, n, 10, 0.0, "ragged PSF")


def test_converged_ragged_vs_oracle(env):
    """e_rel = 1e-3: iteration counts and convergence flags equal the oracle's"""
    scarlet, pool = env
    wl = pc.Workload(B=5, H=64, W=64, K=4)
    images, centers, n = _ragged_scenes(wl, 9800, [1, 2, 3, 4, 4, 3, 2, 1])
    st = _ragged_vs_oracle(scarlet, pool, wl, images, centers, n, 200, 1e-3, "ragged converged", max_exempt=0)
    assert (st["it"] < 200).any()


# ------------------------------------------------------------------ 3./4. absent components, init per source
@pytest.mark.parametrize("B,H,W,K", [(5, 64, 64, 4), (5, 128, 128, 12), (5, 64, 64, 40)])
def test_init_extended_is_per_source(env, B, H, W, K):
    scarlet, _ = env
    wl = pc.Workload(B=B, H=H, W=W, K=K)
    counts = [1 + (i * 7) % K for i in range(6)]
    images, centers, n = _ragged_scenes(wl, 9900 + K, counts)
    b = _batch(scarlet, wl, images, centers, n=n)
    st0 = _state(b)
    b.init_extended(np.ones(B) * 0.1)
    st = _state(b)
    _check_absent(st0, st, n, "init K=%d" % K)
    for i in range(len(n)):
        one = _batch(scarlet, wl, images[i:i + 1], centers[i:i + 1, :n[i]])
        one.init_extended(np.ones(B) * 0.1)
        o = _state(one)
        sed, morph = b.scene(i)
        assert np.array_equal(sed.cpu().numpy(), o["sed"][0][0]), i
        assert np.array_equal(morph.cpu().numpy(), o["morph"][0][0]), i
        assert np.array_equal(st["flags"][i][:n[i]], o["flags"][0]), i
        assert np.array_equal(st["cen"][i][:n[i]], o["cen"][0]), i


def test_step_phases_keep_absent_components_out(env):
    """the three separately callable phases (backward_step, source_update, check_convergence) on a ragged batch"""
    scarlet, _ = env
    wl = pc.Workload(B=5, H=64, W=64, K=6)
    images, centers, n = _ragged_scenes(wl, 9950, [1, 3, 6, 2])
    b = _batch(scarlet, wl, images, centers, n=n)
    b.init_extended(np.ones(5) * 0.1)
    st0 = _state(b)
    for _ in range(4):
        b.step(e_rel=0)
    st = _state(b)
    _check_absent(st0, st, n, "step phases")
    assert (st["it"] == 4).all() and not st["status"].any()


# ------------------------------------------------------------------ 5. bad counts
@pytest.mark.parametrize("B,H,W,K,S", [(5, 64, 64, 4, 1600), (5, 64, 64, 12, 6), (5, 128, 128, 4, 6)])
def test_bad_counts_on_device(env, B, H, W, K, S):
    scarlet, _ = env
    from scarlet_amd import _lib
    wl = pc.Workload(B=B, H=H, W=W, K=K)
    counts = [1 + i % K for i in range(min(S, 16))]
    images, centers, n = _ragged_scenes(wl, 9970 + K, counts)
    reps = (S + len(counts) - 1) // len(counts)
    images, centers, n = (np.tile(images, (reps, 1, 1, 1))[:S], np.tile(centers, (reps, 1, 1))[:S],
                          np.tile(n, reps)[:S])
    for bad in (0, K + 1):
        with pytest.raises(ValueError):
            nb = n.copy(); nb[1] = bad
            scarlet.BlendBatch(images, centers, n_components=nb)
    out = []
    for corrupt in (False, True):
        b = _batch(scarlet, wl, images, centers, n=n)
        if corrupt:
            b.n_components[1] = 0
            b.n_components[3] = K + 1
        st0 = _state(b)
        b.init_extended(np.ones(B) * 0.1)
        b.fit(6, e_rel=0, check_every=3)
        out.append((st0, _state(b)))
    (_, good), (st0, badst) = out
    for i in (1, 3):
        assert badst["status"][i] == _lib.STATUS_BAD_COUNT and badst["active"][i] == 0 and badst["it"][i] == 0
        for key in ("sed", "morph"):
            for j in range(2):
                assert not np.any(badst[key][j][i])
        for key in ("cen", "shifts", "flags"):
            assert np.array_equal(badst[key][i], st0[key][i], equal_nan=True), key
    keep = np.ones(S, bool); keep[[1, 3]] = False
    for key in good:
        if isinstance(good[key], list):
            for j in range(2):
                assert np.array_equal(good[key][j][keep], badst[key][j][keep], equal_nan=True), key
        else:
            assert np.array_equal(good[key][keep], badst[key][keep], equal_nan=True), key
