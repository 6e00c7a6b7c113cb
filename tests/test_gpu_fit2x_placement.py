"""-m gpu: k_fit2x / k_iterate2<4,5,64> place a scene's components on their four pairs of waves by the cost of the
k-space symmetry GEMMs (NTR NTC (NTR + NTC) for a window of NTR x NTC tiles; the largest and the smallest share one
pair of SIMDs, the two middle ones the other), once per scene and launch.  That is scheduling only: every output must
be bit for bit what the identity placement (option NO_PLACE) and what one launch per iteration (NO_PERSIST) give.
Scenes: 5 x 64 x 64, K = 4, centres chosen so that every order of four distinct costs over the component index occurs,
as do ties, a centred component (no GEMM: cost 0) and scenes of 1 to 3 components.
"""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

U, S, K, B, H, W = 160, 1600, 4, 5, 64, 64   # 160 distinct scenes tiled to 1600: more workgroups than the chip holds resident
R_OF_TILES = {2: (8, 15), 3: (16, 23), 4: (24, 31)}     # r = min(c, 63 - c): the window 2 r + 1 covers 2, 3 or 4 tiles of 16
CLASSES = [(2, 2), (2, 3), (3, 3), (3, 4), (4, 4)]      # costs 16, 30, 54, 84, 128


def _cost(cy, cx):
    """the kernel's cost of a present component centred at (cy, cx)"""
    if (cy, cx) == (H // 2, W // 2):
        return 0
    nt = lambda c, n: (2 * min(c, n - 1 - c) + 1 + 15) // 16
    a, b = nt(cy, H), nt(cx, W)
    return a * b * (a + b)


def _centre(rng, tiles):
    """a centre whose window has `tiles` = (NTR, NTC) tiles, or the transposed window"""
    a, b = tiles if rng.integers(2) else tiles[::-1]
    ry, rx = (int(rng.integers(R_OF_TILES[n][0], R_OF_TILES[n][1] + 1)) for n in (a, b))
    return (ry if rng.integers(2) else H - 1 - ry, rx if rng.integers(2) else W - 1 - rx)


def _scene(rng, classes, noise=0.1):
    """Gaussians as in synth.make_scene at centres of the given tile classes ("c": the frame's centre)"""
    centers = []
    while len(centers) < len(classes):
        cls = classes[len(centers)]
        c = (H // 2, W // 2) if cls == "c" else _centre(rng, cls)
        if all(max(abs(c[0] - y), abs(c[1] - x)) >= 4 for y, x in centers):
            centers.append(c)
    yy, xx = np.mgrid[:H, :W].astype(np.float64)
    model = np.zeros((B, H, W))
    for cy, cx in centers:
        smaj, q, th = rng.uniform(1.5, 3.5), rng.uniform(0.5, 1.0), rng.uniform(0, np.pi)
        dy, dx = yy - cy, xx - cx
        u, v = np.cos(th) * dx + np.sin(th) * dy, -np.sin(th) * dx + np.cos(th) * dy
        morph = np.exp(-0.5 * ((u / smaj) ** 2 + (v / (smaj * q)) ** 2))
        sed = np.exp(rng.uniform(np.log(5.0), np.log(50.0))) * rng.uniform(0.2, 1.0, size=B)
        model += sed[:, None, None] * morph
    cen = np.zeros((K, 2), np.int32)
    cen[:len(centers)] = centers
    return (model + rng.normal(0.0, noise, size=model.shape)).astype(np.float32), cen


def _make_data():
    rng = np.random.Generator(np.random.PCG64(20261234))
    perms = list(itertools.permutations(range(4)))
    plans = []
    for i in range(96):                                   # four distinct costs, every order, every choice of four classes
        four = [c for j, c in enumerate(CLASSES) if j != i % 5]
        plans.append([four[p] for p in perms[i % 24]])
    for i in range(16):                                   # two equal costs
        a, b, c = (CLASSES[(i + j) % 5] for j in (0, 2, 3))
        plans.append([[a, a, b, c], [b, a, c, a], [c, b, a, a], [a, c, a, b]][i % 4])
    plans += [[CLASSES[i % 5]] * 4 for i in range(8)]      # four equal costs
    for i in range(16):                                   # a centred component among three others
        p = [CLASSES[(i + j) % 5] for j in range(3)]
        p.insert(i % 4, "c")
        plans.append(p)
    for i in range(24):                                   # 1 to 3 components
        plans.append([CLASSES[(i + 2 * j) % 5] for j in range(1 + i % 3)])
    assert len(plans) == U
    scenes = [_scene(rng, p) for p in plans]
    counts = np.array([len(p) for p in plans], np.int32)
    cen = np.stack([c for _, c in scenes])
    # what the issue asks to be present
    costs = [[_cost(int(y), int(x)) for y, x in cen[i, :counts[i]]] for i in range(U)]
    orders = {tuple(np.argsort(c)) for c in costs if len(c) == 4 and len(set(c)) == 4}
    assert len(orders) == 24
    assert any(len(c) == 4 and len(set(c)) == 3 for c in costs) and any(len(c) == 4 and len(set(c)) == 1 for c in costs)
    assert any(0 in c for c in costs) and sorted(set(counts.tolist())) == [1, 2, 3, 4]
    reps = S // U
    tile = lambda v: np.tile(v, (reps,) + (1,) * (v.ndim - 1))
    return dict(images=tile(np.stack([im for im, _ in scenes])), centers=tile(cen), n=tile(counts))


@pytest.fixture(scope="module")
def env():
    """the library, the batch class, the scenes every test shares (never modified) and the runs made so far"""
    from scarlet_amd import _lib
    _lib.require_gpu()
    from scarlet_amd.batch import BlendBatch
    return _lib, BlendBatch, _make_data(), {}


def _outputs(b):
    torch.cuda.synchronize()
    t = dict(morph0=b.morph[0], morph1=b.morph[1], sed0=b.sed[0], sed1=b.sed[1], mse=b.mse_buf, centers=b.centers,
             shifts=b.shifts, flags=b.flags, it=b.it, lipschitz=b.lipschitz, active=b.active, cur=b.cur, status=b.status)
    return {k: v.cpu().numpy() for k, v in t.items()}


def _run(env, fits, no_place=0, per_iteration=0, dbg=0):
    """init on the device, then one fit() per entry (n, e_rel, check_every) of `fits`; each distinct run is made once"""
    _lib, BB, data, cache = env
    key = (tuple(fits), no_place, per_iteration, dbg)
    if key in cache:
        return cache[key]
    _lib.set_option("NO_PLACE", no_place)
    _lib.set_option("NO_PERSIST", per_iteration)
    _lib.set_option("PERSIST_DBG", dbg)
    try:
        b = BB(data["images"], data["centers"], mse_capacity=64, n_components=data["n"])
        b.init_extended(np.ones(B) * 0.1)
        launched = [b.fit(n, e_rel=e_rel, check_every=ce) for n, e_rel, ce in fits]
        cache[key] = (launched, _outputs(b))
        return cache[key]
    finally:
        for name in ("NO_PLACE", "NO_PERSIST", "PERSIST_DBG"):
            _lib.set_option(name, 0)


def _assert_identical(one, other, what):
    assert one[0] == other[0], (what, one[0], other[0])
    for key in one[1]:
        assert np.array_equal(one[1][key], other[1][key], equal_nan=True), "%s: %s differs" % (what, key)


@pytest.mark.parametrize("fits,dbg", [([(11, 0.0, 0)], 0), ([(7, 0.0, 3), (4, 0.0, 0)], 0), ([(11, 0.0, 0)], 1)])
def test_placed_against_identity(env, fits, dbg):
    """k_fit2x with the components placed against NO_PLACE.  The second fit list re-decides the placement at every
    launch, from centres that may have moved; PERSIST_DBG = 1 makes every re-entered iteration reload its tiles from
    the planes the placed waves stored (the path a NaN result takes).  Eleven iterations cross the centroid
    iterations 5 and 10, and the shifts they find are not all zero."""
    placed, identity = _run(env, fits, dbg=dbg), _run(env, fits, no_place=1, dbg=dbg)
    _assert_identical(placed, identity, "placed vs NO_PLACE %r dbg %d" % (fits, dbg))
    out = placed[1]
    present = np.arange(K)[None, :] < env[2]["n"][:, None]
    assert (out["it"] == 11).all() and not out["status"].any()
    sh = out["shifts"].reshape(S, K, 2)[present]                 # (NaN: no shift yet)
    assert np.isfinite(sh).all() and np.any(sh != 0, axis=-1).mean() > 0.5


def test_placed_against_one_launch_per_iteration(env):
    """the default build (placed, persistent) against k_iterate2<4,5,64> launched once per iteration, which decides
    its placement per launch"""
    fits = [(11, 0.0, 0)]
    _assert_identical(_run(env, fits), _run(env, fits, per_iteration=1), "k_fit2x vs NO_PERSIST")
