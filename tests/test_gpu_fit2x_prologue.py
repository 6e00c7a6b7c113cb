"""-m gpu: the start of a k_fit2x iteration.  A re-entered iteration whose tiles are resident runs its own instance of
the first phase (images requested first, centre / shift / SEDs / component count taken from LDS, no load of the FFT
length table); every other start of an iteration -- a launch's first, a scene taken from the queue onto LDS another
scene left behind, a re-entry without resident tiles -- runs the other one.  Which instance runs changes no operation on
the data: every test compares k_fit2x with k_iterate2<4,5,64> launched once per iteration (NO_PERSIST), all outputs bit
for bit, on 5 x 64 x 64 scenes with K = 4.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

U, S, K, B = 64, 704, 4, 5          # 64 distinct scenes tiled to 704: more than the 512 workgroups the chip holds resident;
                                    # the scene a workgroup takes from the queue is in general no copy of its last one


@pytest.fixture(scope="module")
def env():
    """the library, the batch class and the batches the tests share (never modified): `full` (four components in every
    scene), `few` (its first three scenes: fewer scenes than workgroups) and `ragged` (1 to 4 components)"""
    from scarlet_amd import _lib, synth
    _lib.require_gpu()
    from scarlet_amd.batch import BlendBatch
    reps = S // U
    tile = lambda v: np.tile(v, (reps,) + (1,) * (v.ndim - 1))
    d = synth.make_batch(4100, U)
    full = dict(images=tile(d["images"]), centers=tile(d["centers"]), n=None)
    few = dict(images=d["images"][:3], centers=d["centers"][:3], n=None)
    imgs, cens, counts = [], [], []
    for i in range(U):
        n = 1 + (i * 7 + i // 4) % 4
        sc = synth.make_scene(4300 + i, K=n)
        c = np.zeros((K, 2), np.int32)
        c[:n] = sc["centers"]
        imgs.append(sc["images"]); cens.append(c); counts.append(n)
    assert sorted(set(counts)) == [1, 2, 3, 4]
    ragged = dict(images=tile(np.stack(imgs)), centers=tile(np.stack(cens)), n=tile(np.asarray(counts, np.int32)))
    return _lib, BlendBatch, dict(full=full, few=few, ragged=ragged)


def _outputs(b):
    torch.cuda.synchronize()
    t = dict(morph0=b.morph[0], morph1=b.morph[1], sed0=b.sed[0], sed1=b.sed[1], mse=b.mse_buf, centers=b.centers,
             shifts=b.shifts, flags=b.flags, it=b.it, lipschitz=b.lipschitz, active=b.active, cur=b.cur, status=b.status)
    return {k: v.cpu().numpy() for k, v in t.items()}


def _run(env, data, fits, per_iteration, dbg=0, **attrs):
    """device initialisation, then one fit() per entry (n, e_rel, check_every) of `fits`"""
    _lib, BB = env[0], env[1]
    _lib.set_option("NO_PERSIST", 1 if per_iteration else 0)
    _lib.set_option("PERSIST_DBG", dbg)
    try:
        kw = {} if data["n"] is None else dict(n_components=data["n"])
        b = BB(data["images"], data["centers"], mse_capacity=64, **kw)
        for name, arr in attrs.items():
            setattr(b, name, torch.as_tensor(arr).cuda())
        b._fill_struct()
        b.init_extended(np.ones(B) * 0.1)
        launched = [b.fit(n, e_rel=e_rel, check_every=ce) for n, e_rel, ce in fits]
        return launched, _outputs(b)
    finally:
        _lib.set_option("NO_PERSIST", 0)
        _lib.set_option("PERSIST_DBG", 0)


def _assert_identical(one, many, what):
    assert one[0] == many[0], (what, one[0], many[0])
    for key in one[1]:
        assert np.array_equal(one[1][key], many[1][key], equal_nan=True), "%s: %s differs" % (what, key)


@pytest.mark.parametrize("length", [1, 2, 7])
def test_fewer_scenes_than_workgroups(env, length):
    """three scenes, launches of 1, 2 and 7 iterations (14 in all: the centroid iterations 5 and 10 among them).
    Launches of one iteration go through k_fit2x only with PERSIST_DBG = 2: every iteration is a launch's first."""
    few = env[2]["few"]
    fits = [(14, 0.0, length)]
    one, many = _run(env, few, fits, True), _run(env, few, fits, False, dbg=2 if length == 1 else 0)
    _assert_identical(one, many, "S = 3, launches of %d" % length)
    assert (many[1]["it"] == 14).all() and not many[1]["status"].any()


def test_scenes_stop_and_workgroups_take_new_ones(env):
    """e_rel = 1e-3, 30 iterations in one launch: scenes stop one by one, and a workgroup that takes its next scene from
    the queue finds the LDS another scene left behind (placement and component count, carried centres, shifts, SEDs and
    step size, the length table).  Then a second fit() on the same batch."""
    full = env[2]["full"]
    fits = [(30, 1e-3, 0), (5, 1e-3, 0)]
    one, many = _run(env, full, fits, True), _run(env, full, fits, False)
    _assert_identical(one, many, "ragged stop, S = %d" % S)
    assert len(np.unique(many[1]["it"])) > 2                   # scenes did stop at different iterations


@pytest.mark.parametrize("check_every", [5, 6])
def test_centroid_iterations(env, check_every):
    """e_rel = 0, 30 iterations in launches of 5 (the centroid iteration, it % 5 == 0, is each launch's last) and of 6
    (it is the 5th, 4th, 3rd and 2nd of a launch, then the first): the shift it finds reaches the next iteration through
    LDS when that one is re-entered, and through memory when it starts a launch."""
    full = env[2]["full"]
    fits = [(30, 0.0, check_every)]
    one, many = _run(env, full, fits, True), _run(env, full, fits, False)
    _assert_identical(one, many, "launches of %d" % check_every)
    assert (many[1]["it"] == 30).all()
    sh = many[1]["shifts"].reshape(S, K, 2)
    assert np.isfinite(sh).all() and np.any(sh != 0, axis=-1).mean() > 0.5      # (the shifts are not all zero)


def test_reentry_without_resident_tiles(env):
    """PERSIST_DBG = 1: every re-entered iteration reloads its tiles from memory and solves its step size itself -- the
    re-entered start that does NOT take the resident instance (the path a NaN result takes)"""
    full = env[2]["full"]
    fits = [(11, 1e-3, 0)]
    one, many = _run(env, full, fits, True), _run(env, full, fits, False, dbg=1)
    _assert_identical(one, many, "PERSIST_DBG 1")


def test_ragged_batch_with_fixed_factors(env):
    """n_components of 1 to 4 (the re-entered iteration takes the count from LDS) with fix_sed / fix_morph masks"""
    ragged = env[2]["ragged"]
    fix = np.zeros((S, K), dtype=np.uint8)
    fix[::3, 1] = 1
    fix[1::5, 0] = 1
    for attrs, fits in ((dict(fix_sed=fix), [(11, 0.0, 0)]),
                        (dict(fix_morph=fix), [(12, 1e-3, 5)]),
                        (dict(fix_sed=fix, fix_morph=fix[:, ::-1].copy()), [(7, 0.0, 3), (4, 0.0, 0)])):
        one, many = _run(env, ragged, fits, True, **attrs), _run(env, ragged, fits, False, **attrs)
        _assert_identical(one, many, "ragged %r %r" % (sorted(attrs), fits))
    assert (many[1]["it"] == 11).all()
