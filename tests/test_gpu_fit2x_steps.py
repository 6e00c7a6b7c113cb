"""-m gpu: k_fit2x's step sizes.  Inside a multi-iteration launch the SED step, the SED finalisation and the NEXT
iteration's morphology step size are computed by one wave under the monotonicity sweep (the last partner wave to
arrive after the symmetry phase) instead of on the scene's chain, and the morphology step size travels to the next
iteration through LDS.  None of that changes a single operation on the data: every test here compares k_fit2x with
k_iterate2<4,5,64> launched once per iteration (NO_PERSIST), all outputs bit for bit, on 5 x 64 x 64 scenes with K = 4.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

U, S, K, B = 160, 1600, 4, 5        # 160 distinct scenes tiled to 1600: more workgroups than the chip holds resident


@pytest.fixture(scope="module")
def env():
    """the library, the batch class and the two batches every test shares (never modified): `full` (four components
    in every scene) and `ragged` (1 to 4 components: arrival counts 1..4, absent pairs, a worker that is not pair 0)"""
    from scarlet_amd import _lib, synth
    _lib.require_gpu()
    from scarlet_amd.batch import BlendBatch
    reps = S // U
    tile = lambda v: np.tile(v, (reps,) + (1,) * (v.ndim - 1))
    d = synth.make_batch(2400, U)
    full = dict(images=tile(d["images"]), centers=tile(d["centers"]), n=None)
    imgs, cens, counts = [], [], []
    for i in range(U):
        n = 1 + (i * 7 + i // 4) % 4
        sc = synth.make_scene(2600 + i, K=n)
        c = np.zeros((K, 2), np.int32)
        c[:n] = sc["centers"]
        imgs.append(sc["images"]); cens.append(c); counts.append(n)
    assert sorted(set(counts)) == [1, 2, 3, 4]
    ragged = dict(images=tile(np.stack(imgs)), centers=tile(np.stack(cens)), n=tile(np.asarray(counts, np.int32)))
    return _lib, BlendBatch, full, ragged


def _outputs(b):
    torch.cuda.synchronize()
    t = dict(morph0=b.morph[0], morph1=b.morph[1], sed0=b.sed[0], sed1=b.sed[1], mse=b.mse_buf, centers=b.centers,
             shifts=b.shifts, flags=b.flags, it=b.it, lipschitz=b.lipschitz, active=b.active, cur=b.cur, status=b.status)
    return {k: v.cpu().numpy() for k, v in t.items()}


def _run(env, data, fits, per_iteration, dbg=0, state=None, **attrs):
    """init (device initialisation, or the given state), then one fit() per entry (n, e_rel, check_every) of `fits`"""
    _lib, BB = env[0], env[1]
    _lib.set_option("NO_PERSIST", 1 if per_iteration else 0)
    _lib.set_option("PERSIST_DBG", dbg)
    try:
        kw = {} if data["n"] is None else dict(n_components=data["n"])
        b = BB(data["images"], data["centers"], mse_capacity=64, **kw)
        for name, arr in attrs.items():
            setattr(b, name, torch.as_tensor(arr).cuda())
        b._fill_struct()
        if state is None:
            b.init_extended(np.ones(B) * 0.1)
        else:
            b.set_state(*state)
        launched = [b.fit(n, e_rel=e_rel, check_every=ce) for n, e_rel, ce in fits]
        return launched, _outputs(b)
    finally:
        _lib.set_option("NO_PERSIST", 0)
        _lib.set_option("PERSIST_DBG", 0)


def _assert_identical(one, many, what):
    assert one[0] == many[0], (what, one[0], many[0])
    for key in one[1]:
        assert np.array_equal(one[1][key], many[1][key], equal_nan=True), "%s: %s differs" % (what, key)


def test_ragged_batches(env):
    """n_components of 1 to 4 per scene: the worker is the last of n partner waves to arrive, whichever pair that is"""
    ragged = env[3]
    for fits in ([(11, 0.0, 0)], [(7, 0.0, 3), (4, 0.0, 0)]):
        one, many = _run(env, ragged, fits, True), _run(env, ragged, fits, False)
        _assert_identical(one, many, "ragged %r" % (fits,))
        assert (many[1]["it"] == 11).all() and not many[1]["status"].any()


def _lambda_max_sst(sed):
    """lambda_max(S S^T) of (S, K, B) SEDs in float64"""
    s = sed.astype(np.float64)
    return np.linalg.eigvalsh(s @ s.transpose(0, 2, 1))[:, -1]


@pytest.mark.parametrize("length", [1, 2, 4, 5, 6, 11])
def test_launch_lengths(env, length):
    """launches of `length` iterations (check_every) and a second fit() on the same batch.  The morphology step size
    an iteration leaves behind for the next one must not leak out: lipschitz[:, 1] is the constant of the SEDs the last
    EXECUTED iteration started from (the other SED buffer), not of the SEDs it produced."""
    full = env[2]
    fits = [(11, 0.0, length), (3, 0.0, 0)]
    # (launches of one iteration go through k_fit2x only with PERSIST_DBG = 2)
    one, many = _run(env, full, fits, True), _run(env, full, fits, False, dbg=2 if length == 1 else 0)
    _assert_identical(one, many, "launch length %d" % length)
    o = many[1]
    assert (o["it"] == 14).all()
    sel = np.arange(S)
    sed_in = np.where((o["cur"] == 0)[:, None, None], o["sed1"], o["sed0"])     # what the last iteration read
    sed_out = np.where((o["cur"] == 0)[:, None, None], o["sed0"], o["sed1"])
    used, leaked = _lambda_max_sst(sed_in), _lambda_max_sst(sed_out)
    got = o["lipschitz"][sel, 1]
    # the float64 Newton iteration on the characteristic polynomial is good to ~1e-8 relative at worst (a double top
    # eigenvalue; 1e-16 otherwise), LAPACK to 1e-15: 1e-7 separates that from the SEDs' change per iteration
    assert np.all(np.abs(got - used) <= 1e-7 * used), np.abs(got / used - 1).max()
    moved = np.abs(leaked - used) > 1e-5 * used
    assert moved.sum() > S // 2                                                  # (the guard is not vacuous)
    assert np.all(np.abs(got - used)[moved] < np.abs(got - leaked)[moved])


def test_fixed_factors_and_tight_stop(env):
    """fix_sed / fix_morph masks, and e_rel = 1e-3: scenes stop inside a launch, one by one"""
    full, ragged = env[2], env[3]
    fix = np.zeros((S, K), dtype=np.uint8)
    fix[::3, 1] = 1
    fix[1::5, 0] = 1
    for data, attrs, fits in ((full, dict(fix_sed=fix), [(11, 0.0, 0)]),
                              (full, dict(fix_morph=fix), [(11, 1e-3, 6)]),
                              (ragged, dict(fix_sed=fix), [(12, 1e-3, 5)]),
                              (full, {}, [(30, 1e-3, 0), (5, 1e-3, 0)])):
        one, many = _run(env, data, fits, True, **attrs), _run(env, data, fits, False, **attrs)
        _assert_identical(one, many, "%r %r" % (sorted(attrs), fits))
    assert len(np.unique(many[1]["it"])) > 2                   # the last case: a ragged stop inside the first launch


def test_degenerate_scenes(env):
    """scenes in which one component starts from an all-zero morphology, among normal ones: with the component's SED
    zero as well, or its morphology fixed, the peak stays 0, the normalisation is 0 / 0 and the scene ends
    SCARLET_STATUS_NONFINITE.  The NaN result is written after the SEDs were finalised, so the step size carried to the
    next iteration must be dropped: both paths give the same outputs and the same status."""
    _lib, BB, full = env[0], env[1], env[2]
    b = BB(full["images"], full["centers"])
    b.init_extended(np.ones(B) * 0.1)
    torch.cuda.synchronize()
    sed, morph = b.sed_current.cpu().numpy().copy(), b.morph_current.cpu().numpy().copy()
    cen, sh = b.centers.cpu().numpy().copy(), b.shifts.cpu().numpy().copy()
    del b
    fixm = np.zeros((S, K), dtype=np.uint8)
    zero_both, zero_fixed, zero_morph = np.arange(5, S, 97), np.arange(11, S, 89), np.arange(17, S, 83)
    for n, (scenes, k) in enumerate(((zero_both, 1), (zero_fixed, 2), (zero_morph, 0))):
        morph[scenes, k] = 0
        if n == 0:
            sed[scenes, k] = 0
        if n == 1:
            fixm[scenes, k] = 1
    fits = [(6, 1e-3, 0), (3, 1e-3, 2)]
    state = (sed, morph, cen, sh)
    one = _run(env, full, fits, True, state=state, fix_morph=fixm)
    many = _run(env, full, fits, False, state=state, fix_morph=fixm)
    _assert_identical(one, many, "degenerate scenes")
    status = many[1]["status"]
    assert np.all(status[zero_both] & _lib.STATUS_NONFINITE) and np.all(status[zero_fixed] & _lib.STATUS_NONFINITE)
    normal = np.ones(S, bool)
    normal[np.concatenate([zero_both, zero_fixed, zero_morph])] = False
    assert not status[normal].any()


@pytest.mark.parametrize("dbg,check_every", [(1, 0), (2, 1)])
def test_diagnostic_paths(env, dbg, check_every):
    """PERSIST_DBG 1: every re-entered iteration reloads its tiles from memory (and solves its step size itself);
    2: launches of one iteration go through k_fit2x"""
    ragged = env[3]
    one = _run(env, ragged, [(9, 1e-3, check_every)], True)
    many = _run(env, ragged, [(9, 1e-3, check_every)], False, dbg=dbg)
    _assert_identical(one, many, "PERSIST_DBG %d" % dbg)
