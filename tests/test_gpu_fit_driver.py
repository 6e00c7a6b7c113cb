"""-m gpu: what the one iteration driver behind every fit entry point must preserve (fit_loop in scarlet_hip.hip).

Seven loop forms at the smallest shapes that reach them:

  fused4     four-wave k_iterate<4, 6>        K = 3, B = 6, 24 x 32
  iterate2   eight-wave k_iterate2<4, 5>      K = 3, B = 3, 24 x 32
  fit2x      persistent k_fit2x               K = 4, B = 5, 64 x 64, default switches, 8 scenes
  general    k_grad / k_step / update / test  K = 3, B = 3, 24 x 32, approximate_L
  two_pipe   two half-batches, two streams    1024 scenes (8 tiled), K = 3, B = 2, 24 x 32, a 5 x 5 kernel
  prior      k_prior_step                     K = 3, B = 3, 24 x 32, quadratic prior (weights 0.3 / 2.0)
  two_obs    the observation step             K = 3, channels 3 + 2, 24 x 32

Every expected number follows from the loop as written, none is measured: a call of max_iter iterations with e_rel = 0
launches max_iter; the host looks at `active` after every check_every-th iteration except the last; k_fit2x covers the
iterations up to the next look in one launch.  The reference's convergence test compares with the previous iteration
(blend.py:141-184, `it > 1`; k_converge has the same condition), so the earliest stop of a scene is its SECOND
iteration: with an e_rel that every scene meets at once, every scene ends with it == 2, which the CPU oracle confirms
for the scenes used here, and a look after iteration 3 ends the call."""
import contextlib
import ctypes

import numpy as np
import pytest

import prior_common as prc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
BG = 0.1
ITERS = 7
E_BIG = 1e3           # |x - x_last|^2 <= 1e6 |x|^2: met by every component with a non-zero factor
FIRST_STOP = 2        # the convergence test needs a previous iteration
KEYS = ("sed", "morph", "centers", "shifts", "flags", "mse", "it", "lipschitz")


@pytest.fixture(scope="module")
def scarlet():
    import scarlet_amd
    scarlet_amd._lib.require_gpu()
    from oracle import build as obuild
    obuild.build()
    return scarlet_amd


@contextlib.contextmanager
def option(scarlet, name, value=1):
    old = scarlet._lib.set_option(name, value)
    try:
        yield
    finally:
        scarlet._lib.set_option(name, old)


def state(b):
    torch.cuda.synchronize()
    return dict(sed=b.sed_current.cpu().numpy(), morph=b.morph_current.cpu().numpy(), centers=b.centers.cpu().numpy(),
                shifts=b.shifts.cpu().numpy(), flags=b.flags.cpu().numpy(), mse=b.mse_buf.cpu().numpy(),
                it=b.it.cpu().numpy(), lipschitz=b.lipschitz.cpu().numpy(), active=b.active.cpu().numpy(),
                status=b.status.cpu().numpy())


def assert_identical(a, b, what):
    for key in KEYS:
        assert np.array_equal(a[key], b[key], equal_nan=True), "%s: %s differs" % (what, key)


class Form(object):
    """One loop form: `make()` returns a freshly initialised batch (the same state every time), `fit` runs it through
    BlendBatch.fit, `oracle_it` is the number of iterations the CPU oracle runs from a given start."""
    U = None                 # unique scenes (the rest are tiled copies)

    def __init__(self, scarlet, seed, S, K, B, H, W, approximate_L=False, psf=False, tile=1):
        from scarlet_amd import synth
        self.scarlet, self.K, self.B, self.approximate_L = scarlet, K, B, approximate_L
        sc = [synth.make_scene(seed + i, B=B, H=H, W=W, K=K) for i in range(S)]
        self.U = S
        self.images = np.tile(np.stack([x["images"] for x in sc]), (tile, 1, 1, 1))
        self.centers = np.tile(np.stack([x["centers"] for x in sc]), (tile, 1, 1))
        self.diff = None
        if psf:
            y, x = np.mgrid[:5, :5]
            k = np.exp(-((y - 2) ** 2 + (x - 2) ** 2) / 2.0).astype(np.float32)
            self.diff = np.stack([k / k.sum()] * B)

    def make(self):
        b = self.scarlet.BlendBatch(self.images, self.centers, mse_capacity=ITERS + 1)
        if self.diff is not None:
            b.set_diff_kernel(self.diff)
        return b.init_extended(np.ones(self.B) * BG)

    def prior(self):
        return None

    def fit(self, b, max_iter, e_rel, check_every):
        return b.fit(max_iter, e_rel=e_rel, approximate_L=self.approximate_L, check_every=check_every, prior=self.prior())

    def spec(self, st0, s):
        okw = {} if self.diff is None else dict(diff_kernel=self.diff)
        return dict(images=self.images[s], sed0=st0["sed"][s], morph0=st0["morph"][s], cen0=st0["centers"][s],
                    sh0=st0["shifts"][s], okw=okw, approximate_L=self.approximate_L)

    def oracle_it(self, st0, s, max_iter, e_rel):
        return prc.oracle_fit((self.spec(st0, s), max_iter, e_rel, np.float32))[4]


class PriorForm(Form):
    def prior(self):
        return self.scarlet.QuadraticPrior(sed_weight=0.3, morph_weight=2.0)

    def spec(self, st0, s):
        return dict(Form.spec(self, st0, s), ws=np.full(self.K, 0.3), wm=np.full(self.K, 2.0))


class TwoObsForm(Form):
    def obs(self):
        return [(self.images[:, :3], 0), (self.images[:, 3:], 3)]

    def make(self):
        obs = [self.scarlet.ObservationBatch(im, band0=b0) for im, b0 in self.obs()]
        b = self.scarlet.BlendBatch.from_observations(obs, self.centers, mse_capacity=ITERS + 1)
        return b.init_combined([np.ones(3) * BG, np.ones(2) * BG])

    def oracle_it(self, st0, s, max_iter, e_rel):
        from oracle import pgm
        sh = None if np.isnan(st0["shifts"][s]).any() else st0["shifts"][s]     # (init_combined runs no update)
        sc = pgm.scene_from_state(np.zeros(self.images.shape[1:], np.float32), st0["sed"][s], st0["morph"][s],
                                  st0["centers"][s], sh)
        sc.observations = [dict(images=im[s], band_slice=slice(b0, b0 + im.shape[1])) for im, b0 in self.obs()]
        return pgm.fit(sc, max_iter, e_rel=e_rel).it


FORMS = ("fused4", "iterate2", "fit2x", "general", "two_pipe", "prior", "two_obs")
_cache = {}


def form(scarlet, name):
    if name not in _cache:
        _cache[name] = dict(
            fused4=lambda: Form(scarlet, 7000, 3, 3, 6, 24, 32),
            iterate2=lambda: Form(scarlet, 7010, 3, 3, 3, 24, 32),
            fit2x=lambda: Form(scarlet, 7020, 8, 4, 5, 64, 64),
            general=lambda: Form(scarlet, 7030, 3, 3, 3, 24, 32, approximate_L=True),
            two_pipe=lambda: Form(scarlet, 6500, 8, 3, 2, 24, 32, psf=True, tile=128),
            prior=lambda: PriorForm(scarlet, 7040, 3, 3, 3, 24, 32),
            two_obs=lambda: TwoObsForm(scarlet, 7050, 3, 3, 5, 24, 32))[name]()
    return _cache[name]


def profiled(scarlet, run, capacity=ITERS):
    """(what run() returns, iterations per class, launches per class) of the launches inside run()"""
    L = scarlet._lib.lib
    scarlet._lib.check(L.scarlet_profile_begin(capacity))
    try:
        n = run()
    finally:
        ms, its, launches = (ctypes.c_double * 8)(), (ctypes.c_int64 * 8)(), (ctypes.c_int64 * 8)()
        scarlet._lib.check(L.scarlet_profile_end_ex(ms, its, launches))
    return n, list(its), list(launches)


# ------------------------------------------------------------------------------------------ 1. the host look
@pytest.mark.parametrize("name", FORMS)
def test_host_look_does_not_change_results(scarlet, name):
    f = form(scarlet, name)
    runs = []
    for check_every in (0, 3, 7):
        b = f.make()
        if name == "two_pipe":
            assert int(scarlet._lib.lib.scarlet_batch_pipelines(ctypes.byref(b._c))) == 2
        assert f.fit(b, ITERS, 0, check_every) == ITERS, check_every
        runs.append(state(b))
        assert (runs[-1]["it"] == ITERS).all() and not runs[-1]["status"].any(), check_every
    assert_identical(runs[0], runs[1], "%s: check_every 0 and 3" % name)
    assert_identical(runs[0], runs[2], "%s: check_every 0 and 7" % name)


# ------------------------------------------------------------------------------------------ 2. early stop
@pytest.mark.parametrize("name", FORMS)
def test_early_stop(scarlet, name):
    f = form(scarlet, name)
    b = f.make()
    st0 = state(b)
    for s in range(f.U):                 # on the CPU: the reference stops each scene at its first convergence test
        assert f.oracle_it(st0, s, ITERS, E_BIG) == FIRST_STOP, (name, s)
    assert f.fit(b, ITERS, E_BIG, 3) == 3
    st = state(b)
    assert (st["it"] == FIRST_STOP).all() and not st["active"].any(), (st["it"], st["active"])
    b = f.make()
    assert f.fit(b, ITERS, E_BIG, 0) == ITERS
    st = state(b)
    assert (st["it"] == FIRST_STOP).all() and not st["active"].any(), (st["it"], st["active"])


# ------------------------------------------------------------------------------------------ 3. launches per profile class
def _counts(scarlet, name, check_every=0, capacity=ITERS):
    f = form(scarlet, name)
    b = f.make()
    torch.cuda.synchronize()
    n, its, launches = profiled(scarlet, lambda: f.fit(b, ITERS, 0, check_every), capacity)
    assert n == ITERS
    return its, launches


@pytest.mark.parametrize("name", ["fused4", "iterate2"])
def test_fused_forms_launch_once_per_iteration(scarlet, name):
    its, launches = _counts(scarlet, name)
    assert its == launches == [0, 0, 0, 0, ITERS, 0, 0, 0], (its, launches)


@pytest.mark.parametrize("check_every,expected", [(0, 1), (3, 3)])
def test_persistent_kernel_launches_once_per_host_look(scarlet, check_every, expected):
    """7 iterations: one launch without a look; with a look every 3 the launches cover 3 + 3 + 1"""
    its, launches = _counts(scarlet, "fit2x", check_every)
    assert its == [0, 0, 0, 0, ITERS, 0, 0, 0] and launches == [0, 0, 0, 0, expected, 0, 0, 0], (its, launches)


def test_general_form_records_its_four_classes(scarlet):
    its, launches = _counts(scarlet, "general")
    assert its[:5] == launches[:5] == [ITERS] * 4 + [0], (its, launches)


def test_prior_form_records_the_prior_step_and_the_tail(scarlet):
    its, launches = _counts(scarlet, "prior")
    for cls in (2, 3, 6):
        assert its[cls] == launches[cls] == ITERS, (cls, its, launches)
    assert its[4] == launches[4] == 0, (its, launches)


def test_observation_form_records_its_four_classes(scarlet):
    its, launches = _counts(scarlet, "two_obs")
    assert its[:4] == launches[:4] == [ITERS] * 4, (its, launches)


def test_two_pipelines_record_twice_one_pipeline(scarlet):
    two = _counts(scarlet, "two_pipe", capacity=4 * ITERS)
    with option(scarlet, "NO_PIPELINE"):
        one = _counts(scarlet, "two_pipe", capacity=4 * ITERS)
    assert sum(one[1]) > 0
    for a, b in zip(one, two):
        assert [2 * v for v in a] == b, (one, two)


# ------------------------------------------------------------------------------------------ 4. all-NULL constraints
def _pair(scarlet, name):
    f = form(scarlet, name)
    return f, f.make(), f.make(), ctypes.byref(scarlet._lib.ScarletConstraints())


def _stream(scarlet):
    return scarlet._lib.stream_ptr()


@pytest.mark.parametrize("name", ["fused4", "fit2x", "general"])
def test_all_null_constraints_equal_scarlet_fit(scarlet, name):
    f, a, b, null = _pair(scarlet, name)
    L, approx = scarlet._lib.lib, int(f.approximate_L)
    assert L.scarlet_fit(ctypes.byref(a._c), ITERS, 0.0, approx, 3, _stream(scarlet)) == ITERS
    assert L.scarlet_fit_constrained(ctypes.byref(b._c), null, None, ITERS, 0.0, approx, 3, _stream(scarlet)) == ITERS
    assert_identical(state(a), state(b), name)


def _prior_struct(f, b):
    ps = b._prior_struct(f.prior())
    b._set_given(ps, [])
    return ps


def test_all_null_constraints_equal_scarlet_fit_prior(scarlet):
    f, a, b, null = _pair(scarlet, "prior")
    L = scarlet._lib.lib
    pa, pb = _prior_struct(f, a), _prior_struct(f, b)
    assert L.scarlet_fit_prior(ctypes.byref(a._c), ctypes.byref(pa), ITERS, 0.0, 0, 3, _stream(scarlet)) == ITERS
    assert L.scarlet_fit_constrained(ctypes.byref(b._c), null, ctypes.byref(pb), ITERS, 0.0, 0, 3, _stream(scarlet)) == ITERS
    assert_identical(state(a), state(b), "prior")
    torch.cuda.synchronize()
    assert torch.equal(a.L_components, b.L_components)


def test_all_null_constraints_equal_scarlet_fit_observations(scarlet):
    f, a, b, null = _pair(scarlet, "two_obs")
    L = scarlet._lib.lib

    def lists(x):
        n = len(x._observations)
        ptrs = (ctypes.POINTER(scarlet._lib.ScarletBatch) * n)(*[ctypes.pointer(ob._c) for _, ob in x._observations])
        band0 = np.array([o.band0 for o, _ in x._observations], dtype=np.int32)
        return ptrs, band0, n

    pa, ba, n = lists(a)
    assert L.scarlet_fit_observations(ctypes.byref(a._c), pa, ba.ctypes.data_as(ctypes.c_void_p), n, ITERS, 0.0, 0, 3,
                                      _stream(scarlet)) == ITERS
    pb, bb, n = lists(b)
    assert L.scarlet_fit_observations_constrained(ctypes.byref(b._c), null, pb, bb.ctypes.data_as(ctypes.c_void_p), n, ITERS,
                                                  0.0, 0, 3, _stream(scarlet)) == ITERS
    assert_identical(state(a), state(b), "two_obs")


@pytest.mark.parametrize("in_iteration", [0, 1])
def test_all_null_constraints_equal_scarlet_source_update(scarlet, in_iteration):
    """0: the constructors' update once more on the started batch; 1: inside a full iteration of the three phases"""
    _, a, b, null = _pair(scarlet, "iterate2")
    L, check, s = scarlet._lib.lib, scarlet._lib.check, _stream(scarlet)
    for x, plain in ((a, True), (b, False)):
        c = ctypes.byref(x._c)
        if in_iteration:
            check(L.scarlet_backward_step(c, 0, s))
        check(L.scarlet_source_update(c, in_iteration, s) if plain else
              L.scarlet_source_update_constrained(c, null, None, in_iteration, s))
        if in_iteration:
            check(L.scarlet_check_convergence(c, 0.0, s))
    sa = state(a)
    assert (sa["it"] == in_iteration).all()
    assert_identical(sa, state(b), "source_update(%d)" % in_iteration)


def test_all_null_constraints_equal_scarlet_source_update_prior(scarlet):
    f, a, b, null = _pair(scarlet, "prior")
    L, check, s = scarlet._lib.lib, scarlet._lib.check, _stream(scarlet)
    for x, plain in ((a, True), (b, False)):
        c, ps = ctypes.byref(x._c), _prior_struct(f, x)
        check(L.scarlet_backward_step_prior(c, ctypes.byref(ps), 0, s))
        check(L.scarlet_source_update_prior(c, ctypes.byref(ps), 1, s) if plain else
              L.scarlet_source_update_constrained(c, null, ctypes.byref(ps), 1, s))
        check(L.scarlet_check_convergence(c, 0.0, s))
    sa = state(a)
    assert (sa["it"] == 1).all()
    assert_identical(sa, state(b), "source_update_prior")
