"""CPU: the cases of tests/lipschitz_cases.py are admissible before any device sees them.

For every scene of every route: the float64 spectrum has its class's structure and the centres are usable; the reference's
own arithmetic (oracle.pgm.lipschitz: float32 np.linalg.eigvals) agrees with the float64 expected value to 1e-5, so a
device miss is not the reference's; and the tests have teeth -- a Gram pass that dropped the last pixels of a plane or of
a pixel chunk, the cross term of a pair or the last component of a ragged scene would move the expected value by more
than ten times the bound."""
import numpy as np
import pytest

import lipschitz_cases as lc

NAMES = list(lc.ROUTES)
TEETH = 10 * lc.TOL


@pytest.fixture(scope="module")
def states():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = lc.state(lc.ROUTES[name])
        return cache[name]
    return get


def test_the_table_covers_every_class_and_border():
    morph = {sc.morph for r in lc.ROUTES.values() for sc in r.scenes}
    sed = {sc.sed for r in lc.ROUTES.values() for sc in r.scenes}
    assert morph == set(lc.MORPH_CLASSES) and sed == set(lc.SED_CLASSES)
    pairs = lambda name: {sc.pair for sc in lc.ROUTES[name].scenes if sc.pair}
    assert {(7, 8), (8, 9), (15, 16), (0, 31)} <= pairs("bigk_k32_b8")
    huge = set().union(*(pairs(n) for n in NAMES if n.startswith("hugek")))
    assert {(31, 32), (32, 33), (15, 16), (47, 48), (0, 63), (0, 255), (224, 255)} <= huge
    assert {8, 9, 12} <= {sc.n for sc in lc.ROUTES["bigk_k12_ragged"].scenes}        # on and just after a chunk of eight
    assert {32, 33, 64} <= {sc.n for sc in lc.ROUTES["hugek_k64_ragged"].scenes}
    for r in lc.ROUTES.values():
        assert len(r.scenes) <= 8 and r.H <= 132 and r.W <= 128, r.name
    # the shapes the borders need: a pixel tail, the non-vector Gram, a second pixel chunk
    assert (46 * 50) % 128 and not (46 * 50) % 4 and (45 * 51) % 4 and 132 * 128 > 16384


@pytest.mark.parametrize("name", NAMES)
def test_structure_and_centres(states, name):
    r, st = lc.ROUTES[name], states(name)
    assert st.morph.dtype == np.float32 and st.sed.dtype == np.float32
    for s, sc in enumerate(r.scenes):
        G = lc.gram(st.morph[s], sc.n)
        lam = np.sort(np.linalg.eigvalsh(G))[::-1]
        what = (name, s, sc.morph)
        if sc.morph == "equal":
            assert lam[-1] >= lam[0] * (1 - 1e-7), what
        elif sc.morph == "coupled":
            assert lam[0] - lam[1] >= 1e-3 and lam[1] - lam[-1] <= 1e-6, what
        elif sc.morph == "rank1":
            assert lam[1] <= 1e-12 * lam[0], what
        elif sc.morph == "wide":
            d = np.diag(G)
            assert d.max() >= 1e11 * d.min(), what
        elif sc.morph == "pair":
            v = np.linalg.eigh(G)[1][:, -1]
            assert v[list(sc.pair)] @ v[list(sc.pair)] >= 0.99, what
        elif sc.morph == "twin":
            assert lam[-1] <= 1e-12 * lam[0], what
        elif sc.morph == "rotated_cluster":
            assert np.abs(lam - np.array(lc.CLUSTER[:sc.n])).max() <= 1e-6 and (st.morph[s] < 0).any(), what
        A = st.sed[s, :sc.n].astype(np.float64)
        mu = np.sort(np.linalg.eigvalsh(A.T @ A))[::-1]
        if sc.sed == "colour_twin" and r.B > 1:
            assert mu[1] <= 1e-12 * mu[0], what
        elif sc.sed == "own_band":
            assert mu[sc.n - 1] >= mu[0] * (1 - 1e-7) and not (A.T @ A - np.diag(np.diag(A.T @ A))).any(), what
        elif sc.sed == "rotated_cluster":
            assert np.abs(mu - np.array(lc.CLUSTER[:r.B])).max() <= 1e-6, what
        # absent components: zero planes and SEDs; every pixel of the frame carries weight, nothing lies outside it
        assert not st.morph[s, sc.n:].any() and not st.sed[s, sc.n:].any(), what
        own = np.zeros(r.H * r.W, bool)
        own[lc.own_pixels(r, s)] = True
        flat = st.morph[s].reshape(r.K, -1)
        assert not flat[:, ~own].any() and (np.abs(flat[:sc.n, own]).sum(axis=0) > 0).all(), what
        h, w = lc.frame_of(r, s)
        for k in range(sc.n):
            y, x = st.centers[s, k]
            assert 2 <= y < h - 2 and 2 <= x < w - 2, what + (k,)
            # (a patch that is one of the two outermost columns has no positive pixel 2 inside: lipschitz_cases.centres)
            assert st.morph[s, k, y, x] > 0 or (r.K % r.W == 0 and not (st.morph[s, k, 2:h - 2, 2:w - 2] > 0).any()), what + (k,)
    assert (st.n_components is None) == all(sc.n == r.K for sc in r.scenes)


@pytest.mark.parametrize("name", NAMES)
def test_the_reference_alone_stays_inside_the_bound(states, name):
    from oracle import pgm
    r, st = lc.ROUTES[name], states(name)
    for s, sc in enumerate(r.scenes):
        w_sed, w_morph = lc.want(st.morph[s], st.sed[s], sc.n, lc.n_obs(r))
        LA, LS = pgm.lipschitz(list(st.sed[s, :sc.n]), list(st.morph[s, :sc.n]), n_obs=lc.n_obs(r))
        errs = (LA / w_sed - 1, LS / w_morph - 1)
        print("lipschitz reference %s scene %d %s / %s: L_sed %+.2e L_morph %+.2e" % ((name, s, sc.morph, sc.sed) + errs))
        assert max(abs(e) for e in errs) <= lc.TOL, (name, s, sc, errs)


@pytest.mark.parametrize("name", NAMES)
def test_bounds_are_what_the_solvers_state(states, name):
    """the admitted interval of every constant: never wider than TOL but for the characteristic polynomial's documented
    overshoot on a cluster, which stays below 5e-5; float64 routes hold the code's own figures"""
    r, st = lc.ROUTES[name], states(name)
    for s, sc in enumerate(r.scenes):
        b_sed, b_morph = lc.bounds(r, sc, lc.gram(st.morph[s], sc.n), lc.sed_gram(r, sc, st.sed[s]))
        s_sed, s_morph = lc.solvers(r, sc)
        for (lo, hi), solver in ((b_sed, s_sed), (b_morph, s_morph)):
            assert -lc.TOL <= lo < 0 < hi <= (5e-5 if solver == "charpoly" else lc.TOL), (name, s, sc, lo, hi)
        if s_sed == "hugek":
            assert b_sed[1] == lc.F64 and -b_sed[0] <= 256 / (np.e * 2.0 ** 33) + lc.F64
        if s_morph != "charpoly":
            assert b_morph[1] == lc.F64 and -b_morph[0] <= 32 / (np.e * 2.0 ** 31) + lc.F64


def test_charpoly_upper_of_the_documented_cluster():
    """(1, 1, 1, 0.3) rotated: the floor's distance is 2.17e-5 (measured 2.27e-5 in the CPU restatement); a matrix solved
    by its start gets that start's distance"""
    q = lc._orthogonal(4, np.random.default_rng(7))
    up = lc.charpoly_upper(q @ np.diag(lc.CLUSTER) @ q.T)
    assert 1.5 * 2.16e-5 <= up <= 1.5 * 2.18e-5
    assert lc.charpoly_upper(np.eye(4)) == 0.0
    assert lc.charpoly_upper(np.diag([3.0, 1.0, 0.5, 0.1])) == 0.0


@pytest.mark.parametrize("name", NAMES)
def test_the_tests_have_teeth(states, name):
    r, st = lc.ROUTES[name], states(name)
    base = [lc.want(st.morph[s], st.sed[s], sc.n)[0] for s, sc in enumerate(r.scenes)]

    def moved(mutated):
        return [abs(lc.want(m, st.sed[s], n)[0] / base[s] - 1) for s, (m, n) in enumerate(mutated)]
    # a Gram pass that drops the last 4 pixels of every plane
    tail = moved([(lc.zero_pixels(st.morph[s], lc.last_pixels(r, s)), sc.n) for s, sc in enumerate(r.scenes)])
    print("lipschitz teeth %s: last 4 pixels %s" % (name, np.array2string(np.array(tail), precision=1)))
    assert max(tail) > TEETH, (name, tail)
    if r.K > 32:        # ... of every pixel chunk of k_huge_gram
        chunk = moved([(lc.zero_pixels(st.morph[s], lc.last_pixels(r, s, chunked=True)), sc.n) for s, sc in enumerate(r.scenes)])
        print("lipschitz teeth %s: last 4 pixels of every chunk %s" % (name, np.array2string(np.array(chunk), precision=1)))
        assert max(chunk) > TEETH, (name, chunk)
        if r.H * r.W > 16384:
            first = lc.last_pixels(r, 0, chunked=True)[:4]
            assert first[-1] + 1 == lc.huge_chunk_pix(r.H * r.W) < r.H * r.W
            inner = moved([(lc.zero_pixels(st.morph[s], first), sc.n) for s, sc in enumerate(r.scenes)])
            assert max(inner) > TEETH, (name, inner)
    # a Gram matrix without the pair's cross term: every pair case
    for s, sc in enumerate(r.scenes):
        if sc.pair:
            assert abs(lc.pair_without_cross_term(st.morph[s], sc) / base[s] - 1) > TEETH, (name, s, sc.pair)
    # a ragged scene read one component short
    ragged = [(s, sc) for s, sc in enumerate(r.scenes) if sc.n < r.K]
    if ragged:
        short = [abs(lc.want(st.morph[s], st.sed[s], sc.n - 1)[0] / base[s] - 1) for s, sc in ragged]
        assert max(short) > TEETH, (name, short)


@pytest.mark.parametrize("name", [n for n in NAMES if lc.ROUTES[n].kind != "grad"])
def test_one_iteration_keeps_every_component(states, name):
    """the routes that run a whole iteration (fused kernels, joint fits): from lipschitz_cases.images the float32 oracle's
    iteration leaves every component finite with a positive maximum, so `status` has no reason to be set"""
    from oracle import build as obuild, pgm
    obuild.build()
    r, st = lc.ROUTES[name], states(name)
    im = lc.images(st)
    assert im.dtype == np.float32 and np.isfinite(im).all()
    for s, sc in enumerate(r.scenes):
        h, w = lc.frame_of(r, s)
        assert not im[s, :, h:].any() and not im[s, :, :, w:].any()
        scene = pgm.scene_from_state(im[s, :, :h, :w], st.sed[s, :sc.n], st.morph[s, :sc.n, :h, :w], st.centers[s, :sc.n], None)
        if r.kind == "obs":
            first = np.cumsum((0,) + r.bands)
            scene.observations = [dict(images=im[s, b0:b0 + nb], band_slice=slice(b0, b0 + nb), weights=1, diff_kernel=None)
                                  for b0, nb in zip(first, r.bands)]
        if r.per_component:
            for k, src in enumerate(scene.sources):
                src.symmetric = k % 2 == 0
        pgm.fit(scene, 1, e_rel=0)
        for k, src in enumerate(scene.sources):
            assert np.isfinite(src.morph).all() and np.isfinite(src.sed).all() and src.morph.max() > 0, (name, s, k)
