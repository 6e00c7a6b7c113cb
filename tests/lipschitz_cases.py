"""States with prescribed Gram spectra for tests/test_gpu_lipschitz.py (the device run) and tests/test_lipschitz_cases.py
(their admissibility on the CPU).  Host only: numpy.

Every gradient step divides by L_sed = lambda_max(S S^T) of the morphology Gram matrix and L_morph = lambda_max(A^T A) of
the SED Gram matrix.  The library finds them with four algorithms (engine.h: lambda_max_charpoly4, jacobi_lambda_max,
wave_lambda_max8; the LDS squaring of bigk.h / multiobs_wide.h; the float64 chain of hugek.h) behind a dozen ways of
summing the Gram matrix.  ROUTES lists one small batch per way; each scene of a batch is one spectrum CLASS.

Basis.  One orthonormal non-negative patch e_j per present component on the scene's frame: pixel p (row-major over the
scene's own pixels) belongs to patch p mod n (n = K but in a ragged scene), values uniform in [0.5, 1.5], each patch scaled
to unit norm in float64 -- every pixel of the plane, the last ones included, carries weight in some patch.  A state is
morph = (C @ e).astype(float32), so its Gram matrix is C C^T up to float32 rounding.  SED matrices A (K x B) are built
directly.  The batch's images are the state's own model (`images`), so the iteration's step moves nothing.

Morphology classes (C is n x n over the scene's n present components; the planes of absent ones are zero)
  separated        diag(linspace(1, 2, n)) + 0.3 U[0, 1)
  equal            I: an n-fold top eigenvalue (equal to ~5e-9 after float32 rounding)
  coupled          I + 1e-3: a simple top eigenvalue 1e-3 n above an (n - 1)-fold cluster
  twin             I + 0.2 U with row 1 copied from row 0: a singular Gram matrix
  rank1            every morphology the same shape at another amplitude (the "similar colour" situation of A^T A)
  wide             rows of I + 0.1 U scaled by logspace(-3, 3, n): Gram entries from 1e-6 to 1e6
  pair(i, j)       1e-3 I with C[i, i] = C[j, j] = 1, C[j, i] = 0.7: lambda_max is decided by the Gram entries (i, i),
                   (i, j), (j, j) alone -- placed on the borders each route has (chunks of 8, blocks of 32, MFMA halves)
  rotated_cluster  signed, n <= 4: Q diag(1, 1, 1, 0.3)[:n] Q^T with a random orthogonal Q -- the characteristic polynomial's
                   worst case with a start that is not tight (the constants are computed before any constraint runs)
SED classes
  colour_twin      all SEDs proportional
  own_band         (K <= B) component k in band k only, equal amplitudes: a diagonal multiple root
  separated        diag-like + 0.3 U
  wide             rows scaled by logspace(-3, 3, K)
  rotated_cluster  (B <= 4, K >= B) A^T A = Q diag(1, 1, 1, 0.3)[:B] Q^T
"""
import collections
import math
import zlib

import numpy as np

TOL = 1e-5                      # parity_common.TOL: an L off by more moves the step by as much
FRAMES = ((24, 32), (17, 23), (20, 28))          # the ragged-frames route: scene s has FRAMES[s % 3], planes zero outside

Scene = collections.namedtuple("Scene", "morph sed n pair")
Route = collections.namedtuple("Route", "name kind K B H W scenes opts psf frames per_component bands wide plan classes")

MORPH_CLASSES = ("separated", "equal", "coupled", "twin", "rank1", "wide", "pair", "rotated_cluster")
SED_CLASSES = ("colour_twin", "own_band", "separated", "wide", "rotated_cluster")
CLUSTER = (1.0, 1.0, 1.0, 0.3)


# ------------------------------------------------------------------------------------------------------- the table
def _sed_cycle(K, B, count):
    """SED classes paired with the morphology classes scene by scene: the ones this (K, B) admits, in turn"""
    ok = [c for c in SED_CLASSES if not (c == "own_band" and K > B) and not (c == "rotated_cluster" and (B > 4 or K < B))]
    return [ok[i % len(ok)] for i in range(count)]


def _scenes(K, B, specs):
    """specs: morphology class names, ("pair", i, j), or (class or pair tuple, n) for a ragged scene"""
    seds, out = _sed_cycle(K, B, len(specs)), []
    for spec, sed in zip(specs, seds):
        n = K
        if isinstance(spec, tuple) and spec[0] != "pair":
            spec, n = spec
        pair = None
        if isinstance(spec, tuple):
            pair, spec = (spec[1], spec[2]), "pair"
        assert spec in MORPH_CLASSES and 1 <= n <= K and (pair is None or pair[0] < pair[1] < n)
        out.append(Scene(spec, sed, n, pair))
    return tuple(out)


def _small(K):
    """the classes of a K <= 8 route"""
    s = ["separated", "equal", "coupled", "twin", "rank1", "wide", ("pair", 0, K - 1)]
    s.append("rotated_cluster" if K <= 4 else ("pair", 3, 4))
    return s


def _r(name, kind, K, B, H, W, specs, opts=(), psf=False, frames=False, per_component=False, bands=None, wide=False,
       plan=0, classes="01"):
    return Route(name, kind, K, B, H, W, _scenes(K, B, specs), tuple(opts), psf, frames, per_component, bands, wide, plan, classes)


def _routes():
    R = []
    # ---- the fused one-launch kernels: `fit(1)`; plan = scarlet_debug_fused_plan's kernel, one launch of class 4
    f = dict(kind="fused", classes="4")
    R += [_r("fit2x", K=4, B=5, H=64, W=64, specs=_small(4), opts=[("PERSIST_DBG", 2)], plan=3, **f),
          _r("iterate2_exact", K=4, B=5, H=64, W=64, specs=_small(4), plan=4, **f),
          _r("iterate2_k3_b3", K=3, B=3, H=24, W=32, specs=_small(3), plan=5, **f),
          _r("iterate2_k4_b5", K=4, B=5, H=16, W=16, specs=_small(4), plan=5, **f),
          _r("iterate_b6", K=4, B=6, H=24, W=32, specs=_small(4), plan=6, **f),
          _r("iterate_b8", K=4, B=8, H=24, W=32, specs=_small(4), plan=7, **f),
          _r("iterate_v1", K=2, B=3, H=24, W=32, specs=_small(2), opts=[("FUSED_V1", 1)], plan=6, **f),
          _r("iterate_per_component", K=3, B=6, H=24, W=32, specs=_small(3), per_component=True, plan=1, **f),
          _r("iterate_frames", K=3, B=6, H=24, W=32, specs=_small(3), frames=True, plan=8, **f)]
    # ---- k_grad / k_step (scarlet_backward_gradients: the constants without a step)
    g = dict(kind="grad")
    R += [_r("general_k3_b3", K=3, B=3, H=24, W=32, specs=_small(3), opts=[("NO_FUSED", 1)], **g),
          _r("general_k4_b4_odd", K=4, B=4, H=23, W=31, specs=_small(4), opts=[("NO_FUSED", 1)], **g),
          _r("general_k6_b7_odd", K=6, B=7, H=23, W=31, specs=_small(6), **g),
          _r("general_k8_b8", K=8, B=8, H=24, W=32, specs=_small(8), **g)]
    # ---- a difference kernel: three-pass (k_step_psf4f), four-pass (k_step_psf4), odd plane (k_step_psf)
    for K in (3, 6):
        for B in (3, 5, 7):
            R.append(_r("psf_three_pass_k%d_b%d" % (K, B), K=K, B=B, H=24, W=32, specs=_small(K), psf=True, classes="15", **g))
    R += [_r("psf_four_pass_k3_b3", K=3, B=3, H=24, W=32, specs=_small(3), psf=True, opts=[("NO_PSF3PASS", 1)], classes="015", **g),
          _r("psf_four_pass_k6_b5", K=6, B=5, H=24, W=32, specs=_small(6), psf=True, opts=[("NO_PSF3PASS", 1)], classes="015", **g),
          _r("psf_odd_plane_k3_b5", K=3, B=5, H=23, W=31, specs=_small(3), psf=True, classes="015", **g),
          _r("psf_odd_plane_k6_b7", K=6, B=7, H=23, W=31, specs=_small(6), psf=True, classes="015", **g)]
    # ---- 8 < K <= 32: k_bigk_lipschitz (LDS squaring) beside k_bigk_lmorph; pairs across the chunks of eight
    k9 = ["separated", "equal", "coupled", "twin", "rank1", "wide", ("pair", 7, 8), ("pair", 0, 8)]
    R += [_r("bigk_k9_b3", K=9, B=3, H=32, W=32, specs=k9, **g),
          _r("bigk_k32_b8", K=32, B=8, H=32, W=32, specs=["equal", "coupled", "wide", "rank1", ("pair", 7, 8), ("pair", 8, 9),
                                                         ("pair", 15, 16), ("pair", 0, 31)], **g),
          _r("bigk_k12_ragged", K=12, B=3, H=32, W=32, specs=[("separated", 9), ("separated", 8), (("pair", 7, 8), 9),
                                                             (("pair", 0, 7), 8), ("pair", 8, 9), "wide"], **g),
          _r("bigk_one_stream", K=9, B=8, H=32, W=32, specs=k9, opts=[("NO_SIDE_STREAM", 1)], **g),
          _r("bigk_chunked", K=9, B=8, H=32, W=32, specs=k9, opts=[("NO_BIGK_FUSED", 1)], **g),
          _r("bigk_chunked_no_mfma", K=9, B=8, H=32, W=32, specs=k9, opts=[("NO_BIGK_FUSED", 1), ("NO_GRAM_MFMA", 1)], **g),
          # (the single-lane Jacobi of k_bigk_lipschitz runs only in the chunked form on one stream)
          _r("bigk_chunked_one_stream", K=9, B=8, H=32, W=32, specs=k9, opts=[("NO_BIGK_FUSED", 1), ("NO_SIDE_STREAM", 1)], **g),
          # ... and, with the default switches, behind a difference kernel (the planes tail of backward_step_psf)
          _r("bigk_psf", K=9, B=8, H=32, W=32, specs=k9, psf=True, classes="015", **g)]
    # ---- K > 32: the float64 chain of hugek.h; pairs across the 32-blocks and the 16-row MFMA halves, ragged counts on
    # and just after a block, the pixel tail, the non-vector form (H W % 4 != 0), two pixel chunks (H W > 16384)
    k33 = ["separated", "equal", "coupled", "twin", "rank1", "wide", ("pair", 31, 32), ("pair", 0, 32)]
    R += [_r("hugek_k33_tail", K=33, B=3, H=46, W=50, specs=k33, **g),
          _r("hugek_k33_odd", K=33, B=3, H=45, W=51, specs=k33, **g),
          _r("hugek_k64_ragged", K=64, B=3, H=48, W=48, specs=[("pair", 32, 33), ("pair", 47, 48), ("pair", 15, 16),
                                                              (("pair", 31, 32), 33), ("separated", 33), ("separated", 32),
                                                              ("equal", 32), ("pair", 0, 63)], **g),
          _r("hugek_k40_two_chunks", K=40, B=3, H=132, W=128, specs=["separated", "rank1", "wide", ("pair", 31, 32), "equal"], **g),
          _r("hugek_k256", K=256, B=8, H=32, W=32, specs=[("pair", 224, 255), ("pair", 0, 255), "twin", "coupled", "wide",
                                                         "separated"], **g)]
    # ---- joint fits (`step`): k_obs_head, obs_lipschitz_sed, the factor n_obs; plan = scarlet_debug_contract_plan's kernel
    o = dict(kind="obs", classes="0123")
    R += [_r("joint_k3", K=3, B=5, H=24, W=32, specs=_small(3), bands=(3, 2), plan=1, **o),
          _r("joint_k6", K=6, B=5, H=24, W=32, specs=_small(6), bands=(3, 2), plan=1, **o),
          _r("joint_k9", K=9, B=5, H=32, W=32, specs=k9, bands=(3, 2), plan=2, **o),
          _r("joint_k33", K=33, B=5, H=46, W=50, specs=k33, bands=(3, 2), plan=2, **o)]
    # ---- wide joint fits: k_wide_lmorph over n = min(K, C) <= 32
    k40 = ["separated", "equal", "coupled", "rank1", "wide", ("pair", 31, 32)]
    R += [_r("wide_k3_c17", K=3, B=17, H=24, W=32, specs=_small(3), bands=(8, 8, 1), wide=True, plan=3, **o),
          _r("wide_k9_c32", K=9, B=32, H=32, W=32, specs=k9, bands=(8, 8, 8, 8), wide=True, plan=3, **o),
          _r("wide_k40_c17", K=40, B=17, H=48, W=48, specs=k40, bands=(8, 8, 1), wide=True, plan=3, **o),
          _r("wide_k40_c32", K=40, B=32, H=48, W=48, specs=k40, bands=(8, 8, 8, 8), wide=True, plan=3, **o)]
    return collections.OrderedDict((r.name, r) for r in R)


ROUTES = _routes()


# ------------------------------------------------------------------------------------------------------- the states
def frame_of(r, s):
    return FRAMES[s % len(FRAMES)] if r.frames else (r.H, r.W)


def own_pixels(r, s):
    """flat indices into the padded H x W plane of the scene's own pixels, row-major"""
    h, w = frame_of(r, s)
    return (np.arange(h)[:, None] * r.W + np.arange(w)[None, :]).reshape(-1)


def basis(r, s, rng):
    """(n, H W) float64: one orthonormal non-negative patch per present component on the scene's own pixels"""
    own, n = own_pixels(r, s), r.scenes[s].n
    e = np.zeros((n, r.H * r.W))
    val = rng.uniform(0.5, 1.5, size=len(own))
    for j in range(n):
        e[j, own[j::n]] = val[j::n]
    return e / np.sqrt((e * e).sum(axis=1, keepdims=True))


def _orthogonal(n, rng):
    q, t = np.linalg.qr(rng.standard_normal((n, n)))
    return q * np.sign(np.diag(t))


def mixing(sc, rng):
    """C (n x n) of the scene's class"""
    n, c = sc.n, sc.morph
    if c == "separated":
        return np.diag(np.linspace(1.0, 2.0, n)) + 0.3 * rng.random((n, n))
    if c == "equal":
        return np.eye(n)
    if c == "coupled":
        return np.eye(n) + 1e-3
    if c == "twin":
        C = np.eye(n) + 0.2 * rng.random((n, n))
        C[1] = C[0]
        return C
    if c == "rank1":
        return np.outer(np.linspace(0.5, 2.0, n), np.ones(n) / math.sqrt(n))
    if c == "wide":
        return (np.eye(n) + 0.1 * rng.random((n, n))) * np.logspace(-3, 3, n)[:, None]
    if c == "pair":
        i, j = sc.pair
        C = 1e-3 * np.eye(n)
        C[i, i] = C[j, j] = 1.0
        C[j, i] = 0.7
        return C
    if c == "rotated_cluster":
        C = _orthogonal(n, rng) * np.sqrt(np.array(CLUSTER[:n]))         # C C^T = Q diag Q^T
        return C * np.where(np.diag(C) < 0, -1.0, 1.0)[:, None]          # (row signs: another Q; own patch positive)
    raise ValueError(c)


def sed_matrix(sc, K, B, rng):
    """A (K x B) of the scene's SED class; the rows of absent components are zero"""
    n, c = sc.n, sc.sed
    A = np.zeros((K, B))
    if c == "colour_twin":
        A[:n] = np.outer(np.linspace(0.5, 2.0, n), 0.3 + rng.random(B))
    elif c == "own_band":
        A[:n, :n] = 0.8 * np.eye(n)
    elif c == "separated":
        A[:n] = 0.3 * rng.random((n, B))
        A[np.arange(n), np.arange(n) % B] += np.linspace(1.0, 2.0, n)
    elif c == "wide":
        A[:n] = (0.3 + rng.random((n, B))) * np.logspace(-3, 3, n)[:, None]
    elif c == "rotated_cluster":
        assert n >= B
        A[:B] = np.sqrt(np.array(CLUSTER[:B]))[:, None] * _orthogonal(B, rng).T      # A^T A = Q diag Q^T
    else:
        raise ValueError(c)
    return A


def centres(r, morph):
    """(S, K, 2): for every component the first pixel at least 2 inside its scene's frame where its own plane is positive
    (absent components, whose centres nobody reads: (2, 2)).  Where K is a multiple of the row length a patch is a
    column, and the patches of the two outermost columns have no such pixel: their centres are the first positive pixel
    moved 2 inside.  Only routes that run no constraint (scarlet_backward_gradients with K > 8) have such patches."""
    out = np.full(morph.shape[:2] + (2,), 2, dtype=np.int32)
    for s in range(morph.shape[0]):
        h, w = frame_of(r, s)
        for k in range(r.scenes[s].n):
            inner = morph[s, k, 2:h - 2, 2:w - 2] > 0
            if inner.any():
                y, x = np.unravel_index(int(np.argmax(inner)), inner.shape)
                out[s, k] = (y + 2, x + 2)
            else:
                assert r.kind == "grad" and r.K > 8 and r.K % r.W == 0, (r.name, s, k)
                y, x = np.unravel_index(int(np.argmax(morph[s, k] > 0)), (r.H, r.W))
                out[s, k] = (min(max(y, 2), h - 3), min(max(x, 2), w - 3))
    return out


State = collections.namedtuple("State", "morph sed centers n_components C")


def state(r):
    """the route's batch: morph (S, K, H, W) and sed (S, K, B) float32, centres, counts (None: every scene has K), and the
    float64 mixing matrices the classes were built from"""
    S = len(r.scenes)
    morph, sed, Cs = np.zeros((S, r.K, r.H * r.W), np.float32), np.zeros((S, r.K, r.B), np.float32), []
    for s, sc in enumerate(r.scenes):
        rng = np.random.default_rng([zlib.crc32(r.name.encode()), s])        # (by name: a new route moves no other's state)
        C = mixing(sc, rng)
        morph[s, :sc.n] = (C @ basis(r, s, rng)).astype(np.float32)
        sed[s] = sed_matrix(sc, r.K, r.B, rng).astype(np.float32)
        Cs.append(C)
    morph = morph.reshape(S, r.K, r.H, r.W)
    counts = np.array([sc.n for sc in r.scenes], dtype=np.int32)
    return State(morph, sed, centres(r, morph), None if (counts == r.K).all() else counts, Cs)


def images(st):
    """(S, B, H, W) float32: the state's own model sum_k sed_k x morph_k.  The iteration's gradient then vanishes, so the
    step and the constraints after it leave every component where it is: stepped towards arbitrary data, a component
    1e-3 of its neighbours (wide) can be wiped out, and the normalisation of the empty plane sets
    SCARLET_STATUS_NONFINITE -- a fault of the scene, not of the constants."""
    return np.einsum("skb,skp->sbp", st.sed.astype(np.float64), st.morph.reshape(st.morph.shape[:2] + (-1,)).astype(np.float64)) \
        .reshape((st.sed.shape[0], st.sed.shape[2]) + st.morph.shape[2:]).astype(np.float32)


def n_obs(r):
    return len(r.bands) if r.bands else 1


# ------------------------------------------------------------------------------------------------ expected values
def gram(morph32, n):
    M = np.asarray(morph32[:n], dtype=np.float64).reshape(n, -1)
    return M @ M.T


def want(morph32, sed32, n, n_obs=1):
    """(L_sed, L_morph): n_obs x the largest eigenvalues of the float64 Gram matrices of the float32 arrays"""
    A = np.asarray(sed32[:n], dtype=np.float64)
    return n_obs * np.linalg.eigvalsh(gram(morph32, n)).max(), n_obs * np.linalg.eigvalsh(A.T @ A).max()


def charpoly_upper(G):
    """The relative overshoot lambda_max_charpoly4's stopping floor admits on the symmetric PSD matrix G (n <= 4), from the
    matrix's own float64 spectrum and the constants of engine.h; no solver runs.

    Newton descends from start = min(trace, largest absolute row sum) and stops once p(x) <= 2^-47 x^4.  With the top
    eigenvalue lambda_1 of multiplicity m (eigenvalues within 1e-6 relative: float32 rounding spreads a cluster by ~1e-7)
    and the others at ratios rho_j, p(lambda_1 (1 + d)) = lambda_1^4 d^m prod(1 + d - rho_j), so the floor is reached at
    d = (2^-47 / prod(1 - rho_j))^(1 / m).  The rounding noise of p at the floor is covered by a factor 1.5 (the CPU
    restatement measured 2.27e-5 for (1, 1, 1, 0.3) against d = 2.17e-5).  Never above the start's own distance."""
    G = np.asarray(G, dtype=np.float64)
    lam = np.sort(np.linalg.eigvalsh(G))[::-1]
    top = lam[0]
    cluster = lam >= top * (1 - 1e-6)
    m = int(cluster.sum())
    rho = lam[~cluster] / top
    delta = (2.0 ** -47 / np.prod(1.0 - rho)) ** (1.0 / m)
    start = min(np.trace(G), np.abs(G).sum(axis=1).max())
    return max(0.0, min(start / top - 1.0, 1.5 * delta))


def solvers(r, sc):
    """(solver of L_sed, solver of L_morph) as the host code and the kernels dispatch them for this route and scene"""
    small_morph = "charpoly" if r.B <= 4 else "wave8"
    if r.kind == "fused":
        # K <= 4 is these kernels' admission and lambda_max(A^T A) comes from the smaller of A A^T (K <= B) and A^T A
        return "charpoly", "charpoly"
    if r.kind == "grad":
        if r.K <= 8:
            return ("charpoly" if r.K <= 4 else "wave8"), small_morph
        if r.K <= 32:
            # k_bigk_lmorph is wave_lambda_max8 for every B; the chunked form on one stream, and the planes tail of a
            # difference kernel, leave both constants to k_bigk_lipschitz, whose lambda_max(A^T A) is the Jacobi
            opts = dict(r.opts)
            jacobi = r.psf or (opts.get("NO_SIDE_STREAM") and opts.get("NO_BIGK_FUSED"))
            return "bigk", "jacobi" if jacobi else "wave8"
        return "hugek", "wave8"
    # joint fits: k_obs_head takes the scene's own count; above 8 components obs_lipschitz_sed
    sed = ("charpoly" if sc.n <= 4 else "wave8") if r.K <= 8 else "bigk" if r.K <= 32 else "hugek"
    return sed, "wide" if r.wide else "wave8"


def squaring_deficit(order, q):
    """what the Rayleigh quotient after q trace-normalised squarings of a matrix of (padded) order `order` may miss,
    relative (engine.h, bigk.h, hugek.h: n / (e 2^(q + 1)) "whatever the gaps")"""
    return order / (math.e * 2.0 ** (q + 1))


F64 = 1e-12           # float64 rounding of a Gram sum and a solver at n = 256


def sed_gram(r, sc, sed32):
    """the SED Gram matrix the route's solver sees: A^T A, in the fused kernels A A^T where K <= B (same lambda_max)"""
    A = np.asarray(sed32[:sc.n], dtype=np.float64)
    return A @ A.T if (r.kind == "fused" and r.K <= r.B) else A.T @ A


def bounds(r, sc, G, AtA):
    """((lo, hi) of L_sed, (lo, hi) of L_morph): the admitted got / want - 1.  G: the morphology Gram matrix of the present
    components, AtA: sed_gram.

    Everywhere TOL.  lambda_max_charpoly4 with n >= 3 on a cluster class (equal, own_band, rotated_cluster) may overshoot by
    charpoly_upper, a documented property of that solver.  Where the Gram matrix is summed in float64 and the solver is
    float64 -- hugek's L_sed, every L_morph -- the code's own bounds hold: a Rayleigh quotient never exceeds lambda_max and
    misses at most squaring_deficit; the Jacobi is exact to rounding.  The float32-summed Gram matrices (k_grad, the fused
    kernels, bigk's passes, the contraction) have no sharper bound than TOL."""
    s_sed, s_morph = solvers(r, sc)
    n_sed = r.K if r.kind != "obs" else sc.n
    if s_sed == "charpoly" and sc.morph in ("equal", "rotated_cluster") and n_sed >= 3:
        b_sed = (-TOL, max(TOL, charpoly_upper(G)))
    elif s_sed == "hugek":
        b_sed = (-(squaring_deficit(32 * ((sc.n + 31) // 32), 32) + F64), F64)
    else:
        b_sed = (-TOL, TOL)
    if s_morph == "charpoly":
        hi = max(TOL, charpoly_upper(AtA)) if sc.sed in ("own_band", "rotated_cluster") and len(AtA) >= 3 else TOL
        b_morph = (-TOL, hi)
    elif s_morph == "jacobi":
        b_morph = (-F64, F64)
    else:
        b_morph = (-(squaring_deficit(32 if s_morph == "wide" else 8, 30) + F64), F64)
    return b_sed, b_morph


# ------------------------------------------------------------------------------------------------------ mutations
def huge_chunk_pix(HW):
    """hugek.h: pixels per Gram workgroup"""
    c = min((HW + 16384 - 1) // 16384, 16)
    return ((HW + c - 1) // c + 127) & ~127


def last_pixels(r, s, chunked=False):
    """flat indices of the last 4 pixels of the scene's planes (of every pixel chunk of k_huge_gram with `chunked`)"""
    own = own_pixels(r, s)
    if not chunked:
        return own[-4:]
    per, HW = huge_chunk_pix(r.H * r.W), r.H * r.W
    ends = [min(HW, e) for e in range(per, HW + per, per)]
    return np.concatenate([np.arange(e - 4, e) for e in ends])


def zero_pixels(morph, idx):
    out = morph.reshape(morph.shape[0], -1).copy()
    out[:, idx] = 0
    return out.reshape(morph.shape)


def pair_without_cross_term(morph32, sc):
    """lambda_max of the scene's float64 Gram matrix with entry (i, j) zeroed"""
    G = gram(morph32, sc.n)
    i, j = sc.pair
    G[i, j] = G[j, i] = 0
    return np.linalg.eigvalsh(G).max()
