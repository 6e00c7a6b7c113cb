"""The cases of the launch plans ("One plan"; scarlet_amd/csrc/launch_plan.h): every form the fused launch,
the constraint update, the stand-alone operators and the initialisers can take, each at the smallest shape that
reaches it.  For tools/gradstages_ab.py --cases launch_form_cases: build-against-build dumps and runs for a kernel
trace (the interface of tests/gradient_stage_cases.py: CASES, scenes, make_batch, options, state).

Every case is 2 scenes of 2 to 4 components and 3 iterations at e_rel = 0 (`iters`: a case that needs its own
number, whatever the tool asks for -- the persistent k_fit2x takes a launch of more than one iteration, its
one-iteration twin exactly one).  The scenes are Gaussian blobs on noise, seeded by the shape: the comparison is
between two builds, not against the oracle, so no seed is searched for.  Kinds: `fit` (a batch started with
init_extended, or init_sources with a `group`), `op` (the stand-alone operators on the first planes of the scenes),
`init` (the two initialisers themselves: the compared launches are theirs and their constructor updates').
"""
import collections

import numpy as np

BG = 0.1
ITERS = 3
S = 2
HIPFFT_CASES = []
SIDE_STREAM_CASES = ()

Case = collections.namedtuple("Case", "name kind K B H W approximate_L opts iters batch")


def _c(name, K, B, H, W, kind="fit", opts=(), iters=None, **batch):
    return Case(name, kind, K, B, H, W, False, tuple(opts), iters, batch)


GROUP = [[0, 0, -1]] * S          # a two-layer source beside a source of its own
TAIL = ["NO_FUSED"]
CASES = collections.OrderedDict((c.name, c) for c in [
    # ---- the fused launch (W % 4 == 0, exact constants)
    _c("01_iterate2", 3, 3, 16, 16),                                        # k_iterate2<4, 5>
    _c("02_fused_v1", 3, 3, 16, 16, opts=["FUSED_V1"]),                     # k_iterate<4, 6>
    _c("03_exact_one_iteration", 4, 5, 64, 64, iters=1),                    # k_iterate2<4, 5, 64>
    _c("04_exact_persistent", 4, 5, 64, 64, iters=3),                       # k_fit2x
    _c("05_exact_no_exact", 4, 5, 64, 64, opts=["NO_EXACT"], iters=3),      # k_iterate2<4, 5>
    _c("06_exact_no_persist", 4, 5, 64, 64, opts=["NO_PERSIST"], iters=3),  # k_iterate2<4, 5, 64>
    _c("07_iterate_b6", 2, 6, 16, 16),                                      # k_iterate<4, 6>
    _c("08_iterate_b7", 2, 7, 16, 16),                                      # k_iterate<4, 8>
    _c("09_per_component_b3", 2, 3, 16, 16, symmetric=[True, False]),       # k_iterate<4, 6, FusedArgsPC>
    _c("10_per_component_b7", 2, 7, 16, 16, symmetric=[True, False]),       # k_iterate<4, 8, FusedArgsPC>
    # ---- the tail of a general iteration
    _c("11_wave", 3, 3, 16, 20, opts=TAIL),                                 # k_source_update_w
    _c("12_force_block", 3, 3, 16, 20, opts=TAIL + ["FORCE_BLOCK_UPDATE"]),  # <0>
    _c("13_box_68", 3, 3, 68, 68, opts=TAIL),                               # box <8, 0>, listed, <0> on the flagged
    _c("14_box_68_no_box2", 3, 3, 68, 68, opts=TAIL + ["NO_BOX2"]),
    _c("15_box_68_no_box", 3, 3, 68, 68, opts=TAIL + ["NO_BOX"]),           # <0> on the full frame
    _c("16_not_monotonic_68", 3, 3, 68, 68, opts=TAIL, monotonic=False),    # no box
    _c("17_tile_gscratch_96", 3, 3, 96, 96, opts=TAIL),                     # <1>
    _c("18_plane_132", 3, 3, 132, 132, opts=TAIL),                          # box <16, 0>, <2>
    _c("19_box_128", 3, 3, 128, 128, opts=TAIL),                            # box <8, 128>
    _c("20_box_128_no_exact", 3, 3, 128, 128, opts=TAIL + ["NO_EXACT"]),    # box <8, 0>
    _c("21_box_256", 2, 3, 256, 256, opts=TAIL),                            # box <16, 256>
    _c("22_box_streamed_260", 2, 3, 260, 260, opts=TAIL),                   # box <0, 0>
    _c("23_group", 3, 3, 16, 20, opts=TAIL, group=GROUP),                   # k_group_centers
    # ---- the stand-alone operators
    _c("24_op_wave", 2, 3, 16, 16, kind="op"),                              # k_operator_w
    _c("25_op_nearest", 2, 3, 16, 16, kind="op"),                           # k_operator<false>
    _c("26_op_tile_68", 2, 3, 68, 68, kind="op"),                           # k_operator<false>
    _c("27_op_plane_140", 2, 3, 140, 140, kind="op"),                       # k_operator<true>, with and without scratch
    # ---- the initialisers
    _c("28_init_lds", 3, 3, 16, 16, kind="init"),                           # the float64 tile in LDS
    _c("29_init_hbm", 3, 3, 144, 144, kind="init"),                         # ... in HBM; the update that follows: <2>
])


def scenes(c, seeds=None):
    """images (S, B, H, W), centers (S, K, 2): blobs at least 3 pixels apart and 4 from the edges, noise 0.1 (sources on
    the borders of the same cases come from tests/edge_cases.py)"""
    rng = np.random.default_rng(seeds or [c.K, c.B, c.H, c.W])
    grouped = c.batch.get("group") is not None or c.kind == "init"
    images, centers = np.zeros((S, c.B, c.H, c.W)), np.zeros((S, c.K, 2), np.int32)
    yy, xx = np.mgrid[:c.H, :c.W].astype(np.float64)
    for s in range(S):
        cen = []
        while len(cen) < c.K:
            p = (int(rng.integers(4, c.H - 4)), int(rng.integers(4, c.W - 4)))
            if grouped and len(cen) == 1:
                p = cen[0]                              # the two layers of the group share their centre
            elif any(max(abs(p[0] - y), abs(p[1] - x)) < 3 for y, x in cen):
                continue
            cen.append(p)
        for k, (cy, cx) in enumerate(cen):
            if grouped and k == 1:
                continue
            blob = np.exp(-0.5 * (((yy - cy) / rng.uniform(1.5, 3.0)) ** 2 + ((xx - cx) / rng.uniform(1.5, 3.0)) ** 2))
            images[s] += (rng.uniform(5.0, 50.0) * rng.uniform(0.2, 1.0, size=c.B))[:, None, None] * blob
        centers[s] = cen
    images += rng.normal(0.0, 0.1, size=images.shape)
    return images.astype(np.float32), centers


class _Run(object):
    """an `op` or `init` case behind a batch's face: fit() makes the compared launches, state() returns `arrays`"""

    def __init__(self, scarlet, c, images, centers):
        self.scarlet, self.c, self.images, self.centers, self.arrays = scarlet, c, images, centers, {}

    def fit(self, iters, e_rel=0, approximate_L=False):
        (self._operators if self.c.kind == "op" else self._initialisers)()
        return iters

    def _initialisers(self):
        bg = np.ones(self.c.B) * BG
        b = self.scarlet.BlendBatch(self.images, self.centers).init_extended(bg)
        g = self.scarlet.BlendBatch(self.images, self.centers, group=GROUP).init_sources(bg)
        for tag, x in (("extended_", b), ("sources_", g)):
            self.arrays.update((tag + k, v) for k, v in state(x).items())

    def _operators(self):
        import torch
        from scarlet_amd import operator as op, _lib as L
        from scarlet_amd.batch import default_centroid_weight
        c, cen = self.c, [tuple(int(v) for v in p) for p in self.centers[:, 0]]
        planes = [np.ascontiguousarray(self.images[s, 0]) for s in range(S)]
        for s, (X, p) in enumerate(zip(planes, cen)):
            def keep(name, a, s=s):
                self.arrays["%s_%d" % (name, s)] = np.array(a)
            if c.name == "25_op_nearest":
                keep("nearest", op.prox_strict_monotonic(X.shape, use_nearest=True, center=p)(X.copy(), 0))
                continue
            keep("weighted", op.prox_strict_monotonic(X.shape, center=p)(X.copy(), 0))
            keep("kspace", op.prox_uncentered_symmetry(X.copy(), 0, center=p, shift=np.array([0.25, -0.125])))   # (with scratch)
            keep("sdss", op.prox_uncentered_symmetry(X.copy(), 0, center=p, algorithm="sdss"))
            xs = torch.as_tensor(X[None]).cuda()
            cs = torch.as_tensor(np.array([p], np.int32)).cuda()
            st = torch.zeros(1, dtype=torch.int32, device="cuda")
            sh = torch.zeros((1, 2), dtype=torch.float64, device="cuda")
            psf = torch.as_tensor(default_centroid_weight()).cuda().contiguous()
            L.check(L.lib.scarlet_max_pixel(L.ptr(xs), 1, c.H, c.W, L.ptr(cs), L.ptr(st), L.stream_ptr()))
            keep("max_pixel", cs.cpu().numpy())
            L.check(L.lib.scarlet_psf_weighted_centroid(L.ptr(xs), 1, c.H, c.W, L.ptr(psf), int(psf.shape[0]), L.ptr(cs),
                                                        L.ptr(sh), L.ptr(st), L.stream_ptr()))
            keep("centroid", np.concatenate([cs.cpu().numpy().ravel(), sh.cpu().numpy().ravel(), st.cpu().numpy()]))


def make_batch(scarlet, c, images, centers, mse_capacity=ITERS + 1):
    """the case's freshly initialised batch (the same state every time)"""
    if c.kind != "fit":
        return _Run(scarlet, c, images, centers)
    b = scarlet.BlendBatch(images, centers, mse_capacity=mse_capacity, **c.batch)
    return b.init_sources(np.ones(c.B) * BG) if b.group is not None else b.init_extended(np.ones(c.B) * BG)


def state(b):
    import torch
    torch.cuda.synchronize()
    if isinstance(b, _Run):
        return b.arrays
    return dict(sed=b.sed_current.cpu().numpy(), morph=b.morph_current.cpu().numpy(), centers=b.centers.cpu().numpy(),
                shifts=b.shifts.cpu().numpy(), flags=b.flags.cpu().numpy(), mse=b.mse_buf.cpu().numpy(),
                it=b.it.cpu().numpy(), lipschitz=b.lipschitz.cpu().numpy(), status=b.status.cpu().numpy())


class options(object):
    """the case's diagnostic switches, set for the block"""

    def __init__(self, scarlet, c):
        self.lib, self.names = scarlet._lib, c.opts

    def __enter__(self):
        self.old = [self.lib.set_option(n, 1) for n in self.names]

    def __exit__(self, *exc):
        for n, v in zip(self.names, self.old):
            self.lib.set_option(n, v)
