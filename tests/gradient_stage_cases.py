"""The cases of tests/test_gpu_gradient_stages.py: every combination of launch stages the gradient step is built from
("The gradient step, stage by stage"), each at the smallest shape that still takes the path.  The table is
shared by the test, by tools/pick_gradient_stage_seeds.py (the CPU search for its seeds) and by tools/gradstages_ab.py
(build-against-build dumps and one-iteration runs for a kernel trace).

Every case is 2 scenes and 3 iterations at e_rel = 0.  A PSF is the 5 x 5 Gaussian difference kernel of
tests/test_gpu_fit_driver.py.  `classes`: the profiler classes that record one launch per iteration, written down from
the host code (0 gradient / Gram, 1 step, 2 constraints, 3 convergence test, 5 PSF gradient planes); `hipfft`: the same
under SCARLET_PSF_HIPFFT=1, for the cases that run once more there (the three-pass form needs the LDS-resident
convolution: on the hipFFT chain its cases take k_grad_psf / k_step_psf).

Seeds.  The parity checks take no threshold exemption (tests/parity_common.py; the cap is 0 scenes), so every seed was
chosen on the CPU before any device run, by the rule of tests/constraints_common.py: started from the oracle's own
starts, the float32 and the float64 oracle agree on the support of every morphology after every iteration and differ
by at most 1e-6.  tools/pick_gradient_stage_seeds.py repeats the search; cases of one shape, PSF and kind of constants
share their seeds.
"""
import collections

import numpy as np

BG = 0.1
ITERS = 3
S = 2
KEYS = ("sed", "morph", "centers", "shifts", "flags", "mse", "it", "lipschitz", "status")
OBS_BANDS = (3, 2)            # observation cases: channels 3 + 2, the first observation has the PSF

Case = collections.namedtuple("Case", "name kind K B H W approximate_L psf opts min_sep classes hipfft")


def _c(name, kind, K, B, H, W, approximate_L=False, psf=False, opts=(), min_sep=4, classes="0123", hipfft=None):
    return Case(name, kind, K, B, H, W, approximate_L, psf, tuple(opts), min_sep, classes, hipfft)


CASES = collections.OrderedDict((c.name, c) for c in [
    # no PSF, K <= 8: k_grad / k_step in both K instances
    _c("general_k3", "fit", 3, 3, 24, 32, approximate_L=True),
    _c("general_k6", "fit", 6, 3, 24, 32, min_sep=3, approximate_L=True),
    # PSF, LDS-resident, three-pass: k_psf_model4g, k_step_psf4f<., 4 / 6 / SC_BMAX>, k_sed_step
    _c("psf_three_pass_k3", "fit", 3, 3, 24, 32, psf=True, classes="1235", hipfft="01235"),
    _c("psf_three_pass_k6", "fit", 6, 3, 24, 32, min_sep=3, psf=True, classes="1235"),
    _c("psf_three_pass_k3_b5", "fit", 3, 5, 24, 32, psf=True, classes="1235"),
    _c("psf_three_pass_k6_b5", "fit", 6, 5, 24, 32, min_sep=3, psf=True, classes="1235"),
    _c("psf_three_pass_k3_b7", "fit", 3, 7, 24, 32, psf=True, classes="1235"),
    _c("psf_three_pass_k6_b7", "fit", 6, 7, 24, 32, min_sep=3, psf=True, classes="1235"),
    # four-pass: k_psf_model4, k_grad_psf4 / k_step_psf4
    _c("psf_four_pass_k3", "fit", 3, 3, 24, 32, psf=True, opts=["NO_PSF3PASS"], classes="01235"),
    _c("psf_four_pass_k6", "fit", 6, 3, 24, 32, min_sep=3, psf=True, opts=["NO_PSF3PASS"], classes="01235"),
    # H W % 4 != 0: k_psf_model, k_grad_psf / k_step_psf
    _c("psf_odd_plane_k3", "fit", 3, 3, 23, 31, psf=True, classes="01235"),
    _c("psf_odd_plane_k6", "fit", 6, 3, 23, 31, min_sep=3, psf=True, classes="01235"),
    # 8 < K <= 32 without a PSF: the fused form with and without the second stream, the chunked form with and without
    _c("bigk", "fit", 9, 3, 32, 32, min_sep=3),
    _c("bigk_one_stream", "fit", 9, 3, 32, 32, opts=["NO_SIDE_STREAM"], min_sep=3),
    _c("bigk_chunked", "fit", 9, 3, 32, 32, opts=["NO_BIGK_FUSED"], min_sep=3),
    _c("bigk_chunked_one_stream", "fit", 9, 3, 32, 32, opts=["NO_BIGK_FUSED", "NO_SIDE_STREAM"], min_sep=3),
    _c("bigk_chunked_no_mfma", "fit", 9, 3, 32, 32, opts=["NO_BIGK_FUSED", "NO_GRAM_MFMA"], min_sep=3),
    _c("bigk_approximate", "fit", 9, 3, 32, 32, approximate_L=True, min_sep=3),
    # ... with a PSF: the planes tail
    _c("bigk_psf", "fit", 9, 3, 32, 32, psf=True, min_sep=3, classes="01235", hipfft="01235"),
    _c("bigk_psf_no_mfma", "fit", 9, 3, 32, 32, psf=True, opts=["NO_GRAM_MFMA"], min_sep=3, classes="01235"),
    # K > 32: backward_hugek with and without planes, exact and approximate constants
    _c("hugek", "fit", 33, 3, 48, 48, min_sep=2),
    _c("hugek_approximate", "fit", 33, 3, 48, 48, approximate_L=True, min_sep=2),
    _c("hugek_psf", "fit", 33, 3, 48, 48, psf=True, min_sep=2, classes="01235", hipfft="01235"),
    _c("hugek_psf_approximate", "fit", 33, 3, 48, 48, approximate_L=True, psf=True, min_sep=2, classes="01235"),
    # the observation step, first observation with a PSF: the contraction sums the Gram (K = 3), obs_lipschitz_sed's
    # bigk branch (K = 9) and huge branch (K = 33)
    _c("obs_psf_k3", "obs", 3, 5, 24, 32, psf=True, hipfft="0123"),
    _c("obs_psf_k3_odd_plane", "obs", 3, 5, 23, 31, psf=True),
    _c("obs_psf_k9", "obs", 9, 5, 32, 32, psf=True, min_sep=3, hipfft="0123"),
    _c("obs_psf_k9_approximate", "obs", 9, 5, 32, 32, approximate_L=True, psf=True, min_sep=3),
    _c("obs_psf_k33", "obs", 33, 5, 48, 48, psf=True, min_sep=2),
])
HIPFFT_CASES = [c.name for c in CASES.values() if c.hipfft]
SIDE_STREAM_CASES = ("bigk", "bigk_chunked", "bigk_chunked_no_mfma", "bigk_approximate")   # launches on two streams

# (kind, K, B, H, W, psf, approximate_L) -> the 2 seeds; printed by tools/pick_gradient_stage_seeds.py
SEEDS = {
    ('fit', 3, 3, 24, 32, False, True): [9000, 9001],
    ('fit', 6, 3, 24, 32, False, True): [9002, 9003],
    ('fit', 3, 3, 24, 32, True, False): [9004, 9005],
    ('fit', 6, 3, 24, 32, True, False): [9006, 9007],
    ('fit', 3, 5, 24, 32, True, False): [9008, 9009],
    ('fit', 6, 5, 24, 32, True, False): [9010, 9011],
    ('fit', 3, 7, 24, 32, True, False): [9012, 9013],
    ('fit', 6, 7, 24, 32, True, False): [9014, 9015],
    ('fit', 3, 3, 23, 31, True, False): [9016, 9017],
    ('fit', 6, 3, 23, 31, True, False): [9018, 9019],
    ('fit', 9, 3, 32, 32, False, False): [9020, 9021],
    ('fit', 9, 3, 32, 32, False, True): [9022, 9023],
    ('fit', 9, 3, 32, 32, True, False): [9024, 9026],
    ('fit', 33, 3, 48, 48, False, False): [9027, 9028],
    ('fit', 33, 3, 48, 48, False, True): [9029, 9030],
    ('fit', 33, 3, 48, 48, True, False): [9031, 9032],
    ('fit', 33, 3, 48, 48, True, True): [9033, 9034],
    ('obs', 3, 5, 24, 32, True, False): [9035, 9036],
    ('obs', 3, 5, 23, 31, True, False): [9037, 9038],
    ('obs', 9, 5, 32, 32, True, False): [9039, 9040],
    ('obs', 9, 5, 32, 32, True, True): [9041, 9042],
    ('obs', 33, 5, 48, 48, True, False): [9043, 9044],
}

CONVOLVE = dict(n=3, H=24, W=32, P=5)        # scarlet_convolve_same: nk = 1 and nk = n


def seed_key(c):
    return (c.kind, c.K, c.B, c.H, c.W, c.psf, c.approximate_L)


def diff_kernel(B):
    y, x = np.mgrid[:5, :5]
    k = np.exp(-((y - 2) ** 2 + (x - 2) ** 2) / 2.0).astype(np.float32)
    return np.stack([k / k.sum()] * B)


def scenes(c, seeds=None):
    """images (S, B, H, W), centers (S, K, 2) of the case's seeds"""
    from scarlet_amd import synth
    sc = [synth.make_scene(s, B=c.B, H=c.H, W=c.W, K=c.K, min_sep=c.min_sep) for s in (seeds or SEEDS[seed_key(c)])]
    return np.stack([x["images"] for x in sc]), np.stack([x["centers"] for x in sc])


def obs_data(c, images):
    n = OBS_BANDS[0]
    return [dict(images=images[:, :n], band0=0, diff=diff_kernel(n)), dict(images=images[:, n:], band0=n)]


def make_batch(scarlet, c, images, centers, mse_capacity=ITERS + 1):
    """the case's freshly initialised batch (the same state every time)"""
    if c.kind == "obs":
        obs = []
        for o in obs_data(c, images):
            ob = scarlet.ObservationBatch(o["images"], band0=o["band0"])
            if o.get("diff") is not None:
                ob.set_diff_kernel(o["diff"])
            obs.append(ob)
        b = scarlet.BlendBatch.from_observations(obs, centers, mse_capacity=mse_capacity)
        return b.init_combined([np.ones(n) * BG for n in OBS_BANDS])
    b = scarlet.BlendBatch(images, centers, mse_capacity=mse_capacity)
    if c.psf:
        b.set_diff_kernel(diff_kernel(c.B))
    return b.init_extended(np.ones(c.B) * BG)


def state(b):
    import torch
    torch.cuda.synchronize()
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


def convolve_inputs():
    """planes (n, H, W) and kernels {nk: (nk, P, P)} of the scarlet_convolve_same case"""
    g = CONVOLVE
    rng = np.random.default_rng([g["H"], g["W"], g["P"], g["n"]])
    img = rng.uniform(size=(g["n"], g["H"], g["W"])).astype(np.float32)
    kers = {}
    for nk in (1, g["n"]):
        ker = rng.normal(size=(nk, g["P"], g["P"])) * 0.1
        ker[:, g["P"] // 2, g["P"] // 2] += 1.0
        kers[nk] = ker.astype(np.float32)
    return img, kers
