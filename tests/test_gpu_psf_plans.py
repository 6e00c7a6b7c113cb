"""-m gpu: the PSF convolution at every plan of tests/test_psf_plans.py (all 44 (position, radix) codelet instances of
k_psf_conv, odd and even M, image staged by LDS-DMA or not, even-sized and non-square kernels, kernels larger than the
frame, 3-row frames, the exact-shape instance, the hipFFT chain) against float64 references computed here:

  - fit path: scarlet_backward_gradients' loss, d loss / d sed and d loss / d morph against torch.autograd over the
    float64 forward chain of tests/test_oracle_autograd.py, in the three-pass and the four-pass form (NO_PSF3PASS),
    the 128 x 128 / 41 x 41 case with and without its exact-shape instance (NO_EXACT);
  - scarlet_convolve_same (k_fft_khat + k_fft_convolve) against the oracle's float64 pgm.convolve, one kernel shared
    by the planes and one kernel per plane;
  - both again in a child process with SCARLET_PSF_HIPFFT=1: the batched hipFFT chain and its hand-written placement
    (k_plane_pad, k_psf_pad_kernel, k_plane_crop).  The switch is fixed once a PSF workspace has been sized, so it
    cannot be changed in this process.

Every case is two scenes with random non-negative SEDs and morphologies (set_state: no initialisation, so 3-row frames
and kernels larger than the frame need no valid sources), images of mean -1 (the residual keeps one sign: the gradient
sums do not cancel), and a random difference kernel whose centre carries most of the weight.  Bound: 1e-5 of the
arrays' maxima, as in tests/test_gpu_engine.py::test_device_gradients_equal_autograd.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import rel_err
import parity_common as pc
from test_psf_plans import CASES, case_id, plan_of

pytestmark = pytest.mark.gpu
TOL = pc.TOL
S = 2


def make_inputs(c):
    """the case's random batch, float32; `weights` is None, a float or an (S, B, H, W) array"""
    rng = np.random.default_rng([c.H, c.W, c.Py, c.Px, c.B, c.K])
    f32 = np.float32
    inp = dict(sed=rng.uniform(0.1, 2.0, (S, c.K, c.B)).astype(f32),
               morph=rng.uniform(0.0, 1.0, (S, c.K, c.H, c.W)).astype(f32),
               images=rng.normal(-1.0, 1.0, (S, c.B, c.H, c.W)).astype(f32),
               centers=np.stack([rng.integers(0, c.H, (S, c.K)), rng.integers(0, c.W, (S, c.K))], -1).astype(np.int32))
    diff = rng.normal(size=((S,) if c.per_scene else ()) + (c.B, c.Py, c.Px)) * 0.1
    diff[..., c.Py // 2, c.Px // 2] += 1.0
    inp["diff"] = diff.astype(f32)
    if c.weights == "one":
        inp["weights"] = None
    elif c.weights == "scalar":
        inp["weights"] = 0.7
    else:
        w = rng.uniform(0.2, 2.0, (S, c.B, c.H, c.W))
        w[rng.uniform(size=w.shape) < 0.1] = 0.0                            # masked pixels
        inp["weights"] = w.astype(f32)
    return inp


def reference_gradients(c, inp):
    """per scene: (loss, d loss / d sed, d loss / d morph) by torch.autograd over the float64 forward chain"""
    import torch
    from test_oracle_autograd import _render_torch
    t64 = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    out = []
    for i in range(S):
        ts = t64(inp["sed"][i]).requires_grad_(True)
        tm = t64(inp["morph"][i]).requires_grad_(True)
        model = torch.einsum("kb,kyx->byx", ts, tm)
        rendered = _render_torch(model, t64(inp["diff"][i] if c.per_scene else inp["diff"]))
        w = inp["weights"]
        w = 1.0 if w is None else (w if np.ndim(w) == 0 else t64(w[i]))
        d = w * (rendered - t64(inp["images"][i]))
        tl = 0.5 * (d ** 2).sum()
        ag_sed, ag_morph = torch.autograd.grad(tl, (ts, tm))
        out.append((float(tl.detach()), ag_sed.numpy(), ag_morph.numpy()))
    return out


def read_plan(b):
    from scarlet_amd import _lib
    v = (ctypes.c_int32 * 16)()
    return plan_of(_lib.lib.scarlet_debug_psf_plan(ctypes.byref(b._c), v), list(v))


def device_gradients(c, inp):
    """(the plan the batch runs, per scene (loss, d loss / d sed, d loss / d morph)) from scarlet_backward_gradients"""
    import torch
    from scarlet_amd import _lib
    from scarlet_amd.batch import BlendBatch
    b = BlendBatch(inp["images"], inp["centers"], weights=inp["weights"])
    b.set_diff_kernel(inp["diff"])
    b.set_state(inp["sed"], inp["morph"])
    plan = read_plan(b)
    _lib.check(_lib.lib.scarlet_backward_gradients(ctypes.byref(b._c), 0, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert int(b.status.abs().sum().item()) == 0
    cur = b.cur.cpu().numpy()
    return plan, [(float(b.mse_buf[i, 0].item()), b.sed[1 - cur[i]][i].cpu().numpy(), b.morph[1 - cur[i]][i].cpu().numpy())
                  for i in range(S)]


def gradient_error(got, ref):
    """worst relative error over the scenes and the three quantities"""
    return max(max(rel_err(g[0], r[0]), rel_err(g[1], r[1]), rel_err(g[2], r[2])) for g, r in zip(got, ref))


def convolve_errors(c):
    """scarlet_convolve_same on B planes against pgm.convolve (float64): {nk: relative error} for nk = 1 and nk = B"""
    from oracle import pgm
    from scarlet_amd.psfconv import convolve_same
    rng = np.random.default_rng([c.H, c.W, c.Py, c.Px, c.B, 7])
    n = c.B
    img = rng.uniform(size=(n, c.H, c.W)).astype(np.float32)
    errs = {}
    for nk in (1, n):
        ker = rng.normal(size=(nk, c.Py, c.Px)) * 0.1
        ker[:, c.Py // 2, c.Px // 2] += 1.0
        ker = ker.astype(np.float32)
        ref = pgm.convolve(img.astype(np.float64), np.broadcast_to(ker.astype(np.float64), (n, c.Py, c.Px)), axes=(1, 2))
        errs[nk] = rel_err(convolve_same(img, ker).cpu().numpy(), ref)
    return errs


def _with_options(opts, fn):
    from scarlet_amd import _lib
    try:
        for k, v in opts.items():
            _lib.set_option(k, v)
        return fn()
    finally:
        for k in opts:
            _lib.set_option(k, 0)


@pytest.fixture(scope="module")
def gpu():
    from scarlet_amd import _lib
    _lib.require_gpu()


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_fit_path_gradients_equal_float64_autograd(gpu, c):
    inp = make_inputs(c)
    ref = reference_gradients(c, inp)
    runs = [dict(NO_PSF3PASS=f) for f in (0, 1)]
    if c.plan is not None and c.plan.exact:
        runs += [dict(NO_PSF3PASS=f, NO_EXACT=1) for f in (0, 1)]
    for opts in runs:
        plan, got = _with_options(opts, lambda: device_gradients(c, inp))
        want = c.plan if not (c.plan and opts.get("NO_EXACT")) else c.plan._replace(exact=0)
        assert plan == want, (opts, plan)
        err = gradient_error(got, ref)
        assert err < TOL, (opts, err)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_convolve_same_equals_float64_oracle(gpu, c):
    for nk, err in convolve_errors(c).items():
        assert err <= 1e-5, (nk, err)


def child_main(path):
    """every case once more in this process, which runs the hipFFT chain (SCARLET_PSF_HIPFFT=1): the errors to `path`"""
    from scarlet_amd import _lib
    _lib.require_gpu()
    res = []
    for c in CASES:
        inp = make_inputs(c)
        plan, got = device_gradients(c, inp)
        assert plan is None, (case_id(c), plan)                    # the batch is on the hipFFT chain
        conv = convolve_errors(c)
        res.append(dict(case=case_id(c), grad=gradient_error(got, reference_gradients(c, inp)),
                        conv1=conv[1], convn=conv[c.B]))
    with open(path, "w") as f:
        json.dump(res, f)


def test_hipfft_chain_equals_float64_references(gpu, tmp_path):
    out = str(tmp_path / "hipfft.json")
    env = dict(os.environ, SCARLET_PSF_HIPFFT="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    with open(out) as f:
        res = json.load(f)
    assert [x["case"] for x in res] == [case_id(c) for c in CASES]
    bad = ["%s: gradients %.2e, convolve_same nk = 1 %.2e, nk = B %.2e" % (x["case"], x["grad"], x["conv1"], x["convn"])
           for x in res if not (x["grad"] < TOL and x["conv1"] <= 1e-5 and x["convn"] <= 1e-5)]
    assert not bad, "\n".join(bad)


if __name__ == "__main__":
    child_main(sys.argv[1])
