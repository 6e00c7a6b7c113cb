"""-m gpu: every combination of the launch stages the gradient step is built from (scarlet_hip.hip: psf_args,
psf_gradient_planes, hipfft_convolve, huge_args / launch_huge_lipschitz, the many-component pieces, launch_grad_step;
DESIGN.md "The gradient step, stage by stage"), at the smallest shape that takes each path.  The table of cases, their
shapes and the rule by which their seeds were chosen: tests/gradient_stage_cases.py.

Only the public Python API and scarlet_set_option are used, so the file passes unchanged against a library built from
an older commit (SCARLET_LIB_PATH).  Every case is 2 scenes, 3 iterations at e_rel = 0, and asserts

  parity       with the float32 CPU oracle from the device's own initial state, 1e-5 max-norm relative on sed, morph and
               the loss history, centres exactly, through parity_common.check_fixed_iterations with the threshold
               exemption capped at 0 scenes (observation cases: the helpers of tests/test_gpu_observations.py, which
               have no exemption);
  launches     per profiler class and iteration, as the host code is written (gradient_stage_cases.Case.classes);
  determinism  two runs from the same start are bit-identical.

The cases that reach the hipFFT chain run once more in ONE child process started with SCARLET_PSF_HIPFFT=1 (the switch
freezes with the first PSF workspace), as does scarlet_convolve_same, whose reference is the oracle's float64
pgm.convolve (bound 1e-5, as tests/test_gpu_psf_plans.py)."""
import ctypes
import json
import multiprocessing as mp
import os
import subprocess
import sys
import traceback

import numpy as np
import pytest

from conftest import rel_err
import gradient_stage_cases as gs
import parity_common as pc

pytestmark = pytest.mark.gpu
ITERS = gs.ITERS


class StageWorkload(pc.Workload):
    """parity_common's workload for one case of the table"""

    def __init__(self, c):
        pc.Workload.__init__(self, B=c.B, H=c.H, W=c.W, K=c.K, min_sep=c.min_sep)
        self.case = c

    def batch(self, scarlet, images, centers, mse_capacity):
        return gs.make_batch(scarlet, self.case, images, centers, mse_capacity)

    def oracle_kwargs(self):
        kw = dict(approximate_L=self.case.approximate_L)
        if self.case.psf:
            kw["diff_kernel"] = gs.diff_kernel(self.case.B)
        return kw


def expected_launches(classes):
    return [ITERS if str(i) in classes else 0 for i in range(8)]


def profiled_fit(scarlet, b, approximate_L):
    """(launches per class, iterations per class) of one fit of ITERS iterations"""
    L = scarlet._lib.lib
    scarlet._lib.check(L.scarlet_profile_begin(ITERS))
    try:
        n = b.fit(ITERS, e_rel=0, approximate_L=approximate_L)
    finally:
        ms, its, launches = (ctypes.c_double * 8)(), (ctypes.c_int64 * 8)(), (ctypes.c_int64 * 8)()
        scarlet._lib.check(L.scarlet_profile_end_ex(ms, its, launches))
    assert n == ITERS
    return list(launches), list(its)


def run_case(scarlet, pool, name, classes):
    c = gs.CASES[name]
    images, centers = gs.scenes(c)
    with gs.options(scarlet, c):
        # launches per class, and two runs from the same start
        runs = []
        for profiled in (True, False):
            b = gs.make_batch(scarlet, c, images, centers)
            if profiled:
                launches, its = profiled_fit(scarlet, b, c.approximate_L)
                assert launches == its == expected_launches(classes), (name, launches, its)
            else:
                assert b.fit(ITERS, e_rel=0, approximate_L=c.approximate_L) == ITERS
            runs.append(gs.state(b))
            assert (runs[-1]["it"] == ITERS).all() and not runs[-1]["status"].any(), name
        for key in gs.KEYS:
            assert np.array_equal(runs[0][key], runs[1][key], equal_nan=True), "%s: %s differs between two runs" % (name, key)
        # parity with the float32 oracle, no exemption
        if c.kind == "obs":
            from test_gpu_observations import _check
            _check(gs.make_batch(scarlet, c, images, centers), gs.obs_data(c, images), ITERS, range(gs.S),
                   approximate_L=c.approximate_L)
        else:
            pc.check_fixed_iterations(scarlet, StageWorkload(c), images, centers, pool, ITERS, 0, "gradient stages " + name)


def convolve_errors():
    from oracle import pgm
    from scarlet_amd.psfconv import convolve_same
    img, kers = gs.convolve_inputs()
    errs = {}
    for nk, ker in kers.items():
        ref = pgm.convolve(img.astype(np.float64), np.broadcast_to(ker.astype(np.float64), (len(img),) + ker.shape[1:]),
                           axes=(1, 2))
        a, b = (convolve_same(img, ker).cpu().numpy() for _ in range(2))
        assert np.array_equal(a, b), "convolve_same: two runs differ (nk = %d)" % nk
        errs[nk] = rel_err(a, ref)
    return errs


@pytest.fixture(scope="module")
def env():
    import scarlet_amd
    scarlet_amd._lib.require_gpu()
    from oracle import build as obuild
    obuild.build()
    pool = mp.get_context("spawn").Pool(gs.S)
    yield scarlet_amd, pool
    pool.close(); pool.join()


@pytest.mark.parametrize("name", list(gs.CASES))
def test_stage_combination(env, name):
    scarlet, pool = env
    run_case(scarlet, pool, name, gs.CASES[name].classes)


def test_convolve_same(env):
    for nk, err in convolve_errors().items():
        assert err <= 1e-5, (nk, err)


# ------------------------------------------------------------------------------------------ the hipFFT chain
def child_main(path):
    """the hipFFT cases in this process (SCARLET_PSF_HIPFFT=1): {case: None or the failure's text} to `path`"""
    import scarlet_amd
    scarlet_amd._lib.require_gpu()
    pool = mp.get_context("spawn").Pool(gs.S)
    res = {}
    for name in gs.HIPFFT_CASES + ["convolve_same"]:
        try:
            if name == "convolve_same":
                errs = convolve_errors()
                assert max(errs.values()) <= 1e-5, errs
            else:
                c = gs.CASES[name]
                b = gs.make_batch(scarlet_amd, c, *gs.scenes(c))
                psf_batch = b._observations[0][1] if c.kind == "obs" else b
                plan = (ctypes.c_int32 * 16)()
                assert scarlet_amd._lib.lib.scarlet_debug_psf_plan(ctypes.byref(psf_batch._c), plan) == -1, "not on the hipFFT chain"
                run_case(scarlet_amd, pool, name, c.hipfft)
            res[name] = None
        except Exception:
            res[name] = traceback.format_exc()[-2000:]
    pool.close(); pool.join()
    with open(path, "w") as f:
        json.dump(res, f)


@pytest.fixture(scope="module")
def hipfft_results(env, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hipfft") / "results.json")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(os.environ, SCARLET_PSF_HIPFFT="1"),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    with open(out) as f:
        return json.load(f)


@pytest.mark.parametrize("name", gs.HIPFFT_CASES + ["convolve_same"])
def test_hipfft(hipfft_results, name):
    assert name in hipfft_results
    assert hipfft_results[name] is None, hipfft_results[name]


if __name__ == "__main__":
    child_main(sys.argv[1])
