"""-m gpu: every Lipschitz-constant solver of the library against float64 eigenvalues, one small batch per route
(tests/lipschitz_cases.py: the routes, the spectrum classes, the expected values and the bounds; tests/test_lipschitz_cases.py
shows on the CPU that the cases are what they claim to be and that the reference's own float32 arithmetic stays inside
the bound on each of them).

Per route: set_state, read the state back, run ONE iteration -- `fit(1, e_rel=0)` for the fused kernels,
scarlet_backward_gradients (the constants without a step) for the general, PSF, bigk and hugek paths, `step` for the joint
fits -- and compare `lipschitz` of every scene with n_obs x numpy's eigvalsh of the float64 Gram matrices of the float32
arrays read back.  `status` stays 0.  The route taken is asserted: scarlet_debug_fused_plan's kernel for the fused
launches (and FUSED_NONE elsewhere), scarlet_debug_contract_plan's for the joint fits, and the profiler's launches per
class as the host code is written.

Bounds, relative (got / want - 1; lipschitz_cases.bounds): 1e-5 everywhere; the characteristic polynomial on a cluster from
above by charpoly_upper; where the Gram matrix is summed in float64 and solved in float64 (hugek's L_sed, every L_morph)
the code's own figures: a squaring route within [-(n / (e 2^(q + 1)) + 1e-12), +1e-12], the Jacobi within 1e-12.  Every
figure is printed (`lipschitz ...` lines, and into SCARLET_LOG_REL_ERR; profiles/lipschitz_rel_err.txt is a run's
collection)."""
import ctypes
import os

import numpy as np
import pytest

import lipschitz_cases as lc
from gradient_stage_cases import diff_kernel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scarlet():
    import scarlet_amd
    scarlet_amd._lib.require_gpu()
    return scarlet_amd


def make_batch(scarlet, r, st):
    S = len(r.scenes)
    images = lc.images(st)
    if r.kind == "obs":
        obs, b0 = [], 0
        for nb in r.bands:
            obs.append(scarlet.ObservationBatch(images[:, b0:b0 + nb], band0=b0))
            b0 += nb
        assert b0 == r.B
        return scarlet.BlendBatch.from_observations(obs, st.centers, wide=r.wide, mse_capacity=2)
    kw = dict(mse_capacity=2, n_components=st.n_components)
    if r.frames:
        kw["frame_shapes"] = np.array([lc.frame_of(r, s) for s in range(S)], dtype=np.int32)
    if r.per_component:
        kw["symmetric"] = [k % 2 == 0 for k in range(r.K)]
    b = scarlet.BlendBatch(images, st.centers, **kw)
    if r.psf:
        b.set_diff_kernel(diff_kernel(r.B))
    return b


def assert_plan(scarlet, r, b):
    L = scarlet._lib.lib
    out = (ctypes.c_int32 * 8)()
    if r.kind == "obs":
        assert L.scarlet_debug_contract_plan(r.K, r.B, 0, ctypes.cast(out, ctypes.c_void_p)) == 0
        assert out[0] == r.plan, (r.name, list(out))
        assert (out[1] == (16 if r.B <= 16 else 32)) if r.wide else r.B <= 8, (r.name, list(out))
        return
    frames = ctypes.byref(b._frames) if r.frames else None
    cons = ctypes.byref(b._cons) if (r.frames or r.per_component) else None
    assert L.scarlet_debug_fused_plan(ctypes.byref(b._c), frames, cons, 0, 1, ctypes.cast(out, ctypes.c_void_p)) == 0
    assert out[0] == r.plan and out[3] == 1, (r.name, list(out))


def one_iteration(scarlet, r, b):
    """the launches per profiler class of the route's one iteration"""
    _lib = scarlet._lib
    _lib.check(_lib.lib.scarlet_profile_begin(1))
    try:
        if r.kind == "fused":
            assert b.fit(1, e_rel=0) == 1
        elif r.kind == "grad":
            _lib.check(_lib.lib.scarlet_backward_gradients(ctypes.byref(b._c), 0, _lib.stream_ptr()))
        else:
            b.step(e_rel=0)
    finally:
        ms, its, launches = (ctypes.c_double * 8)(), (ctypes.c_int64 * 8)(), (ctypes.c_int64 * 8)()
        _lib.check(_lib.lib.scarlet_profile_end_ex(ms, its, launches))
    return list(launches)


def log(line):
    print(line)
    path = os.environ.get("SCARLET_LOG_REL_ERR")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@pytest.mark.parametrize("name", list(lc.ROUTES))
def test_route(scarlet, name):
    import torch
    r = lc.ROUTES[name]
    st = lc.state(r)
    old = [(opt, scarlet._lib.set_option(opt, value)) for opt, value in r.opts]
    try:
        b = make_batch(scarlet, r, st)
        b.set_state(st.sed, st.morph)
        morph32, sed32 = b.morph_current.cpu().numpy(), b.sed_current.cpu().numpy()
        assert np.array_equal(morph32, st.morph) and np.array_equal(sed32, st.sed)
        assert_plan(scarlet, r, b)
        try:
            launches = one_iteration(scarlet, r, b)
            torch.cuda.synchronize()
        except NotImplementedError:
            raise
        except RuntimeError as e:
            # a HIP error leaves the device context unusable: the routes after it would only fail on top of it
            pytest.exit("route %s: %s" % (name, e), returncode=3)
    finally:
        for opt, value in old:
            scarlet._lib.set_option(opt, value)
    assert launches == [1 if str(i) in r.classes else 0 for i in range(8)], (name, launches)
    assert not b.status.cpu().numpy().any(), name
    got = b.lipschitz.cpu().numpy()
    assert got.shape == (len(r.scenes), 2) and np.isfinite(got).all(), (name, got)
    bad = []
    for s, sc in enumerate(r.scenes):
        want = lc.want(morph32[s], sed32[s], sc.n, lc.n_obs(r))
        bnd = lc.bounds(r, sc, lc.gram(morph32[s], sc.n), lc.sed_gram(r, sc, sed32[s]))
        solver = lc.solvers(r, sc)
        for i, what in enumerate(("L_sed", "L_morph")):
            rel = got[s, i] / want[i] - 1
            ok = bnd[i][0] <= rel <= bnd[i][1]
            cls = sc.morph + ("(%d,%d)" % sc.pair if sc.pair else "") if i == 0 else sc.sed
            log("lipschitz %-24s scene %d n %3d %-7s %-8s %-16s rel %+.3e in [%+.2e, %+.2e]%s"
                % (name, s, sc.n, what, solver[i], cls, rel, bnd[i][0], bnd[i][1], "" if ok else "  MISSED"))
            if not ok:
                bad.append((s, what, solver[i], cls, rel, bnd[i]))
    assert not bad, (name, bad)
