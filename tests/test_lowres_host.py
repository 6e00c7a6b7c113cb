"""CPU: the host set-up of a low-resolution observation (scarlet_amd.LowResObservation.match, resampling.py) against
what the reference computed (tests/golden/lowres.npz, tools/gen_lowres_golden.py; at the geometries that fill LDS
tests/golden/lowres_limits.npz, tools/gen_lowres_limits_golden.py), the float restatement of the joint fit against the
reference's fit, and the C ABI with its argument checks and its LDS boundary.  Every library call below returns before
a launch."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import lowres_common as lc
from conftest import load_golden, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scarlet_hip.h")
FAKE = 0x1000          # a non-NULL pointer that is never dereferenced
# Measured against the reference's outputs: 1.37e-7 at most (profiles/lowres_rel_err.txt), the float32 cast of the
# reference's own operator and result.  The bound is one decade above.
HOST_TOL = 1.4e-6
FIELDS = ["h", "w", "nfy", "nfx", "B", "uy", "ux", "vy", "vx", "dhat", "v_per_scene", "dhat_per_scene", "workspace"]


@pytest.fixture(scope="module")
def g():
    return lc.fixture()


@pytest.mark.parametrize("name", ["a", "b"])
def test_host_factors_reproduce_the_reference(g, name):
    from scarlet_amd import resampling as rs
    obs, _ = lc.geometry(g, name)
    assert obs.covers and obs.lr_shape == tuple(g[name + "_lr_shape"])
    assert list(obs._fft_shape) == list(g[name + "_fft_shape"])
    assert rel_err(obs._diff_kernels, g[name + "_diff_psf"]) <= HOST_TOL
    w, img = g[name + "_weights_lr"].astype(np.float64), g[name + "_images_lr"].astype(np.float64)
    for i, model in enumerate(g[name + "_models"]):
        out = rs.apply_factors(obs.factors, model)
        err = rel_err(out, g[name + "_renders"][i])
        print("geometry %s model %d: render rel err %.3e" % (name, i, err))
        assert err <= HOST_TOL
        loss = 0.5 * np.sum((w * (out - img)) ** 2)
        assert abs(loss - g[name + "_losses"][i]) <= HOST_TOL * g[name + "_losses"][i]


def test_retained_frequencies_and_placement(g):
    """36-point padded plane: half-spectrum bins 0-3 and 14-18 survive the cut, the frame sits at offset 2"""
    from scarlet_amd import resampling as rs
    k, wgt = rs.kept_frequencies(36)
    assert list(k) == [0, 1, 2, 3, 14, 15, 16, 17, 18]
    assert list(wgt) == [1, 2, 2, 2, 2, 2, 2, 2, 1]
    f, wf = rs.full_frequencies(36)
    assert len(f) == 17 and abs(wf.sum() - 16) < 1e-12 and sorted(f) == sorted(-f)
    assert rs.fast_shape((32, 32)) == [36, 36] and rs.pad_start(32, 36) == 2
    assert rs.fast_shape((43, 43)) == [48, 48] and rs.fast_shape((42, 41))[1] % 2 == 0
    obs, _ = lc.geometry(g, "a")
    assert obs.factors["uy"].shape == (9, 32) and obs.factors["ux"].shape == (17, 32)
    assert obs.factors["vy"].shape == (16, 9) and obs.factors["dhat"].shape == (2, 9, 17)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_sandwich_is_the_reference_algorithm_and_its_adjoint(g, name):
    """the factor sandwich against the reference's algorithm stated directly (also for the non-square geometry c, which
    the reference itself refuses: its error message is in the fixture), and <T x, y> = <x, T^T y> in float64"""
    from scarlet_amd import resampling as rs
    obs, _ = lc.geometry(g, name)
    assert obs.small_axis == (name != "c")
    model = g[name + "_models"][0]
    out = rs.apply_factors(obs.factors, model)
    assert rel_err(out, lc.render_by_planes(obs, model)) <= 1e-12
    y = np.random.default_rng(3).standard_normal(out.shape)
    lhs, rhs = np.sum(out * y), np.sum(model * rs.adjoint_factors(obs.factors, y))
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)
    assert "broadcast" in str(g["c_reference_error"])


@pytest.fixture(scope="module")
def gl():
    return load_golden("lowres_limits")


@pytest.mark.parametrize("name", ["d", "e", "f"])
def test_host_factors_reproduce_the_reference_at_the_limits(gl, name):
    """the geometries that fill LDS (lowres_common.LIMITS), where the reference still runs: 1.3e-7 .. 1.5e-7, the
    float32 cast of the reference's result (profiles/lowres_rel_err.txt)"""
    from scarlet_amd import resampling as rs
    (H, W), (h, w), ratio, origin, psf_px, _ = lc.LIMITS[name]
    assert (tuple(gl[name + "_model_shape"]), tuple(gl[name + "_lr_shape"])) == ((H, W), (h, w))
    assert float(gl[name + "_ratio"]) == ratio and tuple(gl[name + "_origin"]) == origin
    for got, want in zip(lc.limit_psfs(psf_px, 2), (gl[name + "_model_psf"], gl[name + "_lr_psfs"])):
        np.testing.assert_array_equal(got, want)
    obs, _ = lc.limit_geometry(name, B=2)
    assert obs.covers and obs.lr_shape == (h, w)
    assert list(obs._fft_shape) == list(gl[name + "_fft_shape"])
    model = gl[name + "_models"][0]
    out = rs.apply_factors(obs.factors, model)
    err = rel_err(out, gl[name + "_renders"][0])
    print("geometry %s: render rel err %.3e" % (name, err))
    assert err <= HOST_TOL
    wgt, img = gl[name + "_weights_lr"].astype(np.float64), gl[name + "_images_lr"].astype(np.float64)
    loss = 0.5 * np.sum((wgt * (out - img)) ** 2)
    assert abs(loss - gl[name + "_losses"][0]) <= HOST_TOL * gl[name + "_losses"][0]


@pytest.mark.parametrize("name", sorted(lc.LIMITS))
def test_sandwich_is_the_reference_algorithm_at_the_limits(gl, name):
    """as test_sandwich_is_the_reference_algorithm_and_its_adjoint, on d .. j.  g and h pad to planes that are not
    square (75 x 80, 45 x 48), which the reference refuses as it refuses c: its messages are in the fixture."""
    from scarlet_amd import resampling as rs
    (H, W), (h, w) = lc.LIMITS[name][:2]
    obs, _ = lc.limit_geometry(name, B=2)
    assert obs.covers and obs.small_axis == (w <= h)
    rng = np.random.default_rng(5)
    model = rng.random((2, H, W))
    out = rs.apply_factors(obs.factors, model)
    err = rel_err(out, lc.render_by_planes(obs, model))
    print("geometry %s: sandwich vs planes %.3e" % (name, err))
    assert err <= 1e-12
    y = rng.standard_normal(out.shape)
    back = rs.adjoint_factors(obs.factors, y)
    lhs, rhs = np.sum(out * y), np.sum(model * back)
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)
    # (the form the float restatement of the fit uses)
    assert rel_err(lc.apply_by_matmul(obs.factors, model), out) <= 1e-12
    assert rel_err(lc.adjoint_by_matmul(obs.factors, y), back) <= 1e-12
    if name in "gh":
        assert obs._fft_shape[0] != obs._fft_shape[1]
        assert str(gl[name + "_reference_error"]).startswith("ValueError") and "inhomogeneous" in str(gl[name + "_reference_error"])


def _dims(obs):
    (H, W), (h, w) = obs.model_shape, obs.frame.shape[1:]
    return H, W, h, w, obs.factors["uy"].shape[0], obs.factors["ux"].shape[0]


def test_scratch_layouts_of_the_geometries(g):
    """Which product sizes lowres.h's scratch buffers: 2 nfy x ld2x at a .. g, i and j, h x ldw at h alone (pixel ratio
    1.1) -- the only geometry in the suite that runs the other layout, so it must stay in it.  Pure sizes; the footprints
    are those of the table in profiles/lowres_rel_err.txt."""
    largest, kib = {}, {}
    for name in "abc":
        terms, _ = lc.scratch_terms(*_dims(lc.geometry(g, name)[0]))
        largest[name] = max(terms, key=terms.get)
    for name, B in (("d", 8), ("e", 2), ("g", 8), ("h", 1), ("i", 3), ("j", 1), ("f", 6)):
        d = _dims(lc.limit_geometry(name)[0])
        terms, fixed = lc.scratch_terms(*d)
        largest[name] = max(terms, key=terms.get)
        kib[name] = round((fixed + B * 8 * d[4] * d[5]) / 1024.0, 1)
        assert sorted(terms.values())[-1] > sorted(terms.values())[-2]          # no tie decides a layout
    assert largest.pop("h") == "h x ldw"
    assert set(largest.values()) == {"2nfy x ld2x"} and len(largest) == 9
    assert (kib["d"], kib["e"], kib["g"], kib["h"], kib["i"], kib["j"]) == (132.8, 158.1, 156.3, 43.7, 80.4, 9.8)
    assert kib["f"] < kib["e"]
    terms, _ = lc.scratch_terms(*_dims(lc.limit_geometry("h")[0]))
    assert (terms["h x ldw"], terms["2nfy x ld2x"]) == (1332, 1122)
    assert _dims(lc.limit_geometry("j")[0]) == (17, 23, 5, 7, 5, 15)             # every GEMM dimension off 16 and 4


@pytest.mark.parametrize("name", ["a", "b"])
def test_float_restatement_of_the_joint_fit_reproduces_the_reference(g, name):
    obs, start, cw, _ = lc.fit_inputs(g, name)
    sc = lc.fit(lc.scene_from(start, cw), obs, 5)
    tol = 2e-5                      # the float32 bound of the fit_*.npz comparisons in test_oracle_golden.py
    assert rel_err(sc.mse, g[name + "_fit_mse"]) <= tol
    assert rel_err(np.array([c.sed for c in sc.sources]), g[name + "_fit_sed"]) <= tol
    assert rel_err(np.array([c.morph for c in sc.sources]), g[name + "_fit_morph"]) <= tol
    np.testing.assert_array_equal(np.array([c.center for c in sc.sources]), g[name + "_fit_centers"])
    np.testing.assert_array_equal(np.array([c.flags for c in sc.sources]), g[name + "_fit_flags"])


def test_rotated_and_partly_overlapping_geometries(g):
    import scarlet_amd as scarlet
    from scarlet_amd.resampling import AffineWCS
    H = W = 32
    frame = scarlet.Frame((2, H, W), wcs=AffineWCS((H, W), 1.0), psfs=g["a_model_psf"].copy(), channels=["r", "i"])
    th = 0.3
    rot = 2.0 * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    obs = scarlet.LowResObservation(g["a_images_lr"], wcs=AffineWCS((16, 16), pc=rot), psfs=g["a_lr_psfs"].copy(),
                                    channels=["r", "i"])
    with pytest.raises(NotImplementedError, match="rotated"):
        obs.match(frame)
    # an observation that sticks out of the model frame: matched, but refused by the batch class (and by `factors`)
    part, _ = lc.geometry(g, "a", origin=(-6.0, 0.0))
    assert not part.covers and part.lr_shape == (13, 16)
    with pytest.raises(ValueError, match="inside the model frame"):
        scarlet.LowResObservationBatch(np.zeros((3, 2, 16, 16), np.float32), band0=0, geometry=part)
    with pytest.raises(ValueError):
        part.factors
    with pytest.raises(ValueError, match="match"):
        scarlet.LowResObservationBatch(np.zeros((3, 2, 16, 16), np.float32), band0=0,
                                       geometry=scarlet.LowResObservation(g["a_images_lr"], wcs=AffineWCS((16, 16), 2.0),
                                                                          psfs=g["a_lr_psfs"].copy()))
    good, _ = lc.geometry(g, "a")
    with pytest.raises(ValueError, match="geometries for S"):
        scarlet.LowResObservationBatch(np.zeros((3, 2, 16, 16), np.float32), geometry=[good, good])
    with pytest.raises(ValueError, match="geometry describes"):
        scarlet.LowResObservationBatch(np.zeros((3, 2, 12, 12), np.float32), geometry=good)
    lo = scarlet.LowResObservationBatch(np.zeros((3, 2, 16, 16), np.float32), band0=3, geometry=good)
    assert lo.B == 2 and lo.model_shape == (32, 32) and not lo.per_scene
    assert good.pixel_of(12, 13) == (6, 6)
    other, _ = lc.geometry(g, "b")
    assert other.pixel_of(12, 13) == (int((12 - 1.3) / 2.5), int((13 - 0.6) / 2.5))
    hi = scarlet.ObservationBatch(np.zeros((3, 3, 24, 24), np.float32))
    with pytest.raises(ValueError, match="low-resolution observation 1"):
        scarlet.BlendBatch.from_observations([hi, lo], np.zeros((3, 1, 2), np.int32))


def test_init_combined_refuses_a_low_resolution_morphology(g):
    import scarlet_amd as scarlet
    good, _ = lc.geometry(g, "a")
    lo = scarlet.LowResObservationBatch(np.zeros((2, 2, 16, 16), np.float32), band0=3, geometry=good)
    hi = scarlet.ObservationBatch(np.zeros((2, 3, 32, 32), np.float32))
    b = scarlet.BlendBatch.__new__(scarlet.BlendBatch)
    b.torch, b.S, b.B = None, 2, 5
    b._observations = [(hi, None), (lo, None)]
    with pytest.raises(ValueError, match="low-resolution"):
        b.init_combined([np.ones(3), None], obs_idx=1)


# ---------------------------------------------------------------------------------------------- the C ABI
def test_header_library_and_ctypes_agree(tmp_path):
    from scarlet_amd import _lib
    flat = re.sub(r"\s+", " ", open(HEADER).read())
    assert ("int scarlet_fit_observations_lowres(scarlet_batch *state, const scarlet_constraints *c, scarlet_batch *const *obs, "
            "const scarlet_lowres *const *lowres, const int32_t *band0, int n_obs, int max_iter, double e_rel, "
            "int approximate_L, int check_every, void *stream);") in flat
    for fn in ("scarlet_lowres_workspace_bytes", "scarlet_fit_observations_lowres", "scarlet_lowres_render",
               "scarlet_lowres_adjoint"):
        assert re.search(r"\b%s\(" % fn, flat) and fn in _lib.EXPORTS and getattr(_lib.lib, fn)
    assert [f for f, _ in _lib.ScarletLowres._fields_] == FIELDS
    src = tmp_path / "probe.c"
    body = "\n".join('printf("%s %%zu\\n", offsetof(scarlet_lowres, %s));' % (f, f) for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scarlet_hip.h"\n'
                   'int main(void){ printf("sizeof %zu\\n", sizeof(scarlet_lowres));\n'
                   'printf("batch %zu\\n", sizeof(scarlet_batch));\n' + body + '\nreturn 0;}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = {k: int(v) for k, v in (ln.split() for ln in subprocess.check_output([str(exe)]).decode().splitlines())}
    for f in FIELDS:
        assert out[f] == getattr(_lib.ScarletLowres, f).offset, f
    assert out["sizeof"] == 80 == ctypes.sizeof(_lib.ScarletLowres)
    assert out["batch"] == 256 == ctypes.sizeof(_lib.ScarletBatch)          # scarlet_batch did not change


def _batch(S, K, B, H, W):
    from scarlet_amd import _lib
    b = _lib.ScarletBatch()
    b.S, b.K, b.B, b.H, b.W = S, K, B, H, W
    for f in ("images", "cur", "centers", "shifts", "flags", "lipschitz", "mse", "it", "active", "status", "workspace"):
        setattr(b, f, FAKE)
    b.sed[0] = b.sed[1] = b.morph[0] = b.morph[1] = FAKE
    b.mse_capacity = 1
    return b


def _lowres(h=16, w=16, nfy=9, nfx=17, B=2, **kw):
    from scarlet_amd import _lib
    lr = _lib.ScarletLowres()
    lr.h, lr.w, lr.nfy, lr.nfx, lr.B = h, w, nfy, nfx, B
    for f in ("uy", "ux", "vy", "vx", "dhat", "workspace"):
        setattr(lr, f, FAKE)
    for k, v in kw.items():
        setattr(lr, k, v)
    return lr


def _fit(state, obs, lows, band0, with_list=True):
    from scarlet_amd import _lib
    n = len(obs)
    arr = (ctypes.POINTER(_lib.ScarletBatch) * n)(*[ctypes.pointer(o) for o in obs])
    low = (ctypes.POINTER(_lib.ScarletLowres) * n)(*[ctypes.pointer(x) if x is not None else
                                                     ctypes.POINTER(_lib.ScarletLowres)() for x in lows])
    b0 = np.asarray(band0, dtype=np.int32)
    cons = _lib.ScarletConstraints()
    return _lib.lib.scarlet_fit_observations_lowres(ctypes.byref(state), ctypes.byref(cons), arr, low if with_list else None,
                                                    b0.ctypes.data_as(ctypes.c_void_p), n, 1, 0.0, 0, 0, None)


def test_argument_errors_come_back_before_any_launch():
    from scarlet_amd import _lib
    st, hi, lo = _batch(3, 2, 5, 32, 32), _batch(3, 2, 3, 32, 32), _batch(3, 2, 2, 16, 16)
    assert _fit(st, [hi, lo], [None, _lowres()], [0, 3], with_list=False) == _lib.E_ARG
    assert "low-resolution list" in _lib.last_error()
    # the observation's batch against its scarlet_lowres and the model frame
    for bad_lo, lr, b0 in ((_batch(3, 2, 2, 16, 12), _lowres(), 3), (_batch(3, 2, 2, 16, 16), _lowres(h=12), 3),
                           (_batch(2, 2, 2, 16, 16), _lowres(), 3), (_batch(3, 1, 2, 16, 16), _lowres(), 3),
                           (_batch(3, 2, 2, 16, 16), _lowres(), 4), (_batch(3, 2, 2, 16, 16), _lowres(), -1)):
        assert _fit(st, [hi, bad_lo], [None, lr], [0, b0]) == _lib.E_ARG
        assert "low-resolution observation does not fit" in _lib.last_error()
    assert _fit(st, [hi, lo], [None, _lowres(B=3)], [0, 3]) == _lib.E_ARG and "bad shape" in _lib.last_error()
    assert _fit(st, [hi, lo], [None, _lowres(nfy=0)], [0, 3]) == _lib.E_ARG and "bad shape" in _lib.last_error()
    with_kernel = _batch(3, 2, 2, 16, 16)
    with_kernel.diff_kernel, with_kernel.psf_h, with_kernel.psf_w = FAKE, 5, 5
    assert _fit(st, [hi, with_kernel], [None, _lowres()], [0, 3]) == _lib.E_ARG and "diff_kernel" in _lib.last_error()
    counted = _batch(3, 2, 2, 16, 16)
    counted.n_components = FAKE
    assert _fit(st, [hi, counted], [None, _lowres()], [0, 3]) == _lib.E_ARG and "n_components" in _lib.last_error()
    for name in ("uy", "ux", "vy", "vx", "dhat"):
        assert _fit(st, [hi, lo], [None, _lowres(**{name: None})], [0, 3]) == _lib.E_ARG
        assert "null factor" in _lib.last_error()
    assert _fit(st, [hi, lo], [None, _lowres(workspace=None)], [0, 3]) == _lib.E_ARG and "workspace" in _lib.last_error()
    # beyond LDS: 256 x 256 model planes
    big, big_hi, big_lo = _batch(3, 2, 5, 256, 256), _batch(3, 2, 3, 256, 256), _batch(3, 2, 2, 64, 64)
    assert _fit(big, [big_hi, big_lo], [None, _lowres(h=64, w=64, nfy=66, nfx=131)], [0, 3]) == _lib.E_NOTIMPL
    assert "LDS" in _lib.last_error()
    # the limit the header promises: 64 x 64 with 32 x 32 images, an 11-pixel PSF (72-point plane) and 8 bands is sized
    st8, lo8 = _batch(3, 2, 8, 64, 64), _batch(3, 2, 8, 32, 32)
    lr8 = _lowres(h=32, w=32, nfy=19, nfx=37, B=8)           # (nfy, nfx as match() makes them: geometry d)
    n = _lib.lib.scarlet_lowres_workspace_bytes(ctypes.byref(st8), ctypes.byref(lo8), ctypes.byref(lr8))
    assert n == 3 * 8 * 64 * 64 * 4 + 3 * 8 * 8
    assert _lib.lib.scarlet_lowres_workspace_bytes(ctypes.byref(big), ctypes.byref(big_lo),
                                                   ctypes.byref(_lowres(h=64, w=64, nfy=66, nfx=131))) == _lib.E_NOTIMPL
    # the plane operators
    lr = _lowres()
    for fn in (_lib.lib.scarlet_lowres_render, _lib.lib.scarlet_lowres_adjoint):
        assert fn(None, 1, 32, 32, ctypes.byref(lr), None, None, FAKE, None) == _lib.E_ARG and "null plane" in _lib.last_error()
        assert fn(FAKE, -1, 32, 32, ctypes.byref(lr), None, None, FAKE, None) == _lib.E_ARG
        assert fn(FAKE, 1, 32, 32, None, None, None, FAKE, None) == _lib.E_ARG
        assert fn(FAKE, 1, 32, 32, ctypes.byref(_lowres(ux=None)), None, None, FAKE, None) == _lib.E_ARG
        assert fn(FAKE, 1, 1024, 1024, ctypes.byref(lr), None, None, FAKE, None) == _lib.E_NOTIMPL
        assert fn(FAKE, 0, 32, 32, ctypes.byref(lr), None, None, FAKE, None) == 0


def _half(side):
    """side x side model frame, images of half its side on the same corner, 11- and 9-pixel PSFs: the header's family"""
    return ((side, side), (side // 2, side // 2), 2.0, (0.0, 0.0), (11, 9), None)


@pytest.mark.parametrize("side,nf,accepted,refused", [(64, (19, 37), 8, None), (72, (19, 41), 8, None), (76, (21, 41), 6, 7),
                                                      (84, (23, 45), 2, 3), (88, (25, 49), None, 1)])
def test_lds_boundary_is_where_the_header_says(side, nf, accepted, refused):
    """scarlet_hip.h: "64 x 64 ... at B = 8 bands; 72 x 72 with 36 x 36 still fits at B = 8, 76 x 76 up to B = 6,
    84 x 84 up to B = 2; beyond: SCARLET_E_NOTIMPL", with the frequencies match() gives.  The restated footprint
    (lowres_common.scratch_terms) sits on the same side of 159 KiB as the library's answer."""
    from scarlet_amd import _lib
    obs, _ = lc.limit_geometry(_half(side))
    d = _dims(obs)
    assert d[4:] == nf
    _, fixed = lc.scratch_terms(*d)
    for B, ok in ((accepted, True), (refused, False)):
        if B is None:
            continue
        st, lo = _batch(3, 2, B, side, side), _batch(3, 2, B, side // 2, side // 2)
        lr = _lowres(h=side // 2, w=side // 2, nfy=nf[0], nfx=nf[1], B=B)
        n = _lib.lib.scarlet_lowres_workspace_bytes(ctypes.byref(st), ctypes.byref(lo), ctypes.byref(lr))
        lds = fixed + B * 8 * nf[0] * nf[1]
        print("%d x %d, B = %d: %.1f KiB" % (side, side, B, lds / 1024.0))
        assert (lds <= 159 * 1024) == ok
        if ok:
            assert n == (3 * B * side * side * 4 + 15) // 16 * 16 + 3 * B * 8
        else:
            assert n == _lib.E_NOTIMPL and "LDS" in _lib.last_error()
