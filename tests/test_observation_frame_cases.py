"""CPU: the joint-fit ragged-frame cases of tests/observation_frame_cases.py.  Every scene is admissible on its own frame in
the oracle; the float32 and float64 oracle runs agree to 1e-6 with equal supports and centres, so the GPU test needs (and
has) no threshold-straddle exemption; and padding with zero weights is NOT the reference's result for the scene."""
import multiprocessing as mp
import os

import numpy as np
import pytest

from conftest import rel_err
import observation_frame_cases as oc


@pytest.fixture(scope="module")
def pool():
    from oracle import build as obuild
    obuild.build()
    p = mp.get_context("spawn").Pool(min(16, os.cpu_count() or 1))
    yield p
    p.close(); p.join()


@pytest.fixture(scope="module")
def runs(pool):
    """every scene of every case on its own frame, in float32 and in float64: computed once, read-only"""
    jobs = [(name, s, c.iters, dt) for name, c in oc.CASES.items() for s in range(len(c.shapes)) for dt in ("float32", "float64")]
    return dict(zip([j[:2] + j[3:] for j in jobs], pool.map(oc.oracle_own_frame, jobs)))


def test_the_cases_are_the_listed_ones():
    assert list(oc.CASES) == ["wave", "psf", "tile", "wave_k12", "epochs", "wide"]
    for c in oc.CASES.values():
        assert c.iters == 6 and len(c.bands) == 2
        assert all(nb <= 8 for _, nb in c.bands) and max(b0 + nb for b0, nb in c.bands) == c.C
        assert all(1 <= h <= c.H and 1 <= w <= c.W for h, w in c.shapes) and c.W % 4 == 0
    assert oc.CASES["epochs"].bands == ((0, 3), (0, 3)) and oc.CASES["wide"].bands == ((0, 5), (5, 4))
    assert oc.CASES["wide"].C == 9 and oc.CASES["wave_k12"].K == 12 and oc.CASES["psf"].psf
    assert [oc.CASES[n].bands for n in ("wave", "psf", "tile", "wave_k12")] == [((0, 2), (2, 1))] * 4
    d = oc.diff_kernels(oc.CASES["psf"])
    assert d[0].shape[0] == 2 and d[1] is None
    obs, shapes, centers, counts = oc.padded(oc.CASES["wave"], fill=7.0)
    assert obs[0]["images"].shape == (7, 2, 40, 40) and obs[1]["images"].shape == (7, 1, 40, 40) and obs[1]["band0"] == 2
    h, w = shapes[3]
    assert (obs[0]["images"][3, :, h:] == 7).all() and (obs[0]["images"][3, :, :, w:] == 7).all()
    assert np.array_equal(obs[1]["images"][3, :, :h, :w], oc.scene_observations(oc.CASES["wave"], 3)[1])


@pytest.mark.parametrize("name", list(oc.CASES))
def test_every_scene_is_admissible_on_its_own_frame(runs, name):
    """no SourceInitError, no refused max_pixel window (either would raise in the worker), finite results"""
    c = oc.CASES[name]
    for s, (h, w) in enumerate(c.shapes):
        sed, morph, mse, cen, it, _ = runs[(name, s, "float32")]
        assert sed.shape == (c.counts[s], c.C) and morph.shape == (c.counts[s], h, w) and it == len(mse) == c.iters, (name, s)
        assert np.isfinite(sed).all() and np.isfinite(morph).all() and np.isfinite(mse).all(), (name, s)
        assert (morph.max(axis=(1, 2)) > 0).all(), (name, s)
        assert ((cen >= 0) & (cen < np.array([h, w]))).all(), (name, s)


@pytest.mark.parametrize("name", list(oc.CASES))
def test_float32_and_float64_agree_far_inside_the_tolerance(runs, name):
    """the condition under which the GPU test takes no threshold-straddle exemption: no pixel of any scene sits on a
    threshold at float32 precision -- the two runs agree to 1e-6 (a tenth of the GPU tolerance) in every array and have
    the same support and the same centres"""
    c = oc.CASES[name]
    for s in range(len(c.shapes)):
        a, b = runs[(name, s, "float32")], runs[(name, s, "float64")]
        e = dict(sed=rel_err(a[0], b[0]), morph=rel_err(a[1], b[1]), mse=rel_err(a[2], b[2]))
        print("%s scene %d %s: %s" % (name, s, c.shapes[s], {k: "%.1e" % v for k, v in e.items()}))
        assert np.array_equal(a[1] == 0, b[1] == 0), (name, s, int(((a[1] == 0) != (b[1] == 0)).sum()))
        assert np.array_equal(a[3], b[3]), (name, s)
        assert max(e.values()) <= 1e-6, (name, s, e)


def test_zero_weight_padding_is_not_the_own_frame_result(pool):
    """case wave, 10 iterations: the zero-weight-padded joint fit differs from the own-frame one by more than 1e-4 (10 x
    the GPU tolerance) in the morphologies of at least four scenes -- so tests/test_gpu_observations_frames.py can tell an
    implementation that only masks the likelihoods from one that runs the constraints on each scene's own frame"""
    c = oc.CASES["wave"]
    S = len(c.shapes)
    own = pool.map(oc.oracle_own_frame, [("wave", s, 10, "float32") for s in range(S)])
    pad = pool.map(oc.oracle_zero_weight_padded, [("wave", s, 10) for s in range(S)])
    diff = [rel_err(pad[s][1], own[s][1]) for s in range(S)]
    print("\nzero-weight padding vs own frame, morphologies:", ["%s %.2e" % (c.shapes[s], d) for s, d in enumerate(diff)])
    assert diff[0] == 0.0, "the full-size scene is the same computation"
    assert sum(d > 1e-4 for d in diff) >= 4, diff
