"""CPU: the facts that tests/lowres_frame_cases.py and the ragged-frames low-resolution kernels rest on.

  1. every geometry of the cases covers its observation; the (nfy, nfx) of `small` are all different and both
     orientations of w <= h occur; the maxima of `lds_edge` come from different scenes and fit LDS at B = 8, those of
     `streamed` do not fit;
  2. the operator of a scene's own frame is NOT the operator of the padded frame (more than 1e-2 apart on `small`):
     without this the cases would not test the feature;
  3. zero-padding a scene's own factor matrices to the maxima is exact: the render equals the own-frame render to 1e-12
     inside the scene's pixels and is exactly 0 outside, the adjoint is exactly 0 outside the scene's model frame;
  4. LowResObservationBatch.from_frames(geometry=) packs exactly those tables and the `dims` table.
"""
import numpy as np
import pytest

import lowres_frame_cases as fc
from scarlet_amd import resampling as rs


def test_every_geometry_covers_and_the_shapes_are_what_the_cases_say():
    for name in fc.CASES:
        for g in fc.geometries(name):
            assert g.covers, (name, g.model_shape)
    small = fc.geometries("small")
    nf = [fc.dims_of(g)[4:] for g in small]
    assert nf == fc.SMALL_NF and len(set(nf)) == len(nf)
    assert {bool(g.small_axis) for g in small} == {True, False}
    assert fc.maxima("small") == (32, 32, 16, 16, 9, 17)


def test_lds_edge_maxima_come_from_different_scenes_and_fit():
    dims = np.array([fc.dims_of(g) for g in fc.geometries("lds_edge")])
    mx = fc.maxima("lds_edge")
    assert mx == (64, 64, 36, 36, 19, 37)
    owners = [set(np.nonzero(dims[:, i] == mx[i])[0].tolist()) for i in range(6)]
    assert not set.intersection(*owners), owners              # no one scene holds every maximum
    assert owners[2] == owners[3] == {2} and 2 not in owners[0] and 2 not in owners[5]
    B = fc.CASES["lds_edge"][0]
    total = fc.lds_bytes(mx, B)
    assert round(total / 1024, 1) == 134.5 and total <= fc.LDS_LIMIT
    # planned from any one scene's dims the layout would be too small for another scene
    assert all(fc.lds_bytes(tuple(d), B) < total for d in dims)


def test_streamed_maxima_do_not_fit_lds():
    total = fc.lds_bytes(fc.maxima("streamed"), fc.CASES["streamed"][0])
    assert round(total / 1024) == 196 and total > fc.LDS_LIMIT


def test_own_frame_operator_is_not_the_padded_frame_operator():
    B, scenes = fc.CASES["small"]
    Hm, Wm = fc.maxima("small")[:2]
    rng = np.random.default_rng(3)
    worst = 0.0
    for (m, o, r, org), own in zip(scenes, fc.geometries("small")):
        if m == (Hm, Wm):
            continue
        padded = fc.geometry((Hm, Wm), o, r, org, B)
        assert padded.covers
        model = np.zeros((B, Hm, Wm))
        model[:, :m[0], :m[1]] = rng.random((B,) + m)
        a, b = rs.apply_factors(own.factors, model[:, :m[0], :m[1]]), rs.apply_factors(padded.factors, model)
        worst = max(worst, np.abs(a - b).max() / max(np.abs(a).max(), np.abs(b).max()))
    assert worst > 1e-2, worst


@pytest.mark.parametrize("name", list(fc.CASES))
def test_zero_padded_factors_are_exact(name):
    mx = fc.maxima(name)
    H, W, h, w = mx[:4]
    rng = np.random.default_rng(5)
    for g in fc.geometries(name):
        f = g.factors
        Hs, Ws, hs, ws = fc.dims_of(g)[:4]
        B = f["dhat"].shape[0]
        p = fc.pad_factors(f, mx)
        model = np.zeros((B, H, W))
        model[:, :Hs, :Ws] = rng.random((B, Hs, Ws))
        resid = np.zeros((B, h, w))
        resid[:, :hs, :ws] = rng.standard_normal((B, hs, ws))
        want, got = rs.apply_factors(f, model[:, :Hs, :Ws]), rs.apply_factors(p, model)
        assert np.abs(got[:, :hs, :ws] - want).max() <= 1e-12 * np.abs(want).max()
        assert not got[:, hs:].any() and not got[:, :, ws:].any()
        want, got = rs.adjoint_factors(f, resid[:, :hs, :ws]), rs.adjoint_factors(p, resid)
        assert np.abs(got[:, :Hs, :Ws] - want).max() <= 1e-12 * np.abs(want).max()
        assert not got[:, Hs:].any() and not got[:, :, Ws:].any()
        # ... whatever lies in the padding of the inputs
        dirty = rng.random((B, H, W))
        dirty[:, :Hs, :Ws] = model[:, :Hs, :Ws]
        assert np.array_equal(rs.apply_factors(p, dirty), rs.apply_factors(p, model))


@pytest.mark.parametrize("name", list(fc.CASES))
def test_from_frames_packs_the_padded_tables(name):
    from scarlet_amd import LowResObservationBatch
    B = fc.CASES[name][0]
    geos = list(fc.geometries(name))
    images = [np.full((B,) + tuple(g.frame.shape[1:]), s + 1.0, np.float32) for s, g in enumerate(geos)]
    lo = LowResObservationBatch.from_frames(images, band0=3, geometry=geos, weights=2.0)
    S = len(geos)
    dims = np.array([fc.dims_of(g) for g in geos], dtype=np.int32)
    assert lo.dims.dtype == np.int32 and np.array_equal(lo.dims, dims)
    assert np.array_equal(lo.model_shapes, dims[:, :2]) and np.array_equal(lo.frame_shapes, dims[:, 2:4])
    h, w = lo.shape[2:]
    assert lo.shape == (S, B, dims[:, 2].max(), -(-dims[:, 3].max() // 4) * 4)
    mx = (dims[:, 0].max(), dims[:, 1].max(), h, w, dims[:, 4].max(), dims[:, 5].max())
    for s, g in enumerate(geos):
        want = fc.pad_factors(g.factors_f32(), mx)
        for k, v in want.items():
            assert lo.host_factors[k].shape == (S,) + v.shape and lo.host_factors[k].dtype == np.float32
            assert np.array_equal(lo.host_factors[k][s], v), (s, k)
        hs, ws = dims[s, 2:4]
        assert (lo.images[s, :, :hs, :ws] == s + 1.0).all() and not lo.images[s, :, hs:].any() and not lo.images[s, :, :, ws:].any()
    # the padded-block spelling is the same observation
    again = LowResObservationBatch(lo.images, 3, geometry=geos, weights=2.0, frame_shapes=lo.frame_shapes)
    assert np.array_equal(again.dims, lo.dims) and all(np.array_equal(again.host_factors[k], lo.host_factors[k]) for k in lo.host_factors)
