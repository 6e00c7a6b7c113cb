"""CPU: the ragged-frame cases of tests/frame_cases.py are admissible -- the oracle starts and fits every scene on its own
frame with finite results -- and the alternative a user has without frame_shapes, padding with zero weights, is NOT the
reference's result for the scene; and pad_frames."""
import multiprocessing as mp
import os

import numpy as np
import pytest

from conftest import rel_err
import frame_cases as fc


@pytest.fixture(scope="module")
def pool():
    from oracle import build as obuild
    obuild.build()
    p = mp.get_context("spawn").Pool(min(16, os.cpu_count() or 1))
    yield p
    p.close(); p.join()


def test_cases_cover_the_forms_and_the_row_tails():
    forms = {c.name: fc.update_form(c.H, c.W) for c in fc.CASES.values()}
    assert forms == dict(wave="wave", wave_k6="wave", wave_k12="wave", tile="tile", tile_gscratch="tile_gscratch",
                         plane="plane", psf="wave")
    assert fc.PLANE_SIDE == 129
    for c in fc.CASES.values():
        ws = [w for _, w in c.shapes]
        assert any(w % 4 for w in ws), c.name
        assert any(w % 4 == 0 and w < c.W for w in ws), c.name
        assert all(1 <= h <= c.H and 1 <= w <= c.W for h, w in c.shapes), c.name
        assert c.shapes[0] == (c.H, c.W) and max(c.counts) == c.K and len(c.counts) == len(c.shapes), c.name
        assert 5 <= c.iters <= 10
        if c.hand:
            h, w = c.shapes[-1]
            assert fc.scenes(c)[-1][1].tolist() == [[h - 1, w - 1], [2, 2]]
    assert [c.name for c in fc.CASES.values() if c.hand] == ["wave", "tile", "psf"]


@pytest.mark.parametrize("name", list(fc.CASES))
def test_every_scene_is_admissible_on_its_own_frame(pool, name):
    """no SourceInitError, no refused max_pixel window (either would raise in the worker), finite results"""
    c = fc.CASES[name]
    out = pool.map(fc.oracle_own_frame, [(name, s, c.iters) for s in range(len(c.shapes))])
    for s, (sed, morph, mse, cen) in enumerate(out):
        h, w = c.shapes[s]
        assert morph.shape == (c.counts[s], h, w) and len(mse) == c.iters, (name, s)
        assert np.isfinite(sed).all() and np.isfinite(morph).all() and np.isfinite(mse).all(), (name, s)
        assert (morph.max(axis=(1, 2)) > 0).all(), (name, s)
        assert ((cen >= 0) & (cen < np.array([h, w]))).all(), (name, s)


def test_zero_weight_padding_is_not_the_own_frame_result(pool):
    """case wave, 10 iterations: the zero-weight-padded run differs from the own-frame run by more than 1e-4 (10 x the GPU
    tolerance) in the morphologies of at least two scenes -- so tests/test_gpu_frames.py can tell an implementation that
    only masks the likelihood from one that runs the constraints on each scene's own frame."""
    c = fc.CASES["wave"]
    jobs = [("wave", s, 10) for s in range(len(c.shapes))]
    own, pad = pool.map(fc.oracle_own_frame, jobs), pool.map(fc.oracle_zero_weight_padded, jobs)
    diff = [rel_err(pad[s][1], own[s][1]) for s in range(len(jobs))]
    print("\nzero-weight padding vs own frame, morphologies:", ["%s %.2e" % (c.shapes[s], d) for s, d in enumerate(diff)])
    assert diff[0] == 0.0, "the full-size scene is the same computation"
    assert sum(d > 1e-4 for d in diff) >= 2, diff
    assert diff[2] > 1e-4 and diff[3] > 1e-4, diff           # 40 x 27 and 17 x 23


def test_pad_frames():
    from scarlet_amd.batch import pad_frames
    rng = np.random.default_rng(5)
    arrs = [rng.normal(size=s).astype(np.float32) for s in ((3, 17, 23), (3, 40, 27), (3, 5, 1))]
    block, shapes = pad_frames(arrs)
    assert block.shape == (3, 3, 40, 28) and block.dtype == np.float32
    assert shapes.dtype == np.int32 and shapes.tolist() == [[17, 23], [40, 27], [5, 1]]
    for s, a in enumerate(arrs):
        h, w = a.shape[1:]
        assert np.array_equal(block[s, :, :h, :w], a)
        assert not block[s, :, h:].any() and not block[s, :, :, w:].any()
    filled, _ = pad_frames(arrs, fill=7)
    assert (filled[0, :, 17:] == 7).all() and (filled[0, :, :, 23:] == 7).all() and np.array_equal(filled[0, :, :17, :23], arrs[0])
    assert pad_frames([np.zeros((2, 8, 8))])[0].shape == (1, 2, 8, 8)          # W already a multiple of 4
    with pytest.raises(ValueError):
        pad_frames([np.zeros((3, 8, 8)), np.zeros((2, 8, 8))])                  # differing B
    with pytest.raises(ValueError):
        pad_frames([np.zeros((8, 8))])
    with pytest.raises(ValueError):
        pad_frames([])
