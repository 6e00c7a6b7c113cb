"""CPU: the catalogue cases of tests/catalog_cases.py are admissible in the oracle -- every scene starts and fits alone on
its own frame without a refused source -- and they discriminate: the same scenes zero-padded with zero weights give
another result for a grouped component; and the host logic of SourceSpec / catalog_arrays / BlendBatch.from_catalog."""
import multiprocessing as mp
import os

import numpy as np
import pytest

from conftest import rel_err
import catalog_cases as cc
import frame_cases as fc


@pytest.fixture(scope="module")
def pool():
    from oracle import build as obuild
    obuild.build()
    p = mp.get_context("spawn").Pool(min(16, os.cpu_count() or 1))
    yield p
    p.close(); p.join()


@pytest.fixture(scope="module")
def runs(pool):
    """{(case, how): [(start, fit) per scene]} -- computed once, read-only"""
    jobs = [(name, s, cc.ITERS, how) for name, c in cc.CASES.items() for s in range(len(c.shapes)) for how in ("own", "padded")]
    out = pool.map(cc.oracle_run, jobs)
    res = {}
    for (name, s, _, how), r in zip(jobs, out):
        res.setdefault((name, how), []).append(r)
    return res


def test_cases_cover_the_forms_the_row_tails_and_the_source_types():
    forms = {c.name: fc.update_form(*cc.padded_shape(c)) for c in cc.CASES.values()}
    assert forms == dict(wave="wave", tile="tile", plane="plane", plane_gt="plane", psf="wave")
    assert [cc.init_tile_in_lds(c) for c in cc.CASES.values()] == [True, True, True, False, True]
    assert cc.GT_SIDE == 141 and not cc.init_tile_in_lds(cc.CASES["plane_gt"])
    for c in cc.CASES.values():
        H, W = cc.padded_shape(c)
        ws = [w for _, w in c.shapes]
        assert any(w % 4 for w in ws), c.name
        assert any(w % 4 == 0 and w < W for w in ws), c.name
        assert c.shapes[0][0] == H and len(c.catalog) == len(c.shapes), c.name
        # every grouped source lies within the default centroid PSF's radius (20 px) of an end of its own frame
        for (h, w), cat in zip(c.shapes, cc.catalog(c)):
            for (y, x), kind, _ in cat:
                assert 0 <= y < h and 0 <= x < w
                if kind == "multi":
                    assert min(y, x, h - 1 - y, w - 1 - x) < 20, (c.name, (h, w), (y, x))
    wave = cc.CASES["wave"]
    assert wave.catalog[0] == (cc.M, cc.P, cc.E) and wave.catalog[1] == (cc.M3, cc.E) and wave.catalog[3] == (cc.E,)
    assert sorted(set(cc.n_components(wave, s) for s in range(6))) == [1, 2, 3, 4]          # ragged counts
    psf = cc.CASES["psf"]
    s, (y, x) = psf.star
    h, w = psf.shapes[s]
    assert (h - 1 - y, w - 1 - x) == (2, 2) and w < cc.padded_shape(psf)[1]


@pytest.mark.parametrize("name", list(cc.CASES))
def test_every_scene_is_admissible_on_its_own_frame(runs, name):
    """no SourceInitError (NO_VALID_PIXELS), no empty layer (a division by zero -> non-finite), no singular normal matrix
    (np.linalg.inv raises in the worker), no centre that leaves its frame"""
    c = cc.CASES[name]
    for s, (start, fit) in enumerate(runs[(name, "own")]):
        h, w = c.shapes[s]
        n = cc.n_components(c, s)
        for st in (start, fit):
            assert st["morph"].shape == (n, h, w) and st["sed"].shape == (n, c.B), (name, s)
            assert np.isfinite(st["sed"]).all() and np.isfinite(st["morph"]).all(), (name, s)
            assert (st["morph"].max(axis=(1, 2)) > 0).all(), (name, s)
            assert ((st["centers"] >= 0) & (st["centers"] < np.array([h, w]))).all(), (name, s)
        assert fit["it"] == cc.ITERS and np.isfinite(fit["mse"]).all(), (name, s)


def test_zero_weight_padding_is_not_the_own_frame_result_for_grouped_sources(runs):
    """For every case at least one grouped component's morphology after 6 iterations differs between the own-frame run
    and the zero-weight-padded run by more than 1e-4 relative max-norm (10 x the GPU tolerance): a kernel that took the
    padded bounds could not pass tests/test_gpu_catalog.py.  Largest difference over the grouped components of each scene,
    measured with the float32 oracle (scenes in the case's order; the seeds were chosen so that a case differs: a compact
    source whose flux ends before the mirror of its frame's nearest end sees no difference):
      wave      0.0, 0.0, 3.2e-4, (no group), 3.9e-2, 7.5e-9
      tile      0.0, 5.3e-3, 0.0, 1.1e-2
      plane     0.0, 0.0, 5.4e-2
      plane_gt  0.0, 0.0, 7.1e-3
      psf       0.0, 9.2e-7, 4.1e-2"""
    for name, c in cc.CASES.items():
        own, pad = runs[(name, "own")], runs[(name, "padded")]
        diffs = []
        for s in range(len(c.shapes)):
            g = cc.grouped_components(c, s)
            diffs.append(max([rel_err(pad[s][1]["morph"][k], own[s][1]["morph"][k]) for k in g]) if g else None)
        print("\n%s: zero-weight padding vs own frame, grouped morphologies: %s"
              % (name, ["%s %s" % (c.shapes[s], "-" if d is None else "%.1e" % d) for s, d in enumerate(diffs)]))
        assert any(d is not None and d > 1e-4 for d in diffs), (name, diffs)


# ------------------------------------------------------------------ host logic
@pytest.fixture()
def no_gpu(monkeypatch):
    """the device is never asked for: every check below is made on the host first"""
    from scarlet_amd import _lib

    def refuse():
        raise AssertionError("the device was asked for before the host checks were done")
    monkeypatch.setattr(_lib, "require_gpu", refuse)


def _cut(shapes, B=3):
    return [np.zeros((B, h, w), np.float32) for h, w in shapes]


def test_catalog_arrays_of_a_hand_written_catalogue():
    import scarlet_amd as scarlet
    from scarlet_amd import _lib
    from scarlet_amd.batch import catalog_arrays
    S_ = scarlet.SourceSpec
    cat = [[S_((10, 11), kind="multi", flux_percentiles=[25]), S_((20, 5), kind="point"), S_((3, 4))],
           [S_((8, 9), kind="multi", flux_percentiles=[20, 60], symmetric=True, monotonic=False, l0_thresh=0.5)],
           [S_((1, 2), monotonic=False), S_((5, 6), kind="multi", l1_thresh=0.25)]]
    t = catalog_arrays([(30, 30), (16, 12), (9, 9)], cat)
    assert t["centers"].dtype == np.int32 and t["centers"].tolist() == [
        [[10, 11], [10, 11], [20, 5], [3, 4]], [[8, 9], [8, 9], [8, 9], [0, 0]], [[1, 2], [5, 6], [5, 6], [0, 0]]]
    assert t["n_components"].tolist() == [4, 3, 3]
    assert t["group"].tolist() == [[0, 0, -1, -1], [0, 0, 0, -1], [-1, 1, 1, -1]]
    E, Pt = _lib.INIT_EXTENDED, _lib.INIT_POINT
    assert t["kind"].tolist() == [[E, E, Pt, E], [E, E, E, E], [E, E, E, E]]
    assert t["percentiles"].tolist() == [[0, 25, 0, 0], [0, 20, 60, 0], [0, 0, 25, 0]]
    assert t["symmetric"].tolist() == [[1, 1, 1, 1], [1, 1, 1, 0], [1, 1, 1, 0]]
    assert t["monotonic"].tolist() == [[1, 1, 1, 1], [0, 0, 0, 0], [0, 1, 1, 0]]
    assert t["l0_thresh"].tolist() == [[-1, -1, -1, -1], [0.5, 0.5, 0.5, -1], [-1, -1, -1, -1]]
    assert t["l1_thresh"].tolist() == [[-1, -1, -1, -1], [-1, -1, -1, -1], [-1, 0.25, 0.25, -1]]
    assert t["sources"] == [[(0, 2), (2, 1), (3, 1)], [(0, 3)], [(0, 1), (1, 2)]]
    assert scarlet.SourceSpec((1, 1)).kind == "extended" and scarlet.SourceSpec((1, 1), kind="multi").layers() == 2


def test_from_catalog_host_errors_come_before_the_device(no_gpu):
    import scarlet_amd as scarlet
    from scarlet_amd import _lib
    S_ = scarlet.SourceSpec
    shapes = [(20, 24), (12, 30)]
    good = [[S_((5, 5))], [S_((6, 7), kind="multi")]]

    def raises(match, cutouts=None, cat=None, **kw):
        with pytest.raises(ValueError, match=match):
            scarlet.BlendBatch.from_catalog(_cut(shapes) if cutouts is None else cutouts, good if cat is None else cat, **kw)

    raises(r"scene 1, source 0: unknown source kind 'galaxy'", cat=[good[0], [S_((6, 7), kind="galaxy")]])
    raises(r"scene 1, source 0: flux_percentiles \[60.0, 20.0\] must be ascending", cat=[good[0], [S_((6, 7), "multi", [60, 20])]])
    raises(r"scene 0, source 1: flux_percentiles \[0.0\] must be ascending", cat=[[S_((5, 5)), S_((9, 9), "multi", [0])], good[1]])
    raises(r"scene 0, source 0: flux_percentiles \[25.0, 100.0\]", cat=[[S_((5, 5), "multi", [25, 100])], good[1]])
    many = list(range(5, 5 + 5 * _lib.MAX_LAYERS, 5))
    raises(r"scene 1, source 0: %d flux_percentiles give %d layers" % (len(many), len(many) + 1),
           cat=[good[0], [S_((6, 7), "multi", many)]])
    raises(r"scene 1, source 1: centre \(12, 3\) lies outside the scene's own 12 x 30 frame",
           cat=[good[0], [S_((6, 7)), S_((12, 3))]])                       # inside the padded frame, outside its own
    raises(r"scene 0, source 0: centre \(5, 24\) lies outside", cat=[[S_((5, 24), "point")], good[1]])
    raises(r"scene 0, source 0: flux_percentiles belong to a multi source", cat=[[S_((5, 5), "point", [25])], good[1]])
    raises(r"scene 1, source 0: flux_percentiles belong to a multi source", cat=[good[0], [S_((5, 5), flux_percentiles=[25])]])
    raises(r"scene 1 has no sources", cat=[good[0], []])
    raises(r"scene 1 has B = 2 bands, scene 0 has 3", cutouts=[np.zeros((3, 20, 24)), np.zeros((2, 12, 30))])
    raises(r"1 catalogues for 2 scenes", cat=[good[0]])
    raises(r"comes from the catalogue", group=np.zeros((2, 2)))
    # a uniform block goes the same way
    raises(r"scene 1, source 0: centre \(20, 0\) lies outside", cutouts=np.zeros((2, 3, 20, 24), np.float32),
           cat=[good[0], [S_((20, 0))]])
    # the last host step: a good catalogue reaches the device request, and nothing before it needed one
    with pytest.raises(AssertionError, match="the device was asked for"):
        scarlet.BlendBatch.from_catalog(_cut(shapes), good)


def test_pinned_entry_points_still_refuse(no_gpu):
    """the old routes stay closed: a ragged-frame BlendBatch takes no group="""
    import scarlet_amd as scarlet
    with pytest.raises(NotImplementedError):
        scarlet.BlendBatch(_cut([(20, 24), (12, 30)]), np.zeros((2, 2, 2), np.int32), group=np.zeros((2, 2), np.int32))
