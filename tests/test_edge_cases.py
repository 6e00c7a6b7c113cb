"""CPU only: every scene of tests/edge_cases.py is admissible, decided against the oracle alone and before any device
run -- these conditions are what makes the comparison of tests/test_gpu_edges.py fair.  For every scene of every case,
with the float32 and the float64 oracle started from their own constructors (ExtendedSource per catalogue pixel, the
group as a MultiComponentSource):

  * the fit completes, and no centre of any iteration (the constructors' included) has a coordinate below 2: the
    reference's max_pixel raises there;
  * every peak the case places on a limit ends on coordinate 2 or H - 1 / W - 1: the tracker reached the border, it
    did not merely start near it;
  * float32 and float64 agree to 1e-5 on sed, morph and the loss history, with equal centres (every iteration) and
    flags: the scene does not sit on a positivity threshold between the two precisions;
  * frames up to 64 px: component 0 of scene 0 is positive at the pixel farthest from its peak after every iteration,
    so the sweep runs to its last level; larger frames: it has a positive pixel farther than 63 px (Chebyshev) from its
    peak after every iteration, so neither box is complete and the full-frame kernel takes over.

A scene that fails gets another seed in edge_cases.SEEDS.  The layout rules of the table are checked as well."""
import numpy as np
import pytest

import edge_cases as ec
import launch_form_cases as lf

NAMES = list(ec.CASES)


def test_the_table_covers_every_fit_case_and_the_two_psf_forms():
    fit = [n for n, c in lf.CASES.items() if c.kind == "fit"]
    assert NAMES[:len(fit)] == fit and len(fit) == 23
    assert [(ec.CASES[n].B, ec.CASES[n].K, ec.CASES[n].H, ec.CASES[n].W, ec.PSF[n]) for n in NAMES[len(fit):]] == \
        [(3, 3, 32, 40, 9), (5, 4, 64, 64, 41)]
    for n in NAMES:
        c = ec.CASES[n]
        want = 11 if (max(c.H, c.W) <= 20 or n == "04_exact_persistent") else max(c.iters or 0, 6)
        assert ec.iterations(c) == want >= 6
    assert [n for n in NAMES if ec.one_launch_per_iteration(ec.CASES[n])] == ["03_exact_one_iteration"]


@pytest.mark.parametrize("name", NAMES)
def test_peak_layout(name):
    c = ec.CASES[name]
    cor, mid = ec.corners(c), ec.mid_edges(c)
    assert cor == [(2, 2), (2, c.W - 1), (c.H - 1, 2), (c.H - 1, c.W - 1)]
    assert mid == [(2, c.W // 2), (c.H - 1, c.W // 2), (c.H // 2, 2), (c.H // 2, c.W - 1)]
    used, opposite = [], []
    for s in range(ec.S):
        images, pixels, peaks = ec.scene(c, s)
        assert images.shape == (c.B, c.H, c.W) and images.dtype == np.float32 and pixels.shape == (c.K, 2)
        assert all(p in cor + mid for p in peaks)
        low = [p for p in peaks if 2 in p]
        high = [p for p in peaks if p[0] == c.H - 1 or p[1] == c.W - 1]
        assert low and high
        mine = [p for p in peaks if p in cor]
        opposite.append(any((c.H + 1 - p[0], c.W + 1 - p[1]) in mine for p in mine))
        used.append(set(mine))
        distinct = sorted(set(peaks))
        assert len(distinct) == (c.K - 1 if ec.grouped(c) else c.K)
        assert all(max(abs(p[0] - q[0]), abs(p[1] - q[1])) >= 3 for p in distinct for q in distinct if p != q)
        if not ec.displaced(c, s):
            assert [tuple(p) for p in pixels] == peaks and (s == 0 or name in ec.PSF)
        else:
            for p, q in zip(pixels, peaks):
                d = (int(p[0]) - q[0], int(p[1]) - q[1])
                assert d == tuple((1 if v == 2 else -1 if v == n - 1 else 0) for v, n in zip(q, (c.H, c.W))) and d != (0, 0)
        if ec.grouped(c):
            assert peaks[0] == peaks[1] and peaks[0] in cor
    assert used[0] != used[1] and opposite == [False, True]          # (scene 0 keeps its broad source's far corner free)
    img, pix = ec.refused_scene(c)
    assert tuple(pix[-1]) == (1, 10) and img.shape == (c.B, c.H, c.W)


@pytest.mark.parametrize("s", range(ec.S))
@pytest.mark.parametrize("name", NAMES)
def test_scene_is_admissible(name, s):
    c = ec.CASES[name]
    assert ec.admissible(c, s) is None
    r = ec.own_fit(c, s)
    ends = [tuple(int(v) for v in p) for p in r["cen"]]
    print("%s scene %d: %d iterations, centres %s -> %s" % (name, s, r["it"], ec.scene(c, s)[1].tolist(), ends))
    if ec.displaced(c, s):                           # the tracker moved: no source ended on its catalogue pixel
        assert all(e != tuple(p) for e, p in zip(ends, ec.scene(c, s)[1].tolist()))
