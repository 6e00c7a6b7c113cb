"""-m gpu: sources on the frame's borders on every single-observation launch form, against the CPU oracle.  The scenes
are those of tests/edge_cases.py (peaks on rows / columns 2 and H - 1 / W - 1, catalogue pixels of scene 1 one pixel
inside, a broad source that keeps the sweep going to its last level); tests/test_edge_cases.py proves each of them
admissible on the CPU, against the oracle alone.

Per case, under the case's options: the device's initial state against the oracle's own constructors (centres equal,
sed / morph within 1e-5), then the fit from the device's initial state against the float32 oracle -- status 0, the
iteration count asked for, centres, flags and iteration counts bit-exact, sed / morph / loss history within
parity_common.TOL = 1e-5 (parity_common.compare_fixed_iterations).  The float64-anchored threshold exemption of
parity_common may pass at most MAX_EXEMPT = 2 scenes in the WHOLE module (the CPU conditions already show that no
committed scene sits on a threshold in the reference); every use is logged.  Every worst error goes to the file named
by SCARLET_LOG_REL_ERR (`edges ...` lines; profiles/edges_rel_err.txt is a run's collection).

That a case took the form it is named for is read from the library's own launch recorder (scarlet_profile_begin /
_end_ex: class 4 is the one-launch iteration, one launch for the persistent kernel; class 2 the constraint update of a
general iteration, class 5 the PSF chain) and, beyond 64 px, from the box kernels' flags: the stage that served each
component is the one box_update_cases derives from the oracle's result -- the broad component was left to the full-frame
kernel, a box clipped at a corner served others.  Which instance of a kernel a shape and an option select has no hook; there the case's
options are the guarantee.

A centre the reference refuses ((1, 10): max_pixel's window would start at row -1) is a handled input of the kernels
(wave_ops.h wave_max_pixel, prox_ops.h max_pixel_tile): the scene is flagged and keeps the centre, its neighbours in the
batch are bit-identical to a run without it."""
import ctypes
import multiprocessing as mp
import os

import numpy as np
import pytest

from conftest import rel_err
import box_update_cases as bc
from constraints_common import box_fallback
import edge_cases as ec
import parity_common as pc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
TOL = pc.TOL
MAX_EXEMPT = 2
EXEMPT = []                     # the scenes the whole module has passed through the exemption
NAMES = list(ec.CASES)
FUSED = [n for n in NAMES if "NO_FUSED" not in ec.CASES[n].opts and n not in ec.PSF]
BOXED = [n for n in NAMES if max(ec.CASES[n].H, ec.CASES[n].W) > 64 and "NO_BOX" not in ec.CASES[n].opts and
         ec.CASES[n].batch.get("monotonic", True)]                 # (a batch without `monotonic` has no box stage)


@pytest.fixture(scope="module")
def env():
    import scarlet_amd
    scarlet_amd._lib.require_gpu()
    from oracle import build as obuild
    obuild.build()
    pool = mp.get_context("spawn").Pool(min(16, os.cpu_count() or 1))
    yield scarlet_amd, pool
    pool.close(); pool.join()


def log(line):
    print(line)
    path = os.environ.get("SCARLET_LOG_REL_ERR")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def start(scarlet, c, images, centers):
    """the case's batch of the given scenes and its initial state (sed, morph, centres, shifts)"""
    b = ec.make_batch(scarlet, c, images, centers)
    return b, [t.cpu().numpy() for t in (b.sed_current, b.morph_current, b.centers, b.shifts)]


def fit(scarlet, c, b, iters, per_iteration=False, profile=False):
    """`iters` iterations at e_rel = 0 without a host look: one fit call, or one call per iteration (a case of exactly
    one iteration per launch; the exemption's re-run, which keeps the morphologies after every iteration).  Returns
    parity_common.gpu_fit's result and, if asked, (iterations, launches) per profile class."""
    L, snaps, counts = scarlet._lib.lib, [], None
    if profile:
        scarlet._lib.check(L.scarlet_profile_begin(iters + 1))
    try:
        if per_iteration or ec.one_launch_per_iteration(c):
            for _ in range(iters):
                assert b.fit(1, e_rel=0, check_every=0) == 1
                if per_iteration:
                    snaps.append(b.morph_current.cpu().numpy().copy())
        else:
            assert b.fit(iters, e_rel=0, check_every=0) == iters
    finally:
        if profile:
            ms, its, launches = (ctypes.c_double * 8)(), (ctypes.c_int64 * 8)(), (ctypes.c_int64 * 8)()
            scarlet._lib.check(L.scarlet_profile_end_ex(ms, its, launches))
            counts = (list(its), list(launches))
    torch.cuda.synchronize()
    g = dict(sed=b.sed_current.cpu().numpy(), morph=b.morph_current.cpu().numpy(), cen=b.centers.cpu().numpy(),
             it=b.it.cpu().numpy(), flags=b.flags.cpu().numpy(), mse=b.mse_buf.cpu().numpy(), snaps=snaps,
             status=b.status.cpu().numpy())
    return g, counts


def check_form(c, iters, counts):
    its, launches = counts
    if c.name in FUSED:
        assert its == [0, 0, 0, 0, iters, 0, 0, 0], (c.name, its)
        assert launches[4] == (1 if c.name == "04_exact_persistent" else iters), (c.name, launches)
    else:
        assert its[4] == 0 and launches[4] == 0 and its[2] == iters, (c.name, its, launches)
        if c.name in ec.PSF:
            assert its[5] >= iters, (c.name, its)
        if c.name == "30_psf_three_pass_9":
            assert its == launches == [0, iters, iters, iters, 0, iters, 0, 0], (c.name, its, launches)


def check_stages(c, b, ref):
    """beyond 64 px: the box kernels' flags of the last update against the stage box_update_cases derives from the
    oracle's result -- a box of half-size R serves a component iff Lp + 3 <= min(Lall, 2 R), Lp the last sweep level
    with a positive value and Lall the last level of the box clipped to the frame (R = 63; 31 under NO_BOX2)"""
    R = bc.R_SMALL if "NO_BOX2" in c.opts else bc.R_LARGE
    fb = box_fallback(b)
    print("edges %s: box kernels' flags %s" % (c.name, fb.tolist()))
    want = np.zeros_like(fb)
    for s in range(ec.S):
        for k in range(c.K):
            cen = tuple(int(v) for v in ref[s][3][k])
            Lp = int(bc.level_map(c.H, c.W, *cen)[ref[s][1][k] > 0].max())
            want[s, k] = int(Lp + 3 > min(bc.box_lall(c.H, c.W, cen, R), 2 * R))
    assert np.array_equal(fb, want), (c.name, fb.tolist(), want.tolist())
    assert fb[0, 0] == 1, "%s: the broad component reaches beyond 63 px and was served by a box" % c.name
    assert (fb == 0).any(), "%s: no component on the border was served by a clipped box" % c.name


@pytest.mark.parametrize("name", NAMES)
def test_border_scenes_against_the_oracle(env, name):
    scarlet, pool = env
    c = ec.CASES[name]
    iters = ec.iterations(c)
    images, centers = ec.scenes(c)
    with ec.options(scarlet, c):
        b, st0 = start(scarlet, c, images, centers)
        # ---- the constructors at the borders: the sdss symmetry and the thresholded sweep in the float64 tile, then update()
        assert int(np.abs(b.status.cpu().numpy()).sum()) == 0
        for s in range(ec.S):
            sed, morph, cen, _ = ec.oracle_start(c, s, np.float32)
            np.testing.assert_array_equal(st0[2][s], cen, err_msg="%s scene %d: initial centres" % (name, s))
            e = dict(sed=rel_err(st0[0][s], sed), morph=rel_err(st0[1][s], morph))
            log("edges %-24s scene %d initial state: sed %.3e morph %.3e" % (name, s, e["sed"], e["morph"]))
            assert max(e.values()) <= TOL, (name, s, e)
        # ---- the fit, from the device's own initial state
        ref = pool.map_async(ec.oracle_worker, [(ec.spec(c, images[s], *[a[s] for a in st0]), iters) for s in range(ec.S)])
        g, counts = fit(scarlet, c, b, iters, profile=True)
        check_form(c, iters, counts)

        def straddle(i):
            b1, s1 = start(scarlet, c, images[i:i + 1], centers[i:i + 1])
            g1, _ = fit(scarlet, c, b1, iters, per_iteration=True)
            sp = ec.spec(c, images[i], *[a[0] for a in s1])
            o32, o64 = ec.fit_from(sp, iters, np.float32, trace=True), ec.fit_from(sp, iters, np.float64, trace=True)
            if "pre" not in o64:
                return False, "the layers of a group keep no trace of the threshold tests"
            return pc.straddle_verdict([m[0] for m in g1["snaps"]], o32["post"], o64["post"], o64["pre"], iters)

        ref = ref.get()
        if name in BOXED:
            check_stages(c, b, ref)
        worst = pc.compare_fixed_iterations(g, ref, iters, straddle, MAX_EXEMPT, "border scenes, " + name,
                                            exempt=EXEMPT, flags=True)
    log("edges %-24s %2d iterations x %d scenes: worst sed %.3e morph %.3e loss %.3e; exempted so far in the module: %d" % (
        name, iters, ec.S, worst["sed"], worst["morph"], worst["mse"], len(EXEMPT)))
    for s in range(ec.S):                       # the device's trackers ended on the limits too (with the centres bit-exact)
        assert all(ec.on_limit(c, p, q) for p, q in zip(ec.scene(c, s)[2], g["cen"][s])), (name, s, g["cen"][s])


@pytest.mark.parametrize("name", ["04_exact_persistent", "11_wave", "13_box_68"])
def test_a_centre_the_reference_refuses(env, name):
    """a 3-scene batch whose middle scene has a catalogue pixel at (1, 10)"""
    scarlet, _ = env
    L = scarlet._lib
    c = ec.CASES[name]
    iters = c.iters or ec.lf.ITERS
    images, centers = ec.scenes(c)
    bad_images, bad_centers = ec.refused_scene(c)
    assert tuple(bad_centers[-1]) == ec.REFUSED

    def run(im, cen):
        b = ec.make_batch(scarlet, c, im, cen)
        assert b.fit(iters, e_rel=0, check_every=0) == iters
        return ec.state(b)

    with ec.options(scarlet, c):
        three = run(np.stack([images[0], bad_images, images[1]]), np.stack([centers[0], bad_centers, centers[1]]))
        two = run(images, centers)
    for key in two:
        assert np.array_equal(three[key][[0, 2]], two[key], equal_nan=True), "%s: %s of the neighbours differs" % (name, key)
    assert not two["status"].any() and (two["it"] == iters).all()
    assert three["status"][1] & L.STATUS_CENTER_AT_EDGE, three["status"]
    assert tuple(three["centers"][1, -1]) == ec.REFUSED, three["centers"][1]
    assert np.isfinite(three["sed"][1]).all() and np.isfinite(three["morph"][1]).all()
