"""The radial sweep's level loop (wave_ops.h wave_monotonic) at the smallest shapes at which it can go wrong: where it
stops, where it ends by its bound, where it hands over at level 46, and its double-precision instance in the
initialisation.  The loop skips the pixel-less level 1, runs level pairs with one exit at its foot (a sweep that ends on
an even level passes the odd one without a store) and tests its bound once per pair; none of that may change a bit of
any result.

Every case is compared
  * with the CPU oracle (oracle/pgm.py), started from the device's own initial state: status 0, iteration counts, centres
    and flags exact, sed / morph / loss history within parity_common.TOL = 1e-5 (max-norm relative: the tolerance of
    every fit test against the oracle; the fit tests among the launch forms, tests/test_gpu_fit2x_steps.py, ask for
    bit equality, and get it here through the fixture).  No scene may use parity_common's threshold exemption;
  * bit for bit with tests/golden/sweep_levels_parent.npz, recorded on the GPU with the library of the commit BEFORE the
    loop was rewritten (`SCARLET_LIB_PATH=<that library> python tests/test_gpu_sweep_levels.py --record <file>`):
    initial and final morphologies and SEDs, loss history, iteration counts, flags, status, centres; float32 as stored.

Where a component's sweep stops is read off the oracle's trace: the sweep's output (the plane prox_plus is about to
see) has its last positive value on level Lp = max(2 max(|dy|, |dx|) + min(|dy|, |dx|)), and the loop leaves at the third
level without one, Lp + 3, unless the frame ends first (Lall).  `test_the_scenes_stop_where_intended` asserts, on the
CPU alone, what each case is there for:
  exact   5 x 64 x 64, K = 4, 3 iterations, k_fit2x (and k_iterate2<4,5,64> once per iteration, SCARLET_NO_PERSIST=1 in
          a child process): stops on an odd level above 3, on an even level, and on level 3 -- scene 0's second entry is
          a catalogue pixel without flux of its own (noise that passes the detection cut), 13 px from the scene's
          brightest source: its stepped plane is non-positive everywhere but the peak in every iteration;
  g16     5 x 16 x 16 (the generic fused instance), a broad source at (8, 8): Lall = 24, the loop ends by its bound on an
          even level; scene 1 has the broad source on the corner (2, 2), the lowest row and column max_pixel accepts:
          wedges without a valid pixel, walkers whose diagonal neighbours do not exist (Lall = 39);
  g16v1   the same scenes through the four-wave kernel k_iterate<4, 6> (option FUSED_V1), which keeps the sweep's level-by-level
          loop (wave_monotonic<float, false>): both shapes of the loop on the same scenes;
  g15     5 x 16 x 15 (no fused launch: the wave-level constraint kernel), broad source at (8, 7): Lall = 23, odd;
  smooth  one source, images strictly positive and smooth (no noise): no level is quiet, the loop never leaves early;
  big     5 x 128 x 128, K = 8, 2 iterations, one bright extended source: positive beyond level 46, so the compact loop
          hands over with its count of quiet levels (boxupdate.h / engine.h continue from level 47).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import box_update_cases as bc
import edge_cases as ec
import launch_form_cases as lf
import parity_common as pc

TOL = pc.TOL
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sweep_levels_parent.npz")
BG, NOISE = 0.1, 0.1
KEYS = ("sed0", "morph0", "cen0", "sed", "morph", "mse", "it", "flags", "status", "cen")

# (K, B, H, W), iterations
CASES = {
    "exact": (lf._c("sweep_exact", 4, 5, 64, 64), 3),
    "g16": (lf._c("sweep_g16", 2, 5, 16, 16), 3),
    "g16v1": (lf._c("sweep_g16v1", 2, 5, 16, 16, opts=["FUSED_V1"]), 3),
    "g15": (lf._c("sweep_g15", 2, 5, 16, 15), 3),
    "smooth": (lf._c("sweep_smooth", 1, 5, 16, 16), 3),
    "big": (lf._c("sweep_big", 8, 5, 128, 128), 2),
}
INIT_CASES = ("exact", "g16")

# per scene: (cy, cx, kind, amplitude, major sigma, axis ratio, angle); kind "none": a catalogue pixel only
G, BROAD, NONE = "gauss", "broad", "none"
SOURCES = {
    "exact": [
        [(20, 22, G, 45.0, 3.2, 0.8, 0.4), (30, 14, NONE, 0, 0, 0, 0), (44, 40, G, 30.0, 2.2, 0.6, 1.3), (32, 52, G, 22.0, 1.6, 1.0, 0.0)],
        [(14, 40, G, 35.0, 2.8, 0.7, 2.0), (40, 18, G, 40.0, 3.5, 0.9, 0.9), (48, 48, G, 25.0, 1.8, 0.8, 2.6), (26, 28, G, 28.0, 2.4, 0.5, 0.2)],
    ],
    "g16": [
        [(8, 8, BROAD, 40.0, 0, 0, 0), (2, 2, G, 30.0, 1.5, 1.0, 0.0)],
        [(2, 2, BROAD, 40.0, 0, 0, 0), (10, 9, G, 30.0, 1.5, 0.8, 1.0)],
    ],
    "g16v1": None,                                       # (g16's scenes)
    "g15": [
        [(8, 7, BROAD, 40.0, 0, 0, 0), (2, 2, G, 30.0, 1.5, 1.0, 0.0)],
        [(8, 7, BROAD, 40.0, 0, 0, 0), (12, 11, G, 30.0, 1.6, 0.7, 2.2)],
    ],
    "smooth": [
        [(8, 8, BROAD, 40.0, 0, 0, 0)],
        [(7, 8, BROAD, 25.0, 0, 0, 0)],
    ],
    "big": [
        [(64, 64, G, 60.0, 14.0, 0.8, 0.5), (20, 24, G, 30.0, 2.5, 0.7, 1.0), (30, 100, G, 35.0, 3.0, 0.9, 2.0),
         (100, 28, G, 25.0, 2.0, 0.6, 0.3), (104, 100, G, 40.0, 3.5, 0.8, 1.7), (64, 16, G, 20.0, 1.8, 1.0, 0.0),
         (16, 64, G, 28.0, 2.2, 0.7, 2.4), (112, 64, G, 32.0, 2.8, 0.5, 0.8)],
    ],
}


def scenes(name):
    """images (S, B, H, W) float32 and catalogue pixels (S, K, 2) int32 of a case; seeded by the case and the scene"""
    if name == "g16v1":
        return scenes("g16")
    c = CASES[name][0]
    yy, xx = np.mgrid[:c.H, :c.W].astype(np.float64)
    images, centers = [], []
    for s, sources in enumerate(SOURCES[name]):
        rng = np.random.Generator(np.random.PCG64([sorted(CASES).index(name), s, 4711]))
        model = np.zeros((c.B, c.H, c.W))
        for cy, cx, kind, amp, smaj, q, th in sources:
            colour = rng.uniform(0.3, 1.0, size=c.B)
            dy, dx = yy - cy, xx - cx
            if kind == BROAD:
                morph = np.exp(-np.hypot(dy, dx) / (max(c.H, c.W) / 2.0))
            elif kind == G:
                u, v = np.cos(th) * dx + np.sin(th) * dy, -np.sin(th) * dx + np.cos(th) * dy
                morph = np.exp(-0.5 * ((u / smaj) ** 2 + (v / (smaj * q)) ** 2))
            else:
                continue
            model += (amp * colour)[:, None, None] * morph
        if name == "smooth":
            model += 1.0                                     # strictly positive, and no noise
        else:
            model += rng.normal(0.0, NOISE, size=model.shape)
        images.append(model.astype(np.float32))
        centers.append(np.array([(src[0], src[1]) for src in sources], np.int32))
    return np.stack(images), np.stack(centers)


def lall(c, cen):
    return int(bc.level_map(c.H, c.W, int(cen[0]), int(cen[1])).max())


def stops(c, fit):
    """per iteration and component: (the level on which the sweep leaves its loop, or None if it runs to Lall; Lp; Lall)
    from an oracle fit traced by edge_cases.fit_from"""
    out = []
    for t, (_, pre_plus) in enumerate(fit["pre"]):
        row = []
        for k in range(c.K):
            cen = fit["centers"][t][k]
            pos = pre_plus[k] > 0
            Lp = int(bc.level_map(c.H, c.W, int(cen[0]), int(cen[1]))[pos].max()) if pos.any() else 0
            La = lall(c, cen)
            row.append((Lp + 3 if Lp + 3 <= La else None, Lp, La))
        out.append(row)
    return out


def oracle_start(c, images, pixels, dt=np.float32):
    """the oracle's own constructors for one scene: sed, morph, centres, shifts (edge_cases.oracle_start's form)"""
    from oracle import pgm
    bg = np.ones(c.B) * BG
    out = []
    for k in range(c.K):
        px = (int(pixels[k][0]), int(pixels[k][1]))
        sed, morph = pgm.init_extended_source(px, images.astype(dt), bg, monotonic=True)
        src = pgm.Source(sed, morph, px, dt, centroid_weight=pgm.default_centroid_weight())
        pgm.source_update(src, 0)
        out.append((src.sed, src.morph, src.center, src.shift))
    shifts = np.array([(np.nan, np.nan) if o[3] is None else o[3] for o in out], np.float64)
    return np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out]), shifts


def intended(name, all_stops):
    """what the case is there for, asserted on the stops of all its scenes: [scene][iteration][component]"""
    flat = [x for sc in all_stops for row in sc for x in row]
    levels = [x[0] for x in flat]
    if name == "exact":
        assert all(v is not None for v in levels), levels
        assert 3 in [x[0] for row in all_stops[0] for x in row[1:2]], all_stops[0]      # the entry without flux
        assert any(v > 3 and v % 2 == 1 for v in levels) and any(v % 2 == 0 for v in levels), levels
    elif name in ("g16", "g16v1", "g15"):
        want = {"g16": [24, 39], "g16v1": [24, 39], "g15": [23, 23]}[name]
        for s, sc in enumerate(all_stops):
            for row in sc:
                assert row[0] == (None, want[s], want[s]), (name, s, row)      # the broad source: by the bound
    elif name == "smooth":
        for sc in all_stops:
            for row in sc:
                assert row[0][0] is None and row[0][1] == row[0][2], row
    elif name == "big":
        for row in all_stops[0]:
            assert row[0][1] >= 47, row                    # positive beyond the compact levels
            assert any(x[0] is not None and x[0] <= 46 for x in row[1:]), row


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_scenes_stop_where_intended(name):
    """CPU only: the oracle from its own constructors' state"""
    from oracle import build as obuild
    obuild.build()
    c, iters = CASES[name]
    images, pixels = scenes(name)
    got = []
    for s in range(len(images)):
        fit = ec.fit_from(ec.spec(c, images[s], *oracle_start(c, images[s], pixels[s])), iters, trace=True)
        assert fit["it"] == iters
        got.append(stops(c, fit))
    print(name, got)
    intended(name, got)


# ---------------------------------------------------------------------------------------------------- the device
def device_run(scarlet, name):
    """the case on the device: the initial state and the state after the case's iterations (one fit call)"""
    import torch
    c, iters = CASES[name]
    images, pixels = scenes(name)
    with ec.options(scarlet, c):
        return _device_run(scarlet, c, iters, images, pixels)


def _device_run(scarlet, c, iters, images, pixels):
    import ctypes
    import torch
    L = scarlet._lib
    b = ec.make_batch(scarlet, c, images, pixels, mse_capacity=iters + 1)
    torch.cuda.synchronize()
    out = dict(sed0=b.sed_current.cpu().numpy().copy(), morph0=b.morph_current.cpu().numpy().copy(),
               cen0=b.centers.cpu().numpy().copy(), sh0=b.shifts.cpu().numpy().copy(), status0=b.status.cpu().numpy().copy())
    L.check(L.lib.scarlet_profile_begin(iters + 1))
    try:
        assert b.fit(iters, e_rel=0, check_every=0) == iters
    finally:
        ms, its, launches = (ctypes.c_double * 8)(), (ctypes.c_int64 * 8)(), (ctypes.c_int64 * 8)()
        L.check(L.lib.scarlet_profile_end_ex(ms, its, launches))
    torch.cuda.synchronize()
    out.update(fused_launches=np.array([its[4], launches[4]], np.int64),      # class 4: the one-launch iteration
               sed=b.sed_current.cpu().numpy(), morph=b.morph_current.cpu().numpy(), cen=b.centers.cpu().numpy(),
               it=b.it.cpu().numpy(), flags=b.flags.cpu().numpy(), mse=b.mse_buf.cpu().numpy()[:, :iters],
               status=b.status.cpu().numpy())
    return out


@pytest.fixture(scope="module")
def env():
    import scarlet_amd
    scarlet_amd._lib.require_gpu()
    from oracle import build as obuild
    obuild.build()
    runs = {}

    def run(name):
        if name not in runs:
            runs[name] = device_run(scarlet_amd, name)
        return runs[name]
    return scarlet_amd, run, np.load(GOLDEN)


def assert_recorded(name, got, golden, keys=KEYS):
    for key in keys:
        want = golden["%s/%s" % (name, key)]
        assert got[key].dtype == want.dtype, (name, key, got[key].dtype, want.dtype)
        assert np.array_equal(got[key], want, equal_nan=True), "%s: %s differs from the parent's" % (name, key)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_fit_against_the_oracle_and_the_parent(env, name):
    _, run, golden = env
    c, iters = CASES[name]
    images, _ = scenes(name)
    g = run(name)
    assert_recorded(name, g, golden)
    if name == "exact":                                    # the persistent kernel: one launch for the three iterations
        assert g["fused_launches"].tolist() == [iters, 1], g["fused_launches"]
    ref, got = [], []
    for s in range(len(images)):
        fit = ec.fit_from(ec.spec(c, images[s], g["sed0"][s], g["morph0"][s], g["cen0"][s], g["sh0"][s]), iters, trace=True)
        ref.append((fit["sed"], fit["morph"], fit["mse"], fit["cen"], fit["it"], fit["flags"].tolist()))
        got.append(stops(c, fit))
    print(name, got)
    intended(name, got)                                    # (from the device's initial state as well)
    worst = pc.compare_fixed_iterations(g, ref, iters, lambda i: (False, "no exemption in this module"), 0,
                                        "sweep levels, " + name, flags=True)
    print("sweep levels %-6s worst sed %.3e morph %.3e loss %.3e" % (name, worst["sed"], worst["morph"], worst["mse"]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", INIT_CASES)
def test_init_extended_against_the_oracle_and_the_parent(env, name):
    """the double-precision instance with a `floor` (initsrc.h): the detection cut zeroes what the sweep left at or
    below it.  As tests/test_gpu_init_sources.py: centres exact, sed / morph within TOL of the oracle's constructors."""
    _, run, golden = env
    c, _ = CASES[name]
    images, pixels = scenes(name)
    g = run(name)
    assert not g["status0"].any()
    assert_recorded(name, g, golden, ("sed0", "morph0", "cen0"))
    for s in range(len(images)):
        sed, morph, cen, _ = oracle_start(c, images[s], pixels[s])
        np.testing.assert_array_equal(g["cen0"][s], cen)
        e = (pc.rel_err(g["sed0"][s], sed), pc.rel_err(g["morph0"][s], morph))
        print("sweep levels %-6s scene %d initial state: sed %.3e morph %.3e" % (name, s, e[0], e[1]))
        assert max(e) <= TOL, (name, s, e)


@pytest.mark.gpu
def test_exact_shape_one_launch_per_iteration(env, tmp_path):
    """SCARLET_NO_PERSIST=1 (read once, when the library starts: hence a process of its own): k_iterate2<4,5,64> once per
    iteration instead of k_fit2x, the same bits"""
    golden = env[2]
    out = str(tmp_path / "exact.npz")
    child = {k: v for k, v in os.environ.items() if not k.startswith("SCARLET_") or k == "SCARLET_LIB_PATH"}
    child["SCARLET_NO_PERSIST"] = "1"                      # (the same library, no other switch)
    subprocess.run([sys.executable, os.path.abspath(__file__), "--dump", "exact", out], env=child, check=True, timeout=120)
    got = np.load(out)
    iters = CASES["exact"][1]
    assert got["exact/fused_launches"].tolist() == [iters, iters], got["exact/fused_launches"]      # not k_fit2x
    assert_recorded("exact", {k: got["exact/" + k] for k in KEYS}, golden)


def record(path, names):
    import scarlet_amd
    scarlet_amd._lib.require_gpu()
    arrays = {}
    for name in names:
        g = device_run(scarlet_amd, name)
        assert not g["status"].any() and not g["status0"].any(), name
        arrays.update(("%s/%s" % (name, k), g[k]) for k in KEYS + ("fused_launches",))
    np.savez_compressed(path, **arrays)
    print("wrote %s: %d arrays, %d bytes" % (path, len(arrays), os.path.getsize(path)))


if __name__ == "__main__":
    if sys.argv[1] == "--record":
        record(sys.argv[2], sorted(CASES))
    elif sys.argv[1] == "--dump":
        record(sys.argv[3], [sys.argv[2]])
    else:
        sys.exit("usage: test_gpu_sweep_levels.py --record FILE | --dump CASE FILE")
