"""The pair kernel's k-space symmetry GEMMs (wave_ops.h pair_ks_gemm1_impl / pair_ks_gemm2_trim) at every window size
that changes which MFMA steps they issue.  GEMM 1 does not issue the k-steps of its last group of 16 columns that lie
wholly beyond the window (from step ceil((w - k0) / 4) on), GEMM 2 not the steps of its last row tile whose four rows of T
lie beyond it (from step h - 16 (NTR - 1) on).  None of that may change a bit of any result.

Scenes of 5 x 64 x 64, K = 4, four iterations from the device's initial state (no centroid iteration among them: the
windows follow from the catalogue pixels, which the scenes keep on their peaks).  The constructors leave symmetric
morphologies, whose centroid shift is zero -- the k-space operator is then the identity and has no rank-1 term -- so
the test gives every component a shift of its own, seeded, 0.05 <= |dy|, |dx| <= 0.45, before the first iteration.
A component at (cy, cx) has the window h = 2 min(cy, 63 - cy) + 1, w = 2 min(cx, 63 - cx) + 1;
`test_the_windows_are_the_intended_ones` asserts on the CPU that the four scenes cover h and w in {17, 19, 31, 33, 35, 47,
49, 51, 61, 63}: the residues 1, 3, 15 (mod 16) of h (three, one and no step skipped in GEMM 2) and every count of live
steps 1 .. 4 in GEMM 1's last group, for two, three and four column tiles, which every pair splits between its two waves
(tiles {0, 2} and {1, 3}: one or two per wave, both instances of either GEMM).  h = 17 has the transform length
F_y = 45, odd: no rank-1 term, beside windows with it.  Scene 2 holds a centred component (32, 32): no GEMM at all.
Scene 3's third component starts without a shift (dy = NaN): the flip symmetry.  Its second component, at (5, 58), has an
11 x 11 window: one tile either way (GEMM 1's only group is its last, GEMM 2 has nothing but its last row tile).

Every case is compared
  * with the CPU oracle (oracle/pgm.py) from the device's initial state: status 0, iteration counts, centres and flags
    exact, sed / morph / loss history within parity_common.TOL = 1e-5, no exemption;
  * bit for bit with tests/golden/symmetry_trim_parent.npz, recorded on the GPU with the library of the commit BEFORE the
    GEMMs were trimmed (`SCARLET_LIB_PATH=<that library> python tests/test_gpu_symmetry_trim.py --record <file>`), which
    passes this module as well.
The case `exact` runs k_fit2x; child processes run the same scenes through k_iterate2<4,5,64> (SCARLET_NO_PERSIST=1) and
the generic instance k_iterate2<4,5,0> (SCARLET_NO_EXACT=1) and must give the same golden.  `g16v1` is one 16 x 16 case
through k_iterate<4, 6> (FUSED_V1), whose GEMMs keep every step.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import edge_cases as ec
import launch_form_cases as lf
import parity_common as pc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "symmetry_trim_parent.npz")
BG, NOISE, ITERS = 0.1, 0.1, 4
KEYS = ("sed0", "morph0", "cen0", "sed", "morph", "mse", "it", "flags", "status", "cen")
SIZES = (17, 19, 31, 33, 35, 47, 49, 51, 61, 63)

CASES = {
    "exact": lf._c("trim_exact", 4, 5, 64, 64),
    "g16v1": lf._c("trim_g16v1", 2, 5, 16, 16, opts=["FUSED_V1"]),
}
CHILDREN = {"no_persist": "SCARLET_NO_PERSIST", "no_exact": "SCARLET_NO_EXACT"}

# per scene: (cy, cx, amplitude, major sigma, axis ratio, angle)
SOURCES = {
    "exact": [
        [(8, 55, 40.0, 2.0, 0.8, 0.4), (54, 9, 35.0, 2.2, 0.7, 1.3), (15, 48, 30.0, 1.8, 0.9, 2.0), (47, 30, 45.0, 2.6, 0.6, 0.2)],
        [(17, 17, 40.0, 2.4, 0.8, 0.9), (40, 23, 35.0, 2.8, 0.7, 2.6), (24, 39, 45.0, 2.2, 0.9, 0.0), (38, 46, 30.0, 2.0, 0.6, 1.7)],
        [(30, 16, 40.0, 2.6, 0.7, 0.5), (32, 32, 45.0, 2.2, 0.8, 1.1), (12, 38, 30.0, 2.0, 0.9, 2.2), (47, 31, 35.0, 2.4, 0.6, 0.3)],
        [(31, 31, 45.0, 3.0, 0.8, 0.7), (5, 58, 30.0, 1.8, 0.9, 1.9), (52, 50, 35.0, 2.2, 0.7, 2.8), (14, 50, 40.0, 2.0, 0.6, 1.0)],
    ],
    "g16v1": [
        [(6, 9, 40.0, 1.6, 0.8, 0.4), (11, 4, 30.0, 1.4, 1.0, 0.0)],
        [(8, 8, 40.0, 1.6, 0.8, 1.2), (4, 11, 30.0, 1.5, 0.7, 2.0)],
    ],
}
NO_SHIFT = {"exact": [(3, 2)], "g16v1": []}              # (scene, component) started with dy = dx = NaN
CENTRED = (2, 1)


def scenes(name):
    """images (S, B, H, W) float32 and catalogue pixels (S, K, 2) int32 of a case; seeded by the case and the scene"""
    c = CASES[name]
    yy, xx = np.mgrid[:c.H, :c.W].astype(np.float64)
    images, centers = [], []
    for s, sources in enumerate(SOURCES[name]):
        rng = np.random.Generator(np.random.PCG64([sorted(CASES).index(name), s, 1729]))
        model = np.zeros((c.B, c.H, c.W))
        for cy, cx, amp, smaj, q, th in sources:
            colour = rng.uniform(0.3, 1.0, size=c.B)
            dy, dx = yy - cy, xx - cx
            u, v = np.cos(th) * dx + np.sin(th) * dy, -np.sin(th) * dx + np.cos(th) * dy
            model += (amp * colour)[:, None, None] * np.exp(-0.5 * ((u / smaj) ** 2 + (v / (smaj * q)) ** 2))
        model += rng.normal(0.0, NOISE, size=model.shape)
        images.append(model.astype(np.float32))
        centers.append(np.array([(src[0], src[1]) for src in sources], np.int32))
    return np.stack(images), np.stack(centers)


def window(c, cen):
    ry, rx = min(int(cen[0]), c.H - 1 - int(cen[0])), min(int(cen[1]), c.W - 1 - int(cen[1]))
    return 2 * ry + 1, 2 * rx + 1


def oracle_start(c, images, pixels, dt=np.float32):
    """the oracle's own constructors for one scene: sed, morph, centres, shifts"""
    from oracle import pgm
    bg = np.ones(c.B) * BG
    out = []
    for k in range(c.K):
        px = (int(pixels[k][0]), int(pixels[k][1]))
        sed, morph = pgm.init_extended_source(px, images.astype(dt), bg, monotonic=True)
        src = pgm.Source(sed, morph, px, dt, centroid_weight=pgm.default_centroid_weight())
        pgm.source_update(src, 0)
        out.append((src.sed, src.morph, src.center, src.shift))
    return (np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out]),
            np.array([o[3] for o in out], np.float64))


def start_shifts(name, s):
    """the shifts scene s starts with, (K, 2) float64: seeded, away from zero; NaN where the component has none"""
    rng = np.random.Generator(np.random.PCG64([sorted(CASES).index(name), s, 271828]))
    sh = rng.uniform(0.05, 0.45, size=(CASES[name].K, 2)) * rng.choice([-1.0, 1.0], size=(CASES[name].K, 2))
    for sc, k in NO_SHIFT[name]:
        if sc == s:
            sh[k] = np.nan
    return sh


def intended(name, windows, shifts):
    """what the scenes are there for, asserted on the windows [scene][iteration][component] and the initial shifts"""
    from oracle import pgm
    c = CASES[name]
    if name != "exact":
        return
    for sc in windows:
        assert all(row == sc[0] for row in sc), sc                     # the centres do not move
    first = [sc[0] for sc in windows]
    ks = [(s, k, h, w) for s, sc in enumerate(first) for k, (h, w) in enumerate(sc)
          if (s, k) != CENTRED and (s, k) not in NO_SHIFT[name]]
    assert SOURCES[name][CENTRED[0]][CENTRED[1]][:2] == (c.H // 2, c.W // 2)           # centred: no GEMM
    assert set(SIZES) <= set(h for _, _, h, _ in ks), sorted(set(h for _, _, h, _ in ks))
    assert set(SIZES) <= set(w for _, _, _, w in ks), sorted(set(w for _, _, _, w in ks))
    assert set((w + 15) // 16 for _, _, _, w in ks) == {1, 2, 3, 4} and set((h + 15) // 16 for _, _, h, _ in ks) == {1, 2, 3, 4}
    assert (11, 11) in [(h, w) for _, _, h, w in ks]                    # one tile either way: w < 16, NTR = 1
    assert (63, 63) in [(h, w) for _, _, h, w in ks]                    # 4 x 4 tiles
    rank1 = {}
    for s, k, h, w in ks:
        dy = shifts[s][k][0]
        assert np.isfinite(dy) and dy != 0.0, (s, k, dy)
        rank1.setdefault(pgm.next_fast_len(2 * h + 10) % 2 == 0, []).append(h)
    assert 17 in rank1[False] and pgm.next_fast_len(2 * 17 + 10) == 45, rank1
    assert len(set(rank1[True])) >= 5, rank1                           # the term beside it


def oracle_case(name, start):
    """the oracle's fits of a case from `start(s)` -> (sed0, morph0, cen0, sh0); returns the reference tuples and the windows"""
    c = CASES[name]
    images, _ = scenes(name)
    ref, wins, shifts = [], [], []
    for s in range(len(images)):
        sed0, morph0, cen0, sh0 = start(s)
        fit = ec.fit_from(ec.spec(c, images[s], sed0, morph0, cen0, sh0), ITERS, trace=True)
        ref.append((fit["sed"], fit["morph"], fit["mse"], fit["cen"], fit["it"], fit["flags"].tolist()))
        wins.append([[window(c, cen) for cen in row] for row in fit["centers"]])
        shifts.append(sh0)
        assert np.isfinite(fit["sed"]).all() and np.isfinite(fit["morph"]).all() and np.isfinite(fit["mse"]).all(), (name, s)
    return ref, wins, shifts


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_windows_are_the_intended_ones(name):
    """CPU only: the oracle from its own constructors' state runs the scenes to finite results on the intended windows"""
    from oracle import build as obuild
    obuild.build()
    c = CASES[name]
    images, pixels = scenes(name)

    def start(s):
        sed0, morph0, cen0, sh0 = oracle_start(c, images[s], pixels[s])
        np.testing.assert_array_equal(cen0, pixels[s])
        return sed0, morph0, cen0, start_shifts(name, s)
    _, wins, shifts = oracle_case(name, start)
    print(name, [sc[0] for sc in wins])
    intended(name, wins, shifts)


# ---------------------------------------------------------------------------------------------------- the device
def device_run(scarlet, name):
    """the case on the device: the initial state and the state after the case's iterations (one fit call)"""
    import torch
    c = CASES[name]
    images, pixels = scenes(name)
    with ec.options(scarlet, c):
        b = ec.make_batch(scarlet, c, images, pixels, mse_capacity=ITERS + 1)
        sh = np.stack([start_shifts(name, s) for s in range(len(images))])
        b.shifts.copy_(torch.as_tensor(sh, dtype=b.shifts.dtype))
        torch.cuda.synchronize()
        out = dict(sed0=b.sed_current.cpu().numpy().copy(), morph0=b.morph_current.cpu().numpy().copy(),
                   cen0=b.centers.cpu().numpy().copy(), sh0=b.shifts.cpu().numpy().copy(), status0=b.status.cpu().numpy().copy())
        assert b.fit(ITERS, e_rel=0, check_every=0) == ITERS
        torch.cuda.synchronize()
        out.update(sed=b.sed_current.cpu().numpy(), morph=b.morph_current.cpu().numpy(), cen=b.centers.cpu().numpy(),
                   it=b.it.cpu().numpy(), flags=b.flags.cpu().numpy(), mse=b.mse_buf.cpu().numpy()[:, :ITERS],
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
    g = run(name)
    assert not g["status0"].any()
    assert_recorded(name, g, golden)
    ref, wins, shifts = oracle_case(name, lambda s: (g["sed0"][s], g["morph0"][s], g["cen0"][s], g["sh0"][s]))
    intended(name, wins, shifts)                           # (from the device's initial state as well)
    worst = pc.compare_fixed_iterations(g, ref, ITERS, lambda i: (False, "no exemption in this module"), 0,
                                        "symmetry trim, " + name, flags=True)
    print("symmetry trim %-6s worst sed %.3e morph %.3e loss %.3e" % (name, worst["sed"], worst["morph"], worst["mse"]))


@pytest.mark.gpu
@pytest.mark.parametrize("child", sorted(CHILDREN))
def test_the_other_exact_shape_instances(env, tmp_path, child):
    """the switches are read once, when the library starts: hence a process of its own, with the same library"""
    golden = env[2]
    out = str(tmp_path / "exact.npz")
    envs = {k: v for k, v in os.environ.items() if not k.startswith("SCARLET_") or k == "SCARLET_LIB_PATH"}
    envs[CHILDREN[child]] = "1"
    subprocess.run([sys.executable, os.path.abspath(__file__), "--dump", "exact", out], env=envs, check=True, timeout=120)
    got = np.load(out)
    assert_recorded("exact", {k: got["exact/" + k] for k in KEYS}, golden)


def record(path, names):
    import scarlet_amd
    scarlet_amd._lib.require_gpu()
    arrays = {}
    for name in names:
        g = device_run(scarlet_amd, name)
        assert not g["status"].any() and not g["status0"].any(), name
        arrays.update(("%s/%s" % (name, k), g[k]) for k in KEYS)
    np.savez_compressed(path, **arrays)
    print("wrote %s: %d arrays, %d bytes" % (path, len(arrays), os.path.getsize(path)))


if __name__ == "__main__":
    if sys.argv[1] == "--record":
        record(sys.argv[2], sorted(CASES))
    elif sys.argv[1] == "--dump":
        record(sys.argv[3], [sys.argv[2]])
    else:
        sys.exit("usage: test_gpu_symmetry_trim.py --record FILE | --dump CASE FILE")
