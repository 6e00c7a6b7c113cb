"""CPU: the PSF cases of tests/test_gpu_psf_plans.py and the plans of the LDS-resident convolution they get.

fft_make_plan (scarlet_hip.hip) picks, per frame and kernel shape, a column length Fy = R1y R2y and a half-row length
M = R1x R2x, each radix from the menu {4, 5, 6, 7, 8, 9, 10, 12, 14, 15, 16}.  k_psf_conv dispatches each of the four
positions to straight-line codelet code of its own (R1y: cols_A_untangle / cols_Ainv_tangle, R2y: cols_B_mul_Binv,
R1x: rows_Ainv_resid_A / rows_Ainv_store, R2x: the row fft_pass): 44 (position, radix) instances.  The GPU tests run
every case of CASES against float64 references; this module pins what those cases reach:
  - each case gets exactly the plan recorded next to it (a change of fft_make_plan names the cases whose coverage
    moved),
  - together they reach all 44 (position, radix) slots,
  - and the other plan-dependent branches: odd and even M (the pair (M/2, M/2) of the real-row untangling), the image
    staged by LDS-DMA or not (H W % 4 != 0 among the latter), R1 = R2, even-sized and non-square kernels, a kernel
    larger than the frame, 3-row frames, a plan within 4 KB of the LDS bound, the exact-shape instance, and the
    batched hipFFT chain (scarlet_debug_psf_plan returns -1: W odd, or a plane too large for LDS).
scarlet_debug_psf_plan reads the switches PSF_HIPFFT and NO_EXACT, so the plans are read in a child process with both
off.  It does not touch the device.
"""
import collections
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MENU = (4, 5, 6, 7, 8, 9, 10, 12, 14, 15, 16)
POSITIONS = ("R1y", "R2y", "R1x", "R2x")
# fft_make_plan admits a plan whose plane + tables take at most LDS_LIMIT - 4096 bytes (scarlet_hip.hip)
LDS_PLAN_BOUND = 160 * 1024 - 1024 - 4096

# weights: "one" = none (scalar 1), "scalar" = a scalar != 1, "pixel" = per-pixel weights with ~10 % zeros;
# per_scene: the difference kernel is (S, B, Py, Px) instead of (B, Py, Px)
Case = collections.namedtuple("Case", "H W Py Px B K weights per_scene plan")
Plan = collections.namedtuple("Plan", "Fy R1y R2y M R1x R2x dma_image exact")


def _c(H, W, Py, Px, B, K, weights, per_scene, plan):
    return Case(H, W, Py, Px, B, K, weights, per_scene, None if plan is None else Plan(*plan))


CASES = [
    #  H    W   Py   Px  B   K  weights  per_scene  (Fy R1y R2y   M R1x R2x dma exact)
    _c(3, 4, 41, 41, 2, 2, "one", False, (42, 6, 7, 24, 4, 6, 1, 0)),          # kernel larger than a 3-row frame
    _c(3, 38, 25, 25, 3, 3, "scalar", False, (25, 5, 5, 25, 5, 5, 0, 0)),      # R1 = R2 both ways, M odd, H W % 4 = 2
    _c(3, 72, 21, 21, 4, 2, "pixel", False, (24, 4, 6, 42, 6, 7, 1, 0)),
    _c(35, 102, 41, 41, 5, 3, "pixel", True, (56, 7, 8, 63, 7, 9, 0, 0)),
    _c(51, 108, 41, 41, 6, 4, "scalar", False, (72, 8, 9, 64, 8, 8, 1, 0)),
    _c(65, 178, 41, 41, 2, 3, "one", False, (90, 9, 10, 100, 10, 10, 0, 0)),
    _c(101, 4, 25, 25, 8, 3, "pixel", False, (120, 10, 12, 16, 4, 4, 1, 0)),
    _c(141, 94, 41, 41, 3, 10, "one", False, (168, 12, 14, 60, 12, 5, 0, 0)),   # K = 10: bigk.h
    _c(177, 126, 41, 41, 2, 2, "scalar", False, (210, 14, 15, 75, 5, 15, 0, 0)),
    _c(3, 144, 15, 15, 5, 3, "pixel", True, (16, 4, 4, 80, 16, 5, 1, 0)),
    _c(107, 142, 41, 41, 4, 40, "pixel", False, (128, 8, 16, 81, 9, 9, 0, 0)),  # K = 40: hugek.h
    _c(3, 162, 41, 41, 3, 3, "one", False, (42, 6, 7, 96, 8, 12, 0, 0)),
    _c(3, 174, 41, 41, 2, 3, "scalar", False, (42, 6, 7, 98, 14, 7, 0, 0)),
    _c(3, 92, 121, 121, 2, 2, "pixel", False, (126, 9, 14, 80, 16, 5, 1, 0)),
    _c(3, 114, 161, 161, 2, 3, "one", False, (168, 12, 14, 98, 14, 7, 0, 0)),
    _c(3, 410, 81, 81, 2, 3, "scalar", False, (81, 9, 9, 225, 15, 15, 0, 0)),
    _c(3, 194, 121, 121, 2, 2, "pixel", False, (126, 9, 14, 128, 8, 16, 0, 0)),
    _c(3, 212, 121, 121, 2, 3, "one", True, (126, 9, 14, 140, 10, 14, 1, 0)),
    _c(100, 4, 121, 121, 3, 3, "scalar", False, (160, 10, 16, 63, 7, 9, 1, 0)),
    _c(200, 4, 61, 61, 2, 3, "pixel", False, (240, 15, 16, 32, 4, 8, 1, 0)),
    _c(230, 4, 41, 41, 2, 2, "one", False, (256, 16, 16, 24, 4, 6, 1, 0)),
    _c(58, 48, 43, 43, 5, 2, "pixel", False, (80, 8, 10, 35, 5, 7, 1, 0)),     # BASELINE config 1
    _c(128, 128, 41, 41, 5, 8, "one", False, (150, 10, 15, 75, 5, 15, 1, 1)),  # config 3: k_psf_conv_x128
    _c(64, 64, 41, 41, 5, 40, "pixel", True, (84, 7, 12, 42, 6, 7, 1, 0)),
    _c(64, 64, 11, 11, 5, 10, "scalar", False, (70, 7, 10, 35, 5, 7, 1, 0)),
    _c(32, 40, 9, 9, 3, 3, "pixel", False, (36, 6, 6, 24, 4, 6, 1, 0)),
    _c(64, 64, 8, 6, 4, 3, "scalar", True, (70, 7, 10, 35, 5, 7, 1, 0)),      # even-sized, non-square kernels
    _c(45, 62, 8, 6, 3, 4, "pixel", False, (49, 7, 7, 35, 5, 7, 0, 0)),
    _c(33, 20, 6, 9, 3, 10, "pixel", False, (36, 6, 6, 16, 4, 4, 1, 0)),
    _c(172, 172, 41, 41, 2, 3, "pixel", False, (192, 12, 16, 96, 8, 12, 0, 0)),  # within 4 KB of the LDS bound
    _c(32, 31, 9, 9, 3, 3, "pixel", False, None),                              # W odd: hipFFT
    _c(174, 174, 41, 41, 2, 2, "scalar", False, None),                         # plane beyond LDS: hipFFT
    _c(31, 45, 8, 6, 2, 3, "one", True, None),                                 # W odd, even-sized kernel: hipFFT
]


def case_id(c):
    return "%dx%d_k%dx%d_B%d_K%d_%s%s" % (c.H, c.W, c.Py, c.Px, c.B, c.K, c.weights, "_perscene" if c.per_scene else "")


def read_plans(cases):
    """scarlet_debug_psf_plan of every case under this process's switches: a list of (return code, 16 ints)"""
    sys.path.insert(0, ROOT)
    from scarlet_amd import _lib
    out16 = (ctypes.c_int32 * 16)()
    res = []
    for c in cases:
        b = _lib.ScarletBatch()
        b.S, b.K, b.B, b.H, b.W = 2, c.K, c.B, c.H, c.W    # (the GPU tests' two scenes)
        b.diff_kernel = 1                             # (only tested against NULL)
        b.psf_h, b.psf_w, b.diff_kernel_per_scene = c.Py, c.Px, int(c.per_scene)
        for j in range(16):
            out16[j] = 0
        rc = _lib.lib.scarlet_debug_psf_plan(ctypes.byref(b), out16)
        res.append((rc, list(out16)))
    return res


def plan_of(rc, v):
    """the recorded form of a scarlet_debug_psf_plan result (16 ints: H W Fy Fx M RS R1y R2y R1x R2x oky okx dma exact
    lds 0); None for the hipFFT chain"""
    return None if rc != 0 else Plan(v[2], v[6], v[7], v[4], v[8], v[9], v[12], v[13])


_PLANS = []


def plans():
    """the plans of CASES with PSF_HIPFFT and NO_EXACT off, read once in a child process"""
    if not _PLANS:
        env = dict(os.environ, SCARLET_PSF_HIPFFT="0", SCARLET_NO_EXACT="0")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--plans"], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        _PLANS.extend(json.loads(r.stdout.decode().strip().splitlines()[-1]))
        assert len(_PLANS) == len(CASES)
    return _PLANS


def test_every_case_gets_its_recorded_plan():
    moved = []
    for c, (rc, v) in zip(CASES, plans()):
        got = plan_of(rc, v)
        if got != c.plan:
            moved.append("%s: %s, recorded %s" % (case_id(c), got, c.plan))
    assert not moved, "the plan of %d case(s) moved:\n  %s" % (len(moved), "\n  ".join(moved))


def test_cases_reach_every_radix_at_every_position():
    seen = {p: set() for p in POSITIONS}
    for rc, v in plans():
        if rc == 0:
            for p, r in zip(POSITIONS, v[6:10]):
                seen[p].add(r)
    missing = ["%s = %d" % (p, r) for p in POSITIONS for r in MENU if r not in seen[p]]
    assert not missing, "no case runs %s" % ", ".join(missing)
    assert all(seen[p] <= set(MENU) for p in POSITIONS), seen
    print("%d (position, radix) slots covered by %d cases" % (sum(len(s) for s in seen.values()), len(CASES)))


def test_cases_reach_the_other_plan_dependent_branches():
    lds = [(c, v) for c, (rc, v) in zip(CASES, plans()) if rc == 0]
    fft = [c for c, (rc, v) in zip(CASES, plans()) if rc != 0]

    def some(what, pred):
        assert any(pred(c, v) for c, v in lds), "no LDS-path case with " + what

    some("M odd", lambda c, v: v[4] % 2 == 1)
    some("M even", lambda c, v: v[4] % 2 == 0)
    some("the image staged by LDS-DMA", lambda c, v: v[12] == 1)
    some("the image read from global memory, H W % 4 != 0", lambda c, v: v[12] == 0 and c.H * c.W % 4 != 0)
    some("the image read from global memory, H W % 4 == 0", lambda c, v: v[12] == 0 and c.H * c.W % 4 == 0)
    some("R1y = R2y", lambda c, v: v[6] == v[7])
    some("R1x = R2x", lambda c, v: v[8] == v[9])
    some("an even kernel height", lambda c, v: c.Py % 2 == 0)
    some("an even kernel width", lambda c, v: c.Px % 2 == 0)
    some("a non-square kernel", lambda c, v: c.Py != c.Px)
    some("a kernel larger than the frame", lambda c, v: c.Py > c.H and c.Px > c.W)
    some("a frame of 3 rows", lambda c, v: c.H == 3)
    some("a plane within 4 KB of the LDS bound", lambda c, v: LDS_PLAN_BOUND - 4096 < v[14] <= LDS_PLAN_BOUND)
    some("the exact-shape instance", lambda c, v: v[13] == 1 and (c.H, c.W, c.Py, c.Px) == (128, 128, 41, 41))
    some("K > 8 (bigk.h)", lambda c, v: 8 < c.K <= 32)
    some("K > 32 (hugek.h)", lambda c, v: c.K > 32)
    some("per-scene kernels", lambda c, v: c.per_scene)
    for w in ("one", "scalar", "pixel"):
        some("weights " + w, lambda c, v, w=w: c.weights == w)
    assert any(c.W % 2 for c in fft), "no hipFFT case with W odd"
    assert any(c.W % 2 == 0 for c in fft), "no hipFFT case whose plane exceeds LDS"
    assert max(c.B for c in CASES) == 8


if __name__ == "__main__":
    if sys.argv[1] == "--plans":
        print(json.dumps(read_plans(CASES)))
