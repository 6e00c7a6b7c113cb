"""CPU: the layout of a batch's workspace, to the byte.  For a grid of shapes: scarlet_batch_workspace_bytes,
scarlet_batch_pipelines, the plan of the LDS-resident convolution (scarlet_debug_psf_plan) and the offset of its phase
stamps (scarlet_debug_psf_stamps_offset), under the default switches and under each of the three switches that change
the layout (FORCE_HUGEK, PSF_HIPFFT, STAMPS).  They freeze once read, so every setting is recorded in a process of its
own.  None of these entry points touches the device.

tests/golden/workspace_layout.npz was written by this module (`record_fixture`) with the library as it was before the
layout was computed in one place; it is not to be regenerated:
    SCARLET_LIB_PATH=<that library> python tests/test_workspace_layout.py --write tests/golden/workspace_layout.npz
"""
import ctypes
import itertools
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "workspace_layout.npz")

S_GRID = (1, 7, 1024, 4097)
K_GRID = (1, 4, 5, 8, 9, 30, 32, 33, 64, 256)
B_GRID = (1, 5, 6, 8)
HW_GRID = ((3, 3), (64, 64), (64, 60), (65, 64), (128, 128), (150, 90), (256, 256), (300, 257), (1024, 1024))
# (psf_h, psf_w, diff_kernel_per_scene); 0 x 0: no PSF
PSF_GRID = ((0, 0, 0), (11, 11, 0), (41, 41, 0), (41, 41, 1), (8, 6, 0))
SWITCHES = ("FORCE_HUGEK", "PSF_HIPFFT", "STAMPS")
MODES = ("default",) + SWITCHES          # default: every switch off; otherwise that one switch on


def grid():
    return list(itertools.product(S_GRID, K_GRID, B_GRID, HW_GRID, PSF_GRID))


def record():
    """the layout of every batch of the grid under this process's switches"""
    sys.path.insert(0, ROOT)
    from scarlet_amd import _lib
    g = grid()
    ws = np.zeros(len(g), np.int64)
    pipes = np.zeros(len(g), np.int32)
    plan = np.zeros((len(g), 17), np.int32)          # return code, then the 16 ints
    stamps = np.zeros(len(g), np.int64)
    out16 = (ctypes.c_int32 * 16)()
    for i, (S, K, B, (H, W), (ph, pw, per_scene)) in enumerate(g):
        b = _lib.ScarletBatch()
        b.S, b.K, b.B, b.H, b.W = S, K, B, H, W
        if ph:
            b.diff_kernel = 1                         # (only tested against NULL)
            b.psf_h, b.psf_w, b.diff_kernel_per_scene = ph, pw, per_scene
        p = ctypes.byref(b)
        ws[i] = _lib.lib.scarlet_batch_workspace_bytes(p)
        pipes[i] = _lib.lib.scarlet_batch_pipelines(p)
        for j in range(16):
            out16[j] = 0
        plan[i, 0] = _lib.lib.scarlet_debug_psf_plan(p, out16)
        plan[i, 1:] = list(out16)
        stamps[i] = _lib.lib.scarlet_debug_psf_stamps_offset(p)
    return {"workspace_bytes": ws, "pipelines": pipes, "psf_plan": plan, "stamps_offset": stamps}


def _env(mode):
    env = dict(os.environ)
    for s in SWITCHES:
        env["SCARLET_" + s] = "1" if s == mode else "0"
    return env


def record_all():
    """record() under every mode, each in a child process; arrays named <mode>/<quantity>"""
    with tempfile.TemporaryDirectory() as tmp:
        procs = {m: subprocess.Popen([sys.executable, os.path.abspath(__file__), "--record", os.path.join(tmp, m + ".npz")],
                                     env=_env(m), stdout=subprocess.PIPE, stderr=subprocess.PIPE) for m in MODES}
        out = {}
        for m, p in procs.items():
            _, err = p.communicate(timeout=300)
            assert p.returncode == 0, err.decode()[-2000:]
            with np.load(os.path.join(tmp, m + ".npz")) as z:
                out.update({m + "/" + k: z[k] for k in z.files})
    return out


def record_fixture(path):
    g = np.array([(S, K, B, H, W, ph, pw, ps) for S, K, B, (H, W), (ph, pw, ps) in grid()], np.int32)
    np.savez_compressed(path, shapes=g, **record_all())


def test_layout_matches_fixture():
    want = np.load(FIXTURE)
    shapes = np.array([(S, K, B, H, W, ph, pw, ps) for S, K, B, (H, W), (ph, pw, ps) in grid()], np.int32)
    assert np.array_equal(want["shapes"], shapes)
    got = record_all()
    assert sorted(got) == sorted(k for k in want.files if k != "shapes")
    for k, v in got.items():
        bad = np.flatnonzero((v != want[k]).reshape(len(shapes), -1).any(axis=1))
        assert bad.size == 0, "%s differs for %d shapes, first (S, K, B, H, W, psf_h, psf_w, per_scene) = %s: %s != %s" % (
            k, bad.size, shapes[bad[0]].tolist(), v[bad[0]], want[k][bad[0]])
    # the grid reaches every region: both gradient paths of K > 8, both convolutions, the split, the stamps
    assert (want["default/pipelines"] == 2).any() and (want["PSF_HIPFFT/pipelines"] == 1).all()
    assert (want["default/psf_plan"][:, 0] == 0).any() and (want["default/psf_plan"][:, 0] == -1).any()
    assert (want["STAMPS/stamps_offset"] > 0).any() and (want["default/stamps_offset"] == -1).all()
    k30 = shapes[:, 1] == 30
    assert (want["FORCE_HUGEK/workspace_bytes"][k30] > want["default/workspace_bytes"][k30]).all()


def freeze_checks():
    """which calls fix the layout switches for the rest of the process (scarlet_set_option then refuses a change)"""
    sys.path.insert(0, ROOT)
    from scarlet_amd import _lib

    def batch(S, K, H=64, W=64, psf=0):
        b = _lib.ScarletBatch()
        b.S, b.K, b.B, b.H, b.W = S, K, 5, H, W
        if psf:
            b.diff_kernel, b.psf_h, b.psf_w = 1, psf, psf
        return ctypes.byref(b)

    def free(name):
        return _lib.lib.scarlet_set_option(name.encode(), 1) == 0 and _lib.lib.scarlet_set_option(name.encode(), 0) == 1

    def frozen(name):
        return _lib.lib.scarlet_set_option(name.encode(), 1) == _lib.E_ARG

    out16 = (ctypes.c_int32 * 16)()
    # the read-only entry points fix nothing: two pipelines, the LDS plan, stamps with STAMPS off
    for b in (batch(1024, 4, psf=11), batch(7, 30, psf=11), batch(7, 30, 300, 257, psf=11)):
        assert _lib.lib.scarlet_batch_pipelines(b) in (1, 2)
        _lib.lib.scarlet_debug_psf_plan(b, out16)
        assert _lib.lib.scarlet_debug_psf_stamps_offset(b) == -1
    assert all(free(s) for s in SWITCHES)
    # FORCE_HUGEK sizes only 8 < K <= 32
    for K in (1, 8, 33, 256):
        assert _lib.lib.scarlet_batch_workspace_bytes(batch(7, K)) > 0
    assert all(free(s) for s in SWITCHES)
    assert _lib.lib.scarlet_batch_workspace_bytes(batch(7, 32)) > 0
    assert frozen("FORCE_HUGEK") and b"FORCE_HUGEK" in _lib.lib.scarlet_last_error()
    assert free("PSF_HIPFFT") and free("STAMPS")
    # STAMPS on: the stamps of a batch on the hipFFT path do not exist (nothing fixed), those of the LDS path do
    assert _lib.lib.scarlet_set_option(b"STAMPS", 1) == 0
    assert _lib.lib.scarlet_debug_psf_stamps_offset(batch(7, 4, 300, 257, psf=11)) == -1
    assert free("PSF_HIPFFT")
    assert _lib.lib.scarlet_debug_psf_stamps_offset(batch(7, 4, psf=11)) > 0
    assert frozen("PSF_HIPFFT") and _lib.lib.scarlet_set_option(b"STAMPS", 0) == _lib.E_ARG
    assert free("NO_BOX")
    print("freeze ok")


def test_freeze_points():
    env = dict(os.environ, **{"SCARLET_" + s: "0" for s in SWITCHES})
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--freeze"], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0 and b"freeze ok" in out.stdout, out.stderr.decode()[-2000:]


if __name__ == "__main__":
    if sys.argv[1] == "--record":
        np.savez(sys.argv[2], **record())
    elif sys.argv[1] == "--freeze":
        freeze_checks()
    elif sys.argv[1] == "--write":
        record_fixture(sys.argv[2])
