"""CPU: the joint fit with priors at the C ABI (scarlet_fit_observations_prior), and the cases of
tests/test_gpu_observations_prior.py on the oracle's side.

The header declares the entry point, the library exports it and _lib.py binds it.  Its argument errors come back before
any launch, so they are testable with fake pointers and no device.  The last test keeps the GPU tests' exemption cap
honest: on every scene they fit, the float32 and the float64 oracle agree about the support of every morphology after
every iteration, so no case was chosen with a pixel on a threshold."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import observations_prior_common as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scarlet_hip.h")
NAME = "scarlet_fit_observations_prior"
FAKE = 0x1000          # a non-NULL pointer that is never dereferenced (every call below returns before a launch)


def test_header_declares_the_entry_point():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % NAME, text, flags=re.S)
    assert m, NAME + " is not declared"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["scarlet_batch *state", "const scarlet_constraints *c", "const scarlet_prior *p",
                    "scarlet_batch *const *obs", "const scarlet_lowres *const *lowres", "const int32_t *band0", "int n_obs",
                    "int max_iter", "double e_rel", "int approximate_L", "int check_every", "void *stream"]
    assert "do not take priors" not in open(HEADER).read()


def test_library_exports_and_binding():
    from scarlet_amd import _lib
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert NAME in set(ln.split()[-1] for ln in out.splitlines() if ln.strip())
    assert NAME in _lib.EXPORTS
    f = getattr(_lib.lib, NAME)
    assert f.restype is ctypes.c_int and len(f.argtypes) == 12
    assert f.argtypes[0]._type_ is _lib.ScarletBatch and f.argtypes[1]._type_ is _lib.ScarletConstraints
    assert f.argtypes[2]._type_ is _lib.ScarletPrior
    assert f.argtypes[3]._type_._type_ is _lib.ScarletBatch and f.argtypes[4]._type_._type_ is _lib.ScarletLowres


def _batch(S=4, K=3, B=5, H=32, W=32, pointers=True):
    from scarlet_amd import _lib
    b = _lib.ScarletBatch()
    b.S, b.K, b.B, b.H, b.W = S, K, B, H, W
    if pointers:
        for f in ("images", "cur", "centers", "shifts", "flags", "lipschitz", "mse", "it", "active", "status", "workspace"):
            setattr(b, f, FAKE)
        for i in range(2):
            b.sed[i] = FAKE
            b.morph[i] = FAKE
        b.mse_capacity = 8
    return b


def _call(state, p, obs=None, cons=False, n_obs=2, max_iter=1, lowres=None):
    from scarlet_amd import _lib
    obs = [_batch(B=3), _batch(B=2)] if obs is None else obs
    ptrs = (ctypes.POINTER(_lib.ScarletBatch) * len(obs))(*[ctypes.pointer(o) for o in obs])
    band0 = np.array([0, 3][:len(obs)], dtype=np.int32)
    c = _lib.ScarletConstraints()
    return _lib.lib.scarlet_fit_observations_prior(
        None if state is None else ctypes.byref(state), ctypes.byref(c) if cons else None,
        None if p is None else ctypes.byref(p), ptrs, lowres, band0.ctypes.data_as(ctypes.c_void_p), n_obs, max_iter, 0.0, 0,
        0, None)


@pytest.mark.parametrize("cons", [False, True], ids=["c_null", "c_given"])
def test_argument_errors_before_any_launch(cons):
    from scarlet_amd import _lib
    good = _batch()
    # NULL prior
    assert _call(good, None, cons=cons) == _lib.E_ARG
    assert "prior" in _lib.last_error()
    # L_comp missing
    assert _call(good, _lib.ScarletPrior(), cons=cons) == _lib.E_ARG
    assert "L_comp" in _lib.last_error()
    # a target without its weight, on either factor
    for fac in ("sed", "morph"):
        p = _lib.ScarletPrior()
        p.L_comp = FAKE
        setattr(p, "quad_%s_target" % fac, FAKE)
        assert _call(good, p, cons=cons) == _lib.E_ARG
        assert "quad_%s_target" % fac in _lib.last_error() and "quad_%s_weight" % fac in _lib.last_error()
    # what check_observations refuses comes first, whatever the prior
    p = _lib.ScarletPrior()
    p.L_comp = FAKE
    assert _call(_batch(pointers=False), p, cons=cons) == _lib.E_ARG
    assert "null pointer in batch" in _lib.last_error()
    assert _call(_batch(K=257), p, cons=cons) == _lib.E_NOTIMPL
    assert _call(_batch(H=2048), p, cons=cons) == _lib.E_TOO_LARGE
    assert _call(None, p, cons=cons) == _lib.E_ARG
    assert _call(good, p, cons=cons, n_obs=0) == _lib.E_ARG
    assert _call(good, p, cons=cons, n_obs=9) == _lib.E_ARG
    assert _call(good, p, cons=cons, max_iter=-1) == _lib.E_ARG
    assert "max_iter" in _lib.last_error()
    assert _call(good, p, cons=cons, obs=[_batch(B=3), _batch(B=3)]) == _lib.E_ARG          # bands 3 .. 5 of 5
    assert "does not fit the model frame" in _lib.last_error()
    assert _call(good, p, cons=cons, obs=[_batch(B=3), _batch(B=2, H=16)]) == _lib.E_ARG   # another grid, no scarlet_lowres
    assert "does not fit the model frame" in _lib.last_error()


def test_python_layer_no_longer_refuses():
    import inspect
    from scarlet_amd import batch
    assert "does not take priors" not in inspect.getsource(batch)


@pytest.mark.parametrize("name", list(oc.CASES))
def test_float32_and_float64_oracles_agree_on_every_support(name):
    from oracle import build as obuild
    obuild.build()
    case = oc.CASES[name]()
    st0 = case.host_state()
    for i in range(case.S):
        msg = oc.supports_agree((case.spec(st0, i), case.iters))
        assert msg is None, "case %s, scene %d: %s" % (name, i, msg)
    if name == "stopping":
        # ... and the scenes of the stopping case stop on their own, at different counts, within its 10 iterations
        its = [oc.oracle_fit((case.spec(st0, i), case.iters, case.e_rel, np.float32))[4] for i in range(case.S)]
        assert len(set(its)) > 1 and max(its) < case.iters, its
