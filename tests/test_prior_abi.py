"""CPU: priors at the C ABI and in the host layer.

The prior travels in a struct of its own (scarlet_prior); scarlet_batch keeps its size.  The header declares the struct
and the entry points, the library exports them and _lib.py binds them with the offsets the C compiler gives the header.
Argument errors come back before any launch, so they are testable with fake pointers and no device.  The weight
expansion of the Python layer is a plain function."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scarlet_hip.h")
FIELDS = ["grad_sed", "grad_morph", "L_sed", "L_morph", "quad_sed_weight", "quad_sed_target", "quad_morph_weight",
          "quad_morph_target", "L_comp"]
ENTRY_POINTS = ["scarlet_backward_step_prior", "scarlet_source_update_prior", "scarlet_fit_prior"]
FAKE = 0x1000          # a non-NULL pointer that is never dereferenced (every call below returns before a launch)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_struct_and_entry_points():
    text = _header()
    m = re.search(r"typedef struct scarlet_prior \{(.*?)\} scarlet_prior;", text, flags=re.S)
    assert m, "scarlet_prior is not declared"
    names = re.findall(r"\*\s*(\w+)\s*;", m.group(1))
    assert names == FIELDS
    assert re.search(r"double\s*\*\s*L_comp\s*;", m.group(1))             # the only output, float64
    for f in FIELDS[:-1]:
        assert re.search(r"const float\s*\*\s*%s\s*;" % f, m.group(1)), f
    for fn in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(\s*scarlet_batch \*b,\s*const scarlet_prior \*p," % fn, text), fn


def test_library_exports_and_binding():
    from scarlet_amd import _lib
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(ln.split()[-1] for ln in out.splitlines() if ln.strip())
    for fn in ENTRY_POINTS:
        assert fn in exported, fn
        assert fn in _lib.EXPORTS
        f = getattr(_lib.lib, fn)
        assert f.restype is ctypes.c_int
        assert f.argtypes[0]._type_ is _lib.ScarletBatch and f.argtypes[1]._type_ is _lib.ScarletPrior
    assert [f for f, _ in _lib.ScarletPrior._fields_] == FIELDS


def test_struct_offsets_match_the_c_compiler(tmp_path):
    from scarlet_amd import _lib
    src = tmp_path / "probe.c"
    body = "\n".join('printf("%s %%zu\\n", offsetof(scarlet_prior, %s));' % (f, f) for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scarlet_hip.h"\n'
                   'int main(void){ printf("sizeof %zu\\n", sizeof(scarlet_prior));\n'
                   'printf("batch %zu\\n", sizeof(scarlet_batch));\n' + body + '\nreturn 0;}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = {k: int(v) for k, v in (ln.split() for ln in subprocess.check_output([str(exe)]).decode().splitlines())}
    for i, f in enumerate(FIELDS):
        assert out[f] == 8 * i == getattr(_lib.ScarletPrior, f).offset, f
    assert out["sizeof"] == 72 == ctypes.sizeof(_lib.ScarletPrior)
    assert out["batch"] == 256 == ctypes.sizeof(_lib.ScarletBatch)          # scarlet_batch did not change


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


def _calls():
    from scarlet_amd import _lib
    L = _lib.lib
    return [
        ("scarlet_backward_step_prior", lambda b, p: L.scarlet_backward_step_prior(b, p, 0, None)),
        ("scarlet_source_update_prior", lambda b, p: L.scarlet_source_update_prior(b, p, 1, None)),
        ("scarlet_fit_prior", lambda b, p: L.scarlet_fit_prior(b, p, 1, 0.0, 0, 0, None)),
    ]


@pytest.mark.parametrize("which", range(3))
def test_argument_errors_before_any_launch(which):
    from scarlet_amd import _lib
    name, call = _calls()[which]
    good = _batch()
    # NULL prior
    assert call(ctypes.byref(good), None) == _lib.E_ARG
    assert "prior" in _lib.last_error()
    # L_comp missing
    p = _lib.ScarletPrior()
    assert call(ctypes.byref(good), ctypes.byref(p)) == _lib.E_ARG
    assert "L_comp" in _lib.last_error()
    # a target without its weight, on either factor
    for fac in ("sed", "morph"):
        p = _lib.ScarletPrior()
        p.L_comp = FAKE
        setattr(p, "quad_%s_target" % fac, FAKE)
        assert call(ctypes.byref(good), ctypes.byref(p)) == _lib.E_ARG
        assert "quad_%s_target" % fac in _lib.last_error() and "quad_%s_weight" % fac in _lib.last_error()
    # a batch that fails check_batch: its error, whatever the prior
    p = _lib.ScarletPrior()
    p.L_comp = FAKE
    assert call(ctypes.byref(_batch(pointers=False)), ctypes.byref(p)) == _lib.E_ARG
    assert "null pointer in batch" in _lib.last_error()
    assert call(ctypes.byref(_batch(K=257)), ctypes.byref(p)) == _lib.E_NOTIMPL
    assert call(ctypes.byref(_batch(H=2048)), ctypes.byref(p)) == _lib.E_TOO_LARGE
    assert call(None, ctypes.byref(p)) == _lib.E_ARG


def test_fit_prior_refuses_a_negative_iteration_count():
    from scarlet_amd import _lib
    p = _lib.ScarletPrior()
    p.L_comp = FAKE
    assert _lib.lib.scarlet_fit_prior(ctypes.byref(_batch()), ctypes.byref(p), -1, 0.0, 0, 0, None) == _lib.E_ARG
    assert "max_iter" in _lib.last_error()


def test_expand_weights():
    from scarlet_amd.prior import expand_weights
    w = expand_weights(0.5, 3, 2)
    assert w.dtype == np.float32 and w.shape == (3, 2) and (w == 0.5).all() and w.flags["C_CONTIGUOUS"]
    w = expand_weights([1, 2], 3, 2)
    assert w.tolist() == [[1, 2]] * 3
    w = expand_weights(np.arange(6).reshape(3, 2), 3, 2)
    assert w.tolist() == [[0, 1], [2, 3], [4, 5]]
    for bad in ([1, 2, 3], np.zeros((2, 2)), np.zeros((3, 2, 1)), -0.1, [1, -1], float("nan"), float("inf")):
        with pytest.raises(ValueError):
            expand_weights(bad, 3, 2)
    # S == K: a vector is one weight per component
    assert expand_weights([1, 2], 2, 2).tolist() == [[1, 2], [1, 2]]


def test_quadratic_prior_validation_without_a_device():
    import scarlet_amd as scarlet
    from scarlet_amd.prior import split_priors, check_target
    q = scarlet.QuadraticPrior(sed_weight=[0, 0.3], morph_weight=2.0)
    ws, wm = q.host_weights(4, 2)
    assert ws.shape == wm.shape == (4, 2) and ws[3].tolist() == [0, np.float32(0.3)] and (wm == 2).all()
    assert scarlet.QuadraticPrior(morph_weight=1.0).host_weights(4, 2)[0] is None
    with pytest.raises(ValueError):
        scarlet.QuadraticPrior(sed_target=np.zeros((4, 2, 5)))               # a target needs its weight
    with pytest.raises(ValueError):
        scarlet.QuadraticPrior(morph_target=np.zeros((4, 2, 8, 8)), sed_weight=1.0)
    with pytest.raises(ValueError):
        scarlet.QuadraticPrior(sed_weight=-1.0)
    with pytest.raises(ValueError):
        scarlet.QuadraticPrior(morph_weight=[1.0, float("nan")])
    with pytest.raises(ValueError):
        q.host_weights(4, 3)                                                   # (2,) weights on K = 3
    check_target((2, 5), (4, 2, 5), "sed_target")
    with pytest.raises(ValueError):
        check_target((3, 5), (4, 2, 5), "sed_target")
    with pytest.raises(ValueError):
        check_target((1, 4, 2, 5), (4, 2, 5), "sed_target")
    fn = lambda sed, morph: {}
    assert split_priors(q) == (q, [], [])
    assert split_priors([fn, q, dict(L_sed=1.0)]) == (q, [dict(L_sed=1.0)], [fn])
    with pytest.raises(ValueError):
        split_priors([q, q])
    with pytest.raises(ValueError):
        split_priors(dict(grad=1.0))
    with pytest.raises(ValueError):
        split_priors(3)
