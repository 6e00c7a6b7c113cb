"""CPU: per-component constraint switches at the C ABI.

The four settings of the constraint pipeline travel per component in a struct of their own (scarlet_constraints);
scarlet_batch keeps its size.  The header declares the struct and the three entry points, the library exports them and
_lib.py binds them with the offsets the C compiler gives the header.  Argument errors come back before any launch, so
they are testable with fake pointers and no device."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scarlet_hip.h")
FIELDS = ["symmetric", "monotonic", "l0_thresh", "l1_thresh"]
ENTRY_POINTS = ["scarlet_fit_constrained", "scarlet_source_update_constrained", "scarlet_fit_observations_constrained"]
FAKE = 0x1000          # a non-NULL pointer that is never dereferenced (every call below returns before a launch)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_struct_and_entry_points():
    text = _header()
    m = re.search(r"typedef struct scarlet_constraints \{(.*?)\} scarlet_constraints;", text, flags=re.S)
    assert m, "scarlet_constraints is not declared"
    assert re.findall(r"\*\s*(\w+)\s*;", m.group(1)) == FIELDS
    for f in FIELDS[:2]:
        assert re.search(r"const uint8_t\s*\*\s*%s\s*;" % f, m.group(1)), f
    for f in FIELDS[2:]:
        assert re.search(r"const float\s*\*\s*%s\s*;" % f, m.group(1)), f
    for fn in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(\s*scarlet_batch \*\w+,\s*const scarlet_constraints \*c," % fn, text), fn
    # the two single-observation entry points take the prior as an optional third argument
    for fn in ENTRY_POINTS[:2]:
        assert re.search(r"\bint\s+%s\s*\([^)]*const scarlet_prior \*p" % fn, text), fn


def test_header_states_the_rules():
    text = " ".join(open(HEADER).read().split())
    for phrase in ("absent components and of inactive scenes are not read", "c == NULL is SCARLET_E_ARG",
                   "odd-sized centroid_psf", "must agree on `symmetric` and `monotonic`",
                   "workspace layout does not depend on the struct", "OR over its arrays", "With every pointer NULL"):
        assert phrase in text, phrase


def test_library_exports_and_binding():
    from scarlet_amd import _lib
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(ln.split()[-1] for ln in out.splitlines() if ln.strip())
    for fn in ENTRY_POINTS:
        assert fn in exported, fn
        assert fn in _lib.EXPORTS
        f = getattr(_lib.lib, fn)
        assert f.restype is ctypes.c_int
        assert f.argtypes[0]._type_ is _lib.ScarletBatch and f.argtypes[1]._type_ is _lib.ScarletConstraints
    assert _lib.lib.scarlet_fit_constrained.argtypes[2]._type_ is _lib.ScarletPrior
    assert _lib.lib.scarlet_source_update_constrained.argtypes[2]._type_ is _lib.ScarletPrior
    assert [f for f, _ in _lib.ScarletConstraints._fields_] == FIELDS


def test_struct_offsets_match_the_c_compiler(tmp_path):
    from scarlet_amd import _lib
    src = tmp_path / "probe.c"
    body = "\n".join('printf("%s %%zu\\n", offsetof(scarlet_constraints, %s));' % (f, f) for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scarlet_hip.h"\n'
                   'int main(void){ printf("sizeof %zu\\n", sizeof(scarlet_constraints));\n'
                   'printf("batch %zu\\n", sizeof(scarlet_batch));\n'
                   'printf("last %zu\\n", offsetof(scarlet_batch, n_components));\n' + body + '\nreturn 0;}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = {k: int(v) for k, v in (ln.split() for ln in subprocess.check_output([str(exe)]).decode().splitlines())}
    for i, f in enumerate(FIELDS):
        assert out[f] == 8 * i == getattr(_lib.ScarletConstraints, f).offset, f
    assert out["sizeof"] == 32 == ctypes.sizeof(_lib.ScarletConstraints)
    assert out["batch"] == 256 == ctypes.sizeof(_lib.ScarletBatch)          # scarlet_batch did not change
    assert out["last"] == 248 == _lib.ScarletBatch.n_components.offset      # ... and n_components is still last


def _batch(S=4, K=3, B=5, H=32, W=32, pointers=True, centroid_P=0):
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
    if centroid_P:
        b.centroid_psf, b.centroid_P = FAKE, centroid_P
    return b


def _calls():
    from scarlet_amd import _lib
    L = _lib.lib
    band0 = (ctypes.c_int32 * 1)(0)

    def fit_obs(b, c):
        obs = (ctypes.POINTER(_lib.ScarletBatch) * 1)(ctypes.pointer(_batch()))
        return L.scarlet_fit_observations_constrained(b, c, obs, ctypes.cast(band0, ctypes.c_void_p), 1, 1, 0.0, 0, 0, None)

    return [
        ("scarlet_fit_constrained", lambda b, c: L.scarlet_fit_constrained(b, c, None, 1, 0.0, 0, 0, None)),
        ("scarlet_source_update_constrained", lambda b, c: L.scarlet_source_update_constrained(b, c, None, 1, None)),
        ("scarlet_fit_observations_constrained", fit_obs),
    ]


@pytest.mark.parametrize("which", range(3))
def test_argument_errors_before_any_launch(which):
    from scarlet_amd import _lib
    name, call = _calls()[which]
    good = _batch()
    # NULL constraints
    assert call(ctypes.byref(good), None) == _lib.E_ARG
    assert "constraints is NULL" in _lib.last_error()
    # a symmetric array needs the centroid PSF, odd-sized: the message names the field
    c = _lib.ScarletConstraints()
    c.symmetric = FAKE
    for b in (good, _batch(centroid_P=4)):
        for scalar in (0, 1):                  # whatever the batch's own scalar says
            b.symmetric = scalar
            assert call(ctypes.byref(b), ctypes.byref(c)) == _lib.E_ARG
            assert "constraints.symmetric" in _lib.last_error() and "centroid_psf" in _lib.last_error()
    # a batch that fails check_batch: its error, whatever the struct holds
    c = _lib.ScarletConstraints()
    c.monotonic = FAKE
    assert call(ctypes.byref(_batch(pointers=False)), ctypes.byref(c)) == _lib.E_ARG
    assert "null pointer in batch" in _lib.last_error()
    assert call(ctypes.byref(_batch(K=257)), ctypes.byref(c)) == _lib.E_NOTIMPL
    assert call(ctypes.byref(_batch(H=2048)), ctypes.byref(c)) == _lib.E_TOO_LARGE
    assert call(None, ctypes.byref(c)) == _lib.E_ARG


def test_fit_constrained_refuses_a_negative_iteration_count_and_a_bad_prior():
    from scarlet_amd import _lib
    c = _lib.ScarletConstraints()
    c.l0_thresh = FAKE
    assert _lib.lib.scarlet_fit_constrained(ctypes.byref(_batch()), ctypes.byref(c), None, -1, 0.0, 0, 0, None) == _lib.E_ARG
    assert "max_iter" in _lib.last_error()
    p = _lib.ScarletPrior()                    # a prior without its required output
    assert _lib.lib.scarlet_fit_constrained(ctypes.byref(_batch()), ctypes.byref(c), ctypes.byref(p), 1, 0.0, 0, 0, None) == _lib.E_ARG
    assert "L_comp" in _lib.last_error()
    assert _lib.lib.scarlet_source_update_constrained(ctypes.byref(_batch()), ctypes.byref(c), ctypes.byref(p), 1, None) == _lib.E_ARG
    assert "L_comp" in _lib.last_error()
