"""CPU: one request struct behind every fit and update entry point (scarlet_fit_request, scarlet_fit_with).

1. tests/golden/entry_refusals.json holds what the named entry points refused on the host -- code and full text, one and
   two defects at a time -- recorded by tools/record_entry_refusals.py before they were rewritten as shapes of the request.
   The built library must answer every row the same way.
2. scarlet_fit_request_check on every combination of members present or absent against the table of DESIGN.md 5i, written
   out below: a request is accepted iff a named entry point accepts the same members.
3. The struct mirror against the header (gcc offsetof)."""
import ctypes
import importlib.util
import itertools
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "record_entry_refusals.py")
GOLDEN = os.path.join(ROOT, "tests", "golden", "entry_refusals.json")
FAKE = 0x1000


def _tool():
    spec = importlib.util.spec_from_file_location("record_entry_refusals", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_named_entry_points_refuse_what_they_refused():
    from scarlet_amd import _lib
    tool = _tool()
    recorded = tool.unpack(json.load(open(GOLDEN)))          # (asserts that the file holds exactly the tool's cases, in order)
    assert [(e, c) for e, c, _, _ in recorded] == [tuple(x) for x in tool.cases()]          # nothing omitted
    assert len({e for e, _, _, _ in recorded}) == 24 and len(recorded) > 2000
    out = subprocess.run([sys.executable, TOOL, "--lib", _lib.LIB_PATH, "--replay", GOLDEN], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    now = json.loads(out.stdout)
    differ = [(a, b) for a, b in zip(recorded, now) if a != b]
    assert len(now) == len(recorded) and not differ, differ[:10]
    assert not [r for r in recorded if r[2] in (_lib.OK, _lib.E_HIP)]


def test_struct_mirror_matches_header(tmp_path):
    from scarlet_amd import _lib
    fields = [f[0] for f in _lib.ScarletFitRequest._fields_]
    body = "\n".join('printf("%s %%zu\\n", offsetof(scarlet_fit_request, %s));' % (f, f) for f in fields)
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scarlet_hip.h"\n'
                   'int main(void){ printf("sizeof %zu\\n", sizeof(scarlet_fit_request));\n' + body + '\nreturn 0;}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out["sizeof"]) == ctypes.sizeof(_lib.ScarletFitRequest) == 88
    for f in fields:
        assert int(out[f]) == getattr(_lib.ScarletFitRequest, f).offset, f
    for name in ("scarlet_fit_request_check", "scarlet_fit_with", "scarlet_source_update_with"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name)


# ---- the combination table.  Members: constraints, prior, options, frame_hw, group, observations, lowres, lowres_frames,
# wide (more than 8 model channels).  Rows in the order of the library's check: the first whose `with` members are all
# present and whose `without` members are all absent gives the code; no row: SCARLET_OK.
MEMBERS = ("constraints", "prior", "options", "frame_hw", "group", "observations", "lowres", "lowres_frames", "wide")
ARG, NOTIMPL = -1, -4
TABLE = [
    # one observation: the batch's own images
    (("lowres",), ("observations",), ARG),
    (("lowres_frames",), ("observations",), ARG),
    (("prior", "frame_hw"), ("observations",), NOTIMPL),
    (("prior", "options"), ("observations",), NOTIMPL),
    (("wide",), ("observations",), NOTIMPL),                   # at most 8 bands
    # several observations
    (("observations", "options", "group"), (), NOTIMPL),
    (("observations", "options", "wide"), (), NOTIMPL),
    (("observations", "prior", "frame_hw"), (), NOTIMPL),
    (("observations", "options", "prior"), (), NOTIMPL),
    (("observations", "options", "frame_hw"), (), NOTIMPL),
    (("observations", "options", "lowres"), (), NOTIMPL),
    (("observations", "frame_hw", "group"), (), NOTIMPL),
    (("observations", "lowres_frames"), ("lowres",), ARG),
    (("observations", "frame_hw", "lowres"), ("lowres_frames",), NOTIMPL),
    (("observations", "lowres_frames"), ("frame_hw",), ARG),
]
# everything else is accepted: constraints, n_components and group with one of prior, options, frame_hw (one observation:
# options also with frame_hw and group); several observations: a prior with constraints, lowres, wide and group; options with
# constraints alone; frame_hw with each low-resolution observation's own lowres_frames


def expected(present):
    for need, without, code in TABLE:
        if all(m in present for m in need) and not any(m in present for m in without):
            return code
    return 0


def _request(present):
    """(batch, request, what they point to): valid fake arguments with exactly the members of `present`"""
    from scarlet_amd import _lib
    tool = _tool()
    C = 12 if "wide" in present else 5
    first = 8 if "wide" in present else 3

    def batch(**kw):
        return _lib.ScarletBatch.from_buffer_copy(bytes(tool.fake_batch(**kw)))
    b, r, keep = batch(B=C), _lib.ScarletFitRequest(), []
    if "group" in present:
        b.group = FAKE
    r.max_iter = 1
    if "constraints" in present:
        c = _lib.ScarletConstraints()
        c.l0_thresh = FAKE
        r.constraints = ctypes.pointer(c)
    if "prior" in present:
        p = _lib.ScarletPrior()
        p.L_comp = FAKE
        r.prior = ctypes.pointer(p)
    if "options" in present:
        o = _lib.ScarletUpdateOptions()
        o.positive = FAKE
        r.options = ctypes.pointer(o)
    f = _lib.ScarletFrames()                 # (the struct is always there: frame_hw = NULL says uniform frames)
    if "frame_hw" in present:
        f.frame_hw = FAKE
    r.frames = ctypes.pointer(f)
    low = "lowres" in present
    if "observations" in present:
        obs = [batch(B=first), batch(B=C - first, H=8 if low else 32, W=8 if low else 32)]
        r.n_obs = 2
        r.obs = (ctypes.POINTER(_lib.ScarletBatch) * 2)(*[ctypes.pointer(x) for x in obs])
        band0 = (ctypes.c_int32 * 2)(0, first)
        keep.append(band0)
        r.band0 = ctypes.cast(band0, ctypes.c_void_p)
    if low:
        lr = _lib.ScarletLowres()
        lr.h = lr.w = 8
        lr.nfy = lr.nfx = 16
        lr.B = C - first
        lr.uy = lr.ux = lr.vy = lr.vx = lr.dhat = lr.workspace = FAKE
        lr.v_per_scene = lr.dhat_per_scene = 1
        r.lowres = (ctypes.POINTER(_lib.ScarletLowres) * 2)(ctypes.POINTER(_lib.ScarletLowres)(), ctypes.pointer(lr))
    if "lowres_frames" in present:
        lf = _lib.ScarletLowresFrames()
        lf.dims = lf.uy = lf.ux = FAKE
        r.lowres_frames = (ctypes.POINTER(_lib.ScarletLowresFrames) * 2)(ctypes.POINTER(_lib.ScarletLowresFrames)(),
                                                                        ctypes.pointer(lf))
    return b, r, keep


def test_combination_table():
    from scarlet_amd import _lib
    wrong = []
    for bits in itertools.product((False, True), repeat=len(MEMBERS)):
        present = {m for m, on in zip(MEMBERS, bits) if on}
        b, r, keep = _request(present)
        rc = _lib.lib.scarlet_fit_request_check(ctypes.byref(b), ctypes.byref(r))
        if rc != expected(present):
            wrong.append((sorted(present), rc, expected(present), _lib.last_error()))
    assert not wrong, wrong[:10]


@pytest.mark.parametrize("present, words", [
    ({"prior", "frame_hw"}, ("prior", "frame_hw")),
    ({"prior", "options"}, ("prior", "options")),
    ({"observations", "prior", "frame_hw"}, ("prior", "frame_hw")),
    ({"observations", "options", "prior"}, ("prior", "options")),
    ({"observations", "options", "frame_hw"}, ("options", "frame_hw")),
    ({"observations", "options", "lowres"}, ("options", "lowres")),
    ({"lowres"}, ("lowres", "n_obs")),
])
def test_new_refusals_name_both_members(present, words):
    from scarlet_amd import _lib
    b, r, keep = _request(present)
    assert _lib.lib.scarlet_fit_request_check(ctypes.byref(b), ctypes.byref(r)) == expected(present) != 0
    assert all(w in _lib.last_error() for w in words), _lib.last_error()


def test_general_entry_points_check_before_any_launch():
    """scarlet_fit_with and scarlet_source_update_with run the same check: a refused request returns before a launch"""
    from scarlet_amd import _lib
    L = _lib.lib
    b, r, keep = _request({"prior", "frame_hw"})
    assert L.scarlet_fit_with(ctypes.byref(b), ctypes.byref(r), None) == NOTIMPL and "prior" in _lib.last_error()
    assert L.scarlet_source_update_with(ctypes.byref(b), ctypes.byref(r), 1, None) == NOTIMPL and "prior" in _lib.last_error()
    assert L.scarlet_fit_with(ctypes.byref(b), None, None) == ARG and "request" in _lib.last_error()
    assert L.scarlet_source_update_with(ctypes.byref(b), None, 0, None) == ARG
    assert L.scarlet_fit_request_check(ctypes.byref(b), None) == ARG
    plain = _request(set())[1]
    assert L.scarlet_fit_request_check(None, ctypes.byref(plain)) == ARG and _lib.last_error() == "null batch"
    # scarlet_source_update_with reads constraints, prior, options and frames only: the observation members are ignored
    b, r, keep = _request({"lowres"})
    r.prior = ctypes.pointer(_lib.ScarletPrior())          # (no L_comp)
    assert L.scarlet_source_update_with(ctypes.byref(b), ctypes.byref(r), 1, None) == ARG and "L_comp" in _lib.last_error()
