#!/usr/bin/env python3
"""Record what the named fit and update entry points refuse on the host, before anything is launched.

Every row is (entry point, case name, return code, scarlet_last_error() text); the file holds them packed (pack()).
A case is one or two defects applied to an otherwise valid set of arguments whose pointers are fakes: every recorded
call returns before a launch, so no device is needed.  The library is loaded by path with plain ctypes.CDLL and the struct mirrors below, so that the tool runs against
any build:

    python tools/record_entry_refusals.py --lib scarlet_amd/csrc/libscarlet_hip.so --out tests/golden/entry_refusals.json
    python tools/record_entry_refusals.py --lib LIB --replay tests/golden/entry_refusals.json     (all rows, one process)

Recording runs each row in a child process of its own.  A row that returns SCARLET_OK or SCARLET_E_HIP, or whose child
dies, is a mistake in the tables below (the call got past the host checks): recording stops and names it.
"""
import argparse
import collections
import ctypes
import hashlib
import itertools
import json
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from ctypes import POINTER, Structure, c_double, c_float, c_int, c_int32, c_void_p

FAKE = 0x1000          # a non-NULL pointer that is never dereferenced
OK, E_HIP = 0, -3


class Batch(Structure):
    _fields_ = [("S", c_int32), ("K", c_int32), ("B", c_int32), ("H", c_int32), ("W", c_int32),
                ("images", c_void_p), ("weights", c_void_p), ("weight_scalar", c_float),
                ("sed", c_void_p * 2), ("morph", c_void_p * 2), ("cur", c_void_p),
                ("centers", c_void_p), ("shifts", c_void_p), ("flags", c_void_p),
                ("fix_sed", c_void_p), ("fix_morph", c_void_p),
                ("lipschitz", c_void_p), ("mse", c_void_p), ("mse_capacity", c_int32),
                ("it", c_void_p), ("active", c_void_p), ("status", c_void_p),
                ("symmetric", c_int32), ("monotonic", c_int32), ("l0_thresh", c_float), ("l1_thresh", c_float),
                ("centroid_psf", c_void_p), ("centroid_P", c_int32),
                ("diff_kernel", c_void_p), ("psf_h", c_int32), ("psf_w", c_int32), ("diff_kernel_per_scene", c_int32),
                ("workspace", c_void_p), ("group", c_void_p), ("n_components", c_void_p)]


class Frames(Structure):
    _fields_ = [("frame_hw", c_void_p)]


class Prior(Structure):
    _fields_ = [("grad_sed", c_void_p), ("grad_morph", c_void_p), ("L_sed", c_void_p), ("L_morph", c_void_p),
                ("quad_sed_weight", c_void_p), ("quad_sed_target", c_void_p),
                ("quad_morph_weight", c_void_p), ("quad_morph_target", c_void_p), ("L_comp", c_void_p)]


class Constraints(Structure):
    _fields_ = [("symmetric", c_void_p), ("monotonic", c_void_p), ("l0_thresh", c_void_p), ("l1_thresh", c_void_p)]


class UpdateOptions(Structure):
    _fields_ = [("sym_algorithm", c_void_p), ("sym_strength", c_void_p), ("mono_nearest", c_void_p), ("mono_thresh", c_void_p),
                ("positive", c_void_p), ("normalize", c_void_p)]


class Lowres(Structure):
    _fields_ = [("h", c_int32), ("w", c_int32), ("nfy", c_int32), ("nfx", c_int32), ("B", c_int32),
                ("uy", c_void_p), ("ux", c_void_p), ("vy", c_void_p), ("vx", c_void_p), ("dhat", c_void_p),
                ("v_per_scene", c_int32), ("dhat_per_scene", c_int32), ("workspace", c_void_p)]


class LowresFrames(Structure):
    _fields_ = [("dims", c_void_p), ("uy", c_void_p), ("ux", c_void_p)]


# ---- the entry points: their arguments in order.  b: the batch / state; c, p, o, f: the structs; obs, band0, n_obs: the
# observation list; lowres, lrf: the lists of scarlet_lowres / scarlet_lowres_frames pointers
FIT = ("max_iter", "e_rel", "approximate_L", "check_every", "stream")
UPD = ("in_iteration", "stream")
OBS = ("obs", "band0", "n_obs")
ENTRY_POINTS = {
    "scarlet_fit": ("b",) + FIT,
    "scarlet_fit_prior": ("b", "p") + FIT,
    "scarlet_fit_constrained": ("b", "c", "p") + FIT,
    "scarlet_fit_options": ("b", "c", "o") + FIT,
    "scarlet_fit_frames": ("b", "f", "c") + FIT,
    "scarlet_fit_frames_grouped": ("b", "f", "c") + FIT,
    "scarlet_fit_frames_options": ("b", "f", "c", "o") + FIT,
    "scarlet_fit_multi": ("b",) + OBS + FIT,
    "scarlet_fit_observations": ("b",) + OBS + FIT,
    "scarlet_source_update": ("b",) + UPD,
    "scarlet_source_update_prior": ("b", "p") + UPD,
    "scarlet_source_update_constrained": ("b", "c", "p") + UPD,
    "scarlet_source_update_options": ("b", "c", "o") + UPD,
    "scarlet_source_update_frames": ("b", "f", "c") + UPD,
    "scarlet_source_update_frames_grouped": ("b", "f", "c") + UPD,
    "scarlet_source_update_frames_options": ("b", "f", "c", "o") + UPD,
    "scarlet_fit_observations_constrained": ("b", "c") + OBS + FIT,
    "scarlet_fit_observations_options": ("b", "c", "o") + OBS + FIT,
    "scarlet_fit_observations_lowres": ("b", "c", "obs", "lowres", "band0", "n_obs") + FIT,
    "scarlet_fit_observations_lowres_large": ("b", "c", "obs", "lowres", "band0", "n_obs") + FIT,
    "scarlet_fit_observations_prior": ("b", "c", "p", "obs", "lowres", "band0", "n_obs") + FIT,
    "scarlet_fit_observations_wide": ("b", "c", "p", "obs", "lowres", "band0", "n_obs") + FIT,
    "scarlet_fit_observations_frames": ("b", "f", "c") + OBS + FIT,
    "scarlet_fit_observations_frames_lowres": ("b", "f", "c", "obs", "lowres", "lrf", "band0", "n_obs") + FIT,
}
ARGTYPES = dict(b=POINTER(Batch), c=POINTER(Constraints), p=POINTER(Prior), o=POINTER(UpdateOptions), f=POINTER(Frames),
                obs=POINTER(POINTER(Batch)), band0=c_void_p, n_obs=c_int, lowres=POINTER(POINTER(Lowres)),
                lrf=POINTER(POINTER(LowresFrames)), max_iter=c_int, e_rel=c_double, approximate_L=c_int, check_every=c_int,
                stream=c_void_p, in_iteration=c_int)


def fake_batch(S=4, K=3, B=5, H=32, W=32):
    b = Batch()
    b.S, b.K, b.B, b.H, b.W = S, K, B, H, W
    for name in ("images", "cur", "centers", "shifts", "flags", "lipschitz", "mse", "it", "active", "status", "workspace"):
        setattr(b, name, FAKE)
    for i in range(2):
        b.sed[i] = FAKE
        b.morph[i] = FAKE
    b.mse_capacity = 8
    return b


class World:
    """A valid set of arguments for `entry`: a 5-channel state, observations of 3 + 2 channels; where the entry point
    takes low-resolution lists the second observation is an 8 x 8 low-resolution one (with per-scene tables where it
    takes those)."""

    def __init__(self, entry):
        args = ENTRY_POINTS[entry]
        self.b, self.c, self.o, self.f, self.p = fake_batch(), Constraints(), UpdateOptions(), Frames(), Prior()
        self.o.positive = self.f.frame_hw = self.p.L_comp = FAKE
        self.obs = [fake_batch(B=3), fake_batch(B=2)]
        self.band0 = [0, 3]
        self.n_obs = 2
        self.lowres = self.lrf = None
        if "lowres" in args:
            lr = Lowres()
            lr.h = lr.w = 8
            lr.nfy = lr.nfx = 16
            lr.B = 2
            lr.uy = lr.ux = lr.vy = lr.vx = lr.dhat = lr.workspace = FAKE
            self.obs[1].H = self.obs[1].W = 8
            self.lowres = [None, lr]
        if "lrf" in args:
            lf = LowresFrames()
            lf.dims = lf.uy = lf.ux = FAKE
            self.lowres[1].v_per_scene = self.lowres[1].dhat_per_scene = 1
            self.lrf = [None, lf]
        self.max_iter = 1

    def call(self, lib, entry):
        names = ENTRY_POINTS[entry]
        fn = getattr(lib, entry)
        fn.restype, fn.argtypes = c_int, [ARGTYPES[n] for n in names]

        def plist(items, kind):
            if items is None:
                return None
            return (POINTER(kind) * max(len(items), 1))(*[POINTER(kind)() if x is None else ctypes.pointer(x) for x in items])
        band0 = None if self.band0 is None else (c_int32 * len(self.band0))(*self.band0)
        values = dict(b=self.b, c=self.c, p=self.p, o=self.o, f=self.f, obs=plist(self.obs, Batch),
                      band0=None if band0 is None else ctypes.cast(band0, c_void_p), n_obs=self.n_obs,
                      lowres=plist(self.lowres, Lowres), lrf=plist(self.lrf, LowresFrames), max_iter=self.max_iter, e_rel=0.0,
                      approximate_L=0, check_every=0, stream=None, in_iteration=1)
        argv = []
        for n in names:
            v = values[n]
            argv.append(ctypes.byref(v) if isinstance(v, Structure) else v)
        rc = fn(*argv)
        lib.scarlet_last_error.restype = ctypes.c_char_p
        return rc, lib.scarlet_last_error().decode("utf-8", "replace")


def _set(attr, **fields):
    def apply(w):
        x = getattr(w, attr)
        for k, v in fields.items():
            setattr(x, k, v)
    return apply


def _null(attr):
    return lambda w: setattr(w, attr, None)


def _low(w):
    return w.lowres[1]


# ---- the defects: name -> (the arguments the entry point must have, the check helper that catches it at the parent, what
# it does to the World).  Field changes are applied before the defects that take a whole argument away ("null_*").
DEFECTS = {
    "null_batch": ((), "call", _null("b")),
    "null_constraints": (("c",), "call", _null("c")),
    "null_prior": (("p",), "prior", _null("p")),
    "null_options": (("o",), "options", _null("o")),
    "null_frames": (("f",), "frames", _null("f")),
    "null_obs": (("obs",), "obs", _null("obs")),
    "null_band0": (("obs",), "obs", _null("band0")),
    "null_lowres": (("lowres",), "lowlist", _null("lowres")),
    "null_lowres_frames": (("lrf",), "lowlist", _null("lrf")),
    "zero_shape": ((), "call", _set("b", S=0)),
    "H_2048": ((), "call", _set("b", H=2048)),
    "K_257": ((), "call", _set("b", K=257)),
    "B_9": ((), "call", _set("b", B=9)),
    "B_33": ((), "call", _set("b", B=33)),
    "null_images": ((), "call", _set("b", images=None)),
    "symmetric_without_psf": ((), "call", _set("b", symmetric=1)),
    "constraints_symmetric_without_psf": (("c",), "call", _set("c", symmetric=FAKE)),
    "group": ((), "group", _set("b", group=FAKE)),
    "max_iter_negative": (("max_iter",), "call", lambda w: setattr(w, "max_iter", -1)),
    "prior_without_L_comp": (("p",), "prior", _set("p", L_comp=None)),
    "quad_target_without_weight": (("p",), "prior", _set("p", quad_sed_target=FAKE)),
    "n_obs_0": (("obs",), "obs", lambda w: setattr(w, "n_obs", 0)),
    "n_obs_9": (("obs",), "obs", lambda w: setattr(w, "n_obs", 9)),
    "null_obs_entry": (("obs",), "obs", lambda w: w.obs.__setitem__(0, None)),
    "obs_shape": (("obs",), "obs", lambda w: setattr(w.obs[0], "S", 5)),
    "obs_band_range": (("obs",), "obs", lambda w: w.band0.__setitem__(1, 4)),
    "obs_null_images": (("obs",), "obs", lambda w: setattr(w.obs[1], "images", None)),
    "obs_n_components": (("obs",), "obs", lambda w: setattr(w.obs[1], "n_components", FAKE)),
    "state_n_components": (("obs",), "counts", _set("b", n_components=FAKE)),
    "lowres_obs_diff_kernel": (("lowres",), "obs", lambda w: setattr(w.obs[1], "diff_kernel", FAKE)),
    "lowres_null_factor": (("lowres",), "obs", lambda w: setattr(_low(w), "uy", None)),
    "lowres_frames_without_lowres": (("lrf",), "lrf", lambda w: (w.lowres.__setitem__(1, None), setattr(w.obs[1], "H", 32),
                                                                   setattr(w.obs[1], "W", 32))),
    "lowres_frames_without_frame_hw": (("lrf",), "lrf", _set("f", frame_hw=None)),
    "lowres_frames_null_table": (("lrf",), "lrf", lambda w: setattr(w.lrf[1], "dims", None)),
    "lowres_frames_without_per_scene": (("lrf",), "lrf", lambda w: setattr(_low(w), "v_per_scene", 0)),
    "frame_hw_lowres_without_tables": (("lrf",), "lrf", lambda w: w.lrf.__setitem__(1, None)),
}
ORDER = list(DEFECTS)          # (the order of application: the null_* defects, which come first here, go last)


def _apply(w, names):
    for n in sorted(names, key=lambda n: (n.startswith("null_") and n not in ("null_images", "null_obs_entry"), ORDER.index(n))):
        try:
            DEFECTS[n][2](w)
        except (AttributeError, TypeError):          # (the argument it changes is already gone)
            pass


# ---- what the parent's source accepts: (defect, entry point) pairs that are no refusal, each read off scarlet_hip.hip
_C_OPTIONAL = {e for e, a in ENTRY_POINTS.items() if "c" in a} - {
    "scarlet_fit_constrained", "scarlet_source_update_constrained", "scarlet_fit_observations_constrained",
    "scarlet_fit_observations_lowres", "scarlet_fit_observations_lowres_large"}
_P_OPTIONAL = {"scarlet_fit_constrained", "scarlet_source_update_constrained", "scarlet_fit_observations_wide"}
_GROUP_REFUSED = {"scarlet_fit_options", "scarlet_source_update_options", "scarlet_fit_frames", "scarlet_source_update_frames",
                  "scarlet_fit_observations_options", "scarlet_fit_observations_frames",
                  "scarlet_fit_observations_frames_lowres"}
_WIDE = {"scarlet_fit_observations_wide", "scarlet_fit_observations_frames", "scarlet_fit_observations_frames_lowres"}
ACCEPTED = {
    "null_constraints": _C_OPTIONAL,                                  # check_call(b, c != nullptr, c, ...)
    "null_prior": _P_OPTIONAL,                                        # check_prior only where need_p or p
    "null_lowres": {"scarlet_fit_observations_prior", "scarlet_fit_observations_wide"},        # lowres may be NULL
    "group": set(ENTRY_POINTS) - _GROUP_REFUSED,
    "B_9": _WIDE,                                                     # up to SCARLET_MAX_CHANNELS there
    "state_n_components": set(ENTRY_POINTS) - {"scarlet_fit_multi"},  # refuse_counts
}
# scarlet_fit_multi refuses the counts of an observation in refuse_counts, ahead of everything else ("counts")
MULTI_ONLY_TAG = {("obs_n_components", "scarlet_fit_multi"): "counts"}


def applicable(defect, entry):
    need = DEFECTS[defect][0]
    return all(n in ENTRY_POINTS[entry] for n in need) and entry not in ACCEPTED.get(defect, ())


def tag(defect, entry):
    return MULTI_ONLY_TAG.get((defect, entry), DEFECTS[defect][1])


def cases():
    """(entry point, case name): every applicable defect, and every pair that two different check helpers catch"""
    rows = []
    for entry in ENTRY_POINTS:
        ones = [d for d in DEFECTS if applicable(d, entry)]
        rows += [(entry, d) for d in ones]
        rows += [(entry, a + "+" + b) for a, b in itertools.combinations(ones, 2) if tag(a, entry) != tag(b, entry)]
    return rows


def run_row(lib, entry, case):
    w = World(entry)
    _apply(w, case.split("+"))
    return w.call(lib, entry)


def pack(rows):
    """The recorded rows as the file holds them: the distinct answers once, and per entry point the index of the answer to
    each single defect by name ("one") and to each pair in the order of cases() ("two"); cases_sha256 pins that order."""
    messages, doc = [], collections.OrderedDict()
    for e, c, rc, text in rows:
        if [rc, text] not in messages:
            messages.append([rc, text])
        at = doc.setdefault(e, {"one": collections.OrderedDict(), "two": []})
        if "+" in c:
            at["two"].append(messages.index([rc, text]))
        else:
            at["one"][c] = messages.index([rc, text])
    names = "\n".join(e + " " + c for e, c, _, _ in rows).encode()
    return collections.OrderedDict(cases_sha256=hashlib.sha256(names).hexdigest(), messages=messages, entry_points=doc)


def unpack(doc):
    """[entry point, case, code, text] per row of a recorded file, in the order of cases()"""
    rows, two = [], {e: iter(at["two"]) for e, at in doc["entry_points"].items()}
    for e, c in cases():
        at = doc["entry_points"][e]
        rows.append([e, c] + doc["messages"][next(two[e]) if "+" in c else at["one"][c]])
    assert pack(rows) == doc, "the file does not hold the cases of this tool"
    return rows


def dump(doc, fh):
    fh.write('{"cases_sha256": %s,\n "messages": [\n  ' % json.dumps(doc["cases_sha256"]))
    fh.write(",\n  ".join(json.dumps(m) for m in doc["messages"]) + "],\n \"entry_points\": {\n")
    fh.write(",\n".join('  %s: {"one": %s,\n    "two": %s}' % (json.dumps(e), json.dumps(at["one"]), json.dumps(at["two"], separators=(",", ":")))
                         for e, at in doc["entry_points"].items()) + "}}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--out")
    ap.add_argument("--replay", help="a recorded file: run its rows in this process and print them as recorded now")
    ap.add_argument("--row", nargs=2, metavar=("ENTRY", "CASE"))
    a = ap.parse_args()
    if a.row:
        rc, text = run_row(ctypes.CDLL(a.lib), *a.row)
        print(json.dumps([a.row[0], a.row[1], rc, text]))
        return 0
    if a.replay:
        lib = ctypes.CDLL(a.lib)
        json.dump([[e, c] + list(run_row(lib, e, c)) for e, c, _, _ in unpack(json.load(open(a.replay)))], sys.stdout)
        return 0

    def child(row):
        r = subprocess.run([sys.executable, __file__, "--lib", a.lib, "--row", row[0], row[1]], capture_output=True, text=True)
        if r.returncode:
            return [row[0], row[1], None, "child exited with %d: %s" % (r.returncode, r.stderr[-200:])]
        return json.loads(r.stdout)
    with ThreadPoolExecutor(16) as pool:
        rows = list(pool.map(child, cases()))
    bad = [r for r in rows if r[2] is None or r[2] in (OK, E_HIP)]
    for r in bad:
        print("NOT A HOST REFUSAL:", r, file=sys.stderr)
    if bad:
        return 1
    with open(a.out, "w") as fh:
        dump(pack(rows), fh)
    print("%d rows over %d entry points -> %s" % (len(rows), len(ENTRY_POINTS), a.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
