"""The case matrix of tests/test_gpu_matcher_refusals.py and the recorder of its fixture.

A case is ONE direct ctypes call of one compute entry of the block matcher or the semi-global matcher (include/adf_wls.h)
on a tiny image: 32 x 24, numDisparities 16, blockSize 5 where the rule under test allows.  What is recorded is the return
code and adf_last_error(), both exact.  Every output map and cost plane is prefilled with a sentinel byte and must come
back untouched: every refused case is refused by a host check before anything is launched.

    python tests/matcher_refusal_cases.py [output.json]

records tests/matcher_refusals.json on a GPU (a handle needs a device).  The fixture pins the host halves of
csrc/bm_matcher.hip and csrc/sgbm_matcher.hip as they were BEFORE their call record / plan / run refactor: it is never
recorded again from later code, a difference is a bug in that code.

The matrix takes every fail( of the two host halves that a call can reach before a launch through each entry that can
reach it (six block-matcher entries, two semi-global ones), then:
  * double faults, which pin the ORDER in which an entry reports: the device cost entries report a cost-plane fault before
    a NULL handle or a bad numDisparities, adf_bm_compute_cost_host reports it after; a both-views entry reports a NULL
    disp_right before anything else;
  * the rules that hold for device maps only: an odd disp_pair_stride with two pairs is refused by the device entries
    and ACCEPTED by the host entries, which copy by bytes (`accept`: the return code is recorded and the maps are compared
    with the dense call's); with one pair the stride is not read and every entry accepts it.
A message of the two host halves that no case reaches is listed in UNREACHED with its reason; test_every_message_is_pinned
greps the sources and fails on a message that is neither.  Two rules of the recorded code that no call could reach went
with the refactor: "disparity range of the right-view matcher does not fit" (it compared minDisparity + numDisparities - 1
with 32767 and -(minDisparity + numDisparities) + 1 with -32768, so it fired for a sum above 32768, and bm_check has by
then refused every sum above 2047) and
"census size %d is not supported" (adf_bm_set_cost alone writes a handle's cost and census size, and it refuses every
pair that census_dispatch does not list).
"""
import ctypes as C
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "matcher_refusals.json")
CSRC = os.path.join(ROOT, "addingdisparityfiltering_amd", "csrc")

W, H = 32, 24
SENTINEL = 0x5A
SLACK = 64                                            # bytes between the images of a plane (even: the dense call)

# entry -> (matcher, device pointers, the planes behind the views in argument order)
ENTRIES = {
    "adf_bm_compute_device": ("bm", True, ("disp",)),
    "adf_bm_compute_cost_device": ("bm", True, ("disp", "cost")),
    "adf_bm_compute_both_device": ("bm", True, ("disp", "disp_right")),
    "adf_bm_compute_both_cost_device": ("bm", True, ("disp", "disp_right", "cost_left", "cost_right")),
    "adf_bm_compute_host": ("bm", False, ("disp",)),
    "adf_bm_compute_cost_host": ("bm", False, ("disp", "cost")),
    "adf_sgbm_compute_device": ("sgbm", True, ("disp",)),
    "adf_sgbm_compute_host": ("sgbm", False, ("disp",)),
}
BM = [e for e in ENTRIES if ENTRIES[e][0] == "bm"]
SGBM = [e for e in ENTRIES if ENTRIES[e][0] == "sgbm"]
DEVICE = [e for e in ENTRIES if ENTRIES[e][1]]
SHORT = {e: e[len("adf_"):].replace("_compute", "") for e in ENTRIES}

# Edits of a case: (slot, what).  Slots: "handle", "n", "W", "H", "cn", a view ("left", "right") or an output plane.
# For a plane: "null" (pointer), "odd_ptr" (pointer + 1), "short" (row stride one element less than a row),
# "odd_stride" (row stride + 1 byte), "odd_pair" (pair stride - 1 byte: still past the image, odd).
# Handle settings: `params` (adf_bm_set_params / adf_sgbm_set_params names), `cost` (type, census size), `disp12`.
CASES = []


def _case(name, entry, edits=(), params=None, n=1, size=(W, H), cn=1, cost=None, accept=False):
    CASES.append(dict(name="%s:%s" % (SHORT[entry], name), entry=entry, edits=tuple(edits), params=dict(params or {}), n=n,
                      size=size, cn=cn, cost=cost, accept=accept))


# ---- the rules every entry of a matcher states (bm_check / sgbm_check), one fault each ----
COMMON = [
    ("handle-null", [("handle", "null")], {}),
    ("n-zero", [("n", 0)], {}),
    ("left-null", [("left", "null")], {}),
    ("right-null", [("right", "null")], {}),
    ("disp-null", [("disp", "null")], {}),
    ("w-zero", [("W", 0)], {}),
    ("h-zero", [("H", 0)], {}),
    ("left-short", [("left", "short")], {}),
    ("right-short", [("right", "short")], {}),
    ("disp-short", [("disp", "short")], {}),
    ("disp-odd-stride", [("disp", "odd_stride")], {}),
    ("disp-odd-ptr", [("disp", "odd_ptr")], {}),
    ("numdisp-zero", [], {"num_disp": 0}),
    ("numdisp-24", [], {"num_disp": 24}),
    ("block-even", [], {"block": 4}),
    ("range-high", [], {"min_disp": 2040}),
]
BM_ONLY = [
    ("block-3", [], {"block": 3}),
    ("block-23", [], {"block": 23}),
    ("cap-0", [], {"cap": 0}),
    ("cap-64", [], {"cap": 64}),
    ("texthr-negative", [], {"texthr": -1}),
    ("uniq-negative", [], {"uniq": -1}),
    ("mindisp-low", [], {"min_disp": -32769}),
]
SGBM_ONLY = [
    ("channels-2", [("cn", 2)], {}),
    ("mode-7", [], {"mode": 7}),
    ("numdisp-528", [], {"num_disp": 528}),
    ("block-13", [], {"block": 13}),
    ("mindisp-low", [], {"min_disp": -2048}),
    ("p1-negative", [], {"P1": -1}),
    ("p2-negative", [], {"P2": -1}),
    ("p1-8001", [], {"P1": 8001}),
    ("p2-16001", [], {"P2": 16001}),
]
for e in BM:
    for name, edits, params in COMMON + BM_ONLY:
        _case(name, e, edits, params)
    _case("block-not-smaller-than-image", e, params={"block": 13}, size=(32, 12))
    _case("one-pair-odd-pair-stride", e, [(p, "odd_pair") for p in ENTRIES[e][2]], accept=True)
for e in SGBM:
    for name, edits, params in COMMON + SGBM_ONLY:
        _case(name, e, edits, params)
    _case("bgr-left-short", e, [("left", "short")], cn=3)
    _case("census-bgr", e, cn=3, cost=(1, 7))
    _case("left-right-check-6401-columns", e, size=(6401, 24))
    _case("one-pair-odd-pair-stride", e, [("disp", "odd_pair")], accept=True)
    _case("one-pair-odd-pair-stride-bgr", e, [("disp", "odd_pair")], cn=3, accept=True)

# ---- device maps only: the pair stride of a CV_16S plane that a kernel indexes ----
for e in DEVICE:
    _case("two-pairs-odd-pair-stride", e, [("disp", "odd_pair")], n=2)
for e in ("adf_bm_compute_host", "adf_sgbm_compute_host"):
    _case("two-pairs-odd-pair-stride", e, [("disp", "odd_pair")], n=2, accept=True)
_case("two-pairs-odd-pair-stride", "adf_bm_compute_cost_host", [("disp", "odd_pair")], n=2, accept=True)   # (the cost plane's stays even)

# ---- the right map of the both-views entries ----
for e in ("adf_bm_compute_both_device", "adf_bm_compute_both_cost_device"):
    _case("disp-right-null", e, [("disp_right", "null")])
    for what in ("short", "odd_stride", "odd_ptr"):
        _case("disp-right-" + what.replace("_", "-"), e, [("disp_right", what)])
    _case("two-pairs-disp-right-odd-pair-stride", e, [("disp_right", "odd_pair")], n=2)
    # order: NULL disp_right before everything, the left map's pair stride before the right map
    _case("disp-right-null+handle-null", e, [("disp_right", "null"), ("handle", "null")])
    _case("disp-right-null+n-zero", e, [("disp_right", "null"), ("n", 0)])
    _case("disp-right-short+numdisp-zero", e, [("disp_right", "short")], {"num_disp": 0})
    _case("two-pairs-both-maps-odd-pair-stride", e, [("disp", "odd_pair"), ("disp_right", "odd_pair")], n=2)

# ---- the cost planes ----
for e, planes in (("adf_bm_compute_cost_device", ("cost",)), ("adf_bm_compute_cost_host", ("cost",)),
                  ("adf_bm_compute_both_cost_device", ("cost_left", "cost_right"))):
    for p in planes:
        tag = p.replace("_", "-")
        _case(tag + "-null", e, [(p, "null")])
        _case(tag + "-short", e, [(p, "short")])
        _case(tag + "-odd-stride", e, [(p, "odd_stride")])
        _case(tag + "-odd-ptr", e, [(p, "odd_ptr")])
        _case("two-pairs-" + tag + "-odd-pair-stride", e, [(p, "odd_pair")], n=2)
    first = planes[0]
    # double faults: which fault an entry reports first
    _case("handle-null+cost-null", e, [("handle", "null"), (first, "null")])
    _case("numdisp-24+cost-short", e, [(first, "short")], {"num_disp": 24})
    _case("disp-null+cost-odd-ptr", e, [("disp", "null"), (first, "odd_ptr")])
    _case("w-zero+cost-null", e, [("W", 0), (first, "null")])
    _case("two-pairs-disp-and-cost-odd-pair-stride", e, [("disp", "odd_pair"), (first, "odd_pair")], n=2)
_case("disp-right-null+cost-left-null", "adf_bm_compute_both_cost_device", [("disp_right", "null"), ("cost_left", "null")])
_case("cost-left-null+cost-right-short", "adf_bm_compute_both_cost_device", [("cost_left", "null"), ("cost_right", "short")])
_case("cost-right-null+disp-right-short", "adf_bm_compute_both_cost_device", [("cost_right", "null"), ("disp_right", "short")])
_case("cost-right-null+handle-null", "adf_bm_compute_both_cost_device", [("cost_right", "null"), ("handle", "null")])

# ---- more orders inside the shared checks ----
for e in BM + SGBM:
    _case("n-zero+w-zero", e, [("n", 0), ("W", 0)])
    _case("disp-short+numdisp-zero", e, [("disp", "short")], {"num_disp": 0})
    _case("disp-odd-ptr+block-even", e, [("disp", "odd_ptr")], {"block": 4})
for e in DEVICE:
    _case("two-pairs-odd-pair-stride+numdisp-zero", e, [("disp", "odd_pair")], {"num_disp": 0}, n=2)

CASE_NAMES = [c["name"] for c in CASES]
assert len(set(CASE_NAMES)) == len(CASES)

# Message format strings of the two host halves that no case reaches, each with its reason.
UNREACHED = {
    "out is NULL": "adf_*_create's, not a compute entry's",
    "no HIP device": "adf_*_create's, and a machine property",
    "out of host memory": "adf_*_create's, and a machine property",
    "%s": "the runtime's own message after a failed launch, not a rule of the call",
    "too many images per call for the cost kernel's grid":
        "reported between launches (the raw map is already being filled): not a refusal before a launch, and it takes 32768 pairs",
}


def source_messages():
    """The format string of every fail( in the C-ABI halves of the two matcher sources."""
    out = []
    for name in ("bm_matcher.hip", "sgbm_matcher.hip"):
        with open(os.path.join(CSRC, name)) as fh:
            text = fh.read()
        half = text[text.index("// C-ABI (include/adf_wls.h"):]
        found = re.findall(r'\bfail\(\s*ADF_\w+,\s*"((?:[^"\\]|\\.)*)"', half)
        assert found, name
        out += [(name, m) for m in found]
    return out


def message_matches(fmt, message):
    pattern = re.escape(fmt)
    for spec in ("%s", "%d"):
        pattern = pattern.replace(re.escape(spec), ".*")
    return re.fullmatch(pattern, message) is not None


def check_coverage(recorded):
    assert sorted(recorded) == sorted(CASE_NAMES), "the fixture and the case list differ"
    by = {c["name"]: c for c in CASES}
    for name, rec in recorded.items():
        assert (rec["rc"] == 0) == by[name]["accept"], name
    messages = {rec["error"] for rec in recorded.values() if rec["rc"] != 0}
    for src, fmt in source_messages():
        if fmt in UNREACHED:
            continue
        assert any(message_matches(fmt, m) for m in messages), "%s: no case reaches %r" % (src, fmt)
    # every message a case reaches through an entry of a matcher, it reaches through each entry of that matcher that
    # states the rule: the per-matcher lists above are applied to every entry, which this restates from the records
    for entries, names in ((BM, COMMON + BM_ONLY), (SGBM, COMMON + SGBM_ONLY)):
        for name, _, _ in names:
            seen = {recorded["%s:%s" % (SHORT[e], name)]["error"] for e in entries}
            assert len(seen) == 1, (name, seen)


# ---------------------------------------------------------------------------------------------------------------
# running a case
# ---------------------------------------------------------------------------------------------------------------
class _Plane:
    """n images of `rows` rows of `row` bytes in one flat byte buffer, SLACK bytes between and behind them."""

    def __init__(self, device, n, rows, row, fill):
        self.row, self.rows, self.n = row, rows, n
        self.stride, self.pair = row, rows * row + SLACK
        data = np.full(n * self.pair + SLACK, SENTINEL, np.uint8) if fill is None else fill
        if device:
            import torch
            self.buf = torch.from_numpy(data).cuda()
            self.ptr = self.buf.data_ptr()
        else:
            self.buf = data
            self.ptr = data.ctypes.data

    def edit(self, what, elem):
        if what == "null":
            self.ptr = None
        elif what == "odd_ptr":
            self.ptr += 1
        elif what == "short":
            self.stride = self.row - elem
        elif what == "odd_stride":
            self.stride = self.row + 1
        elif what == "odd_pair":
            self.pair -= 1
        else:
            raise ValueError(what)

    def bytes(self):
        return self.buf.cpu().numpy() if hasattr(self.buf, "cpu") else self.buf

    def images(self):
        """The n images as int16 arrays, and whether every other byte still holds the sentinel."""
        b = self.bytes().copy()
        out = []
        for k in range(self.n):
            lo = k * self.pair
            out.append(np.frombuffer(b[lo:lo + self.rows * self.row].tobytes(), np.int16).reshape(self.rows, self.row // 2))
            b[lo:lo + self.rows * self.row] = SENTINEL
        return out, bool((b == SENTINEL).all())


def _handle(L, case):
    kind = ENTRIES[case["entry"]][0]
    h = C.c_void_p()
    p = case["params"]
    if kind == "bm":
        assert L.adf_bm_create(C.byref(h), 16, 5) == 0
        assert L.adf_bm_set_params(h, p.get("min_disp", 0), p.get("num_disp", 16), p.get("block", 5), p.get("cap", 31),
                                   p.get("texthr", 10), p.get("uniq", 15)) == 0
        if case["cost"]:
            assert L.adf_bm_set_cost(h, *case["cost"]) == 0
    else:
        assert L.adf_sgbm_create(C.byref(h), 0, 16, 5) == 0
        assert L.adf_sgbm_set_params(h, p.get("min_disp", 0), p.get("num_disp", 16), p.get("block", 5), p.get("P1", 0),
                                     p.get("P2", 0), 0, 0, p.get("mode", 2)) == 0
        if case["cost"]:
            assert L.adf_sgbm_set_cost(h, *case["cost"]) == 0
    return h


def _call(L, case, edits):
    """One call of the case's entry with `edits` -> (rc, message, {plane name: _Plane})."""
    kind, device, outs = ENTRIES[case["entry"]]
    w, h = case["size"]
    n, cn = case["n"], case["cn"]
    rng = np.random.default_rng(5)
    views = {}
    for side in ("left", "right"):
        data = rng.integers(0, 256, n * (h * w * cn + SLACK) + SLACK, dtype=np.uint8)
        views[side] = _Plane(device, n, h, w * cn, data)
    planes = {name: _Plane(device, n, h, w * 2, None) for name in outs}
    scalars = {"n": n, "W": w, "H": h, "cn": cn}
    handle = _handle(L, case)
    passed = handle
    for slot, what in edits:
        if slot == "handle":
            passed = None
        elif slot in scalars:
            scalars[slot] = what
        elif slot in views:
            views[slot].edit(what, 1)
        else:
            planes[slot].edit(what, 2)
    args = [passed, scalars["n"]]
    for side in ("left", "right"):
        args += [views[side].ptr, views[side].stride, views[side].pair]
    if kind == "sgbm":
        args.append(scalars["cn"])
    args += [scalars["W"], scalars["H"]]
    for name in outs:
        args += [planes[name].ptr, planes[name].stride, planes[name].pair]
    if device:
        args.append(None)                              # the null stream
    try:
        rc = getattr(L, case["entry"])(*args)
        message = L.adf_last_error().decode("utf-8", "replace") if rc else ""
        if device:
            import torch
            torch.cuda.synchronize()
    finally:
        getattr(L, "adf_%s_destroy" % kind)(handle)
    return rc, message, planes


def run_case(lib, case):
    """Run `case` and return its record; raises when an output was touched by a refused call, or when an accepted
    call's maps differ from the dense call's or its padding lost the sentinel."""
    rc, message, planes = _call(lib, case, case["edits"])
    if not case["accept"]:
        for name, p in planes.items():
            assert (p.bytes() == SENTINEL).all(), "%s: %s was written by a refused call" % (case["name"], name)
        return dict(rc=rc, error=message)
    assert rc == 0, (case["name"], rc, message)
    drc, _, dense = _call(lib, case, ())
    assert drc == 0
    for name, p in planes.items():
        got, clean = p.images()
        exp, _ = dense[name].images()
        assert clean, "%s: %s was written outside its images" % (case["name"], name)
        assert all(np.array_equal(g, e) for g, e in zip(got, exp)), "%s: %s differs from the dense call's" % (case["name"], name)
        assert not (np.stack(exp).view(np.uint8) == SENTINEL).all()          # the dense call wrote its maps
    return dict(rc=rc)


def _record(path):
    sys.path.insert(0, ROOT)
    from addingdisparityfiltering_amd import _lib

    recorded = {}
    for case in CASES:
        recorded[case["name"]] = run_case(_lib.lib(), case)
        print(case["name"], json.dumps(recorded[case["name"]]), flush=True)
    check_coverage(recorded)
    with open(path, "w") as fh:
        json.dump(recorded, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", path, len(recorded), "cases")


if __name__ == "__main__":
    _record(sys.argv[1] if len(sys.argv) > 1 else FIXTURE)
