"""The case matrix of tests/test_filter_refusals.py and the recorder of its fixture.

The five stateless edge-aware filters -- weightedMedianFilter, guidedFilter, dtFilter, jointBilateralFilter and
rollingGuidanceFilter (include/adf_wls.h) -- refuse a bad call before a device is touched, so all of this runs without
a GPU.  Section one: a case is ONE direct ctypes call of one of the ten adf_*_{device,host} entries on 6 x 8 maps (as
in tests/test_*_abi.py); recorded are the return code and adf_last_error(), both exact.  The destination and a caller
workspace are prefilled with a sentinel byte and must come back untouched.  Section two: the Python mirror
(addingdisparityfiltering_amd/ximgproc.py) on numpy inputs; recorded are the code and the text of every AdfError the
five functions, their create* objects and the choice parsers (weightType, mode, borderType) raise themselves.

    python tests/filter_refusal_cases.py [output.json]

recorded tests/filter_refusals.json ONCE, from the host halves as they were BEFORE the five filters were given one
image record, one geometry check and one staged call (csrc/adf_host.h).  The fixture is never recorded again from later
code: a difference is a bug in that code.  (Twelve entries -- the NULL joint, the joint's short row stride and its
negative map stride of weightedMedianFilter and jointBilateralFilter -- were recorded later, from a library built from
that same earlier code: the matrix had named their edits by a key run_case did not read, so the calls went out
unedited.  An edit that names nothing of the call now fails where the case is defined, and a return code other than
ADF_EBADARG or ADF_ESIZE fails the case, the recorder and check_coverage: a device's answer is never a refusal.)

The matrix takes every fail( of the five checks, and of what they call (border_check, jbf_params_check,
rgf_params_check, wmf_weights_check, the domain transform's params_check, the two workspace_or_scratch refusals that
need no device, the rolling guidance filter's workspace-overlap refusal), through both entry kinds.  Double faults pin
the ORDER in which an entry reports: one per filter sits at each seam between its own head and the tail all five share
(alignment, W*H, row strides, map strides, destination maps, overlap).  test_every_message_is_pinned greps the five
sources and the shared check and fails on a message that no case reaches; UNREACHED may only list messages that cannot
occur without a device, and is empty: none of these sources words one itself.
"""
import ctypes as C
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "filter_refusals.json")
CSRC = os.path.join(ROOT, "addingdisparityfiltering_amd", "csrc")
SOURCES = ("wmf_kernels.hip", "guided_filter_kernels.hip", "dt_filter_kernels.hip", "joint_bilateral_kernels.hip",
           "rolling_guidance_kernels.hip")
SHARED_CHECK = "int adf::filter_geometry_check("       # in adf_host.hip; the recorded code had five copies instead

W, H = 8, 6
SENTINEL = 0x5A
U8, S16, S32, F32 = 0, 3, 4, 5
ES = {U8: 1, S16: 2, F32: 4}
NAN, INF = float("nan"), float("inf")
REFUSALS = (1, 2)                                      # ADF_EBADARG, ADF_ESIZE: what a check returns; anything else came from a device

# filter -> (entry base name, the name of its guide image or None, has a mask, has a dst depth, its own parameters in
# argument order with the values of a call that would be accepted, the workspace-size function of its device entry)
FILTERS = {
    "wmf": ("adf_weighted_median_filter", "joint", True, False, dict(r=2, sigma=25.5, wt=0), None),
    "gf": ("adf_guided_filter", "guide", False, True, dict(r=2, eps=1.0), "adf_guided_filter_workspace_bytes"),
    "dt": ("adf_dt_filter", "guide", False, True, dict(ss=10.0, sc=20.0, mode=2, iters=3), "adf_dt_filter_workspace_bytes"),
    "jbf": ("adf_joint_bilateral_filter", "joint", False, True, dict(d=5, sc=20.0, ss=2.0, border=4), None),
    "rgf": ("adf_rolling_guidance_filter", None, False, False, dict(d=5, sc=20.0, ss=2.0, iters=3, border=4),
            "adf_rolling_guidance_workspace_bytes"),
}
KINDS = ("device", "host")

# A case's edits: a dict.  Keys "n", "W", "H", "gch", "sdepth", "ddepth", "use_ignore", "ignore" and the filter's own
# parameters replace a scalar.  An image name ("guide" -- the joint of wmf / jbf --, "src", "dst", "mask") takes one or
# more of: "null", "odd_ptr" (+1 byte), "ptr2" (+2 bytes), "short" (row stride one element less than a row),
# "odd_stride" (+1 byte), "odd_map" (map stride +1 byte), "neg_map" (map stride negated), "map_short" (map stride one
# element less than a map), "present" (the mask: given), ("at", other) (the pointer of image `other`).  "ws" (device
# entries): "small" (one byte less than the size function says), "odd" (+1 byte), ("at", image).
CASES = []


SCALARS = ("n", "W", "H", "gch", "sdepth", "ddepth", "use_ignore", "ignore")
IMAGES = ("guide", "src", "dst", "mask")


def _case(f, name, **edits):
    unknown = set(edits) - set(SCALARS) - set(IMAGES) - set(FILTERS[f][4]) - {"ws"}
    assert not unknown, "%s:%s: edits %s name nothing of the call" % (f, name, sorted(unknown))   # (a dropped edit is an accepted call)
    for kind in KINDS:
        if "ws" in edits and kind == "host":
            continue
        CASES.append(dict(name="%s-%s:%s" % (f, kind, name), filter=f, kind=kind, edits=edits))


HUGE = dict(W=65536, H=32768)                          # W*H = 2^31; nothing is read before the refusal
for f, (_, guide, has_mask, has_ddepth, params, ws_fn) in FILTERS.items():
    # ---- the head every filter words itself: NULL, empty, depths, channels ----
    role = {"guide": guide}                                # an edit names the guide "guide"; a case by the filter's word for it
    for im in (["guide"] if guide else []) + ["src", "dst"]:
        _case(f, role.get(im, im) + "-null", **{im: ["null"]})
    for k in ("n", "W", "H"):
        _case(f, k.lower() + "-zero", **{k: 0})
    _case(f, "n-negative", n=-3)
    _case(f, "sdepth-32s", sdepth=S32)
    if has_ddepth:
        _case(f, "ddepth-32s", ddepth=S32)
    if guide:
        _case(f, "channels-2", gch=2)
    # ---- the tail all five share, one fault each, and its order ----
    _case(f, "src-odd-ptr", src=["odd_ptr"])
    _case(f, "dst-odd-ptr", dst=["odd_ptr"])
    _case(f, "src-odd-stride", src=["odd_stride"])
    _case(f, "dst-odd-map", dst=["odd_map"])
    _case(f, "float-src-ptr2", sdepth=F32, src=["ptr2"], **({} if has_ddepth else {"ddepth": F32}))
    _case(f, "w-times-h", **HUGE)
    for im in ["src", "dst"] + (["guide"] if guide else []) + (["mask"] if has_mask else []):
        _case(f, role.get(im, im) + "-short", **{im: ["present", "short"] if im == "mask" else ["short"]})
    if guide:
        _case(f, "three-channels-short", gch=3, guide=["short"])
    for im in ["src"] + (["guide"] if guide else []) + (["mask"] if has_mask else []):
        _case(f, role.get(im, im) + "-negative-map", n=2, **{im: ["present", "neg_map"] if im == "mask" else ["neg_map"]})
    _case(f, "one-map-negative-map+dst-on-src", src=["neg_map"], dst=[("at", "src")])       # (one map: the stride is not read)
    _case(f, "dst-maps-overlap", n=2, dst=["map_short"])
    _case(f, "dst-on-src", dst=[("at", "src")])
    if guide:
        _case(f, "dst-on-" + guide, sdepth=U8, ddepth=U8, dst=[("at", "guide")])
    if has_mask:
        _case(f, "dst-on-mask", sdepth=U8, mask=["present"], dst=[("at", "mask")])
    _case(f, "misaligned+w-times-h", src=["odd_ptr"], **HUGE)
    _case(f, "w-times-h+src-short", src=["short"], **HUGE)
    _case(f, "src-short+negative-map", n=2, src=["short", "neg_map"])
    _case(f, "negative-map+dst-maps-overlap", n=2, src=["neg_map"], dst=["map_short"])
    _case(f, "dst-maps-overlap+dst-on-src", n=2, dst=["map_short", ("at", "src")])
    # ---- the caller's workspace (device entries) ----
    if ws_fn:
        _case(f, "workspace-small", ws="small")
        _case(f, "workspace-odd", ws="odd")
        _case(f, "src-odd-ptr+workspace-small", src=["odd_ptr"], ws="small")

# ---- each filter's own parameters, and the seam between its head and the shared tail ----
for wt in (1, 2, 3, 4, 6, -1):
    _case("wmf", "weight-type-%d" % wt, wt=wt)
for name, sigma in (("zero", 0.0), ("negative", -1.0), ("nan", NAN), ("inf", INF)):
    _case("wmf", "sigma-" + name, sigma=sigma)
for r in (0, 32, -1):
    _case("wmf", "r-%d" % r, r=r)
for name, depth, v in (("fraction", S16, 0.5), ("below-int16", S16, -32769.0), ("above-uint8", U8, 256.0), ("nan", S16, NAN)):
    _case("wmf", "ignore-" + name, sdepth=depth, use_ignore=1, ignore=v)
_case("wmf", "channels-2+weight-type-1", gch=2, wt=1)
_case("wmf", "weight-type-1+sigma-zero", wt=1, sigma=0.0)
_case("wmf", "sigma-zero+r-0", sigma=0.0, r=0)
_case("wmf", "r-0+ignore-fraction", r=0, use_ignore=1, ignore=0.5)
_case("wmf", "ignore-fraction+src-short", use_ignore=1, ignore=0.5, src=["short"])          # the seam
_case("wmf", "ignore-fraction+src-odd-ptr", use_ignore=1, ignore=0.5, src=["odd_ptr"])       # the seam
_case("wmf", "mask-short+dst-on-mask", sdepth=U8, mask=["present", "short"], dst=[("at", "mask")])

for r in (-1, 32, 1 << 20):
    _case("gf", "r-%d" % r, r=r)
for name, eps in (("zero", 0.0), ("negative", -1.0), ("nan", NAN), ("inf", INF)):
    _case("gf", "eps-" + name, eps=eps)
_case("gf", "channels-2+r-32", gch=2, r=32)
_case("gf", "r-32+eps-zero", r=32, eps=0.0)
_case("gf", "r-32+src-odd-ptr", r=32, src=["odd_ptr"])                                       # the seam
_case("gf", "eps-zero+src-odd-ptr", eps=0.0, src=["odd_ptr"])                                # the seam
_case("gf", "ddepth-32s+r-32", ddepth=S32, r=32)

for mode in (0, 1, 3, -1):
    _case("dt", "mode-%d" % mode, mode=mode)
_case("dt", "sigma-spatial-nan", ss=NAN)
_case("dt", "sigma-color-inf", sc=INF)
_case("dt", "sigma-color-beyond-float32", sc=1e300)
_case("dt", "iters-9", iters=9)
_case("dt", "mode-0+src-null", mode=0, src=["null"])                                        # mode first
_case("dt", "mode-3+n-zero", mode=3, n=0)
_case("dt", "sdepth-32s+channels-2", sdepth=S32, gch=2)
_case("dt", "channels-2+sigma-nan", gch=2, ss=NAN)
_case("dt", "sigma-nan+iters-9", ss=NAN, iters=9)
_case("dt", "iters-9+src-odd-ptr", iters=9, src=["odd_ptr"])                                # the seam

_case("jbf", "joint-is-src", guide=[("at", "src")])
_case("jbf", "joint-is-src+n-zero", guide=[("at", "src")], n=0)
_case("jbf", "sigma-color-nan", sc=NAN)
_case("jbf", "sigma-space-beyond-float32", ss=1e300)
_case("jbf", "d-64", d=64)
_case("jbf", "d-zero-sigma-space-25", d=0, ss=25.0)
for b in (0, 3, 5, 16, -1):
    _case("jbf", "border-%d" % b, border=b)
_case("jbf", "sdepth-32s+channels-2", sdepth=S32, gch=2)
_case("jbf", "channels-2+sigma-nan", gch=2, sc=NAN)
_case("jbf", "d-64+border-0", d=64, border=0)
_case("jbf", "border-0+src-odd-ptr", border=0, src=["odd_ptr"])                             # the seam
_case("jbf", "border-5+dst-odd-ptr", border=5, dst=["odd_ptr"])                             # the seam

_case("rgf", "sigma-color-nan", sc=NAN)
_case("rgf", "d-64", d=64)
_case("rgf", "float-sigma-color-tiny", sdepth=F32, ddepth=F32, sc=1e-40)
for it in (-1, 17):
    _case("rgf", "iters-%d" % it, iters=it)
for b in (0, 3, 5):
    _case("rgf", "border-%d" % b, border=b)
_case("rgf", "n-zero+sdepth-32s", n=0, sdepth=S32)
_case("rgf", "d-64+iters-17", d=64, iters=17)
_case("rgf", "iters-17+border-0", iters=17, border=0)
_case("rgf", "border-0+src-odd-ptr", border=0, src=["odd_ptr"])                             # the seam
_case("rgf", "border-5+w-times-h", border=5, **HUGE)                                        # the seam
_case("rgf", "workspace-on-src", ws=("at", "src"))
_case("rgf", "workspace-on-dst", ws=("at", "dst"))
_case("rgf", "small-workspace-on-src", ws=("small-at", "src"))                               # too small is said first
_case("rgf", "dst-on-src+workspace-on-src", dst=[("at", "src")], ws=("at", "src"))

# ---- the table functions the sources word themselves ----
TABLE_CASES = {
    "dt-table:null": ("adf_dt_rf_table_host", (10.0, 20.0, 3, 1, None)),
    "dt-table:channels-2": ("adf_dt_rf_table_host", (10.0, 20.0, 3, 2, "out")),
    "dt-table:sigma-nan": ("adf_dt_rf_table_host", (NAN, 20.0, 3, 1, "out")),
    "dt-table:iters-9": ("adf_dt_rf_table_host", (10.0, 20.0, 9, 1, "out")),
}

CASE_NAMES = [c["name"] for c in CASES]
assert len(set(CASE_NAMES)) == len(CASES)

# Message format strings of the five sources that no case reaches, each with its reason: only what cannot occur
# without a device (a HIP error, scratch refused inside a stream capture, an allocation failure) may stand here.
UNREACHED = {}


# ---------------------------------------------------------------------------------------------------------------
# running a C case
# ---------------------------------------------------------------------------------------------------------------
class _Img:
    """One image of a call: two maps' worth of sentinel bytes (4 bytes a pixel, 3 channels at most) behind a pointer."""

    def __init__(self):
        self.buf = np.full(2 * H * W * 4 * 3 + 64, SENTINEL, np.uint8)
        self.ptr = (self.buf.ctypes.data + 15) & ~15
        self.given = True

    def lay_out(self, width, height, es):
        self.es, self.stride = es, width * es
        self.map = height * self.stride

    def edit(self, what, images):
        if isinstance(what, tuple):
            self.ptr = images[what[1]].ptr
        elif what == "null":
            self.ptr = None
        elif what == "odd_ptr":
            self.ptr += 1
        elif what == "ptr2":
            self.ptr += 2
        elif what == "short":
            self.stride -= self.es
        elif what == "odd_stride":
            self.stride += 1
        elif what == "odd_map":
            self.map += 1
        elif what == "neg_map":
            self.map = -self.map
        elif what == "map_short":
            self.map -= self.es
        elif what == "present":
            self.given = True
        else:
            raise ValueError(what)

    def args(self):
        return (self.ptr, self.stride, self.map) if self.given else (None, 0, 0)

    def clean(self):
        return bool((self.buf == SENTINEL).all())


def run_case(lib, case):
    """Run `case` and return its record; raises when a refused call wrote its destination or its workspace."""
    base, guide, has_mask, has_ddepth, params, ws_fn = FILTERS[case["filter"]]
    e = dict(case["edits"])
    assert set(e) <= set(SCALARS) | set(IMAGES) | set(params) | {"ws"}, case["name"]
    s = dict(n=1, W=W, H=H, gch=1, sdepth=S16, ddepth=S16, use_ignore=0, ignore=0.0, **params)
    if not has_ddepth and "sdepth" in e:
        e.setdefault("ddepth", e["sdepth"])                   # one depth for both
    s.update({k: v for k, v in e.items() if k in s})
    im = {k: _Img() for k in IMAGES}
    im["mask"].given = False
    im["guide"].lay_out(s["W"], s["H"], s["gch"])
    im["src"].lay_out(s["W"], s["H"], ES.get(s["sdepth"], 2))
    im["dst"].lay_out(s["W"], s["H"], ES.get(s["ddepth"], 2))
    im["mask"].lay_out(s["W"], s["H"], 1)
    for name in ("guide", "src", "mask", "dst"):             # (dst last: it may take another image's pointer)
        for what in e.get(name, ()):
            im[name].edit(what, im)
    f = case["filter"]
    G, S, D, M = (im[k].args() for k in ("guide", "src", "dst", "mask"))
    size = (s["W"], s["H"])
    if f == "wmf":
        args = (s["n"],) + G + (s["gch"],) + S + (s["sdepth"],) + D + size + (s["r"], s["sigma"], s["wt"]) + M + (s["use_ignore"], s["ignore"])
    elif f == "gf":
        args = (s["n"],) + G + (s["gch"],) + S + (s["sdepth"],) + D + (s["ddepth"],) + size + (s["r"], s["eps"])
    elif f == "dt":
        args = (s["n"],) + G + (s["gch"],) + S + (s["sdepth"],) + D + (s["ddepth"],) + size + (s["ss"], s["sc"], s["mode"], s["iters"])
    elif f == "jbf":
        args = (s["n"],) + G + (s["gch"],) + S + (s["sdepth"],) + D + (s["ddepth"],) + size + (s["d"], s["sc"], s["ss"], s["border"])
    else:
        args = (s["n"],) + S + D + (s["sdepth"],) + size + (s["d"], s["sc"], s["ss"], s["iters"], s["border"])
    ws = _Img()
    if case["kind"] == "device":
        if ws_fn:
            how = e.get("ws")
            need = {"adf_guided_filter_workspace_bytes": lambda: lib.adf_guided_filter_workspace_bytes(s["n"], s["W"], s["H"], s["gch"]),
                    "adf_dt_filter_workspace_bytes": lambda: lib.adf_dt_filter_workspace_bytes(s["n"], s["W"], s["H"]),
                    "adf_rolling_guidance_workspace_bytes": lambda: lib.adf_rolling_guidance_workspace_bytes(s["n"], s["W"], s["H"], s["sdepth"], s["iters"])}[ws_fn]()
            if how is None:
                args += (None, 0)
            else:
                assert need > 1
                where = im[how[1]].ptr if isinstance(how, tuple) else ws.ptr + (1 if how == "odd" else 0)
                small = how == "small" or (isinstance(how, tuple) and how[0] == "small-at")
                args += (where, need - 1 if small else need)
        args += (None,)                                       # the null stream
    rc = getattr(lib, "%s_%s" % (base, case["kind"]))(*args)
    message = lib.adf_last_error().decode("utf-8", "replace") if rc else ""
    assert rc in REFUSALS, "%s: rc %d (%s): not a refusal of the call's arguments" % (case["name"], rc, message)
    assert im["dst"].clean() and ws.clean(), "%s: a refused call wrote its destination or workspace" % case["name"]
    return dict(rc=rc, error=message)


def run_table_case(lib, name):
    fn, args = TABLE_CASES[name]
    out = np.full(8 * 766, SENTINEL, np.uint8)
    rc = getattr(lib, fn)(*[out.ctypes.data if a == "out" else a for a in args])
    assert rc in REFUSALS and (out == SENTINEL).all(), name
    return dict(rc=rc, error=lib.adf_last_error().decode("utf-8", "replace"))


# ---------------------------------------------------------------------------------------------------------------
# the Python mirror, numpy inputs
# ---------------------------------------------------------------------------------------------------------------
def python_cases(adf):
    """name -> a call that must raise AdfError: what ximgproc.py refuses itself for the five filters, numpy inputs."""
    g8, s16 = np.zeros((H, W), np.uint8), np.zeros((H, W), np.int16)
    g2 = np.zeros((H, W, 2), np.uint8)
    wide = np.zeros((H, W + 1), np.uint8)
    tall16 = np.zeros((H + 1, W), np.int16)
    f32 = np.zeros((H, W), np.float32)
    ws = np.zeros(4096, np.uint8)
    out = {}
    # the stanza the five share, worded per filter: each filter's call with src / guide / dst / dDepth replaced
    calls = {
        "wmf": lambda src=s16, guide=g8, **kw: adf.weightedMedianFilter(guide, src, 2, **kw),
        "gf": lambda src=s16, guide=g8, **kw: adf.guidedFilter(guide, src, 2, 1.0, **kw),
        "dt": lambda src=s16, guide=g8, **kw: adf.dtFilter(guide, src, 10.0, 20.0, **kw),
        "jbf": lambda src=s16, guide=g8, **kw: adf.jointBilateralFilter(guide, src, 5, 20.0, 2.0, **kw),
        "rgf": lambda src=s16, guide=None, **kw: adf.rollingGuidanceFilter(src, **kw),
    }
    for f, call in calls.items():
        add = lambda name, fn, f=f: out.__setitem__("%s:%s" % (f, name), fn)
        add("src-none", lambda call=call: call(src=None))
        add("src-1d", lambda call=call: call(src=np.zeros(W, np.int16)))
        add("src-4d", lambda call=call: call(src=np.zeros((2, 3, H, W), np.int16)))
        add("src-int32", lambda call=call: call(src=s16.astype(np.int32)))
        add("src-float64", lambda call=call: call(src=s16.astype(np.float64)))
        add("src-empty", lambda call=call: call(src=np.zeros((0, W), np.int16)))
        add("dst-taller", lambda call=call: call(dst=tall16))
        add("dst-other-dtype", lambda call=call: call(dst=f32))
        add("dst-batched", lambda call=call: call(dst=np.zeros((2, H, W), np.int16)))
        add("dst-is-src", lambda call=call: call(dst=s16))
        add("src-odd-address", lambda call=call: call(src=np.zeros((H, 2 * W + 1), np.uint8)[:, 1:].view(np.int16)))
        if f != "rgf":
            add("guide-none", lambda call=call: call(guide=None))
            add("guide-2-channels", lambda call=call: call(guide=g2))
            add("guide-int16", lambda call=call: call(guide=s16.copy()))
            add("guide-float32", lambda call=call: call(guide=f32))
            add("guide-wider", lambda call=call: call(guide=wide))
            add("guide-batched", lambda call=call: call(guide=np.zeros((2, H, W), np.uint8)))
            add("guide-not-dense", lambda call=call: call(guide=np.zeros((H, 2 * W), np.uint8)[:, ::2]))
        if f in ("gf", "dt", "jbf"):
            add("ddepth-32s", lambda call=call: call(dDepth=4))
            add("ddepth-6", lambda call=call: call(dDepth=6))
            add("ddepth-32f-dst-int16", lambda call=call: call(dDepth=adf.CV_32F, dst=np.zeros((H, W), np.int16)))
        if f in ("gf", "dt", "rgf"):
            add("workspace-numpy", lambda call=call: call(workspace=ws))
    # each filter's own refusals
    out["wmf:mask-wider"] = lambda: adf.weightedMedianFilter(g8, s16, 2, mask=wide)
    out["wmf:mask-int16"] = lambda: adf.weightedMedianFilter(g8, s16, 2, mask=s16.copy())
    out["wmf:r-0"] = lambda: adf.weightedMedianFilter(g8, s16, 0)
    out["wmf:sigma-zero"] = lambda: adf.weightedMedianFilter(g8, s16, 2, sigma=0.0)
    out["wmf:ignore-fraction"] = lambda: adf.weightedMedianFilter(g8, s16, 2, ignoreValue=0.5)
    for wt in (1, 2, 3, 4, 6, -1, "x", None):
        out["wmf:weight-type-%s" % wt] = lambda wt=wt: adf.weightedMedianFilter(g8, s16, 2, weightType=wt)
        out["wmf-table:weight-type-%s" % wt] = lambda wt=wt: adf.wmfWeightTable(25.5, wt)
    out["wmf-table:sigma-zero"] = lambda: adf.wmfWeightTable(0.0)
    out["wmf:weight-type-1+src-1d"] = lambda: adf.weightedMedianFilter(g8, np.zeros(W, np.int16), 2, weightType=1)
    out["gf:r-32"] = lambda: adf.guidedFilter(g8, s16, 32, 1.0)
    out["gf:eps-zero"] = lambda: adf.guidedFilter(g8, s16, 2, 0.0)
    out["gf-create:guide-none"] = lambda: adf.createGuidedFilter(None, 2, 1.0)
    out["gf-create:r-32"] = lambda: adf.createGuidedFilter(g8, 32, 1.0)
    out["gf-create:r-negative"] = lambda: adf.createGuidedFilter(g8, -1, 1.0)
    for name, eps in (("zero", 0.0), ("nan", NAN), ("inf", INF)):
        out["gf-create:eps-" + name] = lambda eps=eps: adf.createGuidedFilter(g8, 2, eps)
    out["gf-create:filter-src-int32"] = lambda: adf.createGuidedFilter(g8, 2, 1.0).filter(s16.astype(np.int32))
    for m in (0, 1, 3, -1, "x", None):
        out["dt:mode-%s" % m] = lambda m=m: adf.dtFilter(g8, s16, 10.0, 20.0, mode=m)
        out["dt-create:mode-%s" % m] = lambda m=m: adf.createDTFilter(g8, 10.0, 20.0, mode=m)
    out["dt:mode-0+src-1d"] = lambda: adf.dtFilter(g8, np.zeros(W, np.int16), 10.0, 20.0, mode=0)
    out["dt:sigma-nan"] = lambda: adf.dtFilter(g8, s16, NAN, 20.0)
    out["dt:iters-9"] = lambda: adf.dtFilter(g8, s16, 10.0, 20.0, numIters=9)
    out["dt-create:guide-none"] = lambda: adf.createDTFilter(None, 10.0, 20.0)
    out["dt-create:sigma-nan"] = lambda: adf.createDTFilter(g8, NAN, 20.0)
    out["dt-create:sigma-inf"] = lambda: adf.createDTFilter(g8, 10.0, INF)
    out["dt-create:iters-9"] = lambda: adf.createDTFilter(g8, 10.0, 20.0, numIters=9)
    out["dt-create:filter-dst-taller"] = lambda: adf.createDTFilter(g8, 10.0, 20.0).filter(s16, dst=tall16)
    out["dt-table:iters-9"] = lambda: adf.dtRfTable(10.0, 20.0, 9)
    out["dt-table:channels-2"] = lambda: adf.dtRfTable(10.0, 20.0, 3, 2)
    out["dt-table:sigma-nan"] = lambda: adf.dtRfTable(NAN, 20.0)
    for b in (0, 3, 5, 16, -1, "x", None):
        out["jbf:border-%s" % b] = lambda b=b: adf.jointBilateralFilter(g8, s16, 5, 20.0, 2.0, borderType=b)
        out["rgf:border-%s" % b] = lambda b=b: adf.rollingGuidanceFilter(s16, borderType=b)
    out["jbf:joint-is-src"] = lambda: adf.jointBilateralFilter(g8, g8, 5, 20.0, 2.0)
    out["jbf:joint-is-src+border-0"] = lambda: adf.jointBilateralFilter(g8, g8, 5, 20.0, 2.0, borderType=0)
    out["jbf:border-0+src-1d"] = lambda: adf.jointBilateralFilter(g8, np.zeros(W, np.int16), 5, 20.0, 2.0, borderType=0)
    out["jbf:src-int32+joint-float32"] = lambda: adf.jointBilateralFilter(f32, s16.astype(np.int32), 5, 20.0, 2.0)
    out["jbf:joint-float32+ddepth-6"] = lambda: adf.jointBilateralFilter(f32, s16, 5, 20.0, 2.0, dDepth=6)
    out["jbf:d-64"] = lambda: adf.jointBilateralFilter(g8, s16, 64, 20.0, 2.0)
    out["jbf:sigma-nan"] = lambda: adf.jointBilateralFilter(g8, s16, 5, NAN, 2.0)
    out["jbf-tables:channels-2"] = lambda: adf.jbfTables(5, 20.0, 2.0, 2)
    out["rgf:iters-17"] = lambda: adf.rollingGuidanceFilter(s16, numOfIter=17)
    out["rgf:border-0+src-1d"] = lambda: adf.rollingGuidanceFilter(np.zeros(W, np.int16), borderType=0)
    out["rgf:dst-is-src+dst-taller"] = lambda: adf.rollingGuidanceFilter(tall16, dst=tall16)
    out["rgf-tables:depth-int32"] = lambda: adf.rgfTables(np.int32, 5, 20.0, 2.0)
    out["rgf-workspace:depth-int32"] = lambda: adf.rollingGuidanceWorkspaceBytes(1, H, W, np.int32, 3)
    return out


def run_python_case(adf, fn):
    try:
        fn()
    except adf.AdfError as err:
        text = str(err)
        head = "adf error %d: " % err.code
        assert text.startswith(head)
        return dict(code=err.code, error=text[len(head):])
    raise AssertionError("the call was accepted")


# ---------------------------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------------------------
def source_messages(require_shared=True):
    """(source, format string) of every fail( in the five sources and in the check they share (adf_host.hip)."""
    out = []
    pattern = r'\bfail\(\s*ADF_\w+,\s*"((?:[^"\\]|\\.)*)"'
    for name in SOURCES:
        with open(os.path.join(CSRC, name)) as fh:
            found = re.findall(pattern, fh.read())
        assert found, name
        out += [(name, m) for m in found]
    with open(os.path.join(CSRC, "adf_host.hip")) as fh:
        text = fh.read()
    if SHARED_CHECK in text:
        body = text[text.index(SHARED_CHECK):]
        found = re.findall(pattern, body[:body.index("\n}\n")])
        assert len(found) >= 6, found                         # alignment, W*H, rows, map strides, destination maps, overlap
        out += [("adf_host.hip", m) for m in found]
    else:
        assert not require_shared, "adf_host.hip: the shared check is gone"
    return out


def message_matches(fmt, message):
    pattern = re.escape(fmt)
    for spec in ("%s", "%d", "%g"):
        pattern = pattern.replace(re.escape(spec), ".*")
    return re.fullmatch(pattern, message) is not None


def check_coverage(recorded, require_shared=True):
    assert sorted(recorded["c"]) == sorted(CASE_NAMES + list(TABLE_CASES)), "the fixture and the case list differ"
    assert all(set(UNREACHED[m]) for m in UNREACHED)
    for name, rec in recorded["c"].items():                   # a refusal of the arguments, never a device's answer
        assert rec["rc"] in REFUSALS and "HIP" not in rec["error"], (name, rec)
    messages = {rec["error"] for rec in recorded["c"].values()}
    for src, fmt in source_messages(require_shared):
        if fmt in UNREACHED:
            continue
        assert any(message_matches(fmt, m) for m in messages), "%s: no case reaches %r" % (src, fmt)
    # both entry kinds of a filter say the same thing in the same case
    for c in CASES:
        if c["kind"] == "host":
            dev = c["name"].replace("-host:", "-device:")
            assert recorded["c"][dev] == recorded["c"][c["name"]], c["name"]


def _record(path):
    sys.path.insert(0, ROOT)
    import addingdisparityfiltering_amd as adf
    from addingdisparityfiltering_amd import _lib

    recorded = {"c": {}, "python": {}}
    for case in CASES:
        recorded["c"][case["name"]] = run_case(_lib.lib(), case)
    for name in TABLE_CASES:
        recorded["c"][name] = run_table_case(_lib.lib(), name)
    for name, fn in python_cases(adf).items():
        recorded["python"][name] = run_python_case(adf, fn)
    for section in ("c", "python"):
        for name, rec in recorded[section].items():
            print(name, json.dumps(rec), flush=True)
    check_coverage(recorded, require_shared=False)
    with open(path, "w") as fh:
        json.dump(recorded, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", path, len(recorded["c"]), "C cases,", len(recorded["python"]), "Python cases")


if __name__ == "__main__":
    _record(sys.argv[1] if len(sys.argv) > 1 else FIXTURE)
