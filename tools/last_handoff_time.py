"""The row -> column hand-offs as the column pass's register image against the pair plane, by chunk size: batches of
4K pairs (BASELINE config 3: 3840 x 2160, ROI (256, 0, 3584, 2160), radius 2) on three handles of ONE build in one
process -- "all" made under ADF_LAST_HANDOFF_MIN_PX=0 (every hand-off takes the image whatever the chunk), "last" with
ADF_INNER_HANDOFF_IMAGE=0 beside it (the last hand-off only), "none" under ADF_LAST_HANDOFF_IMAGE=0.
The three alternate round by round behind a warm-up of all; every call is bracketed by HIP events, and a second series
with the profile hook on gives the four pass classes (pass_h_first and pass_h write the hand-offs, pass_v and
pass_v_last read them).
This is the series the plan's size threshold (HANDOFF_IMAGE_MIN_PX, adf_api.hip) comes from.

    python tools/last_handoff_time.py [--pairs 1,2,3,4,6,8] [--rounds R]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import addingdisparityfiltering_amd as adf                     # noqa: E402
from addingdisparityfiltering_amd import synthetic             # noqa: E402


def handle(env, radius):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        f = adf.createDisparityWLSFilterGeneric(True)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    f.setLambda(8000.0); f.setSigmaColor(1.5); f.setDepthDiscontinuityRadius(radius)
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="1,2,3,4,6,8")
    ap.add_argument("--rounds", type=int, default=12)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    c = synthetic.CONFIGS[3]
    roi_px1 = c["roi"][2] * c["roi"][3]
    print("pairs of %d x %d, ROI %s, %d rounds, alternating handles; ms per call: median (min .. max)" % (c["W"], c["H"], c["roi"], a.rounds))
    for n in [int(x) for x in a.pairs.split(",")]:
        view, dl, dr = synthetic.make_artificial_batch_torch(n, c["W"], c["H"], c["channels"], synthetic.seed_for(3, 0), c["rect_disparity"], dev)
        out = torch.empty((n, c["H"], c["W"]), dtype=torch.int16, device=dev)
        hs = {"all": handle({"ADF_LAST_HANDOFF_MIN_PX": "0"}, c["radius"]),
              "last": handle({"ADF_LAST_HANDOFF_MIN_PX": "0", "ADF_INNER_HANDOFF_IMAGE": "0"}, c["radius"]),
              "none": handle({"ADF_LAST_HANDOFF_IMAGE": "0"}, c["radius"])}
        ref = {}
        for k, f in hs.items():
            for _ in range(3):
                f.filter(dl, view, out, dr, c["roi"])
            torch.cuda.synchronize()
            ref[k] = out.clone()
            assert (f.getLastHandoff() == adf.HANDOFF_IMAGE) == (k != "none")
            assert (f.getInnerHandoffs()[0] > 0) == (k == "all")
        assert torch.equal(ref["all"], ref["none"]) and torch.equal(ref["last"], ref["none"]), "the hand-offs differ"
        ms = {k: [] for k in hs}
        for _ in range(a.rounds):
            for k, f in hs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); f.filter(dl, view, out, dr, c["roi"]); e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        prof = {k: {"pass_h_first": [], "pass_h": [], "pass_v": [], "pass_v_last": []} for k in hs}
        for _ in range(a.rounds):
            for k, f in hs.items():
                f.enableProfiling(True)
                f.filter(dl, view, out, dr, c["roi"]); torch.cuda.synchronize()
                p = f.readProfile()
                f.enableProfiling(False)
                for cls in prof[k]:
                    prof[k][cls].append(p[cls]["total_ms"])

        def s(v):
            return "%.3f (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))
        for k in hs:
            total = [sum(x) for x in zip(*prof[k].values())]
            print("%d pair(s) = %5.2f Mpx of ROI  %-4s call %s | pass_h_first %s  pass_h %s  pass_v %s  pass_v_last %s  sum %s" % (
                n, n * roi_px1 / 1e6, k, s(ms[k]), s(prof[k]["pass_h_first"]), s(prof[k]["pass_h"]), s(prof[k]["pass_v"]),
                s(prof[k]["pass_v_last"]), s(total)))
        del hs, view, dl, dr, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
