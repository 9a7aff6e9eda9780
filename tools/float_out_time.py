"""filter() against filterFloat() (adf_wls_filter*_f32_*): device time per call of both on ONE handle and one batch of
4K pairs (BASELINE config 3: 3840 x 2160, ROI (256, 0, 3584, 2160), radius 2, as many of its 64 pairs as fit), in one
process on one build.  The two calls alternate round by round behind a warm-up of both, each call bracketed by HIP
events; afterwards the profile hook's line for the last column pass of each.  The float call moves 2 bytes per pixel
more in that one pass (16 instead of 14 B/px).

    python tools/float_out_time.py [--pairs N] [--rounds R] [--solver wave|exact] [--int16-only]

--int16-only times filter() alone: for a build without the float entry points (ADF_WLS_LIB=<older build>)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import addingdisparityfiltering_amd as adf                     # noqa: E402
from addingdisparityfiltering_amd import synthetic             # noqa: E402


def batch(n, dev):
    """Config 3's scene on the device for the largest n' <= n that fits, with both output maps."""
    c = synthetic.CONFIGS[3]
    while True:
        try:
            view, dl, dr = synthetic.make_artificial_batch_torch(n, c["W"], c["H"], c["channels"], synthetic.seed_for(3, 0),
                                                                 c["rect_disparity"], dev)
            outs = {"filter": torch.empty((n, c["H"], c["W"]), dtype=torch.int16, device=dev),
                    "filterFloat": torch.empty((n, c["H"], c["W"]), dtype=torch.float32, device=dev)}
            return n, view, dl, dr, outs, c
        except torch.cuda.OutOfMemoryError:
            if n == 1:
                raise
            n //= 2
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--solver", choices=("wave", "exact"), default="wave")
    ap.add_argument("--int16-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, view, dl, dr, outs, c = batch(a.pairs, dev)
    f = adf.createDisparityWLSFilterGeneric(True)
    f.setLambda(8000.0); f.setSigmaColor(1.5); f.setDepthDiscontinuityRadius(c["radius"])
    f.setSolver(adf.SOLVER_WAVE if a.solver == "wave" else adf.SOLVER_EXACT)
    names = ["filter"] if a.int16_only else ["filter", "filterFloat"]
    calls = {k: (lambda k=k: getattr(f, k)(dl, view, outs[k], dr, c["roi"])) for k in names}
    for _ in range(3):                                         # warm-up: workspace, code objects, both output maps
        for k in names:
            calls[k]()
    torch.cuda.synchronize()
    ms = {k: [] for k in names}
    for _ in range(a.rounds):
        for k in names:                                        # alternating: both see the same machine
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); calls[k](); e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    px = n * c["W"] * c["H"]
    print("%d pairs of %d x %d, ROI %s, %s solver, %d rounds, library %s" % (
        n, c["W"], c["H"], c["roi"], a.solver, a.rounds, os.path.basename(adf._lib.LIB_PATH)))
    for k in names:
        v = ms[k]
        print("%-12s median %.3f ms  min %.3f  max %.3f  (%.2f Gpx/s at the median)" % (
            k, statistics.median(v), min(v), max(v), px / statistics.median(v) / 1e6))
    if not a.int16_only:
        r = statistics.median(ms["filterFloat"]) / statistics.median(ms["filter"])
        print("filterFloat / filter = %.4f (by bytes: 134 / 132 B/px = 1.015)" % r)
        same = bool(torch.equal(outs["filterFloat"].round().clamp(-32768, 32767).to(torch.int16), outs["filter"]))
        print("round(filterFloat) == filter on the timed batch: %s" % same)
    roi_px = n * c["roi"][2] * c["roi"][3]
    for k in names:                                            # the profile hook, a run of its own per call
        f.enableProfiling(True)
        calls[k](); torch.cuda.synchronize()
        p = f.readProfile()["pass_v_last"]
        f.enableProfiling(False)
        print("%-12s pass_v_last: %d launch(es) %.3f ms, alg %.1f B/px, moved %.1f B/px, %.2f TB/s" % (
            k, p["launches"], p["total_ms"], p["alg_bytes"] / roi_px, p["moved_bytes"] / roi_px,
            p["moved_bytes"] / p["total_ms"] / 1e9))


if __name__ == "__main__":
    main()
