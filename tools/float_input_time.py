"""filterFloat() on int16 maps against filterFloat() on float32 maps (adf_wls_filter_typed_*): device time per call of
both on ONE handle and one batch of 4K pairs (BASELINE config 3: 3840 x 2160, ROI (256, 0, 3584, 2160), radius 2, as
many of its 64 pairs as fit), confidence mode, in one process on one build.  The float maps are the int16 maps plus a
fraction of an LSB, so both calls see the same confidence map.  The two calls alternate round by round behind a warm-up
of both, each call bracketed by HIP events; afterwards the per-kernel times of each from the handle's profiling hook (a
run of its own per call, median of --profile-rounds).  By construction the float call adds one launch, quantise_maps
(both maps: 8 B read + 4 B written per frame pixel), and 2 B per ROI pixel in the first row pass.

    python tools/float_input_time.py [--pairs N] [--rounds R] [--solver wave|exact] [--out FILE]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import addingdisparityfiltering_amd as adf                     # noqa: E402
from addingdisparityfiltering_amd import synthetic             # noqa: E402


def batch(n, dev):
    """Config 3's scene on the device for the largest n' <= n that fits: int16 and float32 maps, one float output."""
    c = synthetic.CONFIGS[3]
    while True:
        try:
            view, dl, dr = synthetic.make_artificial_batch_torch(n, c["W"], c["H"], c["channels"], synthetic.seed_for(3, 0),
                                                                 c["rect_disparity"], dev)
            maps = {"int16": (dl, dr), "float32": (dl.to(torch.float32) + 0.37, dr.to(torch.float32) + 0.37)}
            out = torch.empty((n, c["H"], c["W"]), dtype=torch.float32, device=dev)
            return n, view, maps, out, c
        except torch.cuda.OutOfMemoryError:
            if n == 1:
                raise
            n //= 2
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--profile-rounds", type=int, default=5)
    ap.add_argument("--solver", choices=("wave", "exact"), default="wave")
    ap.add_argument("--out", default=None, help="also append the report to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, view, maps, out, c = batch(a.pairs, dev)
    f = adf.createDisparityWLSFilterGeneric(True)
    f.setLambda(8000.0); f.setSigmaColor(1.5); f.setDepthDiscontinuityRadius(c["radius"])
    f.setSolver(adf.SOLVER_WAVE if a.solver == "wave" else adf.SOLVER_EXACT)
    names = list(maps)
    calls = {k: (lambda k=k: f.filterFloat(maps[k][0], view, out, maps[k][1], c["roi"])) for k in names}
    lines = []

    def say(s):
        print(s)
        lines.append(s)

    paths = {}
    for _ in range(3):                                         # warm-up: workspace (the float call's is larger), code objects
        for k in names:
            calls[k]()
            paths[k] = (f.getLastPath(), f.getLastSolverPath())
    torch.cuda.synchronize()
    ms = {k: [] for k in names}
    for _ in range(a.rounds):
        for k in names:                                        # alternating: both see the same machine
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); calls[k](); e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    px = n * c["W"] * c["H"]
    say("%d pairs of %d x %d, ROI %s, confidence mode, %s solver, %d rounds, filterFloat on both kinds of maps" % (
        n, c["W"], c["H"], c["roi"], a.solver, a.rounds))
    for k in names:
        v = ms[k]
        say("%-8s maps: median %.3f ms  min %.3f  max %.3f  (%.2f Gpx/s at the median), path %d / %d" % (
            k, statistics.median(v), min(v), max(v), px / statistics.median(v) / 1e6, *paths[k]))
    say("float32 / int16 = %.4f" % (statistics.median(ms["float32"]) / statistics.median(ms["int16"])))
    say("workspace with the float call's planes: %.2f GB" % (f.workspaceBytes() / 2.0 ** 30))
    prof = {}
    for k in names:                                            # the profile hook: kernels run one after the other
        runs = []
        for _ in range(a.profile_rounds):
            f.enableProfiling(True)
            calls[k](); torch.cuda.synchronize()
            runs.append(f.readProfile())
            f.enableProfiling(False)
        prof[k] = {name: dict(runs[0][name], total_ms=statistics.median(r[name]["total_ms"] for r in runs)) for name in runs[0]}
    say("per-kernel device time (profiling hook, median of %d calls; ms, and TB/s of the bytes moved):" % a.profile_rounds)
    say("%-16s %10s %10s %10s" % ("kernel class", "int16", "float32", "delta"))
    for name in sorted(set(prof["int16"]) | set(prof["float32"])):
        a_, b_ = prof["int16"].get(name), prof["float32"].get(name)
        ta, tb = (a_ or {}).get("total_ms", 0.0), (b_ or {}).get("total_ms", 0.0)
        bw = " ".join("%s %.2f TB/s" % (k, p["moved_bytes"] / p["total_ms"] / 1e9) for k, p in (("int16", a_), ("float32", b_)) if p)
        say("%-16s %10.3f %10.3f %+10.3f   %s" % (name, ta, tb, tb - ta, bw))
    say("%-16s %10.3f %10.3f %+10.3f" % ("sum", sum(p["total_ms"] for p in prof["int16"].values()),
                                         sum(p["total_ms"] for p in prof["float32"].values()),
                                         sum(p["total_ms"] for p in prof["float32"].values()) - sum(p["total_ms"] for p in prof["int16"].values())))
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
