"""Device time of the block matcher with and without its winning-cost plane, of validateDisparity and of the
computeFull chain (csrc/bm_matcher.hip, csrc/validate_kernels.hip), ms per call:

  * the existing entries, compute() with cv::StereoBM's defaults (the instantiation with the uniqueness test) and
    computeBoth() with the filter factory's settings (the one without): one 3840 x 2160 pair and a batch of 8,
    64 disparities, blockSize 9, SAD and census dense 7.  Each case is timed `--repeats` times over; the spread of the
    repeats' medians is the yardstick for a difference between two builds.  Run the same command with ADF_WLS_LIB
    pointing at another build of the library (alternating the two) to compare them: a build without the cost entries
    times the existing entries only;
  * computeWithCost() / computeBothWithCost() on the same shapes;
  * validateDisparity per 4K map, CV_16S and CV_32S cost, one map and a batch of 64, on the matcher's own map and cost
    of a realistic pair (the KITTI fixture tiled to 4K), every timed call from a fresh copy of the map (the copy is
    outside the events).  It moves 2 + sizeof(cost) bytes per pixel in and 2 bytes per invalidated pixel out; the floor
    printed beside it is those bytes at 8 TB/s;
  * the chain computeFull() (match with cost, validateDisparity at disp12MaxDiff 1, filterSpeckles(100, 32)) on that pair.

    python tools/bm_cost_time.py [--iters N] [--repeats R] [--json OUT]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H4, W4, ND, BS = 2160, 3840, 64, 9
HBM_BYTES_PER_S = 8e12


def views(n, dev):
    """n textured 4K pairs whose right view is the left one shifted by a disparity that changes with the row band."""
    import torch

    rng = np.random.default_rng(11)
    base = rng.integers(0, 256, (H4, W4 + 128), dtype=np.uint8)
    base = (base // 2 + np.roll(base, 1, 1) // 4 + np.roll(base, 1, 0) // 4).astype(np.uint8)
    L, R = [], []
    for k in range(n):
        b = np.roll(base, 17 * k, 0)
        right = b[:, 64:64 + W4].copy()
        for band, s in enumerate((5, 19, 33, 47)):
            rows = slice(band * H4 // 4, (band + 1) * H4 // 4)
            right[rows] = b[rows, 64 + s:64 + s + W4]
        L.append(b[:, 64:64 + W4]); R.append(right)
    return torch.from_numpy(np.stack(L)).to(dev), torch.from_numpy(np.stack(R)).to(dev)


def kitti_4k(dev):
    """The KITTI fixture pair tiled to 3840 x 2160: real texture, occlusions and mismatches in every tile."""
    import torch
    from PIL import Image

    out = []
    for name in ("kitti_left.bmp", "kitti_right.bmp"):
        g = np.array(Image.open(os.path.join(ROOT, "tests", "golden", name)).convert("L"))
        out.append(torch.from_numpy(np.ascontiguousarray(np.tile(g, (H4 // g.shape[0] + 1, W4 // g.shape[1] + 1))[:H4, :W4])).to(dev))
    return out


def timed(fn, iters, repeats, prep=None):
    """Medians (ms) of `repeats` windows of `iters` event-timed calls of fn(), after a warm-up call; prep() runs before
    every call, outside the events."""
    import torch

    if prep:
        prep()
    fn()
    torch.cuda.synchronize()
    meds = []
    for _ in range(repeats):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
        for e0, e1 in ev:
            if prep:
                prep()
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
        meds.append(ms[len(ms) // 2])
    return meds


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    import torch

    import addingdisparityfiltering_amd as adf
    from addingdisparityfiltering_amd import _lib

    dev = torch.device("cuda:0")
    have_cost = hasattr(_lib.lib(), "adf_bm_compute_cost_device")    # (an older build named by ADF_WLS_LIB may lack them)
    print("library %s (%s the cost entries); %d x %d, %d disparities, blockSize %d; %d repeats of %d timed calls; device %s"
          % (_lib.LIB_PATH, "with" if have_cost else "WITHOUT", W4, H4, ND, BS, args.repeats, args.iters, torch.cuda.get_device_name(dev)))
    L8, R8 = views(8, dev)
    rows = []

    def report(case, meds, n, note=""):
        med = sorted(meds)[len(meds) // 2]
        rows.append(dict(case=case, n=n, medians_ms=meds, median_ms=med, spread_ms=max(meds) - min(meds)))
        print("%-64s median %8.3f ms  repeats min %8.3f max %8.3f (spread %5.2f %%)  = %7.3f ms/pair%s"
              % (case, med, min(meds), max(meds), 100 * (max(meds) - min(meds)) / med, med / n, note))

    def matcher(cost, filter_settings):
        bm = adf.StereoBM.create(ND, BS)
        bm.setCostType(cost); bm.setCensusSize(7)
        if filter_settings:
            bm.setTextureThreshold(0); bm.setUniquenessRatio(0)
        return bm

    for cname, cost in (("SAD", adf.BM_COST_SAD), ("census dense 7", adf.BM_COST_CENSUS_DENSE)):
        for n in (1, 8):
            Lv, Rv = (L8[0], R8[0]) if n == 1 else (L8, R8)
            shape = (H4, W4) if n == 1 else (n, H4, W4)
            d0, d1, c0, c1 = (torch.empty(shape, dtype=torch.int16, device=dev) for _ in range(4))
            bm, bmf = matcher(cost, False), matcher(cost, True)
            report("compute, %s, cv defaults, %d pair(s)" % (cname, n), timed(lambda: bm.compute(Lv, Rv, d0), args.iters, args.repeats), n)
            report("computeBoth, %s, filter settings, %d pair(s)" % (cname, n),
                   timed(lambda: bmf.computeBoth(Lv, Rv, d0, d1), args.iters, args.repeats), n)
            if have_cost:
                report("computeWithCost, %s, cv defaults, %d pair(s)" % (cname, n),
                       timed(lambda: bm.computeWithCost(Lv, Rv, d0, c0), args.iters, args.repeats), n)
                report("computeBothWithCost, %s, filter settings, %d pair(s)" % (cname, n),
                       timed(lambda: bmf.computeBothWithCost(Lv, Rv, d0, d1, c0, c1), args.iters, args.repeats), n)
    if have_cost:
        del L8, R8
        KL, KR = kitti_4k(dev)
        bm = matcher(adf.BM_COST_SAD, False)
        disp, cost = bm.computeWithCost(KL, KR)
        for tname, ctensor in (("CV_16S", cost), ("CV_32S", cost.to(torch.int32))):
            for n in (1, 64):
                src = disp if n == 1 else disp.expand(n, H4, W4).contiguous()
                cst = ctensor if n == 1 else ctensor.expand(n, H4, W4).contiguous()
                work = src.clone()
                adf.validateDisparity(work, cst, 0, ND, 1)
                gone = int((work != src).sum().item())
                floor_ms = 1e3 * (src.numel() * (2 + cst.element_size()) + 2 * gone) / HBM_BYTES_PER_S
                meds = timed(lambda: adf.validateDisparity(work, cst, 0, ND, 1), args.iters, args.repeats, prep=lambda: work.copy_(src))
                report("validateDisparity, %s cost, %d map(s)" % (tname, n), meds, n,
                       "   HBM floor %.4f ms/map, %.2f %% of pixels invalidated" % (floor_ms / n, 100.0 * gone / src.numel()))
                del src, cst, work
        full = adf.StereoBM.create(ND, BS)
        full.setDisp12MaxDiff(1); full.setSpeckleWindowSize(100); full.setSpeckleRange(32)
        out = torch.empty((H4, W4), dtype=torch.int16, device=dev)
        report("computeFull (match + validate 1 + speckles 100/32), SAD, 1 pair", timed(lambda: full.computeFull(KL, KR, out), args.iters, args.repeats), 1)
        plain = adf.StereoBM.create(ND, BS)
        report("compute alone, SAD, 1 pair (for the chain above)", timed(lambda: plain.compute(KL, KR, out), args.iters, args.repeats), 1)
        speck = out.clone()
        report("filterSpeckles alone (100, 32) on that map", timed(lambda: adf.filterSpeckles(speck, -16, 100, 32), args.iters, args.repeats,
                                                                   prep=lambda: speck.copy_(out)), 1)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(library=_lib.LIB_PATH, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
