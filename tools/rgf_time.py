"""Device time of rollingGuidanceFilter (csrc/rolling_guidance_kernels.hip) per 3840 x 2160 map, beside the yardstick:
numOfIter calls of the existing jointBilateralFilter with a gray 8-bit joint at the same radius and source depth -- the
same taps and the same LDS traffic, code that has no rolling guidance in it.  HIP events around each of N calls after
warm-up calls, the two alternating call by call in one process; the median, the minimum and the spread (max - min) of
the N, and the ratio of the medians, which is the ratio per iteration.

  * input: a seeded synthetic disparity map (plateaus 64 levels apart and noise of +-8) as uint8, int16 or float32
    (the int16 map / 16), one map rolled by a few pixels per map of a batch; the yardstick's joint is smooth regions with
    edges and a little noise;
  * cases: the three depths at the defaults (d = -1, sigmaSpace 3: r = 4; sigmaColor 25; 4 iterations) and at d = 17
    (r = 8), a single map and a batch of 16 (the time per map of the batch), with a caller's workspace, the destination
    allocated once outside the timed calls;
  * below: int16 with range tables that do not fit in LDS (sigmaColor 1000 and 5000: 14422 and 65536 entries) on the
    same map and on a map of noise over the whole range, where most taps read the table from device memory.

    python tools/rgf_time.py [--iters N] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H4, W4 = 2160, 3840
NUM_ITER = 4
CASES = [(-1, 3.0), (17, 3.0)]          # (d, sigmaSpace)


def inputs(n, dtype, rng, noise=False):
    """n maps of `dtype` and the yardstick's gray joints: one seeded map each, rolled by a few pixels per map."""
    if noise:
        src = rng.integers(-32768, 32768, (H4, W4), dtype=np.int16)
    else:
        src = (((np.add.outer(np.arange(H4) // 90, np.arange(W4) // 120) % 24) * 64).astype(np.int16) + rng.integers(-8, 9, (H4, W4), dtype=np.int16)).astype(np.int16)
    if dtype == np.uint8:
        src = np.clip(src // 8, 0, 255).astype(np.uint8)
    elif dtype == np.float32:
        src = (src.astype(np.float32) / np.float32(16.0)).astype(np.float32)
    base = (np.add.outer(np.arange(H4) // 40 * 9, np.arange(W4) // 64 * 14) % 256).astype(np.int16)
    joint = np.clip(base + rng.integers(-6, 7, (H4, W4), dtype=np.int16), 0, 255).astype(np.uint8)
    return np.stack([np.roll(src, 3 * k, axis=1) for k in range(n)]), np.stack([np.roll(joint, 3 * k, axis=1) for k in range(n)])


def time_case(src, joint, d, sc, ss, iters, dev):
    """((median, min, spread) of rollingGuidanceFilter, the same of NUM_ITER jointBilateralFilter calls), ms per map."""
    import torch

    import addingdisparityfiltering_amd as adf

    ts, tj = torch.from_numpy(src).to(dev), torch.from_numpy(joint).to(dev)
    dst = torch.empty_like(ts)
    n = src.shape[0]
    ws = torch.empty(adf.rollingGuidanceWorkspaceBytes(n, H4, W4, src.dtype, NUM_ITER), dtype=torch.uint8, device=dev)

    def rolling():
        adf.rollingGuidanceFilter(ts, d, sc, ss, NUM_ITER, dst=dst, workspace=ws)

    def yardstick():
        for _ in range(NUM_ITER):
            adf.jointBilateralFilter(tj, ts, d, 25.0, ss, dst=dst)

    for _ in range(2):                                                   # warm-up: the code objects, the tables, the clock
        rolling()
        yardstick()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(iters)]
    for e in ev:
        e[0].record()
        rolling()
        e[1].record()
        yardstick()
        e[2].record()
    torch.cuda.synchronize()

    def stats(a, b):
        ms = sorted(e[a].elapsed_time(e[b]) / n for e in ev)
        return ms[len(ms) // 2], ms[0], ms[-1] - ms[0]

    return stats(0, 1), stats(1, 2)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args(argv)
    import torch

    import addingdisparityfiltering_amd as adf

    dev = torch.device("cuda:0")
    lines = ["rollingGuidanceFilter, %d x %d, %d iterations, BORDER_REFLECT_101, %d timed calls each (ms per map); device %s"
             % (W4, H4, NUM_ITER, args.iters, torch.cuda.get_device_name(dev)),
             "yardstick: %d calls of jointBilateralFilter, gray joint, sigmaColor 25, the same source, radius and depth; ratio = rolling / yardstick, per iteration"
             % NUM_ITER]
    print("\n".join(lines), flush=True)
    rng = np.random.default_rng(7)

    def run(src, joint, d, sc, ss, what):
        n = src.shape[0]
        colour, _, r, _ = adf.rgfTables(src.dtype, d, sc, ss)
        (med, best, spread), (ymed, ybest, yspread) = time_case(src, joint, d, sc, ss, args.iters, dev)
        lines.append("%-14s sigmaColor %4g, r = %d, table %5d, %-11s rolling median %7.3f ms (min %7.3f, spread %6.3f)   yardstick median %7.3f ms (min %7.3f, spread %6.3f)   ratio %5.2f"
                     % (what, sc, r, len(colour), "1 map" if n == 1 else "batch of %d" % n, med, best, spread, ymed, ybest, yspread, med / ymed))
        print(lines[-1], flush=True)

    for n in (1, 16):
        for dtype in (np.uint8, np.int16, np.float32):
            src, joint = inputs(n, dtype, rng)
            for d, ss in CASES:
                run(src, joint, d, 25.0 / 16 if dtype == np.float32 else 25.0, ss, np.dtype(dtype).name)
    for noise in (False, True):                                          # range tables that LDS does not hold
        src, joint = inputs(1, np.int16, rng, noise)
        for sc in (25.0, 1000.0, 5000.0):
            run(src, joint, -1, sc, 3.0, "int16 noise" if noise else "int16")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
