"""Device time of jointBilateralFilter (csrc/joint_bilateral_kernels.hip) per 3840 x 2160 map: HIP events around each of
N calls after warm-up calls, the median, the minimum and the spread (max - min) of the N.

  * input: a seeded synthetic int16 map (steps and noise) and a gray or BGR joint of smooth regions with edges and a
    little noise.  The kernel has no data-dependent branch, but the bank conflicts of its gather from the colour table do
    depend on the joint: a second joint of uniform noise over the whole range (every lane another table entry) shows the
    worst of them;
  * cases: gray and BGR joints, int16 source and output, d = 5, 9, 17 and d = -1 with sigmaSpace = 8 (r = 12), a single map
    and a batch of 16 (the time per map of the batch); the destination is allocated once, outside the timed calls;
  * next to each time: the taps per pixel; the VALU lane-operations per second at VALU_PER_TAP operations per tap (the
    read's address, the L1 difference, two multiplies, two adds -- counted in the kernel's ISA) against the part's issue
    rate of 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz; and the LDS-array cycles per second at LDS_PER_TAP cycles per wave and
    tap (an 8-byte read and a conflict-free 4-byte gather, two cycles each) against 256 CUs x 2.4 GHz.  The larger share
    is what bounds the kernel; a share the noise joint lowers is cycles lost to bank conflicts.

    python tools/jbf_time.py [--iters N] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H4, W4 = 2160, 3840
SIGMA_COLOR = 25.0
CLOCK, CUS = 2.4e9, 256
VALU_RATE = CUS * 4 * 32 * CLOCK        # lane-operations per second
LDS_RATE = CUS * CLOCK                  # LDS-array cycles per second
VALU_PER_TAP, LDS_PER_TAP = 6, 4        # per lane and tap; per wave (64 lanes) and tap
CASES = [(5, 3.0), (9, 3.0), (17, 3.0), (-1, 8.0)]      # (d, sigmaSpace)


def inputs(n, ch, rng, noise=False):
    """n maps: one seeded map, rolled by a few pixels per map (a batch of 16 fresh maps costs minutes of host time)."""
    if noise:
        joint = rng.integers(0, 256, (H4, W4, ch), dtype=np.uint8)
    else:
        base = (np.add.outer(np.arange(H4) // 40 * 9, np.arange(W4) // 64 * 14) % 256).astype(np.int16)
        joint = np.clip(base[:, :, None] + rng.integers(-6, 7, (H4, W4, ch), dtype=np.int16), 0, 255).astype(np.uint8)
    src = (((np.add.outer(np.arange(H4) // 90, np.arange(W4) // 120) % 24) * 64).astype(np.int16) + rng.integers(-8, 9, (H4, W4), dtype=np.int16)).astype(np.int16)
    joints = np.stack([np.roll(joint, 3 * k, axis=1) for k in range(n)])
    srcs = np.stack([np.roll(src, 3 * k, axis=1) for k in range(n)])
    return (joints if ch == 3 else joints[..., 0]), srcs


def time_case(joint, src, d, ss, iters, dev):
    import torch

    import addingdisparityfiltering_amd as adf

    tj, ts = torch.from_numpy(joint).to(dev), torch.from_numpy(src).to(dev)
    dst = torch.empty_like(ts)
    n = src.shape[0]
    for _ in range(2):                                                   # warm-up: the code object, the tables, the clock
        adf.jointBilateralFilter(tj, ts, d, SIGMA_COLOR, ss, dst=dst)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for e0, e1 in ev:
        e0.record()
        adf.jointBilateralFilter(tj, ts, d, SIGMA_COLOR, ss, dst=dst)
        e1.record()
    torch.cuda.synchronize()
    ms = sorted(e0.elapsed_time(e1) / n for e0, e1 in ev)
    return ms[len(ms) // 2], ms[0], ms[-1] - ms[0]


def taps_of(r):
    return sum(1 for i in range(-r, r + 1) for j in range(-r, r + 1) if i * i + j * j <= r * r)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args(argv)
    import torch

    import addingdisparityfiltering_amd as adf

    dev = torch.device("cuda:0")
    lines = ["jointBilateralFilter, %d x %d, int16 source and output, sigmaColor %g, BORDER_REFLECT_101, %d timed calls each (ms per map); device %s"
             % (W4, H4, SIGMA_COLOR, args.iters, torch.cuda.get_device_name(dev)),
             "VALU: %d lane-operations per tap against %.1f T/s; LDS: %d array cycles per wave and tap against %.0f G cycles/s"
             % (VALU_PER_TAP, VALU_RATE / 1e12, LDS_PER_TAP, LDS_RATE / 1e9)]
    print("\n".join(lines), flush=True)
    rng = np.random.default_rng(7)

    def run(joint, src, d, ss, what):
        n, ch = src.shape[0], 3 if joint.ndim == 4 else 1
        r = adf.jbfTables(d, SIGMA_COLOR, ss, ch)[2]
        taps = taps_of(r)
        med, best, spread = time_case(joint, src, d, ss, args.iters, dev)
        lane_taps = float(W4) * H4 * taps / (med * 1e-3)
        lines.append("%-5s joint, d = %2d (r = %2d, %4d taps), %-11s median %8.3f ms  (min %8.3f, spread %6.3f)   VALU %5.1f %%   LDS %5.1f %%"
                     % (what, d, r, taps, "1 map" if n == 1 else "batch of %d" % n, med, best, spread,
                        100 * lane_taps * VALU_PER_TAP / VALU_RATE, 100 * lane_taps / 64 * LDS_PER_TAP / LDS_RATE))
        print(lines[-1], flush=True)

    for n in (1, 16):
        for ch in (1, 3):
            joint, src = inputs(n, ch, rng)
            for d, ss in CASES:
                run(joint, src, d, ss, "gray" if ch == 1 else "BGR")
    for ch in (1, 3):                                                    # the colour gather's worst case
        joint, src = inputs(1, ch, rng, noise=True)
        run(joint, src, 9, 3.0, "noise" if ch == 1 else "nois3")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
