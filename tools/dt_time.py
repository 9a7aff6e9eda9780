"""Device time of dtFilter, mode DTF_RF (csrc/dt_filter_kernels.hip) per 3840 x 2160 map: HIP events around each of N calls
after a warm-up call, the median and the minimum.

  * input: a seeded synthetic int16 map (steps and noise) and a gray or 3-channel guide of smooth regions with edges; the
    kernels have no data-dependent branch, so the data does not move the time;
  * cases: gray and 3-channel guides, int16 source and output, sigmaSpatial 10, sigmaColor 30, 3 iterations, a single map
    and a batch of 16 (the time per map of the batch); the destination and the workspace are allocated once, outside the
    timed calls;
  * next to each time: the call's bytes per pixel -- each of the 2 N passes reads the map, writes it, reads what it wrote
    and writes it again (16 bytes in float; the first read and the last write are 2-byte int16) and reads the guide once
    per sweep: 16 * 6 - 4 + 12 * channels = 104 bytes with a gray guide, 128 with 3 channels -- and the time those bytes
    take at the 6.3 TB/s a streaming kernel reaches on this part.

    python tools/dt_time.py [--iters N] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H4, W4 = 2160, 3840
SS, SR, NIT = 10.0, 30.0, 3
STREAM = 6.3e12     # bytes per second


def inputs(n, ch, rng):
    base = (np.add.outer(np.arange(H4) // 40 * 9, np.arange(W4) // 64 * 14) % 256).astype(np.int16)
    guide = np.clip(base[None, :, :, None] + rng.integers(-6, 7, (n, H4, W4, ch), dtype=np.int16), 0, 255).astype(np.uint8)
    src = ((np.add.outer(np.arange(H4) // 90, np.arange(W4) // 120) % 24) * 64).astype(np.int16)[None] + rng.integers(-8, 9, (n, H4, W4), dtype=np.int16)
    return (guide if ch == 3 else guide[..., 0]), src.astype(np.int16)


def time_case(guide, src, iters, dev):
    import torch

    import addingdisparityfiltering_amd as adf

    tg, ts = torch.from_numpy(guide).to(dev), torch.from_numpy(src).to(dev)
    dst = torch.empty_like(ts)
    n = src.shape[0]
    ws = torch.empty(adf.dtFilterWorkspaceBytes(n, H4, W4), dtype=torch.uint8, device=dev)
    adf.dtFilter(tg, ts, SS, SR, adf.DTF_RF, NIT, dst=dst, workspace=ws)   # warm-up: the code object
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for e0, e1 in ev:
        e0.record()
        adf.dtFilter(tg, ts, SS, SR, adf.DTF_RF, NIT, dst=dst, workspace=ws)
        e1.record()
    torch.cuda.synchronize()
    ms = sorted(e0.elapsed_time(e1) / n for e0, e1 in ev)
    return ms[len(ms) // 2], ms[0]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args(argv)
    import torch

    dev = torch.device("cuda:0")
    lines = ["dtFilter DTF_RF, %d x %d, int16 source and output, sigmaSpatial %g, sigmaColor %g, %d iterations, %d timed calls each (ms per map); device %s"
             % (W4, H4, SS, SR, NIT, args.iters, torch.cuda.get_device_name(dev))]
    print(lines[0], flush=True)
    rng = np.random.default_rng(7)
    for n in (1, 16):
        for ch in (1, 3):
            guide, src = inputs(n, ch, rng)
            bytes_px = 16 * 2 * NIT - 4 + 2 * 2 * NIT * ch
            floor = W4 * H4 * bytes_px / STREAM * 1e3
            med, best = time_case(guide, src, args.iters, dev)
            lines.append("%-8s guide, %-11s median %8.3f ms  (min %8.3f)   %3d B/px = %6.3f ms at 6.3 TB/s   %5.1f x that"
                         % ("gray" if ch == 1 else "3-chan.", "1 map" if n == 1 else "batch of %d" % n, med, best, bytes_px, floor, med / floor))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
