"""Device time of guidedFilter (csrc/guided_filter_kernels.hip) per 3840 x 2160 map: HIP events around each of N calls
after a warm-up call, the median and the minimum.

  * input: a seeded synthetic int16 map (steps and noise) and a gray or 3-channel guide of smooth regions with edges; the
    kernels have no data-dependent branch, so the data does not move the time;
  * cases: gray and 3-channel guides, int16 source and output, r = 4, 8, 16, eps = 100, a single map and a batch of 16
    (the time per map of the batch); the destination and the workspace are allocated once, outside the timed calls;
  * next to each time: the algorithmic bytes per pixel -- stage 1 reads guide + source and writes (channels + 1) float
    planes, stage 2 reads them + the guide and writes dst: 22 bytes with a gray guide, 42 with 3 channels -- and the time
    those bytes take at the 6.3 TB/s a streaming kernel reaches on this part (sections 7 and 11).

    python tools/gf_time.py [--iters N] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H4, W4 = 2160, 3840
EPS = 100.0
STREAM = 6.3e12     # bytes per second


def inputs(n, ch, rng):
    base = (np.add.outer(np.arange(H4) // 40 * 9, np.arange(W4) // 64 * 14) % 256).astype(np.int16)
    guide = np.clip(base[None, :, :, None] + rng.integers(-6, 7, (n, H4, W4, ch), dtype=np.int16), 0, 255).astype(np.uint8)
    src = ((np.add.outer(np.arange(H4) // 90, np.arange(W4) // 120) % 24) * 64).astype(np.int16)[None] + rng.integers(-8, 9, (n, H4, W4), dtype=np.int16)
    return (guide if ch == 3 else guide[..., 0]), src.astype(np.int16)


def time_case(guide, src, r, iters, dev):
    import torch

    import addingdisparityfiltering_amd as adf

    tg, ts = torch.from_numpy(guide).to(dev), torch.from_numpy(src).to(dev)
    dst = torch.empty_like(ts)
    n, ch = src.shape[0], 3 if guide.ndim == 4 else 1
    ws = torch.empty(adf.guidedFilterWorkspaceBytes(n, H4, W4, ch), dtype=torch.uint8, device=dev)
    adf.guidedFilter(tg, ts, r, EPS, dst=dst, workspace=ws)               # warm-up: the code object
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for e0, e1 in ev:
        e0.record()
        adf.guidedFilter(tg, ts, r, EPS, dst=dst, workspace=ws)
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
    lines = ["guidedFilter, %d x %d, int16 source and output, eps %g, %d timed calls each (ms per map); device %s"
             % (W4, H4, EPS, args.iters, torch.cuda.get_device_name(dev))]
    print(lines[0], flush=True)
    rng = np.random.default_rng(7)
    for n in (1, 16):
        for ch in (1, 3):
            guide, src = inputs(n, ch, rng)
            bytes_px = (ch + 2 + 4 * (ch + 1)) + (4 * (ch + 1) + ch + 2)
            floor = W4 * H4 * bytes_px / STREAM * 1e3
            for r in (4, 8, 16):
                med, best = time_case(guide, src, r, args.iters, dev)
                lines.append("%-8s guide, r = %2d, %-11s median %8.3f ms  (min %8.3f)   %2d B/px = %6.3f ms at 6.3 TB/s   %5.1f x that"
                             % ("gray" if ch == 1 else "3-chan.", r, "1 map" if n == 1 else "batch of %d" % n, med, best, bytes_px, floor, med / floor))
                print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
