"""Device time of dtWindowFilter, mode DTF_NC (csrc/dt_window_kernels.hip) per 3840 x 2160 map: HIP events around each of N
calls after a warm-up call, the median and the minimum.

  * input: a seeded synthetic int16 map (steps and noise) and a gray or 3-channel guide of smooth regions with edges.  The
    window walk IS data-dependent: the guide decides how far each pixel walks.  Next to each time stands the mean number of
    taps of a window, measured on 256 rows and 256 columns of the first map with the NumPy statement (tests/dt_window_ref.py);
  * cases: a gray guide at sigmaSpatial 10, sigmaColor 30 (radii 15, 7, 3) and at 80, 50 (radii 120, 60, 30), a single map
    and a batch of 16 (the time per map of the batch), a 3-channel guide, and a flat guide (every window has all its
    2 R + 1 taps: the longest walk), 3 iterations each, int16 source and output;
    the destination and the workspace are allocated once, outside the timed calls;
  * next to each time: the call's bytes per pixel -- each of the 2 N passes reads the map and writes it (8 bytes in float;
    the first read and the last write are 2-byte int16) and reads the guide once: 8 * 6 - 4 + 6 * channels = 50 bytes with
    a gray guide, 62 with 3 channels, halos not counted -- and the time those bytes take at the 6.3 TB/s a streaming kernel
    reaches on this part.

    python tools/dt_window_time.py [--iters N] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H4, W4 = 2160, 3840
NIT = 3
STREAM = 6.3e12     # bytes per second
# maps, channels, sigmaSpatial, sigmaColor, flat guide (every window has its 2 R + 1 taps: the longest walk)
CASES = [(1, 1, 10.0, 30.0, False), (1, 1, 80.0, 50.0, False), (16, 1, 10.0, 30.0, False), (16, 1, 80.0, 50.0, False),
         (1, 3, 10.0, 30.0, False), (1, 3, 80.0, 50.0, False), (1, 1, 10.0, 30.0, True), (1, 1, 80.0, 50.0, True)]


def inputs(n, ch, rng):
    base = (np.add.outer(np.arange(H4) // 40 * 9, np.arange(W4) // 64 * 14) % 256).astype(np.int16)
    guide = np.clip(base[None, :, :, None] + rng.integers(-6, 7, (n, H4, W4, ch), dtype=np.int16), 0, 255).astype(np.uint8)
    src = ((np.add.outer(np.arange(H4) // 90, np.arange(W4) // 120) % 24) * 64).astype(np.int16)[None] + rng.integers(-8, 9, (n, H4, W4), dtype=np.int16)
    return (guide if ch == 3 else guide[..., 0]), src.astype(np.int16)


def mean_taps(adf, guide, ss, sr):
    """Taps per window, averaged over the passes of a call, on a band of the first map."""
    import dt_ref
    import dt_window_ref as ref

    Lh, Lv = dt_ref.l1_steps(guide[0][:256])[0], dt_ref.l1_steps(guide[0][:, :256])[1]   # 256 whole rows; 256 whole columns
    k, taps = ref.factor(ss, sr), []
    for r in adf.dtNcRadii(ss, NIT):
        for L in (Lh, np.ascontiguousarray(Lv.T)):
            left, right = ref.windows(L, r, k)
            taps.append(float((left + right + 1).mean()))
    return float(np.mean(taps))


def time_case(adf, guide, src, ss, sr, iters, dev):
    import torch

    tg, ts = torch.from_numpy(guide).to(dev), torch.from_numpy(src).to(dev)
    dst = torch.empty_like(ts)
    n = src.shape[0]
    ws = torch.empty(adf.dtWindowFilterWorkspaceBytes(n, H4, W4), dtype=torch.uint8, device=dev)
    adf.dtWindowFilter(tg, ts, ss, sr, adf.DTF_NC, NIT, dst=dst, workspace=ws)   # warm-up: the code object
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for e0, e1 in ev:
        e0.record()
        adf.dtWindowFilter(tg, ts, ss, sr, adf.DTF_NC, NIT, dst=dst, workspace=ws)
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

    import addingdisparityfiltering_amd as adf

    dev = torch.device("cuda:0")
    lines = ["dtWindowFilter DTF_NC, %d x %d, int16 source and output, %d iterations, %d timed calls each (ms per map); device %s"
             % (W4, H4, NIT, args.iters, torch.cuda.get_device_name(dev))]
    print(lines[0], flush=True)
    rng = np.random.default_rng(7)
    made = {}
    for n, ch, ss, sr, flat in CASES:
        if (n, ch) not in made:
            made = {(n, ch): inputs(n, ch, rng)}                          # (one set of inputs at a time: a batch of 16 is 400 MB)
        guide, src = made[(n, ch)]
        if flat:
            guide = np.full_like(guide, 117)
        bytes_px = 8 * 2 * NIT - 4 + 2 * NIT * ch
        floor = W4 * H4 * bytes_px / STREAM * 1e3
        med, best = time_case(adf, guide, src, ss, sr, args.iters, dev)
        lines.append("%-8s guide, %-11s sigmas %3g, %3g (%5.1f taps per window)  median %8.3f ms  (min %8.3f)   %3d B/px = %6.3f ms at 6.3 TB/s   %5.1f x that"
                     % ("flat" if flat else "gray" if ch == 1 else "3-chan.", "1 map" if n == 1 else "batch of %d" % n, ss, sr, mean_taps(adf, guide, ss, sr),
                        med, best, bytes_px, floor, med / floor))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
