"""Device time of amFilter (csrc/am_filter_kernels.hip) per 3840 x 2160 map: HIP events around each of N calls after a
warm-up call, the median and the minimum.

  * input: a seeded synthetic int16 map (steps and noise) and a gray or BGR joint of smooth regions with edges.  The tree is
    complete and every kernel visits every pixel, so the time does not depend on the data;
  * cases: sigma_s 16, sigma_r 0.2 (df 4, 7 manifolds) and sigma_s 40, sigma_r 0.1 (df 8, 15 manifolds), a gray and a BGR
    joint, adjust_outliers off and on, a single map and a batch of 8 (the time per map of the batch), int16 source and
    output; the destination and the workspace are allocated once, outside the timed calls;
  * next to each time: the launches of a call -- 5 per call, 5 per manifold, 5 per split with a gray joint and 6 with a BGR
    one, a memset with a BGR joint.

Which kernel the time goes to is a question for a profiler: run one case under it with --only.

    python tools/am_time.py [--iters N] [--only K] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H4, W4 = 2160, 3840
# maps, channels, sigma_s, sigma_r, adjust_outliers
CASES = [(n, ch, ss, sr, adjust) for n in (1, 8) for ch in (1, 3) for ss, sr in ((16.0, 0.2), (40.0, 0.1)) for adjust in (False, True)]


def inputs(n, ch, rng):
    base = (np.add.outer(np.arange(H4) // 40 * 9, np.arange(W4) // 64 * 14) % 256).astype(np.int16)
    joint = np.clip(base[None, :, :, None] + rng.integers(-6, 7, (n, H4, W4, ch), dtype=np.int16) + np.arange(ch, dtype=np.int16) * 40, 0, 255).astype(np.uint8)
    src = ((np.add.outer(np.arange(H4) // 90, np.arange(W4) // 120) % 24) * 64).astype(np.int16)[None] + rng.integers(-8, 9, (n, H4, W4), dtype=np.int16)
    return (joint if ch == 3 else joint[..., 0]), src.astype(np.int16)


def launches(height, ch):
    nodes, splits = 2 ** height - 1, 2 ** (height - 1) - 1
    return 5 + 5 * nodes + (6 if ch == 3 else 5) * splits + (1 if ch == 3 and height > 1 else 0)


def time_case(adf, joint, src, ss, sr, adjust, iters, dev):
    import torch

    tj, ts = torch.from_numpy(joint).to(dev), torch.from_numpy(src).to(dev)
    dst = torch.empty_like(ts)
    n = src.shape[0]
    ws = torch.empty(adf.amFilterWorkspaceBytes(n, H4, W4, 3 if joint.ndim == 4 else 1, ss, sr), dtype=torch.uint8, device=dev)
    adf.amFilter(tj, ts, ss, sr, adjust, dst=dst, workspace=ws)          # warm-up: the code object
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for e0, e1 in ev:
        e0.record()
        adf.amFilter(tj, ts, ss, sr, adjust, dst=dst, workspace=ws)
        e1.record()
    torch.cuda.synchronize()
    ms = sorted(e0.elapsed_time(e1) / n for e0, e1 in ev)
    return ms[len(ms) // 2], ms[0], ws.numel()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only", type=int, default=None, help="run case K alone (0-based)")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args(argv)
    import torch

    import addingdisparityfiltering_amd as adf

    dev = torch.device("cuda:0")
    lines = ["amFilter, %d x %d, int16 source and output, %d timed calls each (ms per map); device %s" % (W4, H4, args.iters, torch.cuda.get_device_name(dev))]
    print(lines[0], flush=True)
    rng = np.random.default_rng(7)
    made = {}
    for k, (n, ch, ss, sr, adjust) in enumerate(CASES):
        if args.only is not None and k != args.only:
            continue
        if (n, ch) not in made:
            made = {(n, ch): inputs(n, ch, rng)}                          # (one set of inputs at a time)
        joint, src = made[(n, ch)]
        p = adf.amPlan(ss, sr, -1, W4, H4)
        med, best, ws = time_case(adf, joint, src, ss, sr, adjust, args.iters, dev)
        lines.append("%-4s joint, %-10s sigmas %3g, %4g (df %d, %2d manifolds, small plane %4d x %3d), adjust_outliers %-3s  median %8.3f ms  (min %8.3f)   %3d launches   workspace %6.1f MiB per map"
                     % ("gray" if ch == 1 else "BGR", "1 map" if n == 1 else "batch of %d" % n, ss, sr, p["df"], p["manifolds"], p["sw"], p["sh"],
                        "on" if adjust else "off", med, best, launches(p["height"], ch), ws / n / 2 ** 20))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
