"""Device time of initUndistortRectifyMap, remap and rectifyViews (csrc/rectify_kernels.hip) for 64 views of
3840 x 2160, BGR and gray, and for one 1242 x 375 frame, with a KITTI-like model (five distortion coefficients, a rotation
of one degree about each axis).

HIP events around each call, warm-up first, one process.  Beside every case stands THE FLOOR it is judged against, timed in
the same process: a device-to-device copy that moves the same bytes (half of them read, half written) -- for remap the
source, the two maps and the destination, for rectifyViews the source and the destination, for the maps their 8 bytes
per pixel.  The last column is the copy's time over the case's: the achieved fraction of the copy's rate.  The fused form
saves 16 bytes per pixel over the two-step form: 8 written by initUndistortRectifyMap, 8 read by remap.  No pass / fail gate.

    python tools/rectify_time.py [--iters N] [--views N] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters):
    """Median and minimum device ms of fn() between two events."""
    import torch

    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    return ms[len(ms) // 2], ms[0]


def model(w, h):
    """KITTI's calibration scaled to w x h: (K, dist, R, P)."""
    s = w / 1242.0
    K = np.array([[984.2439 * s, 0.0, 690.0 * s], [0.0, 980.8141 * s, h / 2.0 + 3.0], [0.0, 0.0, 1.0]])
    P = np.array([[721.5377 * s, 0.0, 609.5593 * s, 44.85728 * s], [0.0, 721.5377 * s, h / 2.0 - 2.0, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]])
    c, sn = np.cos(np.deg2rad(1.0)), np.sin(np.deg2rad(1.0))
    Rx = np.array([[1, 0, 0], [0, c, -sn], [0, sn, c]])
    Ry = np.array([[c, 0, -sn], [0, 1, 0], [sn, 0, c]])
    Rz = np.array([[c, -sn, 0], [sn, c, 0], [0, 0, 1]])
    return K, [-0.3728755, 0.2037299, 0.002219027, 0.001383707, -0.07233722], Rz @ Ry @ Rx, P


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import torch

    import addingdisparityfiltering_amd as adf

    dev = torch.device("cuda:0")
    lines = ["initUndistortRectifyMap / remap / rectifyViews, %d timed calls each (median); device %s; library %s"
             % (args.iters, torch.cuda.get_device_name(dev), os.environ.get("ADF_WLS_LIB", "in tree")),
             "%-46s %9s %9s %10s %8s %9s %8s" % ("case", "ms/call", "min", "ms/view", "GB/s", "copy ms", "of copy")]
    print("\n".join(lines), flush=True)

    def copy_ms(nbytes):
        """A device-to-device copy that moves nbytes in all (half read, half written)."""
        a = torch.empty(max(nbytes // 2, 1), dtype=torch.uint8, device=dev)
        b = torch.empty_like(a)
        return timed(lambda: b.copy_(a), args.iters)[0]

    def report(name, n, med, best, nbytes):
        floor = copy_ms(nbytes)
        lines.append("%-46s %9.4f %9.4f %10.5f %8.0f %9.4f %6.0f %%" % (name, med, best, med / n, nbytes / (med * 1e-3) / 1e9, floor,
                                                                        100 * floor / med))
        print(lines[-1], flush=True)

    rng = np.random.default_rng(0)
    for n, W, H in ((args.views, 3840, 2160), (1, 1242, 375)):
        K, dist, R, P = model(W, H)
        px = W * H
        mx, my = adf.initUndistortRectifyMap(K, dist, R, P, (W, H), device=dev)
        inside = float(((mx > 0) & (mx < W - 1) & (my > 0) & (my < H - 1)).float().mean())
        lines.append("-- %d view(s) of %d x %d; %.1f %% of the destination samples inside the source" % (n, W, H, 100 * inside))
        print(lines[-1], flush=True)
        med, best = timed(lambda: adf.initUndistortRectifyMap(K, dist, R, P, (W, H), device=dev), args.iters)
        report("initUndistortRectifyMap (2 planes, allocated)", 1, med, best, px * 8)
        for ch, cname in ((3, "BGR"), (1, "gray")):
            one = torch.from_numpy(rng.integers(0, 256, (H, W, ch) if ch == 3 else (H, W), dtype=np.uint8)).to(dev)
            src = one.unsqueeze(0).repeat((n,) + (1,) * one.dim()).contiguous()
            del one
            dst = torch.empty_like(src)
            med, best = timed(lambda: adf.remap(src, mx, my, dst=dst), args.iters)
            report("remap %s" % cname, n, med, best, 2 * n * px * ch + 8 * px)
            two = dst.clone()
            med, best = timed(lambda: adf.rectifyViews(src, K, dist, R, P, dst=dst), args.iters)
            report("rectifyViews %s" % cname, n, med, best, 2 * n * px * ch)
            assert torch.equal(two, dst)
            if n > 2:                                               # the per-frame case: one view of one camera
                med, best = timed(lambda: adf.rectifyViews(src[:1], K, dist, R, P, dst=dst[:1]), args.iters)
                report("rectifyViews %s, 1 view" % cname, 1, med, best, 2 * px * ch)
            del src, dst, two
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
