"""Device time of reprojectImageTo3D and of the point list (csrc/reproject_kernels.hip) on 16 maps of 3840 x 2160:

  * the image: int16 and float32 maps, XYZ and Z only, aligned (16-byte loads and stores) and unaligned (source and
    destination 4 bytes off: the element-by-element path), no missing values; and with handleMissingValues (the minimum
    reduction in front, caller workspace);
  * the point list at 100 %, 50 % and 1 % valid pixels (int16 maps, missingValue = -16, caller workspace, adf_point_cloud_device
    itself: the mirror's trim would add a host read).

HIP events around each call, warm-up first, one process.  For each case: ms per call and per map, algorithmic bytes
(source read once, result written once: 2 or 4 B/px in, 12 or 4 B/px out; the list: 2 B/px in, 12 B per valid point out)
over that time, and that rate as a fraction of STREAM_GBS, the rate DESIGN.md section 11 records for the fused view
preparation kernel on this part.  No pass / fail gate.

    python tools/reproject_time.py [--iters N] [--maps N] [--out FILE]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H4, W4 = 2160, 3840
STREAM_GBS = 6110.0          # fused half + gray on 64 x 4K pairs
Q = np.array([[1.0, 0, 0, -1919.5], [0, 1.0, 0, -1079.5], [0, 0, 0, 2100.0], [0, 0, 1.0 / 0.12, 0]])


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


def shifted(torch, shape, dtype, dev, off_bytes):
    """A contiguous tensor of `shape` whose base is `off_bytes` past an allocation's start."""
    n = int(np.prod(shape))
    off = off_bytes // torch.empty((), dtype=dtype).element_size()
    return torch.zeros(n + off, dtype=dtype, device=dev)[off:].view(shape)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--maps", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import torch

    import addingdisparityfiltering_amd as adf
    from addingdisparityfiltering_amd import _lib

    dev = torch.device("cuda:0")
    n, px = args.maps, H4 * W4
    rng = np.random.default_rng(0)
    base = rng.integers(16, 4000, (n, H4, W4)).astype(np.int16)
    lines = ["reprojectImageTo3D / point list, %d maps of %d x %d, %d timed calls each (median); device %s; yardstick %.0f GB/s"
             % (n, W4, H4, args.iters, torch.cuda.get_device_name(dev), STREAM_GBS),
             "%-58s %9s %9s %9s %8s %7s" % ("case", "ms/call", "min", "ms/map", "GB/s", "of yard")]

    def report(name, med, best, nbytes):
        gbs = nbytes / (med * 1e-3) / 1e9
        lines.append("%-58s %9.3f %9.3f %9.4f %8.0f %6.0f %%" % (name, med, best, med / n, gbs, 100 * gbs / STREAM_GBS))
        print(lines[-1], flush=True)

    print("\n".join(lines), flush=True)
    buf = torch.zeros(adf.reprojectWorkspaceBytes(n), dtype=torch.uint8, device=dev)
    for dtype, tname, esz in ((torch.int16, "int16", 2), (torch.float32, "float32", 4)):
        for z_only, oname, ch in ((False, "XYZ", 3), (True, "Z", 1)):
            for off, aname in ((0, "aligned"), (4, "unaligned (+4 B)")):
                src = shifted(torch, (n, H4, W4), dtype, dev, off)
                src.copy_(torch.from_numpy(base).to(dev))
                dst = shifted(torch, (n, H4, W4) + (() if z_only else (3,)), torch.float32, dev, off)
                med, best = timed(lambda: adf.reprojectImageTo3D(src, Q, dst=dst, dispScale=1.0 / 16, zOnly=z_only), args.iters)
                report("image %s -> %s, %s" % (tname, oname, aname), med, best, n * px * (esz + 4 * ch))
                if off == 0:
                    med, best = timed(lambda: adf.reprojectImageTo3D(src, Q, True, dst=dst, dispScale=1.0 / 16, zOnly=z_only, buf=buf), args.iters)
                    report("image %s -> %s, aligned, handleMissingValues" % (tname, oname), med, best, n * px * (esz + 4 * ch))
                del src, dst
    # the point list
    prm = _lib.ReprojectParams()
    prm.Q[:] = [float(v) for v in Q.ravel()]
    prm.disp_scale, prm.missing_mode, prm.missing_value = 1.0 / 16, _lib.MISSING_VALUE, -16.0
    points = torch.empty((n, px, 3), dtype=torch.float32, device=dev)
    counts = torch.zeros(n, dtype=torch.int32, device=dev)
    ws = torch.zeros(adf.pointCloudWorkspaceBytes(n, H4, W4), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for share in (1.0, 0.5, 0.01):
        maps = base.copy()
        if share < 1.0:
            maps[rng.random(maps.shape, dtype=np.float32) >= share] = -16
        src = torch.from_numpy(maps).to(dev)

        def call():
            _lib.check(_lib.lib().adf_point_cloud_device(
                n, src.data_ptr(), _lib.DEPTH_16S, W4 * 2, px * 2, W4, H4, C.byref(prm), None, -np.inf, np.inf, None, 0, 0, 0,
                points.data_ptr(), px * 12, None, 0, None, 0, px, counts.data_ptr(), ws.data_ptr(), ws.numel(), stream))

        med, best = timed(call, args.iters)
        valid = int(counts.sum().item())
        assert valid == int((maps != -16).sum())
        report("point list int16, %.0f %% valid (%d points)" % (100 * share, valid), med, best, n * px * 2 + valid * 12)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
