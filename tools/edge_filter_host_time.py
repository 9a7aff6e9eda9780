"""Host time per call of the five edge-aware filters (weightedMedianFilter, guidedFilter, dtFilter, jointBilateralFilter,
rollingGuidanceFilter) on a 64 x 48 int16 map with a gray guide, where the kernels are short and the host half is what a
call costs:

  * issue: the host time to queue one device-entry call -- perf_counter around 2000 calls on CUDA tensors with no
    synchronisation inside, the median, minimum and maximum of 7 such batches (us per call);
  * host entry: the wall clock of one call on numpy arrays (copies in, the filter, copy out, two synchronisations) -- the
    median and minimum of 300 calls (us).

To compare two commits, run it in alternating processes, `--package-root DIR` naming a checkout of the other commit with
its library built: that tree's Python package and library are measured instead of this tree's.

    python tools/edge_filter_host_time.py [--package-root DIR]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 48, 64


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--package-root", default=ROOT, help="the checkout whose package and library are measured")
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torch

    import addingdisparityfiltering_amd as adf

    dev = torch.device("cuda:0")
    print("package %s; %d x %d int16 map, gray guide; device %s" % (os.path.dirname(os.path.abspath(adf.__file__)), W, H, torch.cuda.get_device_name(dev)), flush=True)
    rng = np.random.default_rng(7)
    guide = rng.integers(0, 256, (H, W), dtype=np.uint8)
    src = rng.integers(-500, 500, (H, W)).astype(np.int16)
    calls = {
        "wmf": lambda g, s, d: adf.weightedMedianFilter(g, s, 2, 20.0, dst=d),
        "gf": lambda g, s, d: adf.guidedFilter(g, s, 2, 50.0, dst=d),
        "dt": lambda g, s, d: adf.dtFilter(g, s, 8.0, 30.0, dst=d),
        "jbf": lambda g, s, d: adf.jointBilateralFilter(g, s, 5, 30.0, 2.0, dst=d),
        "rgf": lambda g, s, d: adf.rollingGuidanceFilter(s, 5, 40.0, 2.0, 3, dst=d),
    }
    tg, ts = torch.from_numpy(guide).to(dev), torch.from_numpy(src).to(dev)
    td, hd = torch.empty_like(ts), np.empty_like(src)
    for name, call in calls.items():
        for _ in range(20):                                                  # warm-up: the tables, the code objects, the scratch
            call(tg, ts, td)
        torch.cuda.synchronize()
        issue = []
        for _ in range(7):
            t0 = time.perf_counter()
            for _ in range(2000):
                call(tg, ts, td)
            issue.append((time.perf_counter() - t0) / 2000 * 1e6)
            torch.cuda.synchronize()
        issue.sort()
        for _ in range(20):
            call(guide, src, hd)
        wall = []
        for _ in range(300):
            t0 = time.perf_counter()
            call(guide, src, hd)
            wall.append((time.perf_counter() - t0) * 1e6)
        wall.sort()
        print("%-4s issue: median %6.2f us (min %6.2f, max %6.2f)   host entry: median %6.1f us (min %6.1f)"
              % (name, issue[3], issue[0], issue[-1], wall[150], wall[0]), flush=True)


if __name__ == "__main__":
    main()
