"""Times the device semi-global matcher (left view, then the right-view matcher of createRightMatcher) on synthetic
pairs: python tools/sgbm_time.py [--cost {bt,dense,sparse,mct-dense,mct-sparse,cs}] [--census-size K] [--against-bt] [--reps R] [W H ndisp block n channels mode]
(mode: 2 = MODE_SGBM_3WAY (default), 0 = MODE_SGBM, 1 = MODE_HH; --cost: the Birchfield-Tomasi block cost (default) or a
census descriptor with a Hamming distance, adf_sgbm_set_cost; --against-bt: the same two handles also run the
Birchfield-Tomasi cost, the two costs taking turns, and the ratio of the two whole compute() times is printed)"""
import argparse
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
import addingdisparityfiltering_amd as adf

ap = argparse.ArgumentParser()
ap.add_argument("--cost", choices=("bt", "dense", "sparse", "mct-dense", "mct-sparse", "cs"), default="bt")
ap.add_argument("--census-size", type=int, default=7)
ap.add_argument("--against-bt", action="store_true")
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("shape", nargs="*")
opt = ap.parse_args()
W, H, nd, bs, n, cn, mode = (int(v) for v in (opt.shape[:7] + ["3840", "2160", "256", "3", "2", "1", "2"][len(opt.shape):]))
rng = np.random.default_rng(0)
shape = (n, H, W + 64) + ((cn,) if cn > 1 else ())
base = rng.integers(0, 256, shape, dtype=np.uint8)
left = torch.from_numpy(np.ascontiguousarray(base[:, :, 32:32 + W])).cuda()
right = torch.from_numpy(np.ascontiguousarray(np.roll(base, -9, 2)[:, :, 32:32 + W])).cuda()
lm = adf.StereoSGBM.create(0, nd, bs)
lm.setP1(24 * bs * bs); lm.setP2(96 * bs * bs); lm.setPreFilterCap(63); lm.setMode(mode)
lm.setCensusSize(opt.census_size)
wls = adf.createDisparityWLSFilter(lm)                 # samples/disparity_filtering.cpp:166-172
rm = adf.createRightMatcher(lm)
COST = {"bt": adf.SGBM_COST_BT, "dense": adf.SGBM_COST_CENSUS_DENSE, "sparse": adf.SGBM_COST_CENSUS_SPARSE,
        "mct-dense": adf.SGBM_COST_MCT_DENSE, "mct-sparse": adf.SGBM_COST_MCT_SPARSE, "cs": adf.SGBM_COST_CENSUS_CS}
costs = ["bt", opt.cost] if opt.against_bt and opt.cost != "bt" else [opt.cost]
dl = torch.empty((n, H, W), dtype=torch.int16, device="cuda")
dr = torch.empty_like(dl)
e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]


def both_views(cost):
    """(left, right) milliseconds of one compute() per view with `cost` (a handle changes cost between calls)."""
    lm.setCostType(COST[cost]); rm.setCostType(COST[cost])
    e[0].record(); lm.compute(left, right, dl); e[1].record(); rm.compute(right, left, dr); e[2].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])


for c in costs:                                        # warm-up: the workspace, the code objects
    both_views(c)
times = {c: [0.0, 0.0] for c in costs}
for _ in range(opt.reps):
    for c in costs:
        tl, tr = both_views(c)
        times[c][0] += tl / opt.reps; times[c][1] += tr / opt.reps
px = n * W * H
for c in costs:
    tl, tr = times[c]
    name = "Birchfield-Tomasi" if c == "bt" else "census %s %d" % (c, opt.census_size)
    print("semi-global matcher (%s, %s): %dx%dx%d ndisp %d block %d, %d pairs: left %.2f ms + right %.2f ms = %.3f ms/pair both views "
          "(%.2f Gpx/s, %.1f G(px*disp)/s per view)" % ({2: "3-way", 0: "5 paths", 1: "8 paths"}[mode], name, W, H, cn, nd, bs, n, tl, tr, (tl + tr) / n,
                                                        px / (tl + tr) / 1e6, 2 * px * nd / (tl + tr) / 1e6))
if len(costs) == 2:
    print("  census / Birchfield-Tomasi, whole compute(), both views, mean of %d alternating runs: %.3f" % (opt.reps, sum(times[costs[1]]) / sum(times["bt"])))
