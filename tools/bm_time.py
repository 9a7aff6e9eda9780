"""Times the device block matcher (both views) on synthetic pairs:
python tools/bm_time.py [--cost {sad,dense,sparse,mct-dense,mct-sparse,cs}] [--census-size K] [--against-sad | --against COST:K] [--reps R] [W H ndisp wsz n [uniq texture]]
(uniq / texture: uniquenessRatio and textureThreshold of the LEFT matcher, default 0 as the filter factory sets them;
--cost: SAD on the x-Sobel prefiltered views (default) or a census descriptor with a Hamming distance, adf_bm_set_cost;
--against-sad: a second handle runs the SAD cost, the two costs take turns with computeBoth -- the filter's settings, texture
and uniqueness 0 -- and the median time of each and their ratio are printed; --against COST:K: the same with another
census cost as the second handle, e.g. the descriptor with the same number of byte planes)"""
import argparse
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
import addingdisparityfiltering_amd as adf

COST = {"sad": adf.BM_COST_SAD, "dense": adf.BM_COST_CENSUS_DENSE, "sparse": adf.BM_COST_CENSUS_SPARSE,
        "mct-dense": adf.BM_COST_MCT_DENSE, "mct-sparse": adf.BM_COST_MCT_SPARSE, "cs": adf.BM_COST_CENSUS_CS}
ap = argparse.ArgumentParser()
ap.add_argument("--cost", choices=tuple(COST), default="sad")
ap.add_argument("--census-size", type=int, default=7)
ap.add_argument("--against-sad", action="store_true")
ap.add_argument("--against", metavar="COST:K", default=None)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("shape", nargs="*")
opt = ap.parse_args()
W, H, nd, wsz, n = (int(v) for v in (opt.shape[:5] + ["3840", "2160", "256", "15", "4"][len(opt.shape):]))
rng = np.random.default_rng(0)
base = rng.integers(0, 256, (n, H, W + 64), dtype=np.uint8)
left = torch.from_numpy(np.ascontiguousarray(base[:, :, 32:32 + W])).cuda()
right = torch.from_numpy(np.ascontiguousarray(np.roll(base, -9, 2)[:, :, 32:32 + W])).cuda()
dl = torch.empty((n, H, W), dtype=torch.int16, device="cuda")
dr = torch.empty_like(dl)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
name = opt.cost if opt.cost == "sad" else "%s %d" % (opt.cost, opt.census_size)


def matcher(cost, size=opt.census_size):
    m = adf.StereoBM.create(nd, wsz)
    m.setTextureThreshold(0); m.setUniquenessRatio(0)
    m.setCostType(COST[cost]); m.setCensusSize(size)
    return m


def timed(fn, reps):
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


if opt.against_sad or opt.against:
    if opt.cost == "sad" or len(opt.shape) > 5:
        sys.exit("--against-sad / --against compare a census cost with another cost in the filter's configuration")
    if opt.against:
        bcost, bsize = opt.against.split(":")
        base_name, base = "%s %s" % (bcost, bsize), matcher(bcost, int(bsize))
    else:
        base_name, base = "sad", matcher("sad")
    ms = {base_name: base, name: matcher(opt.cost)}
    times = {c: [] for c in ms}
    for c, m in ms.items():                      # warm up: code objects, the view buffers
        for _ in range(2):
            m.computeBoth(left, right, dl, dr)
    torch.cuda.synchronize()
    inner = max(1, int(40 // max(1, n * W * H * nd / 1.3e8)))     # calls per timed window: a few milliseconds at the least
    for _ in range(max(opt.reps, 5)):            # the two costs take turns
        for c, m in ms.items():
            times[c].append(timed(lambda: m.computeBoth(left, right, dl, dr), inner))
    med = {c: float(np.median(t)) for c, t in times.items()}
    print("matcher both views, one launch: %dx%d ndisp %d block %d, %d pairs: %s %.3f ms (min %.3f max %.3f), %s %.3f ms "
          "(min %.3f max %.3f), ratio %.3f" % (W, H, nd, wsz, n, base_name, med[base_name], min(times[base_name]), max(times[base_name]), name,
                                              med[name], min(times[name]), max(times[name]), med[name] / med[base_name]))
    sys.exit(0)

lm = matcher(opt.cost)
rm = adf.createRightMatcher(lm)
if len(opt.shape) > 5:
    lm.setUniquenessRatio(int(opt.shape[5])); rm.setUniquenessRatio(int(opt.shape[5]))
if len(opt.shape) > 6:
    lm.setTextureThreshold(int(opt.shape[6])); rm.setTextureThreshold(int(opt.shape[6]))


def two_calls():
    lm.compute(left, right, dl); rm.compute(right, left, dr)


for _ in range(2):
    two_calls()
torch.cuda.synchronize()
ms = timed(two_calls, opt.reps)
px = n * W * H
both = None
if len(opt.shape) <= 5:                       # the filter's configuration: also time both views in one launch
    for _ in range(2):
        lm.computeBoth(left, right, dl, dr)
    torch.cuda.synchronize()
    both = timed(lambda: lm.computeBoth(left, right, dl, dr), opt.reps)
print("matcher%s both views: %dx%d ndisp %d block %d, %d pairs: %.2f ms  (%.3f ms/pair, %.2f Gpx/s, %.1f G(px*disp)/s per view)" %
      ("" if opt.cost == "sad" else " (%s)" % name, W, H, nd, wsz, n, ms, ms / n, px / ms / 1e6, 2 * px * nd / ms / 1e6) +
      ("" if both is None else "; one launch for both views: %.2f ms (%.3f ms/pair)" % (both, both / n)))
