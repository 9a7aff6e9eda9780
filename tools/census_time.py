"""Times censusTransform alone on the device: python tools/census_time.py [--reps R] [W H n] COST:K [COST:K ...]
(COST: dense, sparse, mct-dense, mct-sparse, cs; the descriptors take turns on the same image in one process, R timed
windows each; the median, minimum and maximum of the windows are printed in microseconds per call, and the ratio of every
median to the first descriptor's)"""
import argparse
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
import addingdisparityfiltering_amd as adf

COST = {"dense": adf.SGBM_COST_CENSUS_DENSE, "sparse": adf.SGBM_COST_CENSUS_SPARSE, "mct-dense": adf.SGBM_COST_MCT_DENSE,
        "mct-sparse": adf.SGBM_COST_MCT_SPARSE, "cs": adf.SGBM_COST_CENSUS_CS}
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("args", nargs="+")
opt = ap.parse_args()
shape = [a for a in opt.args if ":" not in a]
specs = [a for a in opt.args if ":" in a]
W, H, n = (int(v) for v in (shape[:3] + ["3840", "2160", "1"][len(shape):]))
img = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (n, H, W), dtype=np.uint8)).cuda()
dst = torch.empty((n, H, W), dtype=torch.int64, device="cuda")
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
calls = [(s, COST[s.split(":")[0]], int(s.split(":")[1])) for s in specs]
for _, ctype, k in calls:                        # warm up: code objects
    for _ in range(3):
        adf.censusTransform(img, k, ctype, dst)
torch.cuda.synchronize()
inner = max(1, int(4e8 // (n * W * H)))          # calls per timed window: a few milliseconds
times = {s: [] for s, _, _ in calls}
for _ in range(opt.reps):
    for s, ctype, k in calls:
        e0.record()
        for _ in range(inner):
            adf.censusTransform(img, k, ctype, dst)
        e1.record(); torch.cuda.synchronize()
        times[s].append(1e3 * e0.elapsed_time(e1) / inner)
first = float(np.median(times[specs[0]]))
for s in specs:
    med = float(np.median(times[s]))
    print("censusTransform %dx%d, %d image(s), %s: %.1f us (min %.1f max %.1f), %.3f x %s" % (W, H, n, s, med, min(times[s]), max(times[s]), med / first, specs[0]))
