"""Host-visible time of the matchers' calls on one 1242 x 375 frame (64 disparities, block 15; semi-global: block 3):
per call the wall time until the call returns (the host's share: Python, ctypes, checks, plan, launches) and the wall
time of call + synchronisation; medians over 400 calls (semi-global: 100) after 30 warm-up calls.
    python tools/matcher_call_time.py"""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
import addingdisparityfiltering_amd as adf

W, H, ND = 1242, 375, 64
rng = np.random.default_rng(0)
base = rng.integers(0, 256, (H, W + 64), dtype=np.uint8)
hl = np.ascontiguousarray(base[:, 32:32 + W]); hr = np.ascontiguousarray(np.roll(base, -9, 1)[:, 32:32 + W])
dl, dr = torch.from_numpy(hl).cuda(), torch.from_numpy(hr).cuda()
o = [torch.empty((H, W), dtype=torch.int16, device="cuda") for _ in range(4)]
ho = [np.empty((H, W), np.int16) for _ in range(2)]
bm = adf.StereoBM.create(ND, 15); bm.setTextureThreshold(0); bm.setUniquenessRatio(0)
bmc = adf.StereoBM.create(ND, 15); bmc.setTextureThreshold(0); bmc.setUniquenessRatio(0)
bmc.setCostType(adf.BM_COST_CENSUS_DENSE); bmc.setCensusSize(7)
sg = adf.StereoSGBM.create(0, ND, 3); sg.setP1(24 * 9); sg.setP2(96 * 9); sg.setMode(adf.StereoSGBM.MODE_SGBM_3WAY)
CASES = [
    ("BM compute, device", lambda: bm.compute(dl, dr, o[0])),
    ("BM computeBoth, device", lambda: bm.computeBoth(dl, dr, o[0], o[1])),
    ("BM computeWithCost, device", lambda: bm.computeWithCost(dl, dr, o[0], o[2])),
    ("BM computeBothWithCost, device", lambda: bm.computeBothWithCost(dl, dr, o[0], o[1], o[2], o[3])),
    ("BM census computeBothWithCost, device", lambda: bmc.computeBothWithCost(dl, dr, o[0], o[1], o[2], o[3])),
    ("BM compute, host arrays", lambda: bm.compute(hl, hr, ho[0])),
    ("BM computeWithCost, host arrays", lambda: bm.computeWithCost(hl, hr, ho[0], ho[1])),
    ("SGBM compute, device", lambda: sg.compute(dl, dr, o[0])),
    ("SGBM compute, host arrays", lambda: sg.compute(hl, hr, ho[0])),
]
for name, fn in CASES:
    n = 400 if "SGBM" not in name else 100
    for _ in range(30):
        fn()
    torch.cuda.synchronize()
    ret, whole = [], []
    for _ in range(n):
        t0 = time.perf_counter(); fn(); t1 = time.perf_counter(); torch.cuda.synchronize(); t2 = time.perf_counter()
        ret.append(t1 - t0); whole.append(t2 - t0)
    print("%-40s | returns after %8.2f us | call + sync %8.2f us" % (name, 1e6 * np.median(ret), 1e6 * np.median(whole)), flush=True)
