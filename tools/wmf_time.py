"""Device time of weightedMedianFilter (csrc/wmf_kernels.hip) per 3840 x 2160 map: events around 20 calls after a warm-up
call, the median and the minimum.

  * input: device StereoBM(64, 9) output of the KITTI pair tiled to 4K (holes of -16 included, ignoreValue = -16), the
    gray left view tiled the same way as the joint; the 3-channel joint is the colour view; the float map is the int16
    map / 16;
  * cases: int16 with a gray joint at r = 3, 7, 15; a 3-channel joint at r = 7; float32 at r = 7; sigma = 10;
  * next to each time: the sweeps of the window a wave performs (1 for the total + the selection steps, which a wave
    repeats until its slowest pixel is done), counted by a NumPy model of the kernel's search on a 256 x 256 crop, the
    tap reads per pixel that implies, (2r+1)^2 x sweeps, and the tap rate against the LDS limit: a tap is one 8-byte read
    (2 LDS cycles per wave) and, for a gray joint, one 4-byte table read (2 more when free of conflicts): 32 / 16 taps
    per clock per CU, 256 CUs at 2.4 GHz.

    python tools/wmf_time.py [--iters N]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H4, W4 = 2160, 3840
SIGMA, IGNORE = 10.0, -16
CUS, CLOCK = 256, 2.4e9


def inputs(dev):
    """(disparity int16, gray joint, colour joint) at 4K, as numpy arrays."""
    import torch
    from PIL import Image

    import addingdisparityfiltering_amd as adf

    left = Image.open(os.path.join(ROOT, "tests", "golden", "kitti_left.bmp"))
    right = Image.open(os.path.join(ROOT, "tests", "golden", "kitti_right.bmp"))
    gl, gr, colour = np.array(left.convert("L")), np.array(right.convert("L")), np.array(left.convert("RGB"))
    d = adf.StereoBM.create(64, 9).compute(torch.from_numpy(gl).to(dev), torch.from_numpy(gr).to(dev)).cpu().numpy()
    reps = (H4 // d.shape[0] + 1, W4 // d.shape[1] + 1)
    tile = lambda a: np.ascontiguousarray(np.tile(a, reps + (1,) * (a.ndim - 2))[:H4, :W4])
    return tile(d), tile(gl), tile(colour)


def wave_sweeps(joint, src, r, table, ignore):
    """The kernel's search on one crop, in NumPy: per pixel the sweeps of the window (1 + selection steps), and the mean
    over waves (32 x 2 pixels) of the largest count among a wave's pixels."""
    from wmf_ref import keys_of

    H, W = src.shape
    MARK = np.int64(0xFFFFFFFF)
    used = src.astype(np.float64) != float(ignore)
    if src.dtype == np.float32:
        used &= ~np.isnan(src)
    key = np.where(used, keys_of(src), MARK)
    j = joint.astype(np.int64).reshape(H, W, -1)
    n = 2 * r + 1
    K = np.full((n * n, H, W), MARK, np.int64)
    Wt = np.zeros((n * n, H, W), np.int64)
    k = 0
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            ys, ye, xs, xe = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            q, p = (slice(ys + dy, ye + dy), slice(xs + dx, xe + dx)), (slice(ys, ye), slice(xs, xe))
            K[k][p] = key[q]
            Wt[k][p] = np.where(key[q] != MARK, table[((j[p] - j[q]) ** 2).sum(-1)], 0)
            k += 1
    tot = Wt.sum(0)
    lo, hi = K.min(0), np.where(K != MARK, K, -1).max(0)
    sweeps = np.ones((H, W), np.int64)
    live = (tot > 0) & (lo < hi)
    while live.any():
        mid = lo + (hi - lo) // 2
        le = K <= mid[None]
        L = np.where(le, Wt, 0).sum(0)
        below = np.maximum(lo, np.where(le, K, -1).max(0))
        above = np.minimum(hi, np.where(le, MARK, K).min(0))
        down = 2 * L >= tot
        hi = np.where(live & down, below, hi)
        lo = np.where(live & ~down, above, lo)
        sweeps += live
        live &= lo < hi
    waves = sweeps[:H // 2 * 2, :W // 32 * 32].reshape(H // 2, 2, W // 32, 32).max(axis=(1, 3))
    return float(sweeps.mean()), float(waves.mean())


def time_case(joint, src, r, ignore, iters, dev):
    import torch

    import addingdisparityfiltering_amd as adf

    tj, ts = torch.from_numpy(joint).to(dev), torch.from_numpy(src).to(dev)
    dst = torch.empty_like(ts)
    adf.weightedMedianFilter(tj, ts, r, SIGMA, ignoreValue=ignore, dst=dst)       # warm-up: the table's upload, the code object
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for e0, e1 in ev:
        e0.record()
        adf.weightedMedianFilter(tj, ts, r, SIGMA, ignoreValue=ignore, dst=dst)
        e1.record()
    torch.cuda.synchronize()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    filled = float(((ts == ignore) & (dst != ignore)).float().mean().item())
    return ms[len(ms) // 2], ms[0], filled


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args(argv)
    import torch

    import addingdisparityfiltering_amd as adf

    dev = torch.device("cuda:0")
    d16, gray, colour = inputs(dev)
    f32 = (d16.astype(np.float32) / 16.0).astype(np.float32)
    table = adf.wmfWeightTable(SIGMA).astype(np.int64)
    cases = [("int16, gray joint, r = 3", gray, d16, 3), ("int16, gray joint, r = 7", gray, d16, 7),
             ("int16, gray joint, r = 15", gray, d16, 15), ("int16, 3-channel joint, r = 7", colour, d16, 7),
             ("float32, gray joint, r = 7", gray, f32, 7)]
    print("weightedMedianFilter, %d x %d, sigma %g, ignoreValue %d, %d timed calls each; device %s"
          % (W4, H4, SIGMA, IGNORE, args.iters, torch.cuda.get_device_name(dev)))
    for name, joint, src, r in cases:
        ignore = IGNORE if src.dtype != np.float32 else IGNORE / 16.0    # the float map is the int16 map / 16, its holes too
        med, best, filled = time_case(joint, src, r, ignore, args.iters, dev)
        c = 128 if r > 7 else 256                                         # the model's crop
        mean_sw, wave_sw = wave_sweeps(joint[400:400 + c, 896:896 + c], src[400:400 + c, 896:896 + c], r, table, ignore)
        taps = (2 * r + 1) ** 2 * wave_sw
        rate = W4 * H4 * taps / (med * 1e-3)
        limit = CUS * CLOCK * (16 if joint.ndim == 2 else 32)
        print("%-30s median %8.3f ms  (min %8.3f)   sweeps/pixel %5.2f, per wave %5.2f   tap reads/pixel %8.0f   %6.2f Ttap/s = %4.1f %% of the LDS limit   holes filled %5.2f %% of pixels"
              % (name, med, best, mean_sw, wave_sw, taps, rate / 1e12, 100.0 * rate / limit, filled * 100))


if __name__ == "__main__":
    main()
