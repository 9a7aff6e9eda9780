"""Device time of filterSpeckles (csrc/speckle_kernels.hip), ms per map, with a caller workspace:

  * one 4K map, a batch of 16 4K maps, the tutorial-size map (ambush, 1024 x 436);
  * realistic input = device StereoBM output: the KITTI pair's map tiled to 3840 x 2160 (each map of the batch
    starts at another offset), the ambush pair's StereoBM(128, 9) map as it is;
  * adversarial input: one serpentine component through every tile, and a checkerboard of singletons;
  * for context, the CPU restatement tests/speckle_ref.c on the same 4K map, one thread.

Each timed call starts from a fresh copy of its input (the copy is outside the events).  Target: <= 0.1 ms
per 4K map in a batch of 16, <= 0.2 ms for one 4K map, adversarial within 4x of realistic.

    python tools/speckle_time.py [--iters N] [--json OUT]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H4, W4 = 2160, 3840
NV, MAX_SIZE, MAX_DIFF = -16, 100, 32


def kitti_4k(n, dev):
    import torch
    from PIL import Image

    import addingdisparityfiltering_amd as adf

    gl = np.array(Image.open(os.path.join(ROOT, "tests", "golden", "kitti_left.bmp")).convert("L"))
    gr = np.array(Image.open(os.path.join(ROOT, "tests", "golden", "kitti_right.bmp")).convert("L"))
    d = adf.StereoBM.create(64, 9).compute(torch.from_numpy(gl).to(dev), torch.from_numpy(gr).to(dev)).cpu().numpy()
    reps = np.tile(d, (H4 // d.shape[0] + 2, W4 // d.shape[1] + 2))
    return np.stack([reps[(37 * k) % d.shape[0]:][:H4, (101 * k) % d.shape[1]:][:, :W4] for k in range(n)])


def ambush_map(dev):
    import torch

    import addingdisparityfiltering_amd as adf
    import tutorial_replay as tr

    left, right, _, _ = tr.load_fixtures()
    bm = adf.StereoBM.create(tr.RAW_NUM_DISP, tr.RAW_WSIZE)
    return bm.compute(torch.from_numpy(tr.bgr2gray(left)).to(dev), torch.from_numpy(tr.bgr2gray(right)).to(dev)).cpu().numpy()


def time_filter(maps, iters, dev):
    """Median and minimum device ms per call of filterSpeckles on `maps` ((H,W) or (N,H,W)), and removed share."""
    import torch

    import addingdisparityfiltering_amd as adf

    src = torch.from_numpy(np.ascontiguousarray(maps)).to(dev)
    work = src.clone()
    n, H, W = (1,) + src.shape if src.dim() == 2 else tuple(src.shape)
    buf = torch.empty(adf.speckleWorkspaceBytes(n, H, W), dtype=torch.uint8, device=dev)
    adf.filterSpeckles(work, NV, MAX_SIZE, MAX_DIFF, buf)                   # warm-up
    removed = float(((work != src) & (src != NV)).float().mean().item())
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for e0, e1 in ev:
        work.copy_(src)
        e0.record()
        adf.filterSpeckles(work, NV, MAX_SIZE, MAX_DIFF, buf)
        e1.record()
    torch.cuda.synchronize()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    return ms[len(ms) // 2], ms[0], n, removed


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    import torch

    from test_gpu_speckles import serpentine
    from test_speckle_ref import speckle_ref

    dev = torch.device("cuda:0")
    k16 = kitti_4k(16, dev)
    yy, xx = np.mgrid[0:H4, 0:W4]
    checker = np.where((xx + yy) % 2 == 0, 100, 300).astype(np.int16)
    serp = serpentine(H4, W4)
    amb = ambush_map(dev)
    cases = [
        ("4K realistic (KITTI BM, tiled), 1 map", k16[0]),
        ("4K realistic (KITTI BM, tiled), batch 16", k16),
        ("tutorial size (ambush BM(128,9), 1024x436), 1 map", amb),
        ("4K serpentine, 1 map", serp),
        ("4K serpentine, batch 16", np.broadcast_to(serp, (16, H4, W4))),
        ("4K checkerboard of singletons, 1 map", checker),
        ("4K checkerboard of singletons, batch 16", np.broadcast_to(checker, (16, H4, W4))),
    ]
    print("filterSpeckles(newVal %d, maxSpeckleSize %d, maxDiff %d), caller workspace, %d timed calls each; device %s"
          % (NV, MAX_SIZE, MAX_DIFF, args.iters, torch.cuda.get_device_name(dev)))
    rows = []
    for name, maps in cases:
        med, best, n, removed = time_filter(maps, args.iters, dev)
        rows.append(dict(case=name, maps=n, median_ms=med, min_ms=best, ms_per_map=med / n, removed_share=removed))
        print("%-52s median %8.3f ms  (min %8.3f)  = %7.4f ms/map   removed %5.2f %% of pixels"
              % (name, med, best, med / n, removed * 100))
    t = time.perf_counter()
    speckle_ref(k16[0], NV, MAX_SIZE, MAX_DIFF)
    cpu = (time.perf_counter() - t) * 1e3
    rows.append(dict(case="CPU restatement (tests/speckle_ref.c, 1 thread), 4K realistic", ms_per_map=cpu))
    print("%-52s %8.1f ms/map" % ("CPU restatement (speckle_ref.c, 1 thread), 4K realistic", cpu))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
