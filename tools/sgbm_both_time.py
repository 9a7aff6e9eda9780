"""Times the semi-global matcher's ways to both views' maps on synthetic pairs, hipEvent times per call:
    compute            the left view alone (adf_sgbm_compute_device)
    two computes       the left matcher, then the right matcher of createRightMatcher on its own handle
    both (matcher)     adf_sgbm_compute_both_device, ADF_SGBM_RIGHT_MATCHER
    both (volume)      adf_sgbm_compute_both_device, ADF_SGBM_RIGHT_FROM_VOLUME
python tools/sgbm_both_time.py [--lib PATH] [--reps R] [--label TEXT] [W H ndisp block n]
MODE_SGBM_3WAY, P1 = 24*w*w, P2 = 96*w*w, preFilterCap 63, disp12MaxDiff 1000000, one channel.  The legs take turns
inside every repetition; each line gives the median and the range over the repetitions.  --lib: another build of the
library, straight on its C-ABI (an older build without the both-views entries runs the first two legs only), so that
two builds can be compared in one session by running this tool on each in turn."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "addingdisparityfiltering_amd", "libadf_wls.so"))
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--label", default="")
ap.add_argument("shape", nargs="*")
opt = ap.parse_args()
W, H, nd, bs, n = (int(v) for v in (opt.shape[:5] + ["3840", "2160", "256", "3", "1"][len(opt.shape):]))

lib = C.CDLL(opt.lib)
vp, i32, pd = C.c_void_p, C.c_int, C.c_ssize_t
lib.adf_sgbm_create.argtypes = [C.POINTER(vp), i32, i32, i32]
lib.adf_sgbm_set_params.argtypes = [vp] + [i32] * 8
lib.adf_sgbm_set_disp12_max_diff.argtypes = [vp, i32]
lib.adf_sgbm_destroy.argtypes = [vp]
lib.adf_sgbm_destroy.restype = None
lib.adf_last_error.restype = C.c_char_p
plane = [vp, pd, pd]
lib.adf_sgbm_compute_device.argtypes = [vp, i32] + plane * 2 + [i32] * 3 + plane + [vp]
has_both = hasattr(lib, "adf_sgbm_compute_both_device")
if has_both:
    lib.adf_sgbm_compute_both_device.argtypes = [vp, i32] + plane * 2 + [i32] * 3 + plane * 2 + [i32, vp]


def ok(rc):
    if rc:
        sys.exit("adf error %d: %s" % (rc, lib.adf_last_error().decode()))


def matcher(md):
    h = vp()
    ok(lib.adf_sgbm_create(C.byref(h), md, nd, bs))
    ok(lib.adf_sgbm_set_params(h, md, nd, bs, 24 * bs * bs, 96 * bs * bs, 63, 0, 2))
    ok(lib.adf_sgbm_set_disp12_max_diff(h, 1000000))
    return h


rng = np.random.default_rng(0)
base = rng.integers(0, 256, (n, H, W + 64), dtype=np.uint8)
left = torch.from_numpy(np.ascontiguousarray(base[:, :, 32:32 + W])).cuda()
right = torch.from_numpy(np.ascontiguousarray(np.roll(base, -9, 2)[:, :, 32:32 + W])).cuda()
dl = torch.empty((n, H, W), dtype=torch.int16, device="cuda")
dr = torch.empty_like(dl)
lm, rm = matcher(0), matcher(1 - nd)                   # createRightMatcher: minDisparity = -(0 + nd) + 1
stream = torch.cuda.current_stream().cuda_stream


def views(a, b):
    return (a.data_ptr(), W, W * H, b.data_ptr(), W, W * H, 1, W, H)


def maps(*ms):
    return tuple(v for m in ms for v in (m.data_ptr(), 2 * W, 2 * W * H))


def compute():
    ok(lib.adf_sgbm_compute_device(lm, n, *views(left, right), *maps(dl), stream))


def two_computes():
    compute()
    ok(lib.adf_sgbm_compute_device(rm, n, *views(right, left), *maps(dr), stream))


def both(source):
    return lambda: ok(lib.adf_sgbm_compute_both_device(lm, n, *views(left, right), *maps(dl, dr), source, stream))


legs = [("compute (left view only)", compute), ("two computes (left + right matcher)", two_computes)]
if has_both:
    legs += [("computeBoth, right matcher's map", both(0)), ("computeBoth, right map from the volume", both(1))]
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
times = {name: [] for name, _ in legs}
for rep in range(opt.reps + 1):                        # repetition 0 is the warm-up: workspaces, code objects
    for name, fn in legs:
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        if rep:
            times[name].append(e0.elapsed_time(e1))
print("semi-global matcher (3-way)%s: %dx%d ndisp %d block %d, %d pair(s) per call, %d repetitions, ms per call: median [min .. max]"
      % (" " + opt.label if opt.label else "", W, H, nd, bs, n, opt.reps))
for name, _ in legs:
    t = times[name]
    print("  %-40s %8.3f  [%.3f .. %.3f]   %.3f ms per pair" % (name, statistics.median(t), min(t), max(t), statistics.median(t) / n))
if has_both:
    two, vol = statistics.median(times[legs[1][0]]), statistics.median(times[legs[3][0]])
    print("  volume source / two computes: %.3f" % (vol / two))
for h in (lm, rm):
    lib.adf_sgbm_destroy(h)
