"""Device time of the matcher's view preparation (csrc/view_prep_kernels.hip): the fused call (half size + BGR2GRAY) and
the three unfused cases, HIP-event time per call, for 1 and 64 pairs of 3840 x 2160 BGR views and for one 1242 x 375 pair,
with the achieved GB/s on algorithmic bytes (source read once, destination written once) against the ~6.3 TB/s a
streaming kernel reaches on this part (DESIGN.md section 7's basis).  As the yardstick, the same result composed from
torch ops (int32 intermediates, bit-identical, checked) on the same tensors in the same run.  Then the sample's whole
default chain per 64 x 4K pairs: prepare -> StereoBM.computeBoth -> filter() with the full-size colour guide.

    python tools/view_prep_time.py [--iters N] [--pairs 64] [--no-chain]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import addingdisparityfiltering_amd as adf  # noqa: E402

HBM_ACHIEVABLE = 6.3e12


def torch_shrink(x):
    """The whole 2x2 cells only: an odd last row / column is cropped (the check below compares what this covers)."""
    s = x[:, :x.shape[1] // 2 * 2, :x.shape[2] // 2 * 2].to(torch.int32)
    s = s[:, 0::2, 0::2] + s[:, 0::2, 1::2] + s[:, 1::2, 0::2] + s[:, 1::2, 1::2]
    return (s + 2) >> 2


def torch_gray(c):
    return (c[..., 0] * 1868 + c[..., 1] * 9617 + c[..., 2] * 4899 + 8192) >> 14


TORCH = {
    "fused (half + gray)": lambda x: torch_gray(torch_shrink(x)).to(torch.uint8),
    "shrink colour": lambda x: torch_shrink(x).to(torch.uint8),
    "shrink gray": lambda x: torch_shrink(x).to(torch.uint8),
    "gray": lambda x: torch_gray(x.to(torch.int32)).to(torch.uint8),
}
OURS = {
    "fused (half + gray)": lambda x, d: adf.matcherViews(x, 0.5, True, dst=d),
    "shrink colour": lambda x, d: adf.resize(x, None, 0.5, 0.5, dst=d),
    "shrink gray": lambda x, d: adf.resize(x, None, 0.5, 0.5, dst=d),
    "gray": lambda x, d: adf.cvtColor(x, adf.COLOR_BGR2GRAY, dst=d),
}


def timed(fn, iters):
    """Median and minimum HIP-event ms of fn() over `iters` calls (after two warm-up calls)."""
    fn(); fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    return ms[len(ms) // 2], ms[0]


def views(n_images, H, W, dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.randint(0, 256, (n_images, H, W, 3), dtype=torch.uint8, device=dev, generator=g)


def one_geometry(pairs, W, H, iters, dev):
    x = views(2 * pairs, H, W, dev, pairs * 7 + W)
    gray_in = x[..., 1].contiguous()
    print("%d pair(s) of %d x %d BGR views (%d images per call)" % (pairs, W, H, 2 * pairs))
    fused_ms = torch_ms = None
    for name in OURS:
        src = gray_in if name == "shrink gray" else x
        exp = TORCH[name](src)
        dst = OURS[name](src, None)
        assert torch.equal(dst[:, :exp.shape[1], :exp.shape[2]], exp), "%s: the torch composition and the kernel disagree" % name
        nbytes = src.numel() + dst.numel()
        med, best = timed(lambda: OURS[name](src, dst), iters)
        tmed, tbest = timed(lambda: TORCH[name](src), max(3, iters // 4))
        print("  %-20s kernel median %8.4f ms (min %8.4f)  %7.1f MB algorithmic  %7.1f GB/s = %4.1f %% of 6.3 TB/s   |   "
              "torch ops median %8.3f ms (min %8.3f)  = %5.1f x"
              % (name, med, best, nbytes / 1e6, nbytes / med / 1e6, 100 * nbytes / (med * 1e-3) / HBM_ACHIEVABLE,
                 tmed, tbest, tmed / med))
        if name.startswith("fused"):
            fused_ms, torch_ms = med, tmed
        del exp, dst
    return fused_ms, torch_ms


def chain(pairs, W, H, iters, dev):
    """prepare -> computeBoth -> scaled filter on `pairs` pairs; the views are a textured image and its shifted copy."""
    from addingdisparityfiltering_amd import synthetic

    left, _, _ = synthetic.make_artificial_batch_torch(pairs, W, H, 3, 1, 64, dev)
    both = torch.stack([left, torch.roll(left, -24, dims=2)])                  # (2, pairs, H, W, 3): all left, then all right
    flat = both.view(2 * pairs, H, W, 3)
    h, w = adf.halfSize(H), adf.halfSize(W)
    small = torch.empty((2 * pairs, h, w), dtype=torch.uint8, device=dev)
    bm = adf.StereoBM.create(64, 7)
    wls = adf.createDisparityWLSFilter(bm)
    wls.setLambda(8000.0); wls.setSigmaColor(1.5)
    dl = torch.empty((pairs, h, w), dtype=torch.int16, device=dev)
    dr = torch.empty_like(dl)
    out = torch.empty((pairs, H, W), dtype=torch.int16, device=dev)

    def prepare():
        adf.matcherViews(flat, dst=small)

    def match():
        bm.computeBoth(small[:pairs], small[pairs:], dl, dr)

    def filt():
        wls.filter(dl, both[0], out, dr)

    def whole():
        prepare(); match(); filt()

    print("the sample's default chain, %d pairs of %d x %d colour views, StereoBM(64, 7) on %d x %d:" % (pairs, W, H, w, h))
    tot = 0.0
    for name, fn in (("prepare (matcherViews)", prepare), ("StereoBM.computeBoth", match), ("filter (scaled, wave solver)", filt)):
        med, best = timed(fn, iters)
        tot += med
        print("  %-30s median %8.3f ms (min %8.3f) per call = %7.4f ms per pair" % (name, med, best, med / pairs))
    med, best = timed(whole, iters)
    print("  %-30s median %8.3f ms (min %8.3f) per call = %7.4f ms per pair  (sum of the stages %.3f)"
          % ("all three, back to back", med, best, med / pairs, tot))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--no-chain", action="store_true")
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    print("view preparation, %d timed calls each; device %s" % (args.iters, torch.cuda.get_device_name(dev)))
    one_geometry(1, 1242, 375, args.iters, dev)
    one_geometry(1, 3840, 2160, args.iters, dev)
    fused, composed = one_geometry(args.pairs, 3840, 2160, args.iters, dev)
    print("condition (fused call not slower than the torch composition on %d x 4K pairs): %s (%.3f ms against %.3f ms)"
          % (args.pairs, "met" if fused <= composed else "MISSED", fused, composed))
    torch.cuda.empty_cache()
    if not args.no_chain:
        chain(args.pairs, 3840, 2160, max(5, args.iters // 3), dev)


if __name__ == "__main__":
    main()
