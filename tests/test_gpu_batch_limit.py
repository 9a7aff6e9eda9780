"""The second iteration of THE batch loop (csrc/adf_host.h: for_batches): every stateless operator on a batch one image
longer than a single launch holds -- L = 65535 images for most, 65535 x 4 for the two sampling calls, whose grid rows serve
four images each.  The launch of the second iteration re-points every pointer of the call by L images (and the per-map
workspace slots with them), so images 0, L - 1, L and n - 1 of the batched result must equal, bit for bit, the single-image
call on each of them, and those equal the operator's NumPy / C restatement.

The images are tiny (the largest buffer is about 5 MB) and pseudo-random, image k from a splitmix64 stream seeded with k: no
two images are alike, so a pointer that is off by any number of images shows."""
import numpy as np
import pytest

import rectify_ref
import reproject_ref
from census_ref import census_transform
from test_reproject_ref import rectified_q
from test_speckle_ref import speckle_ref
from test_view_prep_ref import view_prep_ref

pytestmark = pytest.mark.gpu

L = 65535                                              # images per launch: the grid's y / z limit
Q = rectified_q()
# a model whose coordinates fall between the pixels of a 2 x 2 source: mapx = u + 0.25, mapy = v + 0.5
K_SHIFT = np.array([[1.0, 0.0, 0.25], [0.0, 1.0, 0.5], [0.0, 0.0, 1.0]])
MODEL = (K_SHIFT, None, None, np.eye(3))
BORDER = 9


def images(n, shape, lo, hi, dtype):
    """(n,) + shape values in [lo, hi): image k is the splitmix64 stream of seed k."""
    k = np.arange(1, n + 1, dtype=np.uint64)[:, None] * np.uint64(0x9E3779B97F4A7C15)
    x = k + np.arange(1, int(np.prod(shape)) + 1, dtype=np.uint64)[None, :] * np.uint64(0xD1B54A32D192ED03)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    x ^= x >> np.uint64(31)
    return (lo + (x % np.uint64(hi - lo)).astype(np.int64)).astype(dtype).reshape((n,) + tuple(shape))


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a)
    return a.view(np.uint8)


def check(n, per_launch, batched, single, reference):
    """batched[k] / single(k) / reference(k): image k of the batched result, the single-image call on it, the restatement."""
    assert n > per_launch
    picks = sorted({0, per_launch - 1, per_launch, n - 1})
    ones = [single(k) for k in picks]
    for k, one in zip(picks, ones):
        assert np.array_equal(bits(batched[k]), bits(one)), "image %d of the batch differs from the single call" % k
        assert np.array_equal(bits(one), bits(reference(k))), "the single call on image %d differs from the reference" % k
    assert len({bits(o).tobytes() for o in ones}) > 1                # the results tell the images apart


@pytest.mark.parametrize("call", ["matcherViews", "resize"])
def test_view_prep(adf, call):
    n = L + 2
    src = images(n, (2, 2), 0, 256, np.uint8)
    t = _dev(src)
    run = (lambda v: adf.matcherViews(v)) if call == "matcherViews" else (lambda v: adf.resize(v, fx=0.5, fy=0.5))
    out = run(t)
    assert tuple(out.shape) == (n, 1, 1)
    check(n, L, out, lambda k: run(t[k]), lambda k: view_prep_ref(src[k], True, False))


def test_census_transform(adf):
    n = L + 2
    src = images(n, (3, 3), 0, 256, np.uint8)
    t = _dev(src)
    out = adf.censusTransform(t, 3, adf.SGBM_COST_CENSUS_DENSE)
    check(n, L, out, lambda k: adf.censusTransform(t[k], 3, adf.SGBM_COST_CENSUS_DENSE), lambda k: census_transform(src[k], 3, False))


@pytest.mark.parametrize("workspace", ["library_scratch", "caller_workspace"])
def test_filter_speckles(adf, workspace):
    import torch
    n = L + 2
    # four levels 16 apart and the fill: with maxDiff 16 and maxSpeckleSize 2 some maps keep a component, some lose all
    src = (images(n, (2, 2), 0, 5, np.int16) * 16 - 16).astype(np.int16)
    buf = lambda m: torch.zeros(adf.speckleWorkspaceBytes(m, 2, 2), dtype=torch.uint8, device="cuda:0") if workspace == "caller_workspace" else None
    run = lambda a, m: adf.filterSpeckles(_dev(a), -16, 2, 16, buf=buf(m))[0]
    out = run(src, n).cpu().numpy()
    assert (out != src).any() and (out != -16).any()
    check(n, L, out, lambda k: run(src[k], 1), lambda k: speckle_ref(src[k], -16, 2, 16))


def _maps(n):
    return images(n, (1, 4), 16, 24, np.int16)                       # 4 x 1, few levels: the minimum differs from map to map


def test_reproject_image_to_3d(adf):
    n = L + 2
    src = _maps(n)
    t = _dev(src)
    run = lambda d: adf.reprojectImageTo3D(d, Q, handleMissingValues=True, dispScale=1.0 / 16)
    out = run(t)
    assert tuple(out.shape) == (n, 1, 4, 3)
    check(n, L, out, lambda k: run(t[k]), lambda k: reproject_ref.reproject(src[k], Q, 1.0 / 16, reproject_ref.MISSING_MIN))


def test_point_cloud(adf):
    n = L + 2
    src = _maps(n)
    t = _dev(src)
    run = lambda d: adf.pointCloud(d, Q, handleMissingValues=True, dispScale=1.0 / 16, withIndex=True)
    P, Cl, I, counts = run(t)
    assert Cl[0] is None and len(counts) == n
    pack = lambda p, i, c: np.concatenate([bits(p).ravel(), bits(i).ravel(), np.array([c], np.int64).view(np.uint8)])

    def single(k):
        p, _, i, c = run(t[k])
        return pack(p, i, c)

    def reference(k):
        p, _, i = reproject_ref.point_cloud(src[k], Q, disp_scale=1.0 / 16, mode=reproject_ref.MISSING_MIN)
        return pack(p, i, len(p))

    check(n, L, {k: pack(P[k], I[k], counts[k]) for k in (0, L - 1, L, n - 1)}, single, reference)
    assert min(counts) < max(counts) == 3                            # every map has missing pixels, most have valid ones


@pytest.mark.parametrize("call", ["remap", "rectifyViews"])
def test_sampling(adf, call):
    per_launch = L * 4
    n = per_launch + 1
    src = images(n, (2, 2), 0, 256, np.uint8)
    t = _dev(src)
    ex, ey = rectify_ref.init_map(rectify_ref.params(*MODEL), 2, 2)
    if call == "remap":
        mx, my = adf.initUndistortRectifyMap(*MODEL, (2, 2), device=t.device)
        assert rectify_ref.same_bits(mx.cpu().numpy(), ex) and rectify_ref.same_bits(my.cpu().numpy(), ey)
        run = lambda v: adf.remap(v, mx, my, borderValue=BORDER)
    else:
        run = lambda v: adf.rectifyViews(v, *MODEL, size=(2, 2), borderValue=BORDER)
    out = run(t)
    assert tuple(out.shape) == (n, 2, 2)
    check(n, per_launch, out, lambda k: run(t[k]), lambda k: rectify_ref.remap(src[k], ex, ey, BORDER))
