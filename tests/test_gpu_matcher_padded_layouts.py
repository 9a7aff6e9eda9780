"""Every compute entry of the two matchers on padded layouts: a 2-pair batch of 70 x 37 whose views, maps and cost planes
sit in rows 6 elements longer than a row and in pairs 2 rows further apart than an image.  The outputs equal the dense
call's and the padding keeps its sentinel.  (numDisparities 16, blockSize 5; SAD / Birchfield-Tomasi and one census cost.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, H, W = 2, 37, 70
SENTINEL = 12345


def _padded(dense, fill, device):
    """`dense` (N,H,W[,C]) inside a block with 6 more columns and 2 more rows per pair -> (the block, the view of it)."""
    shape = (N, H + 2, W + 6) + dense.shape[3:]
    if fill is None:                                   # a view's padding: bytes that must not be read as image
        block = np.random.default_rng(9).integers(0, 256, shape).astype(dense.dtype)
    else:
        block = np.full(shape, fill, dense.dtype)
    block[:, :H, :W] = dense
    if device:
        import torch
        block = torch.from_numpy(block).cuda()
    return block, block[:, :H, :W]


def _views(channels):
    rng = np.random.default_rng(70 + channels)
    base = rng.integers(0, 256, (N, H, W + 8) + ((3,) if channels == 3 else ()), dtype=np.uint8)
    base = (base // 2 + np.roll(base, 1, 2) // 2).astype(np.uint8)
    return np.ascontiguousarray(base[:, :, 6:6 + W]), np.ascontiguousarray(base[:, :, :W])   # the right view: shifted by 6


def _check(method, channels, n_out, device):
    """method(left, right, *outputs) on padded planes against the same call on dense arrays with new outputs."""
    left, right = _views(channels)
    if device:
        import torch
        dense = method(torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda(), *[None] * n_out)
        torch.cuda.synchronize()
    else:
        dense = method(left, right, *[None] * n_out)
    dense = [dense] if n_out == 1 else list(dense)
    dense = [d.cpu().numpy() if device else d for d in dense]
    assert any((d != dense[0][0, 0, 0]).any() for d in dense)                   # something was matched
    (_, pl), (_, pr) = _padded(left, None, device), _padded(right, None, device)
    outs = [_padded(np.zeros((N, H, W), np.int16), SENTINEL, device) for _ in range(n_out)]
    method(pl, pr, *[view for _, view in outs])
    for (block, _), exp in zip(outs, dense):
        if device:
            import torch
            torch.cuda.synchronize()
            block = block.cpu().numpy()
        assert np.array_equal(block[:, :H, :W], exp)
        pad = block.copy()
        pad[:, :H, :W] = SENTINEL
        assert (pad == SENTINEL).all()


@pytest.mark.parametrize("cost", ["sad", "census"])
@pytest.mark.parametrize("entry", ["compute_device", "compute_host", "compute_cost_device", "compute_cost_host",
                                   "compute_both_device", "compute_both_cost_device"])
def test_block_matcher(adf, entry, cost):
    bm = adf.StereoBM.create(16, 5)
    if cost == "census":
        bm.setCostType(adf.BM_COST_CENSUS_SPARSE); bm.setCensusSize(7)
    method, n_out = {"compute": (bm.compute, 1), "compute_cost": (bm.computeWithCost, 2), "compute_both": (bm.computeBoth, 2),
                     "compute_both_cost": (bm.computeBothWithCost, 4)}[entry.rsplit("_", 1)[0]]
    _check(method, 1, n_out, entry.endswith("_device"))


@pytest.mark.parametrize("cost,channels", [("bt", 1), ("bt", 3), ("census", 1)])
@pytest.mark.parametrize("device", [True, False], ids=["compute_device", "compute_host"])
def test_semi_global_matcher(adf, device, cost, channels):
    sg = adf.StereoSGBM.create(0, 16, 5)
    if cost == "census":
        sg.setCostType(adf.SGBM_COST_CENSUS_DENSE); sg.setCensusSize(5)
    _check(sg.compute, channels, 1, device)
