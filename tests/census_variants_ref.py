"""Direct statements (plain numpy, independent of the product code) of the modified census transform and of the
centre-symmetric census -- the definitions in include/adf_wls.h (adf_census_transform_*: ADF_SGBM_COST_MCT_DENSE,
_MCT_SPARSE, _CENSUS_CS) -- and the two matchers' statements with one of them as the descriptor.

Common to both, as for census_ref.census_transform: CV_8UC1 input, neighbour coordinates clamped to the image
(replicated edge), comparisons in raster order, the first comparison the most significant of the bits used, a bit is 1
on strict `>`.

    mct_transform   Froeba & Ernst 2004: the offsets of the dense / sparse census at k, (0, 0) skipped; S is the sum of all
                    k * k pixels of the clamped window, centre included; a bit is k * k * neighbour > S.
    cs_transform    Spangenberg et al. 2013: the offsets before (0, 0) in raster order; a bit is
                    p(y + dy, x + dx) > p(y - dy, x - dx).

The matchers are tests/bm_census_ref.bm_census and tests/census_ref.naive_census_sgbm, unchanged: `transform_swapped`
puts another descriptor in the place of their census_transform for the length of one call."""
import contextlib

import numpy as np

import bm_census_ref
import census_ref
from census_ref import DENSE_BITS, SPARSE_BITS, census_offsets

DENSE, SPARSE, MCT_DENSE, MCT_SPARSE, CS = 1, 2, 4, 5, 6      # ADF_SGBM_COST_* (= ADF_BM_COST_*) of include/adf_wls.h
CS_BITS = {3: 4, 5: 12, 7: 24, 9: 40}
# the eleven new (type, size) pairs, and the bits of each
VARIANTS = ([(MCT_DENSE, k) for k in DENSE_BITS] + [(MCT_SPARSE, k) for k in SPARSE_BITS] + [(CS, k) for k in CS_BITS])
VARIANT_BITS = {**{(MCT_DENSE, k): b for k, b in DENSE_BITS.items()}, **{(MCT_SPARSE, k): b for k, b in SPARSE_BITS.items()},
                **{(CS, k): b for k, b in CS_BITS.items()}}


_census_transform = census_ref.census_transform                # the statement itself, whatever transform_swapped has put in its place


def _shifted(a, dy, dx):
    """a(y + dy, x + dx) with both coordinates clamped to the image."""
    H, W = a.shape
    return a[np.clip(np.arange(H) + dy, 0, H - 1)][:, np.clip(np.arange(W) + dx, 0, W - 1)]


def mct_transform(img, k, sparse):
    assert k in (SPARSE_BITS if sparse else DENSE_BITS), (k, sparse)
    a = np.asarray(img).astype(np.int64)
    n2 = k // 2
    total = np.zeros(a.shape, np.int64)
    for dy in range(-n2, n2 + 1):                              # the whole window, on the sparse grids too
        for dx in range(-n2, n2 + 1):
            total += _shifted(a, dy, dx)
    out = np.zeros(a.shape, np.uint64)
    for dy in census_offsets(k, sparse):
        for dx in census_offsets(k, sparse):
            if dy == 0 and dx == 0:
                continue
            out = (out << np.uint64(1)) | (k * k * _shifted(a, dy, dx) > total).astype(np.uint64)
    return out


def cs_transform(img, k):
    assert k in CS_BITS, k
    a = np.asarray(img).astype(np.int64)
    n2 = k // 2
    out = np.zeros(a.shape, np.uint64)
    for dy in range(-n2, 1):
        for dx in range(-n2, n2 + 1):
            if dy == 0 and dx >= 0:
                break
            out = (out << np.uint64(1)) | (_shifted(a, dy, dx) > _shifted(a, -dy, -dx)).astype(np.uint64)
    return out


def transform(img, ctype, k):
    """The descriptor of any of the five types."""
    if ctype in (DENSE, SPARSE):
        return _census_transform(img, k, ctype == SPARSE)
    if ctype in (MCT_DENSE, MCT_SPARSE):
        return mct_transform(img, k, ctype == MCT_SPARSE)
    assert ctype == CS, ctype
    return cs_transform(img, k)


@contextlib.contextmanager
def transform_swapped(ctype):
    """Inside: the matcher statements form their descriptors with transform(img, ctype, k) (what monkeypatch.setattr does,
    for helpers that are called outside a test function too); their `sparse` argument is not looked at."""
    saved = census_ref.census_transform, bm_census_ref.census_transform

    def swapped(img, k, sparse):
        return transform(img, ctype, k)

    census_ref.census_transform = bm_census_ref.census_transform = swapped
    try:
        yield
    finally:
        census_ref.census_transform, bm_census_ref.census_transform = saved


def bm_variant(left, right, nd, bs, md=0, uniq=0, ctype=CS, k=7):
    """bm_census_ref.bm_census with the descriptor (ctype, k)."""
    with transform_swapped(ctype):
        return bm_census_ref.bm_census(left, right, nd, bs, md, uniq, k, False)


def sgbm_variant(img1, img2, nd, bs, md=0, P1=0, P2=0, ur=0, mode=2, disp12=1000000, ctype=CS, k=7):
    """census_ref.naive_census_sgbm (the raw map, before the 3 x 3 median) with the descriptor (ctype, k)."""
    with transform_swapped(ctype):
        return census_ref.naive_census_sgbm(img1, img2, nd, bs, md, P1, P2, ur, mode, disp12, k, False)
