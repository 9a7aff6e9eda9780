"""Cases shared by tests/test_banded_f64.py (CPU) and tests/test_gpu_wave_f64.py (GPU): every chunk-length bucket of
the wave solver, the guides and sources that stress its seams, the float64 reference on the library's own
coefficients, and the acceptance criterion.

The criterion: e(x) = max|x - ref64| / max|src| per channel, and a float32 solver passes when
e(x) <= factor * e_scalar + 1e-6, e_scalar being the scalar-order oracle's error on the same input.  Normalised by
the source, not the solution: on a flat guide the solution of a noise source is tiny, and a bound relative to it
would measure the rounding of the source's own scale.  The factor depends on the coefficient pattern (factor())."""
import numpy as np

LAM, SIGMA, ATTEN, NUM_ITER = 8000.0, 1.5, 0.25, 3
FLOOR = 1e-6
# Factors measured on the MI355X over every bucket, guide and channel layout of tests/test_gpu_wave_f64.py (ratio
# e_wave / e_scalar):
#  - couplings that vary along the line (ramp, noisy and the ramp-based cut / seam guides): at most 6.6 (noisy guide,
#    lambda 1e5, 4352-row half strips); most cases 0.2..2.  The wave solver re-associates the elimination (v_rcp plus
#    one Newton step, FMAs, cyclic reduction of the 64 / 128 separator rows), and e_scalar is itself a noisy yardstick:
#    on the same systems it scatters up to 7x between the channels of one source while e_wave stays put.
#  - couplings exactly -lambda inside the chunks (flat and the flat-based cut / seam guides): up to 63.  There the
#    scalar order is unusually exact -- with C = -1, every coefficient it forms (lambda*C, 1 - a - c = 1 + 2 lambda) is
#    an exact float32 integer -- while the wave solver's separator rows (separator_row, pcr64 in
#    csrc/fgs_wave_common.h) form be = (1 - a - c) - c*P - a*Q, with P + Q within ~M/lambda of 1: the "1" of the
#    identity is recovered by cancellation against terms of size lambda and keeps only ~log2(M/lambda) + 24 bits,
#    which shows in the mean of each line.  In absolute terms these errors stay within what the scalar order itself
#    reaches in these tests (largest flat-pattern e_wave 2.0e-4 of max|src|; largest e_scalar 4.6e-4, flat guide at
#    lambda 1e5).
VARIED_FACTOR = 8.0
FLAT_FACTOR = 96.0

# Mirrors ROW_BUCKETS (csrc/fgs_wave_h.hip): one wavefront per row of 64 chunks of M elements up to 4096 columns,
# two wavefronts (128 chunks) above.  (M, chunks); a bucket takes the lengths (previous bucket's chunks*M, chunks*M].
ROW_BUCKETS = [(4, 64), (8, 64), (16, 64), (20, 64), (28, 64), (40, 64), (56, 64), (60, 64), (64, 64),
               (40, 128), (48, 128), (56, 128), (60, 128), (64, 128)]
# Mirrors COL_BUCKETS (csrc/fgs_wave_v.hip): full strips of 64 chunks up to 2176 rows, half strips of 128 chunks
# above.  (M, chunks per column).
COL_BUCKETS = [(2, 64), (4, 64), (8, 64), (12, 64), (18, 64), (26, 64), (34, 64), (20, 128), (26, 128), (34, 128)]
COL_WIDTHS = (40, 50)      # partial 16-column strips, and a pitch padded to 64


def _lengths(buckets):
    """(M, chunks, shortest, longest) per bucket: the shortest is the previous bucket's longest + 1 (2 for the first),
    which leaves the upper chunks of the bucket empty (257 in the row M=8 bucket: 33 of 64 chunks hold data)."""
    out, prev = [], 1
    for m, chunks in buckets:
        hi = chunks * m
        out.append((m, chunks, prev + 1, hi))
        prev = hi
    return out


ROW_LENGTHS = _lengths(ROW_BUCKETS)
COL_LENGTHS = _lengths(COL_BUCKETS)


class Geom:
    """One bucket at one length: the row pass (axis 'row') or the column pass (axis 'col') runs the bucket of
    `chunks` chunks of m elements on lines of `n` elements; `other` is the image's extent along the other axis."""

    def __init__(self, axis, m, chunks, n, other):
        self.axis, self.m, self.chunks, self.n, self.other = axis, m, chunks, n, other

    @property
    def shape(self):
        return (self.other, self.n) if self.axis == "row" else (self.n, self.other)

    @property
    def id(self):
        if self.axis == "row":
            return "row-M%d-%dwave-n%d" % (self.m, self.chunks // 64, self.n)
        return "col-M%d-%s-n%d" % (self.m, "half" if self.chunks == 128 else "full", self.n)

    def separators(self):
        """Elements l*M + M - 1 that end a chunk and have a neighbour: the couplings that cross chunks."""
        return np.arange(self.m - 1, self.n - 1, self.m)


def geometries():
    out = []
    for k, (m, ch, lo, hi) in enumerate(ROW_LENGTHS):
        for j, n in enumerate((lo, hi)):
            out.append(Geom("row", m, ch, n, 2 + (2 * k + j) % 3))        # 2..4 rows
    for k, (m, ch, lo, hi) in enumerate(COL_LENGTHS):
        for j, n in enumerate((lo, hi)):
            out.append(Geom("col", m, ch, n, COL_WIDTHS[(k + j) % 2]))
    return out


GEOMS = geometries()
GUIDES = ("flat", "ramp", "noisy", "cut-flat", "cut-ramp", "cutm1-flat", "cutm1-ramp", "seam-flat", "seam-ramp")
SEAM_LEVELS = 8


def _tri(t):
    t = np.mod(t, 510)
    return np.where(t <= 255, t, 510 - t)


def make_guide(g, kind, seed=0):
    """3-channel uint8 guide of geometry `g`.
    flat: constant, every coupling -lambda (the strongest coupling, the worst conditioning).
    ramp: neighbours differ by 1..3 levels per channel along both axes: strong, varied couplings.
    noisy: uniform random.
    cut-*: channel 0 steps by 255 levels across every separator of the bucket (the table entry is -0.0 there: the chunks
    decouple exactly); cutm1-* puts the step one element earlier, between l*M + M - 2 and l*M + M - 1.
    seam-*: channel 0 steps by SEAM_LEVELS across every separator: a moderate coupling (lambda * w ~ 20..40 at
    lambda 8000, sigma 1.5) inside strong ones, so the solution keeps a visible jump at every seam and an error in how a
    solver couples its chunks shows (flat and ramp smooth the jumps away: a 1 % seam error stays within 4 x the scalar
    order's rounding there)."""
    h, w = g.shape
    rng = np.random.default_rng(seed + 7 * h + w)
    if kind == "noisy":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    base = kind.split("-")[-1]
    if base == "flat":
        out = np.full((h, w, 3), 128, np.int64)
    else:
        cx = np.cumsum(rng.integers(1, 4, w))
        cy = np.cumsum(rng.integers(1, 4, h))
        t = cx[None, :] + cy[:, None]
        out = np.stack([_tri(t), _tri(t + 85), _tri(t + 170)], axis=2)
    if kind.startswith(("cut", "seam")):
        shift = 1 if kind.startswith("cutm1") else 0
        lo, hi = (0, 255) if kind.startswith("cut") else (128 - SEAM_LEVELS // 2, 128 + SEAM_LEVELS // 2)
        step = np.where((((np.arange(g.n) + shift) // g.m) % 2) == 1, hi, lo)
        if g.axis == "row":
            out[:, :, 0] = step[None, :]
        else:
            out[:, :, 0] = step[:, None]
    return out.astype(np.uint8)


def make_source(g, cn, seed=0):
    """float32 (h, w, cn): N(0, 1000) noise, +-1e4 impulses on every separator element of the bucket's axis and on the
    first and last element of every row and column."""
    h, w = g.shape
    rng = np.random.default_rng(seed + 13 * h + w + 1000 * cn)
    src = rng.normal(0, 1000, (h, w, cn))
    imp = lambda shape: 1e4 * rng.choice([-1.0, 1.0], shape)     # noqa: E731
    sep = g.separators()
    if g.axis == "row":
        src[:, sep] = imp((h, len(sep), cn))
    else:
        src[sep, :] = imp((len(sep), w, cn))
    src[:, 0] = imp((h, cn)); src[:, -1] = imp((h, cn))
    src[0, :] = imp((w, cn)); src[-1, :] = imp((w, cn))
    return src.astype(np.float32)


def err(x, ref, src):
    """Per-channel max|x - ref| / max|src| of (h, w, cn) arrays."""
    x, ref, src = (np.asarray(a, np.float64) for a in (x, ref, src))
    return np.abs(x - ref).max(axis=(0, 1)) / np.abs(src).max(axis=(0, 1))


def factor(kind):
    return FLAT_FACTOR if kind.split("-")[-1] == "flat" else VARIED_FACTOR


def accepts(e_x, e_scalar, factor):
    return np.all(np.asarray(e_x) <= factor * np.asarray(e_scalar) + FLOOR)


def scalar_fgs(oracle, guide, src, lam=LAM, sigma=SIGMA, atten=ATTEN, num_iter=NUM_ITER):
    """The scalar-order float32 oracle (FGS.cpp's own order) on every channel of `src` (h, w, cn)."""
    planes = oracle.fgs_planes(guide, np.moveaxis(src, 2, 0), lam, sigma, atten, num_iter, threads=4)
    return np.moveaxis(planes, 0, 2)


def ref64(oracle, guide, src, lam=LAM, sigma=SIGMA, atten=ATTEN, num_iter=NUM_ITER):
    from oracle.banded_f64 import fgs_f64_coeffs

    chor, cvert = oracle.weights(guide, sigma)
    return fgs_f64_coeffs(chor, cvert, src, lam, atten, num_iter)


def case(oracle, gi, kind, cn):
    """(guide, src, ref64, scalar oracle) of GEOMS[gi] with guide `kind` and a cn-channel source."""
    g = GEOMS[gi]
    guide = make_guide(g, kind)
    src = make_source(g, cn)
    return guide, src, ref64(oracle, guide, src), scalar_fgs(oracle, guide, src)
