"""Cases shared by tests/test_float_output_abi.py (CPU) and tests/test_gpu_float_output.py (GPU): the synthetic pairs
the float32 filtered map is compared on against a float64 solve, and that reference.

ref64 = fgs_f64(conf * disp) / (fgs_f64(conf) + EPS) on the ROI, both solves on the library's own float32 couplings
(oracle.weights) as tests/wave_f64_cases.py does; the comparison runs on the ROI pixels whose float64 filtered
confidence is >= 1.0 (of 255) -- below that the ratio is ill-conditioned by construction.  The mask is a condition, not
a measurement: the seeds below keep at least half of the ROI with the oracle's confidence map alone (checked on the
CPU by test_float_output_abi.py)."""
import numpy as np

import wave_f64_cases as wc

EPS = np.float32(1e-43)          # DF.cpp:47
F64_CASES = [(96, 64, 3, 21), (75, 130, 1, 5), (160, 45, 3, 8)]      # (W, H, view channels, seed of make_artificial_example)


def f64_reference(oracle, view, dl, roi, conf):
    """(ref64 on the ROI, mask, the float32 right-hand sides (h, w, 2)) for the ROI crop `conf` of a confidence map."""
    from oracle.banded_f64 import fgs_f64_coeffs

    x, y, w, h = roi
    disp = dl[y:y + h, x:x + w].astype(np.float32)
    rhs = np.stack([conf * disp, conf], axis=2).astype(np.float32)                   # DF.cpp:288-290
    chor, cvert = oracle.weights(np.ascontiguousarray(view[y:y + h, x:x + w]), wc.SIGMA)
    u = fgs_f64_coeffs(chor, cvert, rhs, wc.LAM, wc.ATTEN, wc.NUM_ITER)
    return u[:, :, 0] / (u[:, :, 1] + float(EPS)), u[:, :, 1] >= 1.0, rhs
