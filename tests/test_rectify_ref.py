"""tests/rectify_ref.py, the NumPy statement the device rectification is compared with, against facts that do not depend
on it: the identity model, a pure translation, one hand-computed sample and the inverse times its matrix."""
import numpy as np

import rectify_ref as ref


def _image(h, w, ch, seed=3):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w, ch) if ch == 3 else (h, w), dtype=np.uint8)


def _K(w, h):
    return np.array([[533.25, 0.0, float(w // 2)], [0.0, 529.5, float(h // 2)], [0.0, 0.0, 1.0]])


def test_identity_model_gives_the_pixel_grid_and_the_source():
    w, h = 37, 23
    K = _K(w, h)
    mx, my = ref.init_map(ref.params(K, None, None, K), w, h)
    assert mx.dtype == np.float32 and my.dtype == np.float32
    u, v = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    assert np.array_equal(mx, u) and np.array_equal(my, v)
    for ch in (1, 3):
        src = _image(h, w, ch)
        assert np.array_equal(ref.remap(src, mx, my, 0), src)
    assert np.array_equal(ref.rectify(_image(h, w, 3), K, [0.0] * 5, np.eye(3), K), _image(h, w, 3))


def test_shifted_principal_point_is_a_translation_with_border_fill():
    w, h, n = 41, 17, 5
    K = _K(w, h)
    P = K.copy()
    P[0, 2] += n                                             # destination column u shows source column u - n
    for ch, border in ((1, 9), (3, (7, 200, 99))):
        src = _image(h, w, ch)
        out = ref.rectify(src, K, None, None, P, border_value=border)
        assert np.array_equal(out[:, n:], src[:, :w - n])
        fill = np.broadcast_to(np.asarray(border, np.uint8), out[:, :n].shape)
        assert np.array_equal(out[:, :n], fill)


def test_hand_computed_half_pixel_sample():
    src = np.array([[10, 20], [30, 41]], np.uint8)
    half = np.full((1, 1), 0.5, np.float32)                  # ax = ay = 16: every weight 256
    assert (101 * 256 + 512) >> 10 == 25
    assert ref.remap(src, half, half, 0)[0, 0] == 25
    # a tap outside the source is the border value: at (1.5, 0.5) the right column is 200
    out = ref.remap(src, np.full((1, 1), 1.5, np.float32), half, 200)
    assert out[0, 0] == ((20 + 41 + 200 + 200) * 256 + 512) >> 10


def test_rounding_ties_and_the_ok_range():
    src = np.arange(64, dtype=np.uint8).reshape(1, 64) * 4
    zero = np.zeros((1, 1), np.float32)
    # 3.015625 * 32 = 96.5 -> 96 (even), 3.046875 * 32 = 97.5 -> 98
    assert ref.remap(src, np.full((1, 1), 3.015625, np.float32), zero, 0)[0, 0] == 12
    assert ref.remap(src, np.full((1, 1), 3.046875, np.float32), zero, 0)[0, 0] == (12 * 30 + 16 * 2 + 16) >> 5
    for bad in (np.nan, np.inf, -np.inf, 1e30, -1e30, 32768.0, -32768.03125):
        assert ref.remap(src, np.full((1, 1), bad, np.float32), zero, 77)[0, 0] == 77
    # exactly -1.0: only the right tap column exists, with weight 0
    assert ref.remap(src, np.full((1, 1), -1.0, np.float32), zero, 77)[0, 0] == 77
    assert ref.remap(src, np.full((1, 1), -0.5, np.float32), zero, 100)[0, 0] == (100 * 16 * 32 + 0 * 16 * 32 + 512) >> 10


def test_adjugate_inverse_of_a_kitti_like_matrix():
    P = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]])
    a = np.deg2rad(2.0)
    A = ref.product3(P, ref.rot(a, -a, a))
    assert np.allclose(A, P[:, :3] @ ref.rot(a, -a, a), rtol=1e-14, atol=0)
    inv = ref.inverse3(A)
    # entries <= ~1e3, eps 1.1e-16: the error is ~1e-12; 1e-9 is a sanity cap, not a measurement
    assert np.max(np.abs(inv @ A - np.eye(3))) < 1e-9
    assert np.array_equal(ref.product3(P, None), P[:, :3])


def test_params_layout_and_refusals():
    K = _K(64, 48)
    (fx, fy, cx, cy), d, ir = ref.params(K, [0.1, 0.2, 0.3, 0.4], None, None)
    assert (fx, fy, cx, cy) == (533.25, 529.5, 32.0, 24.0)
    assert d.tolist() == [0.1, 0.2, 0.3, 0.4, 0.0, 0.0, 0.0, 0.0] and ir.shape == (9,)
    for bad in (lambda: ref.params(K, [0.0] * 12, None, None), lambda: ref.inverse3(np.ones((3, 3)))):
        try:
            bad()
        except ValueError:
            continue
        raise AssertionError("not refused")
