"""The yardstick of the overlap kernel (tests/rect_exact.py) against closed forms and exact rational arithmetic."""
import math
import time
from fractions import Fraction

import numpy as np

import rect_exact as rx


def test_corners_follow_the_kernel_convention():
    # ry = pi/2 turns +x (the length axis) to -y: x' = sin * py, y' = -sin * px
    c = rx.corners(np.array([[1.0, 2.0, 4.0, 2.0, np.pi / 2]]))[0]
    want = np.array([[1 - 1, 2 + 2], [1 + 1, 2 + 2], [1 + 1, 2 - 2], [1 - 1, 2 - 2]])
    assert np.allclose(c, want, atol=1e-6)
    # the float32 rounding of the parameters is the kernel's input
    b = np.array([[0.1, 0.0, 1.0, 1.0, 0.0]])
    assert rx.corners(b)[0, 2, 0] == float(np.float32(0.1)) + 0.5


def test_axis_aligned_closed_forms():
    # [0, 4] x [0, 2] against [1, 5] x [-1, 1]: 3 x 1
    a = np.array([[2.0, 1.0, 4.0, 2.0, 0.0]])
    b = np.array([[3.0, 0.0, 4.0, 2.0, 0.0]])
    assert rx.inter_area(a, b)[0] == 3.0
    assert rx.bev_value(b, a, -1)[0] == 3.0 / (8 + 8 - 3)
    assert rx.bev_value(b, a, 0)[0] == 3.0 / 8
    assert rx.bev_value(b, a, 2)[0] == 3.0
    # a 90-degree turn is the same rectangle as (w, l)
    c = np.array([[3.0, 0.0, 2.0, 4.0, np.pi / 2]])
    assert abs(rx.inter_area(a, c)[0] - 3.0) < 1e-6              # cos(float32(pi/2)) = -4.4e-8


def test_nested_and_disjoint():
    big = np.array([[0.0, 0.0, 20.0, 20.0, 0.3]])
    small = np.array([[0.5, -0.5, 0.25, 0.125, 1.1]])
    assert abs(rx.inter_area(big, small)[0] - 0.25 * 0.125) < 1e-15
    assert abs(rx.bev_value(small, big, 0)[0] - 0.25 * 0.125 / 400) < 1e-12 * 0.25 * 0.125 / 400
    assert abs(rx.bev_value(small, big, 1)[0] - 1.0) < 1e-12
    far = np.array([[30.0, 0.0, 20.0, 20.0, 0.0]])
    assert rx.inter_area(big, far)[0] == 0.0
    touching = np.array([[20.0, 0.0, 20.0, 20.0, 0.0]])            # shares the edge x = 10
    assert rx.inter_area(np.array([[0.0, 0.0, 20.0, 20.0, 0.0]]), touching)[0] == 0.0


def test_octagon():
    s = 2.0
    a = np.array([[0.0, 0.0, s, s, 0.0]])
    b = np.array([[0.0, 0.0, s, s, np.pi / 4]])
    want = 2 * (math.sqrt(2) - 1) * s * s
    assert abs(rx.inter_area(a, b)[0] - want) < 1e-6              # float32 pi/4
    # exactly turned corners: the rational clip gives the closed form up to the corners' own rounding
    h = s / 2
    sq = [(-h, -h), (-h, h), (h, h), (h, -h)]
    r = h * math.sqrt(2)
    dia = [(0.0, -r), (-r, 0.0), (0.0, r), (r, 0.0)]
    assert abs(float(rx.clip_area_exact(sq, dia)) - want) < 1e-14
    assert abs(rx.clip_area(np.array([sq]), np.array([dia]))[0] - want) < 1e-14


def test_three_four_five_rotation_equals_the_rational_clip():
    cos, sin = Fraction(4, 5), Fraction(3, 5)
    rng = np.random.default_rng(0)
    for _ in range(40):
        cx, cy = (Fraction(int(v), 8) for v in rng.integers(-16, 17, 2))
        l, w = (Fraction(int(v), 4) for v in rng.integers(1, 24, 2))
        px, py = [-l / 2, -l / 2, l / 2, l / 2], [-w / 2, w / 2, w / 2, -w / 2]
        q = [(cos * x + sin * y + cx, -sin * x + cos * y + cy) for x, y in zip(px, py)]
        L, W = (Fraction(int(v), 4) for v in rng.integers(1, 24, 2))
        X, Y = (Fraction(int(v), 8) for v in rng.integers(-16, 17, 2))
        r = [(X - L / 2, Y - W / 2), (X - L / 2, Y + W / 2), (X + L / 2, Y + W / 2), (X + L / 2, Y - W / 2)]
        exact = rx.clip_area_exact(q, r)
        assert exact == rx.clip_area_exact(r, q)
        qf = np.array([[[float(x), float(y)] for x, y in q]])
        rf = np.array([[[float(x), float(y)] for x, y in r]])
        assert abs(rx.clip_area(qf, rf)[0] - float(exact)) <= 1e-14 * max(1.0, float(exact))
        assert abs(rx.clip_area(rf, qf)[0] - float(exact)) <= 1e-14 * max(1.0, float(exact))
        # the same box through corners(): cos 0.8 and sin 0.6 up to float64 rounding
        ry = math.atan2(0.6, 0.8)                                # float32-rounded by corners(): 3e-8
        b = np.array([[float(cx), float(cy), float(l), float(w), ry]])
        assert abs(rx.corners(b)[0] - qf[0]).max() < 1e-6


def test_swapping_the_boxes_is_symmetric_and_fast():
    rng = np.random.default_rng(1)
    n = 4000
    a = np.concatenate([rng.uniform(-5, 5, (n, 2)), rng.uniform(0.2, 20, (n, 2)), rng.uniform(-8 * np.pi, 8 * np.pi, (n, 1))], 1)
    b = np.concatenate([rng.uniform(-5, 5, (n, 2)), rng.uniform(0.2, 20, (n, 2)), rng.uniform(-8 * np.pi, 8 * np.pi, (n, 1))], 1)
    t0 = time.perf_counter()
    ab = rx.inter_area(a, b)
    dt = time.perf_counter() - t0
    ba = rx.inter_area(b, a)
    assert dt < 1.0, dt
    scale = np.maximum(rx.box_area(a), rx.box_area(b))
    assert np.all(np.abs(ab - ba) <= 1e-12 * scale)
    assert np.all(ab <= np.minimum(rx.box_area(a), rx.box_area(b)) * (1 + 1e-12))
    assert (ab > 0).mean() > 0.5
    # -1 is symmetric, 0 and 1 exchange
    assert np.allclose(rx.bev_value(a, b, -1), rx.bev_value(b, a, -1), rtol=0, atol=1e-12)
    assert np.allclose(rx.bev_value(a, b, 0), rx.bev_value(b, a, 1), rtol=0, atol=1e-12)
    # a few against the rational clip of the same float64 corners
    ca, cb = rx.corners(a[:30]), rx.corners(b[:30])
    for k in range(30):
        ex = rx.clip_area_exact([tuple(map(Fraction, p)) for p in ca[k]], [tuple(map(Fraction, p)) for p in cb[k]])
        assert abs(ab[k] - float(ex)) <= 1e-12 * scale[k]


def test_height_overlap_and_3d_criteria():
    # camera y points down: a box spans [y - h, y]
    dt = np.array([[0.0, 2.0, 0.0, 4.0, 2.0, 2.0, 0.0],       # [0, 2]
                   [0.0, 2.0, 0.0, 4.0, 2.0, 2.0, 0.0],
                   [0.0, -1.0, 0.0, 4.0, 3.0, 2.0, 0.0],      # [-4, -1]
                   [0.0, 2.0, 0.0, 4.0, 2.0, 2.0, 0.0]])
    gt = np.array([[0.0, 4.0, 0.0, 4.0, 2.0, 2.0, 0.0],       # [2, 4]: stacked, iw == 0
                   [0.0, 1.5, 1.0, 4.0, 1.0, 2.0, 0.0],       # [0.5, 1.5] inside [0, 2]; BEV half
                   [0.0, -2.0, 0.0, 4.0, 1.0, 2.0, 0.0],      # [-3, -2] inside [-4, -1]
                   [9.0, 2.0, 0.0, 4.0, 2.0, 2.0, 0.0]])      # no BEV overlap
    assert np.array_equal(rx.height_overlap(dt, gt), [0.0, 1.0, 1.0, 2.0])
    v = rx.d3_value(dt, gt, -1)
    assert v[0] == 0 and v[3] == 0
    assert v[1] == 4.0 / (16 + 8 - 4)
    assert v[2] == 8.0 / (24 + 8 - 8)
    assert rx.d3_value(dt, gt, 0)[1] == 4.0 / 16          # over the dt volume
    assert rx.d3_value(dt, gt, 1)[1] == 4.0 / 8           # over the gt volume
    assert np.array_equal(rx.d3_value(dt, gt, 2), [0.0, 1.0, 1.0, 0.0])


def test_well_conditioned():
    a = np.array([[0.0, 0.0, 4.0, 2.0, 0.0]] * 3)
    b = np.array([[1.0, 0.5, 4.0, 2.0, 0.0],                # corners 0.5 from the edges
                  [4.0, 0.0, 4.0, 2.0, 0.0],                # touching edges
                  [0.0, 0.0, 4.0, 2.0, 1e-7]])              # nearly coincident
    assert rx.well_conditioned(a, b, 1e-4).tolist() == [True, False, False]
    assert rx.well_conditioned(a[:1], b[:1], 0.6).tolist() == [False]
