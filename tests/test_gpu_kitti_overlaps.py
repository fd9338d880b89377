"""The overlap kernel (csrc/kitti_eval.hip, ke_overlaps) against exact geometry (tests/rect_exact.py), every criterion.

Tolerances.  The kernel mirrors the reference's float32 polygon walk, so it is compared with exact geometry of the
float32-rounded boxes, not bit for bit:
  * near the origin (|corner| < 16 m), on pairs where no corner lies within 1e-4 m of the other box's boundary, 2e-5
    absolute on ratios and 2e-5 of the larger box area on raw areas (TIGHT).  There a float32 corner is off by a few
    roundings of its coordinates (cos * px, sin * py, their sum, + cx, and cosf / sinf themselves: |delta| <= 2 sqrt 2
    eps32 R for corners within R of the origin), so no inside or crossing test can turn; moving every vertex of the
    convex intersection by delta moves its area by at most delta times its perimeter, which is at most the smaller
    box's perimeter P.  Where a small denominator magnifies that (a ratio over a thin box's area), the tolerance is
    4 eps32 R P over the ratio's denominator instead (near_tol);
  * far from the origin (z = 60-80 m, KITTI's last range bucket) the edge crossing is the weak step: ABBA = A0 * B1 -
    B0 * A1 and CDDC cancel, each product of size R^2, so the crossing point is off by about eps32 * R^2 divided by the
    edge length (times 1 / sin of the crossing angle), and the area by about eps32 * R^2 per crossing vertex.  With at
    most 8 such vertices and crossing angles of 30 degrees or more, |error| <= 16 * eps32 * R^2 of area, over the
    ratio's denominator (far_tol).  The reference fixture's measured worst case, 1e-3, is the ceiling.
Near-coincident boxes (a 1-ulp shift) are ill-conditioned for the walk (which corners count as inside is decided by
rounding) and are held only to 0 <= v <= 1 plus the corner rounding's share of the box area (near_tol's bound, at
least 1e-6); exactly coincident boxes give exactly 1.
"""
import numpy as np
import pytest

import rect_exact as rx

pytestmark = pytest.mark.gpu

TIGHT = 2e-5
CEILING = 1e-3
EPS32 = 2.0 ** -23
BEV_CRITS = (-1, 0, 1, 2, 3)
RATIO = (-1, 0, 1)


def _ke():
    from modest_amd import kitti_eval as ke
    return ke


def _gpu_bev(dt, gt, crit):
    """rotate_iou_gpu_eval(dt, gt, crit) for the pairs (dt[k], gt[k]): the diagonals of dense blocks"""
    ke = _ke()
    out = [np.diag(ke.rotate_iou_gpu_eval(dt[s:s + 256], gt[s:s + 256], crit)) for s in range(0, len(dt), 256)]
    return np.concatenate(out).astype(np.float64)


def _gpu_d3(dt7, gt7, crit):
    ke = _ke()
    out = [np.diag(ke.d3_box_overlap(dt7[s:s + 256], gt7[s:s + 256], crit)) for s in range(0, len(dt7), 256)]
    return np.concatenate(out).astype(np.float64)


def _scale(dt, gt, crit):
    """what an error is measured against: 1 for ratios, the larger box area for raw areas"""
    return 1.0 if crit in RATIO else np.maximum(rx.box_area(dt), rx.box_area(gt))


def _dens(dt, gt, crit):
    """the ratio's denominator of each pair (the larger box area for raw areas)"""
    a1, a2 = rx.box_area(gt), rx.box_area(dt)
    return {-1: a1 + a2 - rx.inter_area(gt, dt), 0: a1, 1: a2}.get(crit, np.maximum(a1, a2))


def _reach(dt, gt):
    return np.max(np.abs(np.concatenate([rx.corners(dt), rx.corners(gt)], 1)), axis=(1, 2))


def near_tol(dt, gt, crit):
    """TIGHT, or 4 eps32 R P of area over the ratio's denominator (see the module docstring)"""
    dt, gt = np.asarray(dt, np.float64).reshape(-1, 5), np.asarray(gt, np.float64).reshape(-1, 5)
    p = 2 * np.minimum(rx.f32(dt)[:, 2] + rx.f32(dt)[:, 3], rx.f32(gt)[:, 2] + rx.f32(gt)[:, 3])
    return np.maximum(TIGHT, 4 * EPS32 * _reach(dt, gt) * p / _dens(dt, gt, crit))


def _check_bev(dt, gt, tol, what):
    dt, gt = np.asarray(dt, np.float64).reshape(-1, 5), np.asarray(gt, np.float64).reshape(-1, 5)
    for crit in BEV_CRITS:
        got, want = _gpu_bev(dt, gt, crit), rx.bev_value(dt, gt, crit)
        err = np.abs(got - want) / _scale(dt, gt, crit)
        t = np.broadcast_to(tol(dt, gt, crit), err.shape)
        k = np.argmax(err / t)
        print("%-28s crit %2d: %5d pairs, largest |gpu - exact| %.3g (tolerance %.3g; %.3g of its own tolerance)"
              % (what, crit, len(dt), err.max(), t[np.argmax(err)], err[k] / t[k]))
        bad = np.nonzero(err > t)[0]
        assert len(bad) == 0, (what, crit, dt[bad[:3]], gt[bad[:3]], got[bad[:3]], want[bad[:3]])
    return got


def _random_pairs(seed, n, centre=(0.0, 0.0), spread=5.0, smallest=0.2, thin=0.15):
    """n pairs: centres within spread of centre, l and w log-uniform in [smallest, 20] m (w = 0.05 for a share thin),
    ry in [-8 pi, 8 pi]; the second centre is drawn near the first, so that most pairs overlap"""
    rng = np.random.default_rng(seed)

    def sizes():
        lw = np.exp(rng.uniform(np.log(smallest), np.log(20.0), (n, 2)))
        lw[rng.random(n) < thin, 1] = 0.05
        return lw

    lw1, lw2 = sizes(), sizes()
    c1 = rng.uniform(-spread, spread, (n, 2))
    reach = 0.5 * np.maximum(lw1.max(1), lw2.max(1))[:, None]
    c2 = np.clip(c1 + rng.uniform(-1, 1, (n, 2)) * reach, -spread, spread)
    ry1, ry2 = rng.uniform(-8 * np.pi, 8 * np.pi, (2, n, 1))
    o = np.asarray(centre)
    return np.concatenate([o + c1, lw1, ry1], 1), np.concatenate([o + c2, lw2, ry2], 1)


def test_random_pairs_near_the_origin_every_criterion():
    dt, gt = _random_pairs(0, 6000)
    keep = rx.well_conditioned(dt, gt, 1e-4)
    dt, gt = dt[keep], gt[keep]
    assert len(dt) >= 4000
    assert (rx.inter_area(dt, gt) > 0).sum() >= 3000
    assert ((dt[:, 3] == 0.05) | (gt[:, 3] == 0.05)).sum() >= 500
    _check_bev(dt, gt, near_tol, "random, near the origin")
    assert (near_tol(dt, gt, -1) == TIGHT).mean() > 0.95


def _families(o=(0.0, 0.0)):
    """(name, dt (N, 5), gt (N, 5)) of constructed shapes around the point o"""
    ox, oy = o
    out = []
    # octagon: equal squares, one turned 45 degrees (2 (sqrt 2 - 1) s^2)
    s = np.array([1.0, 2.5, 4.0])
    for tilt in (0.0, 0.3):
        a = np.stack([ox + 0 * s, oy + 0 * s, s, s, tilt + 0 * s], 1)
        b = a.copy()
        b[:, 4] += np.pi / 4
        out.append(("octagon", b, a))
    # crosses of thin boxes, at 90 and 60 degrees
    for ang in (np.pi / 2, np.pi / 3):
        a = np.array([[ox, oy, 4.0, 0.5, 0.2], [ox + 0.3, oy - 0.2, 6.0, 0.25, -1.0], [ox, oy, 3.0, 0.05, 2.0]])
        b = a.copy()
        b[:, 4] += ang
        b[:, :2] += [0.1, -0.05]
        out.append(("cross", b, a))
    # hexagon: a strip across a square's diagonal keeps two of its corners
    a = np.array([[ox, oy, 2.0, 2.0, 0.0], [ox, oy, 3.0, 3.0, 0.7]])
    b = np.array([[ox, oy, 10.0, 1.0, np.pi / 4], [ox + 0.1, oy, 10.0, 1.5, 0.7 + np.pi / 4]])
    out.append(("hexagon", b, a))
    # a single corner poking in: a 45-degree square whose corner enters an edge by d (a triangle of area d^2)
    d = np.array([0.1, 0.3, 0.05])
    r = np.sqrt(2) / 2
    a = np.stack([ox + 0 * d, oy + 0 * d, 2 + 0 * d, 2 + 0 * d, 0 * d], 1)
    b = np.stack([ox + 1 + r - d, oy + 0 * d, 1 + 0 * d, 1 + 0 * d, np.pi / 4 + 0 * d], 1)
    out.append(("corner poke", b, a))
    # a 0.2 m box inside a 20 m box
    a = np.array([[ox, oy, 20.0, 20.0, 0.1], [ox, oy, 20.0, 20.0, 1.3]])
    b = np.array([[ox + 3.0, oy - 2.0, 0.2, 0.2, 0.7], [ox - 1.0, oy + 4.0, 0.2, 0.05, -2.2]])
    out.append(("tiny in huge", b, a))
    # nested with a 1 cm gap on every side
    a = np.array([[ox, oy, 4.0, 1.6, 0.4], [ox, oy, 2.0, 0.8, -2.9]])
    b = a.copy()
    b[:, 2:4] -= 0.02
    out.append(("nested, 1 cm gap", b, a))
    # ry at 0, +-pi/2, pi and 7 pi + x: a 4 x 1.6 box against a shifted, turned one
    for ry in (0.0, np.pi / 2, -np.pi / 2, np.pi, 7 * np.pi + 0.3):
        a = np.array([[ox, oy, 4.0, 1.6, ry], [ox, oy, 3.6, 1.5, ry]])
        b = np.array([[ox + 0.7, oy + 0.3, 3.8, 1.7, ry + 0.25], [ox - 0.4, oy, 1.6, 3.6, ry + np.pi / 2 + 0.1]])
        out.append(("ry %.3g" % ry, b, a))
    return out


def test_constructed_families_near_the_origin():
    for name, dt, gt in _families():
        assert rx.well_conditioned(dt, gt, 1e-3).all(), name
        _check_bev(dt, gt, near_tol, name)
    # the yardstick's closed forms
    s = 2.5
    oct_ = _families()[0]
    assert abs(rx.inter_area(oct_[1], oct_[2])[1] - 2 * (np.sqrt(2) - 1) * s * s) < 1e-5
    poke = [f for f in _families() if f[0] == "corner poke"][0]
    assert np.allclose(rx.inter_area(poke[1], poke[2]), [0.01, 0.09, 0.0025], rtol=1e-5)
    huge = [f for f in _families() if f[0] == "tiny in huge"][0]
    assert np.allclose(rx.inter_area(huge[1], huge[2]), rx.box_area(huge[1]), rtol=1e-12)


def test_dyadic_edge_sharing_boxes_are_exact():
    """ry = 0 and dyadic parameters: every corner and crossing is exact in float32, and the walk's inclusive inside
    test and strict crossing test alone decide the polygon"""
    a = [0.0, 0.0, 4.0, 2.0, 0.0]                  # [-2, 2] x [-1, 1]
    cases = [([2.0, 0.0, 4.0, 2.0, 0.0], 4.0),     # half-length shift: collinear long edges
             ([1.0, 0.0, 4.0, 2.0, 0.0], 6.0),     # quarter shift
             ([0.0, 0.5, 4.0, 2.0, 0.0], 6.0),     # half-width shift
             ([1.5, 0.5, 1.0, 1.0, 0.0], 1.0),     # inside, two corners on edges, one on a corner
             ([2.0, 1.0, 2.0, 2.0, 0.0], 1.0),     # corner on corner: a quarter of the small box
             ([4.0, 0.0, 4.0, 2.0, 0.0], 0.0),     # touching edges
             ([2.5, 1.5, 1.0, 1.0, 0.0], 0.0),     # touching corners
             ([0.0, 0.0, 4.0, 1.0, 0.0], 4.0),     # same length, half width: both long edges inside
             ([0.0, 0.0, 2.0, 2.0, 0.0], 4.0)]     # same width, half length
    dt = np.array([c for c, _ in cases])
    gt = np.array([a] * len(cases))
    inter = np.array([v for _, v in cases])
    a1, a2 = rx.box_area(gt), rx.box_area(dt)
    assert np.array_equal(rx.inter_area(dt, gt), inter)
    want = {-1: inter / (a1 + a2 - inter), 0: inter / a1, 1: inter / a2, 2: inter}
    assert want[-1][0] == 1 / 3
    for crit, w in want.items():
        got = _gpu_bev(dt, gt, crit)
        print("dyadic crit %2d: largest |gpu - exact| %.3g" % (crit, np.abs(got - w).max()))
        assert np.all(np.abs(got - w) <= 1e-6), (crit, got, w)


def _far_bound(dt, gt, crit):
    return 16 * EPS32 * _reach(dt, gt) ** 2 / _dens(dt, gt, crit)


def far_tol(dt, gt, crit):
    """16 eps32 R^2 of area over the ratio's denominator, at most CEILING (see the module docstring)"""
    return np.minimum(CEILING, np.maximum(TIGHT, _far_bound(dt, gt, crit)))


@pytest.mark.parametrize("z", [60.0, 80.0])
def test_constructed_families_at_far_range(z):
    for name, dt, gt in _families((7.5, z)):
        _check_bev(dt, gt, far_tol, "%s at z = %g" % (name, z))
    # random pairs whose bound stays under the ceiling (boxes of 0.1 m^2 there have bounds of 0.1 and more)
    dt, gt = _random_pairs(1, 3000, (-12.0, z - 10), 10.0, smallest=2.0, thin=0.0)
    keep = rx.well_conditioned(dt, gt, 1e-3) & np.all([_far_bound(dt, gt, c) <= CEILING for c in RATIO], 0)
    dt, gt = dt[keep], gt[keep]
    assert len(dt) >= 1000 and (rx.inter_area(dt, gt) > 0).sum() >= 500
    _check_bev(dt, gt, far_tol, "random at z = %g" % z)


def test_invariances():
    dt, gt = _random_pairs(2, 1500)
    keep = rx.well_conditioned(dt, gt, 1e-3) & (np.abs(dt[:, 4]) < 3 * np.pi)
    dt, gt = dt[keep][:1000], gt[keep][:1000]
    base = {c: _gpu_bev(dt, gt, c) for c in BEV_CRITS}
    exact = {c: rx.bev_value(dt, gt, c) for c in BEV_CRITS}

    def same(dt2, gt2, what):
        # each variant is its own float32 rectangle: held to the yardstick, and to the base by the yardstick's change
        for c in BEV_CRITS:
            got, want = _gpu_bev(dt2, gt2, c), rx.bev_value(dt2, gt2, c)
            s, t = _scale(dt2, gt2, c), near_tol(dt2, gt2, c)
            assert np.all(np.abs(got - want) / s <= t), (what, c)
            assert np.all(np.abs(got - base[c]) / s <= np.abs(want - exact[c]) / s + 2 * t), (what, c)

    for k in (1, -1):
        d2 = dt.copy()
        d2[:, 4] += k * np.pi
        same(d2, gt, "ry + %d pi" % k)
    for k in range(-5, 6):
        d2, g2 = dt.copy(), gt.copy()
        d2[:, 4] += 2 * np.pi * k
        g2[:, 4] -= 2 * np.pi * k
        same(d2, g2, "ry + 2 pi %d" % k)
    d2 = dt[:, [0, 1, 3, 2, 4]].copy()
    d2[:, 4] += np.pi / 2
    same(d2, gt, "(w, l, ry + pi/2)")
    # swapping the boxes: -1 unchanged, 0 and 1 exchanged, raw area unchanged
    sw = {c: _gpu_bev(gt, dt, c) for c in BEV_CRITS}
    assert np.all(np.abs(sw[-1] - base[-1]) <= 2 * near_tol(dt, gt, -1))
    assert np.all(np.abs(sw[0] - base[1]) <= 2 * near_tol(dt, gt, 1))
    assert np.all(np.abs(sw[1] - base[0]) <= 2 * near_tol(dt, gt, 0))
    assert np.all(np.abs(sw[2] - base[2]) <= 2 * TIGHT * _scale(dt, gt, 2))


def test_coincident_and_near_coincident_boxes():
    rng = np.random.default_rng(3)
    n = 300
    b = np.concatenate([rng.uniform(-40, 40, (n, 1)), rng.uniform(0, 80, (n, 1)), rng.uniform(0.05, 20, (n, 2)),
                        rng.uniform(-8 * np.pi, 8 * np.pi, (n, 1))], 1)
    b = b.astype(np.float32).astype(np.float64)
    for c in RATIO:
        assert np.all(_gpu_bev(b, b, c) == 1.0), c
    assert np.array_equal(_gpu_bev(b, b, 2), (b[:, 2].astype(np.float32) * b[:, 3].astype(np.float32)).astype(np.float64))
    # a 1-ulp shift of the centre: the walk is ill-conditioned there, only the range is held, up to the corner
    # rounding's share of the box area (4 eps32 R P / A, as near_tol; a 0.05 m box at 80 m reaches 1.2e-3)
    _near_coincident_in_range(b, (0, 1))


@pytest.mark.xfail(strict=True, reason="a 1-ulp longer, wider or turned box: two edges nearly collinear pass both "
                                       "orientation tests, and the float32 crossing (DH near 0) lands far off the "
                                       "edges; the walk then gives values from -53 to 87, or NaN where DH == 0")
def test_one_ulp_longer_wider_or_turned_box_stays_in_range():
    rng = np.random.default_rng(3)
    n = 300
    b = np.concatenate([rng.uniform(-40, 40, (n, 1)), rng.uniform(0, 80, (n, 1)), rng.uniform(0.05, 20, (n, 2)),
                        rng.uniform(-8 * np.pi, 8 * np.pi, (n, 1))], 1)
    _near_coincident_in_range(b.astype(np.float32).astype(np.float64), (2, 3, 4))


def _near_coincident_in_range(b, params):
    for k in params:
        b2 = b.astype(np.float32)
        b2[:, k] = np.nextafter(b2[:, k], np.float32(np.inf))
        b2 = b2.astype(np.float64)
        for c in RATIO:
            v = _gpu_bev(b2, b, c)
            slack = np.maximum(1e-6, 4 * EPS32 * _reach(b2, b) * 2 * (b[:, 2] + b[:, 3]) / rx.box_area(b))
            print("1-ulp shift of parameter %d, crit %2d: values in [%.9g, %.9g], largest excess over 1: %.3g of "
                  "its slack" % (k, c, v.min(), v.max(), np.max((v - 1) / slack)))
            assert np.all((v >= 0) & (v <= 1 + slack)), (k, c, v.min(), v.max())


# ------------------------------------------------------------------------------------------------ 3-D
def _box7(bev, y, h):
    """camera boxes (x, y, z, l, h, w, ry) from BEV boxes (x, z, l, w, ry) and heights"""
    bev = np.asarray(bev, np.float64).reshape(-1, 5)
    n = len(bev)
    return np.stack([bev[:, 0], np.broadcast_to(y, n), bev[:, 1], bev[:, 2], np.broadcast_to(h, n), bev[:, 3],
                     bev[:, 4]], 1).astype(np.float64)


def test_d3_every_criterion_and_height_edge():
    base = np.array([[1.0, 20.0, 4.0, 1.6, 0.3]])
    shifted = np.array([[1.6, 20.4, 3.8, 1.7, 0.6]])
    far = np.array([[9.0, 20.0, 4.0, 1.6, 0.3]])
    rows = [  # (name, dt bev, dt y, dt h, gt bev, gt y, gt h, expected criterion-2 value)
        ("stacked, touching", base, 1.5, 1.5, base, 3.0, 1.5, 0.0),
        ("stacked, touching, dyadic", shifted, -0.5, 2.0, base, 1.5, 2.0, 0.0),
        ("height inside", base, 1.6, 1.6, shifted, 1.2, 0.7, 1.0),
        ("height around", shifted, 1.2, 0.5, base, 1.6, 1.6, 1.0),
        ("partial height", base, 1.6, 1.5, shifted, 1.0, 1.4, 1.0),
        ("negative y", shifted, -2.0, 1.5, base, -2.5, 1.0, 1.0),
        ("negative y, apart", shifted, -2.0, 1.5, base, -3.6, 1.0, 0.0),
        ("BEV only", base, 1.5, 1.5, shifted, 4.0, 1.5, 0.0),
        ("height only", base, 1.5, 1.5, far, 1.5, 1.5, 0.0),
        ("same BEV box", base, 1.5, 1.5, base, 1.7, 1.9, 1.0),
    ]
    dt7 = np.concatenate([_box7(r[1], r[2], r[3]) for r in rows])
    gt7 = np.concatenate([_box7(r[4], r[5], r[6]) for r in rows])
    # plus random pairs near the origin with random heights
    d5, g5 = _random_pairs(4, 2000)
    keep = rx.well_conditioned(d5, g5, 1e-4)
    d5, g5 = d5[keep], g5[keep]
    rng = np.random.default_rng(5)
    rd = _box7(d5, rng.uniform(-2, 3, len(d5)), rng.uniform(0.2, 3, len(d5)))
    rg = _box7(g5, rng.uniform(-2, 3, len(g5)), rng.uniform(0.2, 3, len(g5)))
    assert (rx.height_overlap(rd, rg) > 0).mean() > 0.4
    dt7, gt7 = np.concatenate([dt7, rd]), np.concatenate([gt7, rg])
    assert np.array_equal(rx.d3_value(dt7[:len(rows)], gt7[:len(rows)], 2), [r[7] for r in rows])
    # the BEV tolerance applied to the ratio: the area's error bound times the height overlap over the denominator
    b_dt, b_gt = dt7[:, [0, 2, 3, 5, 6]], gt7[:, [0, 2, 3, 5, 6]]
    iw = np.maximum(rx.height_overlap(dt7, gt7), 0)
    v1, v2 = dt7[:, 3] * dt7[:, 4] * dt7[:, 5], gt7[:, 3] * gt7[:, 4] * gt7[:, 5]
    area_err = near_tol(b_dt, b_gt, 2) * np.maximum(rx.box_area(b_dt), rx.box_area(b_gt))
    for crit in (-1, 0, 1, 2):
        got, want = _gpu_d3(dt7, gt7, crit), rx.d3_value(dt7, gt7, crit)
        err = np.abs(got - want)
        den = {-1: v1 + v2 - iw * rx.inter_area(b_gt, b_dt), 0: v1, 1: v2}.get(crit)
        tol = TIGHT if den is None else np.maximum(TIGHT, iw * area_err / den)
        print("3-D crit %2d: %5d pairs, largest |gpu - exact| %.3g (tolerance %.3g)"
              % (crit, len(dt7), err.max(), np.broadcast_to(tol, err.shape)[np.argmax(err)]))
        assert np.all(err <= tol), (crit, np.nonzero(err > tol)[0][:5])
        # exact zeros where either overlap is empty (stacked boxes: iw == 0)
        z = (rx.height_overlap(dt7, gt7) <= 0) | (rx.inter_area(gt7[:, [0, 2, 3, 5, 6]], dt7[:, [0, 2, 3, 5, 6]]) == 0)
        assert np.all(got[z] == 0.0), crit
    # criterion 2 (the reference's ua = inc): exactly 1 wherever the boxes overlap
    got = _gpu_d3(dt7, gt7, 2)
    assert set(np.unique(got).tolist()) <= {0.0, 1.0}
    assert np.array_equal(got[:len(rows)], [r[7] for r in rows])


# ------------------------------------------------------------------------------------------------ image boxes
def _img_set(dt_bbox, gt_bbox):
    ke = _ke()
    N, K = len(dt_bbox), len(gt_bbox)

    def anno(bb, n):
        return {"name": np.array(["Car"] * n), "bbox": np.asarray(bb, np.float64), "location": np.zeros((n, 3)),
                "dimensions": np.ones((n, 3)), "rotation_y": np.zeros(n), "alpha": np.zeros(n), "score": np.ones(n),
                "occluded": np.zeros(n), "truncated": np.zeros(n)}

    es = ke.EvalSet([anno(gt_bbox, K)], [anno(dt_bbox, N)])
    es._events = []
    return es


def _gpu_img(dt_bbox, gt_bbox, crit):
    es = _img_set(dt_bbox, gt_bbox)
    out, _ = es._launch_overlaps(("img",), 0, es.F, (-1, -1, crit))
    return out["img"][:len(dt_bbox) * len(gt_bbox)].cpu().numpy().reshape(len(dt_bbox), len(gt_bbox))


def test_image_box_overlap_is_bit_identical():
    ke = _ke()
    rng = np.random.default_rng(6)
    n = 400
    x1, y1 = np.round(rng.uniform(0, 1240, n), 2), np.round(rng.uniform(0, 370, n), 2)
    gt = np.stack([x1, y1, x1 + np.round(rng.uniform(1, 200, n), 2), y1 + np.round(rng.uniform(1, 150, n), 2)], 1)
    dt = np.round(gt + rng.normal(0, 6, gt.shape), 2)                # jittered: most pairs k, k overlap
    special_gt = [[0, 0, 10, 10]] * 7 + [[712.41, 143.07, 722.41, 153.07]] * 3 + [[100.25, 50.5, 110.25, 60.5]] * 2
    special_dt = [[0, 0, 10, 10],          # identical
                  [2, 3, 5, 7],            # nested
                  [10, 0, 20, 10],         # touching: iw == 0
                  [4, 4, 4, 9],            # zero width
                  [8, 8, 2, 2],            # inverted
                  [0, 0, 10, 7],           # IoU exactly 0.7 in real arithmetic
                  [0, 0, 10, 5],           # exactly 0.5
                  [712.41, 143.07, 722.41, 150.07],      # 0.7 with KITTI's 2-decimal coordinates
                  [712.41, 143.07, 722.41, 148.07],      # 0.5
                  [712.41, 143.07, 719.41, 153.07],      # 0.7 the other way
                  [100.25, 50.5, 110.25, 57.5],          # 0.7, dyadic
                  [100.25, 50.5, 105.25, 60.5]]          # 0.5, dyadic
    gt = np.concatenate([gt, special_gt])
    dt = np.concatenate([dt, special_dt])
    for crit in (-1, 0, 1, 2):
        got, want = _gpu_img(dt, gt, crit), ke.image_box_overlap(dt, gt, crit)
        assert np.array_equal(got, want), (crit, np.abs(got - want).max())
    v = np.diag(_gpu_img(dt, gt, -1))[n:]
    assert v[0] == 1.0 and v[1] == 12 / 100 and v[2] == 0.0 and v[3] == 0.0 and v[4] == 0.0
    assert v[5] == 0.7 and v[6] == 0.5 and v[10] == 0.7 and v[11] == 0.5
    assert not (v[5] > 0.7)                   # at min_overlap 0.7 this detection is no TP: 0.7 > 0.7 is false
    # and numpy's plain statement of the same pairs agrees to the last bit
    iw = np.minimum(dt[:, 2], gt[:, 2]) - np.maximum(dt[:, 0], gt[:, 0])
    ih = np.minimum(dt[:, 3], gt[:, 3]) - np.maximum(dt[:, 1], gt[:, 1])
    ua = (dt[:, 2] - dt[:, 0]) * (dt[:, 3] - dt[:, 1]) + (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1]) - iw * ih
    plain = np.where((iw > 0) & (ih > 0), iw * ih / np.where(ua == 0, 1, ua), 0.0)
    assert np.array_equal(np.diag(_gpu_img(dt, gt, -1)), plain)
