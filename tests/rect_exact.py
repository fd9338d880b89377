"""Exact geometry of KITTI's rotated boxes: the yardstick of the overlap kernel (csrc/kitti_eval.hip, ke_overlaps).

A BEV box is (cx, cy, l, w, ry).  Its corners follow the kernel's convention (rbbox_to_corners):
    x' =  cos(ry) * px + sin(ry) * py + cx
    y' = -sin(ry) * px + cos(ry) * py + cy,      px = +-l/2, py = +-w/2,
evaluated in float64 on the float32-rounded parameters, which are the values the kernel receives.  The intersection of
two boxes is one convex quad clipped by the four half-planes of the other (Sutherland-Hodgman) and measured by the
shoelace formula.  This is independent of the reference's float32 polygon walk (corners inside, edge crossings, angular
sort, triangle fan) that the kernel mirrors.  ``clip_area_exact`` runs the same clip on ``Fraction`` corners.

Roles, as the kernel assigns them:
  * BEV (rotate_iou_gpu_eval(boxes=dt, query_boxes=gt)): area1 is the query (gt) box, area2 the dt box;
  * 3-D (d3_box_overlap_kernel, boxes=dt, qboxes=gt): area1 is the dt volume, area2 the gt volume, and the height
    overlap is iw = min(y_dt, y_gt) - max(y_dt - h_dt, y_gt - h_gt) (camera y points down; a box spans [y - h, y]).
"""
from fractions import Fraction

import numpy as np


def f32(a):
    """the float32 rounding of a, as float64"""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def corners(boxes):
    """(..., 5) boxes (cx, cy, l, w, ry) -> (..., 4, 2) float64 corners of the float32-rounded boxes"""
    b = f32(boxes)
    cx, cy, l, w, ry = (b[..., k, None] for k in range(5))
    c, s = np.cos(ry), np.sin(ry)
    px = np.concatenate([-l, -l, l, l], -1) / 2
    py = np.concatenate([-w, w, w, -w], -1) / 2
    return np.stack([c * px + s * py + cx, -s * px + c * py + cy], -1)


def _ccw(q):
    """(N, 4, 2) quads in counter-clockwise order (the kernel's corners turn clockwise for l, w > 0)"""
    x, y = q[..., 0], q[..., 1]
    signed = (x * np.roll(y, -1, -1) - np.roll(x, -1, -1) * y).sum(-1)
    return np.where((signed < 0)[:, None, None], q[:, ::-1], q)


def clip_area(c1, c2):
    """area of the intersection of convex quads c1, c2 ((N, 4, 2) float64 corners, either orientation)"""
    c1, c2 = np.asarray(c1, np.float64).reshape(-1, 4, 2), _ccw(np.asarray(c2, np.float64).reshape(-1, 4, 2))
    N = len(c1)
    M = 9                                          # a quad clipped by 4 half-planes keeps at most 8 vertices
    poly = np.zeros((N, M, 2))
    poly[:, :4] = c1
    cnt = np.full(N, 4)
    rows = np.arange(N)[:, None]
    for e in range(4):
        a, b = c2[:, e], c2[:, (e + 1) % 4]
        ab = b - a
        idx = np.arange(M)[None, :]
        valid = idx < cnt[:, None]
        nxt = np.where(idx + 1 < cnt[:, None], idx + 1, 0)
        p, q = poly, poly[rows, nxt]
        dp = ab[:, None, 0] * (p[..., 1] - a[:, None, 1]) - ab[:, None, 1] * (p[..., 0] - a[:, None, 0])
        dq = ab[:, None, 0] * (q[..., 1] - a[:, None, 1]) - ab[:, None, 1] * (q[..., 0] - a[:, None, 0])
        inp, inq = dp >= 0, dq >= 0
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(inp != inq, dp / (dp - dq), 0.0)
        x = p + t[..., None] * (q - p)
        # candidates in order: p (if inside), then the crossing of p -> q (if the edge changes side)
        cand = np.stack([p, x], 2).reshape(N, 2 * M, 2)
        keep = np.stack([valid & inp, valid & (inp != inq)], 2).reshape(N, 2 * M)
        order = np.argsort(~keep, axis=1, kind="stable")
        cnt = keep.sum(1)
        assert cnt.max(initial=0) <= M
        poly = cand[rows, order[:, :M]]
    idx = np.arange(M)[None, :]
    nxt = np.where(idx + 1 < cnt[:, None], idx + 1, 0)
    q = poly[rows, nxt]
    term = np.where(idx < cnt[:, None], poly[..., 0] * q[..., 1] - q[..., 0] * poly[..., 1], 0.0)
    return np.where(cnt >= 3, np.abs(term.sum(1)) / 2, 0.0)


def clip_area_exact(c1, c2):
    """the same clip in exact rational arithmetic: c1, c2 are 4 corners each, as pairs of Fractions (or ints)"""
    c1 = [(Fraction(x), Fraction(y)) for x, y in c1]
    c2 = [(Fraction(x), Fraction(y)) for x, y in c2]

    def signed(p):
        return sum(p[i][0] * p[(i + 1) % len(p)][1] - p[(i + 1) % len(p)][0] * p[i][1] for i in range(len(p))) / 2

    if signed(c2) < 0:
        c2 = c2[::-1]
    poly = c1
    for e in range(4):
        a, b = c2[e], c2[(e + 1) % 4]
        out = []
        for k in range(len(poly)):
            p, q = poly[k], poly[(k + 1) % len(poly)]
            dp = (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])
            dq = (b[0] - a[0]) * (q[1] - a[1]) - (b[1] - a[1]) * (q[0] - a[0])
            if dp >= 0:
                out.append(p)
            if (dp >= 0) != (dq >= 0):
                t = dp / (dp - dq)
                out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
        poly = out
        if not poly:
            return Fraction(0)
    return abs(signed(poly)) if len(poly) >= 3 else Fraction(0)


def inter_area(b1, b2):
    """exact (float64) intersection area of (N, 5) BEV boxes b1, b2, pair by pair"""
    return clip_area(corners(b1), corners(b2))


def box_area(b):
    b = f32(b).reshape(-1, 5)
    return b[:, 2] * b[:, 3]


def bev_value(dt, gt, criterion=-1):
    """rotate_iou_gpu_eval(dt, gt, criterion) pair by pair: -1 IoU, 0 over the gt (query) area, 1 over the dt area,
    anything else the raw intersection area"""
    dt, gt = np.asarray(dt, np.float64).reshape(-1, 5), np.asarray(gt, np.float64).reshape(-1, 5)
    inter = inter_area(gt, dt)
    a1, a2 = box_area(gt), box_area(dt)
    if criterion == -1:
        return inter / (a1 + a2 - inter)
    if criterion == 0:
        return inter / a1
    if criterion == 1:
        return inter / a2
    return inter


def height_overlap(dt7, gt7):
    """iw of d3_box_overlap_kernel for camera boxes (x, y, z, l, h, w, ry)"""
    dt7, gt7 = np.asarray(dt7, np.float64).reshape(-1, 7), np.asarray(gt7, np.float64).reshape(-1, 7)
    return np.minimum(dt7[:, 1], gt7[:, 1]) - np.maximum(dt7[:, 1] - dt7[:, 4], gt7[:, 1] - gt7[:, 4])


def d3_value(dt7, gt7, criterion=-1):
    """d3_box_overlap(dt7, gt7, criterion) pair by pair: -1 IoU, 0 over the dt volume, 1 over the gt volume, anything
    else 1 wherever the boxes overlap (the reference's ua = inc); 0 where they do not"""
    dt7, gt7 = np.asarray(dt7, np.float64).reshape(-1, 7), np.asarray(gt7, np.float64).reshape(-1, 7)
    inter = inter_area(gt7[:, [0, 2, 3, 5, 6]], dt7[:, [0, 2, 3, 5, 6]])
    iw = height_overlap(dt7, gt7)
    v1, v2 = dt7[:, 3] * dt7[:, 4] * dt7[:, 5], gt7[:, 3] * gt7[:, 4] * gt7[:, 5]
    inc = iw * inter
    if criterion == -1:
        ua = v1 + v2 - inc
    elif criterion == 0:
        ua = v1
    elif criterion == 1:
        ua = v2
    else:
        ua = inc
    with np.errstate(divide="ignore", invalid="ignore"):
        v = inc / ua
    return np.where((inter > 0) & (iw > 0), v, 0.0)


def _seg_dist(p, a, b):
    """distance of points p (N, 2) from segments a -> b (N, 2)"""
    ab, ap = b - a, p - a
    t = np.clip((ap * ab).sum(-1) / np.maximum((ab * ab).sum(-1), 1e-300), 0.0, 1.0)
    return np.hypot(*(ap - t[:, None] * ab).T)


def boundary_distance(pts, quad):
    """distance of points (N, K, 2) from the boundary of quads (N, 4, 2)"""
    d = np.full(pts.shape[:2], np.inf)
    for k in range(pts.shape[1]):
        for e in range(4):
            d[:, k] = np.minimum(d[:, k], _seg_dist(pts[:, k], quad[:, e], quad[:, (e + 1) % 4]))
    return d


def well_conditioned(a, b, margin):
    """True for pairs where no corner of either box lies within margin of the other box's boundary (float64 distances
    of the exact corners): there the polygon walk's inside tests and crossing tests cannot turn on a rounding"""
    ca, cb = corners(np.asarray(a, np.float64).reshape(-1, 5)), corners(np.asarray(b, np.float64).reshape(-1, 5))
    return (boundary_distance(ca, cb).min(1) > margin) & (boundary_distance(cb, ca).min(1) > margin)
