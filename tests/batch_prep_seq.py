"""Numpy restatement of training-batch preparation (modest_amd/csrc/batch_prep.hip): the arithmetic the
kernels are held to bit for bit, written the way the reference's DataBaseSampler / DataAugmentor / DataProcessor apply it
to one sample, and the reference's stage-2 code (sample_points, shuffle_points) run on row numbers.

A case (tests/batch_prep_cases.py) is a dict:
  F, range (6,), extra (3,), road_plane, steps (names of ops.BATCH_PREP_STEPS in order), want_near, remove_outside, min_corners,
  db_points (Nd, F) float32, db_offsets (objects + 1,) int64,
  samples: per sample points (n, F), gt_boxes (G, 7), gt_classes (G,), cand_boxes (C, 7), cand_classes, cand_groups,
           cand_objects (C,), mv_height (C,) float64, cand_z (C,) float32, flip_x, flip_y, cos, sin, angle, scale
"""
import ctypes
import ctypes.util

import numpy as np

from oracle import labels as ol

F32 = np.float32
PI_F = F32(np.pi)
TWO_PI_F = F32(2 * np.pi)
MARGIN = np.float64(F32(1e-2))   # roiaware_pool3d.cpp:131, the CPU path (the device kernels have 1e-5)

_M = None


def _libm():
    global _M
    if _M is None:
        _M = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        _M.cosf.restype = _M.sinf.restype = ctypes.c_float
        _M.cosf.argtypes = _M.sinf.argtypes = [ctypes.c_float]
    return _M


def host_trig(h):
    """(n, 4) float32: cosf(h), sinf(h), cosf(-h), sinf(-h) of the host's C library"""
    m = _libm()
    h = np.asarray(h, F32).ravel()
    return np.array([[m.cosf(float(v)), m.sinf(float(v)), m.cosf(-float(v)), m.sinf(-float(v))] for v in h], F32).reshape(-1, 4)


def fmaf(a, b, c):
    """float32 fma(a, b, c), exactly: the product of two float32 is exact in float64; the float64 sum's own error (TwoSum)
    decides the one case in which rounding it again to float32 would go the wrong way, a sum on a float32 midpoint"""
    a, b, c = (np.asarray(v, F32).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        r = s.astype(F32)
        rd = r.astype(np.float64)
        other = np.where(rd < s, np.nextafter(r, F32(np.inf)), np.nextafter(r, F32(-np.inf))).astype(np.float64)
        mid = np.isfinite(s) & np.isfinite(other) & (rd != s) & ((rd + other) / 2 == s) & (e != 0)
        up = np.maximum(rd, other).astype(F32)
        dn = np.minimum(rd, other).astype(F32)
        fix = np.where(e > 0, up, dn)
    return np.where(mid, fix, r).astype(F32)


def collide(gt7, cand7, groups):
    """database_sampler.py:183-204 on the candidates of all groups -> (C,) bool.  IoU as the kernel evaluates it: the host's
    cosf / sinf, atan2 as the double function (oracle arith "atan2_f64")."""
    gt7 = np.asarray(gt7, F32).reshape(-1, 7)
    cand7 = np.asarray(cand7, F32).reshape(-1, 7)
    groups = np.asarray(groups).ravel()
    valid = np.zeros(len(cand7), bool)
    existed = gt7
    g0 = 0
    while g0 < len(cand7):
        g1 = g0 + 1
        while g1 < len(cand7) and groups[g1] == groups[g0]:
            g1 += 1
        sampled = cand7[g0:g1]
        iou2 = ol.boxes_iou_bev(sampled, sampled, arith="atan2_f64")
        iou2[range(len(sampled)), range(len(sampled))] = 0
        iou1 = ol.boxes_iou_bev(sampled, existed, arith="atan2_f64") if len(existed) else iou2
        iou1 = iou1 if iou1.shape[1] > 0 else iou2
        with np.errstate(invalid="ignore"):
            ok = (iou1.max(axis=1) + iou2.max(axis=1)) == 0
        valid[g0:g1] = ok
        existed = np.concatenate((existed, sampled[ok]), axis=0)
        g0 = g1
    return valid


def f32_down(d):
    f = np.asarray(d, np.float64).astype(F32)
    return np.where(f.astype(np.float64) > d, np.nextafter(f, F32(-np.inf)), f).astype(F32)


def f32_up(d):
    f = np.asarray(d, np.float64).astype(F32)
    return np.where(f.astype(np.float64) < d, np.nextafter(f, F32(np.inf)), f).astype(F32)


def in_boxes(pts, boxes7, trig_neg):
    """(n,) bool: inside any box; roiaware_pool3d.cpp:121-168 with the comparisons in float64, as kitti_infos.points_in_boxes_host"""
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    hit = np.zeros(len(pts), bool)
    for b, (cosa, sina) in zip(boxes7, trig_neg):
        with np.errstate(invalid="ignore", over="ignore"):
            zok = ~(np.abs(z - b[2]).astype(np.float64) > np.float64(b[5]) / 2.0)
            sx, sy = x - b[0], y - b[1]
            lx = sx * cosa + sy * (-sina)
            ly = sx * sina + sy * cosa
            assert lx.dtype == F32
            inx = np.abs(lx).astype(np.float64) < np.float64(b[3]) / 2.0 + MARGIN
            iny = np.abs(ly).astype(np.float64) < np.float64(b[4]) / 2.0 + MARGIN
        hit |= zok & inx & iny
    return hit


def augment(case, s, xyz, boxes):
    """the augmentor steps in order on (n, 3) points and (m, 7) boxes, both float32, in place"""
    with np.errstate(invalid="ignore", over="ignore"):
        for step in case["steps"]:
            if step == "flip_x":
                if s["flip_x"]:
                    xyz[:, 1] = -xyz[:, 1]
                    boxes[:, 1] = -boxes[:, 1]
                    boxes[:, 6] = -boxes[:, 6]
            elif step == "flip_y":
                if s["flip_y"]:
                    xyz[:, 0] = -xyz[:, 0]
                    boxes[:, 0] = -boxes[:, 0]
                    boxes[:, 6] = -(boxes[:, 6] + PI_F)
            elif step == "rotation":
                c, sn = F32(s["cos"]), F32(s["sin"])
                for a in (xyz, boxes):
                    x, y = a[:, 0].copy(), a[:, 1].copy()
                    a[:, 0] = fmaf(y, -sn, x * c)
                    a[:, 1] = fmaf(y, c, x * sn)
                boxes[:, 6] = boxes[:, 6] + F32(s["angle"])
            elif step == "scaling":
                xyz[:, :3] *= F32(s["scale"])
                boxes[:, :6] *= F32(s["scale"])
            else:
                raise ValueError(step)
    assert xyz.dtype == F32 and boxes.dtype == F32


U32 = 2.0 ** -24          # the unit roundoff of float32


def exact_xy(case, s, xy):
    """The exact counterpart of `augment` on x and y, and the derived float32 bound around it (the pattern of
    tests/box_decode_seq.py).  xy (n, 2) float32, the coordinates ahead of the augmentors.  Carried per step: the exact value e of the same float32 inputs under the same float32 c, s and
    scale (float64 arithmetic, whose own error of 2^-53 relative is 2^-29 of a float32 ulp), and a bound B >= |any float32
    evaluation - e|:
      flip       e = -e, B unchanged (a sign is exact)
      rotation   x' = x c - y s: the inputs carry Bx, By; a float32 evaluation rounds the two products and the sum (fused: one
                 product and the sum), each by at most U32 of its magnitude, so
                 B' = |c| Bx + |s| By + 2 U32 (|x c| + |y s| + |c| Bx + |s| By) + U32^2 terms, taken as the factor 2.0001
      scaling    e' = e sc,  B' = |sc| B + U32 (|e'| + |sc| B)
    -> (e (n, 2) float64, B (n, 2) float64)"""
    e = np.asarray(xy, F32).astype(np.float64)
    B = np.zeros_like(e)
    for step in case["steps"]:
        if step == "flip_x" and s["flip_x"]:
            e[:, 1] = -e[:, 1]
        elif step == "flip_y" and s["flip_y"]:
            e[:, 0] = -e[:, 0]
        elif step == "rotation":
            c, sn = np.float64(F32(s["cos"])), np.float64(F32(s["sin"]))
            ex, ey, bx, by = e[:, 0].copy(), e[:, 1].copy(), B[:, 0].copy(), B[:, 1].copy()
            e[:, 0], e[:, 1] = ex * c - ey * sn, ex * sn + ey * c
            inx = abs(c) * bx + abs(sn) * by
            iny = abs(sn) * bx + abs(c) * by
            B[:, 0] = inx + 2.0001 * U32 * (np.abs(ex * c) + np.abs(ey * sn) + inx)
            B[:, 1] = iny + 2.0001 * U32 * (np.abs(ex * sn) + np.abs(ey * c) + iny)
        elif step == "scaling":
            sc = np.float64(F32(s["scale"]))
            e = e * sc
            B = abs(sc) * B + 1.0001 * U32 * (np.abs(e) + abs(sc) * B)
    return e, B


def limit_period(h):
    with np.errstate(invalid="ignore", over="ignore"):
        return (h - np.floor(h / TWO_PI_F + F32(0.5)) * TWO_PI_F).astype(F32)


def corners_inside(boxes7, rng):
    """(m,) int: corners of each box whose three coordinates are inside the range, ends included"""
    rng = np.asarray(rng, F32)
    b = np.asarray(boxes7, F32)
    h64 = b[:, 6].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        c, s = np.cos(h64).astype(F32), np.sin(h64).astype(F32)
        count = np.zeros(len(b), np.int64)
        for q in range(8):
            lx = b[:, 3] * F32(-0.5 if q & 1 else 0.5)
            ly = b[:, 4] * F32(-0.5 if q & 2 else 0.5)
            lz = b[:, 5] * F32(-0.5 if q & 4 else 0.5)
            cx = fmaf(ly, -s, lx * c) + b[:, 0]
            cy = fmaf(ly, c, lx * s) + b[:, 1]
            cz = lz + b[:, 2]
            count += ((cx >= rng[0]) & (cx <= rng[3]) & (cy >= rng[1]) & (cy <= rng[4]) & (cz >= rng[2]) & (cz <= rng[5]))
    return count


def stage1_sample(case, s):
    """-> dict(valid (C,) bool, points (k, F) float32 the survivors in the concatenation's order, near (k,) bool,
    gt (m, 8) float32 the kept boxes with their class index)"""
    Fn = case["F"]
    gt = np.asarray(s["gt_boxes"], F32).reshape(-1, 7)
    cand = np.asarray(s["cand_boxes"], F32).reshape(-1, 7)
    C = len(cand)
    valid = collide(gt, cand, s["cand_groups"]) if C else np.zeros(0, bool)
    off = np.asarray(case["db_offsets"], np.int64)
    pts = np.asarray(s["points"], F32).reshape(-1, Fn)
    low = cand.copy()
    if case["road_plane"] and C:
        low[:, 2] = np.asarray(s["cand_z"], F32)
    obj = []
    for j in np.nonzero(valid)[0]:
        o = int(s["cand_objects"][j])
        op = case["db_points"][off[o]:off[o + 1]].astype(F32).copy()
        with np.errstate(invalid="ignore", over="ignore"):
            op[:, :3] += cand[j, :3]
            if case["road_plane"]:
                op[:, 2] = (op[:, 2].astype(np.float64) - np.float64(s["mv_height"][j])).astype(F32)
        obj.append(op)
    if valid.any():
        big = low[valid].copy()
        with np.errstate(invalid="ignore", over="ignore"):
            big[:, 3:6] += np.asarray(case["extra"], F32)[None, :]
        pts = pts[~in_boxes(pts, big, host_trig(big[:, 6])[:, 2:4])]
    allp = np.concatenate(obj + [pts], axis=0) if obj else pts.copy()
    boxes = np.concatenate([gt, low[valid]], axis=0).astype(F32)
    cls = np.concatenate([np.asarray(s["gt_classes"]).reshape(-1), np.asarray(s["cand_classes"]).reshape(-1)[valid]]).astype(np.int64)
    xyz = allp[:, :3].copy()
    pe, pb = exact_xy(case, s, xyz[:, :2])
    ge, gb = exact_xy(case, s, boxes[:, :2])
    augment(case, s, xyz, boxes)
    allp[:, :3] = xyz
    boxes[:, 6] = limit_period(boxes[:, 6])
    keepb = cls > 0
    if case["remove_outside"]:
        keepb &= corners_inside(boxes, case["range"]) >= case["min_corners"]
    rng = np.asarray(case["range"], F32)
    with np.errstate(invalid="ignore", over="ignore"):
        m = (allp[:, 0] >= rng[0]) & (allp[:, 0] <= rng[3]) & (allp[:, 1] >= rng[1]) & (allp[:, 1] <= rng[4])
        out = allp[m]
        near = np.sqrt((out[:, 0] * out[:, 0] + out[:, 1] * out[:, 1]) + out[:, 2] * out[:, 2]) < F32(40.0)
    gt_out = np.concatenate([boxes[keepb], cls[keepb, None].astype(F32)], axis=1).astype(F32)
    return {"valid": valid, "points": out, "near": near, "gt": gt_out, "exact_xy": pe[m], "bound_xy": pb[m], "gt_exact_xy": ge[keepb],
            "gt_bound_xy": gb[keepb]}


def stage1(case):
    return [stage1_sample(case, s) for s in case["samples"]]


def sample_points_rows(near, num_points, rs):
    """data_processor.py:82-118 on the row numbers of a sample whose survivors carry the near flags `near` -> the chosen rows"""
    n = len(near)
    if num_points == -1:
        return np.arange(n)
    if num_points < n:
        far_idxs_choice = np.where(near == 0)[0]
        near_idxs = np.where(near == 1)[0]
        if num_points > len(far_idxs_choice):
            near_idxs_choice = rs.choice(near_idxs, num_points - len(far_idxs_choice), replace=False)
            choice = np.concatenate((near_idxs_choice, far_idxs_choice), axis=0) if len(far_idxs_choice) > 0 else near_idxs_choice
        else:
            choice = np.arange(0, n, dtype=np.int32)
            choice = rs.choice(choice, num_points, replace=False)
        rs.shuffle(choice)
    else:
        choice = np.arange(0, n, dtype=np.int32)
        while num_points > len(choice):
            extra_choice = rs.choice(n, min(n, num_points - len(choice)), replace=False)
            choice = np.concatenate((choice, extra_choice), axis=0)
        rs.shuffle(choice)
    return choice


def order_rows(stage, processors, rs):
    """the rows of each sample's survivors, in the order the processors leave them; the draws of sample 0, then sample 1, ..."""
    rows = []
    for st in stage:
        cur = np.arange(len(st["points"]))
        for proc in processors:
            if proc[0] == "sample_points":
                cur = cur[sample_points_rows(st["near"][cur], proc[1], rs)]
            elif proc[0] == "shuffle_points":
                cur = cur[rs.permutation(len(cur))]
            else:
                raise ValueError(proc)
        rows.append(cur)
    return rows


def batch(case, stage, rows=None):
    """(points (N, 1 + F) with the sample in column 0, gt_boxes (B, Gmax, 8) zero-padded) as collate_batch stacks them"""
    pts = []
    for b, st in enumerate(stage):
        p = st["points"] if rows is None else st["points"][rows[b]]
        pts.append(np.concatenate([np.full((len(p), 1), b, F32), p], axis=1))
    g = max([len(st["gt"]) for st in stage] + [0])
    gt = np.zeros((len(stage), g, 8), F32)
    for b, st in enumerate(stage):
        gt[b, :len(st["gt"])] = st["gt"]
    return (np.concatenate(pts, axis=0) if pts else np.zeros((0, 1 + case["F"]), F32)), gt


def same_bits(a, b):
    """equal shapes and equal bits; a NaN equals a NaN (a new NaN's sign and payload are the processor's, not the arithmetic's)"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    if a.shape != b.shape:
        return False
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
