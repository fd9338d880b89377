"""numpy restatement of ``PointHeadTemplate.assign_stack_targets`` (set_ignore_flag=True, use_ball_constraint=False)
with ``PointResidualCoder.encode_torch`` under the contract of DESIGN.md section 7l (not a test module;
tests/test_point_targets_cpu.py, tests/test_gpu_point_targets.py and tools/make_golden_point_targets.py import it).
Membership is ``roipool_seq.inside_mask`` (the predicate of section 7e).

All arithmetic is float32 in the written order (numpy does not fuse); log / cos / sin are the double functions rounded
once.
"""
import numpy as np

import roipool_seq

F = np.float32
TINY = F(1e-5)
U = 2.0 ** -24          # half a float32 ulp relative to the value's binade: the unit roundoff


def f32_of_double(fn, v):
    return fn(np.asarray(v, dtype=F).astype(np.float64)).astype(F)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    """equal bit for bit, a NaN equal to any NaN (the payload of an invalid operation differs between machines)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    return bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def sample_of(points, B):
    """(N,) int: k where points[i, 0] == float(k) for a k in [0, B), else -1"""
    bs = np.asarray(points, dtype=F)[:, 0]
    k = np.full(len(bs), -1, dtype=np.int64)
    for s in range(B):
        k[bs == F(s)] = s
    return k


def membership(points, gt, ext):
    """-> (k, idx, ext_hit): sample, lowest gt box of the sample holding the point or -1, any enlarged box holding it"""
    points = np.asarray(points, dtype=F)
    B, M = gt.shape[0], gt.shape[1]
    k = sample_of(points, B)
    idx = np.full(len(points), -1, dtype=np.int64)
    hit = np.zeros(len(points), dtype=bool)
    for s in range(B):
        sel = np.flatnonzero(k == s)
        if len(sel) == 0 or M == 0:
            continue
        xyz = points[sel, 1:4]
        idx[sel] = roipool_seq.points_in_boxes(np.ascontiguousarray(gt[s:s + 1, :, :7]), xyz[None])[0]
        hit[sel] = roipool_seq.inside_mask(xyz, np.ascontiguousarray(ext[s, :, :7])).any(axis=0)
    return k, idx, hit


def encode(box, xyz, cls, mean_size):
    """PointResidualCoder.encode_torch: box (n, 7), xyz (n, 3), cls (n,) int64, mean_size (n_cls, 3) or None -> (n, 8)"""
    box, xyz = np.asarray(box, dtype=F), np.asarray(xyz, dtype=F)
    out = np.zeros((len(box), 8), dtype=F)
    dg = np.maximum(box[:, 3:6], TINY)
    d = box[:, 0:3] - xyz
    with np.errstate(all="ignore"):
        if mean_size is not None:
            mean_size = np.asarray(mean_size, dtype=F).reshape(-1, 3)
            n_cls = len(mean_size)
            r = cls - 1
            r = np.where(r < 0, r + n_cls, r)
            inside = (r >= 0) & (r < n_cls)          # beyond the table: outside the contract, nothing read, NaN
            da = mean_size[np.where(inside, r, 0)]
            diag = np.sqrt(da[:, 0] * da[:, 0] + da[:, 1] * da[:, 1])
            out[:, 0] = d[:, 0] / diag
            out[:, 1] = d[:, 1] / diag
            out[:, 2] = d[:, 2] / da[:, 2]
            out[:, 3:6] = f32_of_double(np.log, dg / da)
            out[~inside, 0:6] = np.nan
        else:
            out[:, 0:3] = d
            out[:, 3:6] = f32_of_double(np.log, dg)
    out[:, 6] = f32_of_double(np.cos, box[:, 6])
    out[:, 7] = f32_of_double(np.sin, box[:, 6])
    assert out.dtype == F
    return out


def part_offsets(box, xyz, clamped):
    """the point in the box's frame / (dx, dy, dz) + 0.5; the sizes clamped to 1e-5 iff the coder ran before (it clamps
    the foreground rows in place) -> (n, 3)"""
    box, xyz = np.asarray(box, dtype=F), np.asarray(xyz, dtype=F)
    size = np.maximum(box[:, 3:6], TINY) if clamped else box[:, 3:6]
    a = -box[:, 6]
    c, s = f32_of_double(np.cos, a), f32_of_double(np.sin, a)
    sx, sy, sz = xyz[:, 0] - box[:, 0], xyz[:, 1] - box[:, 1], xyz[:, 2] - box[:, 2]
    with np.errstate(all="ignore"):
        lx = sx * c + sy * (-s)
        ly = sx * s + sy * c
        out = np.stack([lx / size[:, 0] + F(0.5), ly / size[:, 1] + F(0.5), sz / size[:, 2] + F(0.5)], axis=1)
    assert out.dtype == F
    return out


def assign(points, gt, ext, num_class, mean_size=None, want_box=False, want_part=False):
    """-> dict(point_cls_labels (N) int64, point_box_labels (N, 8) float32 or None, point_part_labels (N, 3) or None)"""
    points, gt, ext = (np.asarray(a, dtype=F) for a in (points, gt, ext))
    N = len(points)
    k, idx, hit = membership(points, gt, ext)
    fg = idx >= 0
    rows = gt[k[fg], idx[fg]] if fg.any() else np.zeros((0, 8), dtype=F)
    with np.errstate(invalid="ignore"):
        cls = np.trunc(rows[:, 7]).astype(np.int64)
    labels = np.zeros(N, dtype=np.int64)
    labels[fg ^ hit] = -1
    labels[fg] = 1 if num_class == 1 else cls
    box = part = None
    if want_box:
        box = np.zeros((N, 8), dtype=F)
        box[fg] = encode(rows[:, :7], points[fg, 1:4], cls, mean_size)
    if want_part:
        part = np.zeros((N, 3), dtype=F)
        part[fg] = part_offsets(rows[:, :7], points[fg, 1:4], clamped=want_box)
    return {"point_cls_labels": labels, "point_box_labels": box, "point_part_labels": part}


def part_bound(points, gt, ext, want_box):
    """(N, 3) float64: how far a part label computed by torch (cos / sin within 1 ulp, a matmul that may sum in any order
    and may fuse) can lie from the restatement's -- DESIGN.md section 7l, computed from the inputs"""
    points, gt = np.asarray(points, dtype=F), np.asarray(gt, dtype=F)
    k, idx, _ = membership(points, gt, ext)
    fg = idx >= 0
    out = np.zeros((len(points), 3))
    if not fg.any():
        return out
    rows = gt[k[fg], idx[fg]].astype(F)
    xyz = points[fg, 1:4]
    size = np.maximum(rows[:, 3:6], TINY) if want_box else rows[:, 3:6]
    ours = part_offsets(rows[:, :7], xyz, clamped=want_box).astype(np.float64)
    sx = np.abs((xyz[:, 0] - rows[:, 0]).astype(np.float64))
    sy = np.abs((xyz[:, 1] - rows[:, 1]).astype(np.float64))
    A = sx + sy
    e_l = 6.0 * U * A                                      # 1.5 u A from the trig values, 2 u A (1 + u) from each side's arithmetic
    b = np.zeros((len(rows), 3))
    with np.errstate(all="ignore"):
        for c in range(2):
            d = np.abs(size[:, c].astype(np.float64))
            q = np.abs(ours[:, c] - 0.5) + U * (np.abs(ours[:, c]) + 0.5)   # |l / d| of ours, its own roundings given back
            e = e_l / d
            b[:, c] = e + 2.0 * U * (q + e) + 2.0 * U * (q + e + 0.5)
    b *= 1.0 + 2.0 ** -20                                  # the second-order terms dropped above
    out[fg] = np.where(np.isfinite(b), b, np.inf)
    return out


# ---- the fixture (tools/make_golden_point_targets.py writes it, tests/test_point_targets_cpu.py reads it) -------------
def scenes(rec):
    import json
    return json.loads(str(rec["scenes"]))


def scene_inputs(rec, name):
    import json
    cfg = json.loads(str(rec[name + "_cfg"]))
    mean = rec[name + "_mean_size"] if cfg["use_mean_size"] else None
    return cfg, rec[name + "_points"], rec[name + "_gt"], rec[name + "_ext"], mean


def recorded(rec, name):
    cfg = scene_inputs(rec, name)[0]
    return {"point_cls_labels": rec[name + "_labels"],
            "point_box_labels": rec[name + "_box"] if cfg["want_box"] else None,
            "point_part_labels": rec[name + "_part"] if cfg["want_part"] else None}


def mismatches(ours, ref, bound=None):
    """[text] of what differs: labels and box labels bit for bit; part labels bit for bit, or within `bound` (N, 3)"""
    why = []
    if not same_bits(ours["point_cls_labels"], ref["point_cls_labels"]):
        why.append("point_cls_labels differ at %s" % np.flatnonzero(ours["point_cls_labels"] != ref["point_cls_labels"])[:8])
    for key in ("point_box_labels", "point_part_labels"):
        a, b = ours[key], ref[key]
        if (a is None) != (b is None):
            why.append(f"{key}: one is None")
            continue
        if a is None:
            continue
        if a.shape != b.shape or a.dtype != b.dtype:
            why.append(f"{key}: {a.shape} {a.dtype} against {b.shape} {b.dtype}")
        elif key == "point_part_labels" and bound is not None:
            with np.errstate(invalid="ignore"):
                d = np.abs(a.astype(np.float64) - b.astype(np.float64))
            bad = ~((d <= bound) | (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b)))
            if bad.any():
                at = np.argwhere(bad)[0]
                why.append(f"{key}: {int(bad.sum())} beyond the bound, first at {tuple(at)}: {a[tuple(at)]!r} against "
                           f"{b[tuple(at)]!r}, bound {bound[tuple(at)]!r}")
        elif not same_bits(a, b):
            at = np.argwhere(~((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))[0]
            why.append(f"{key}: differ, first at {tuple(at)}: {a[tuple(at)]!r} against {b[tuple(at)]!r}")
    return why


def enlarge(gt, extra=(0.2, 0.2, 0.2)):
    """box_utils.enlarge_box3d on (B, M, 8): the three sizes grown in float32, the rest as given"""
    out = np.array(gt, dtype=F)
    out[..., 3:6] = out[..., 3:6] + np.asarray(extra, dtype=F)
    return out


def fixture_cases(rec):
    """name -> bool for every case the fixture promises, read from its recorded arrays alone"""
    got = {"foreground": False, "ignored": False, "background inside a sample": False, "point of no sample": False,
           "two boxes hold a point": False, "class 0 wraps": False, "num_class 1": False, "no mean size": False,
           "box and part": False, "part alone": False, "box alone": False, "labels alone": False,
           "a size at the clamp": False, "zero row holds the origin": False, "B > 1": False}
    for name in scenes(rec):
        cfg, pts, gt, ext, mean = scene_inputs(rec, name)
        ref = recorded(rec, name)
        k, idx, hit = membership(pts, gt, ext)
        fg = idx >= 0
        lab = ref["point_cls_labels"]
        got["foreground"] |= bool(fg.any())
        got["ignored"] |= bool((lab == -1).any())
        got["background inside a sample"] |= bool(((k >= 0) & ~fg & ~hit).any())
        got["point of no sample"] |= bool((k < 0).any())
        got["B > 1"] |= gt.shape[0] > 1
        got["num_class 1"] |= cfg["num_class"] == 1 and bool(fg.any())
        got["no mean size"] |= (not cfg["use_mean_size"]) and cfg["want_box"] and bool(fg.any())
        got["box and part"] |= cfg["want_box"] and cfg["want_part"]
        got["part alone"] |= cfg["want_part"] and not cfg["want_box"]
        got["box alone"] |= cfg["want_box"] and not cfg["want_part"]
        got["labels alone"] |= not cfg["want_box"] and not cfg["want_part"]
        for s in range(gt.shape[0]):
            sel = np.flatnonzero(k == s)
            if len(sel) and gt.shape[1]:
                m = roipool_seq.inside_mask(pts[sel, 1:4], np.ascontiguousarray(gt[s, :, :7]))
                got["two boxes hold a point"] |= bool((m.sum(axis=0) >= 2).any())
        rows = gt[k[fg], idx[fg]]
        if len(rows):
            got["class 0 wraps"] |= cfg["use_mean_size"] and cfg["want_box"] and cfg["num_class"] > 1 and bool((rows[:, 7] == 0).any())
            got["a size at the clamp"] |= cfg["want_box"] and bool((rows[:, 3:6] < TINY).any())
            got["zero row holds the origin"] |= bool((~rows.any(axis=1)).any())
    return got
