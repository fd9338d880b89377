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


# the faults membership_tiled can be asked for: each is a way the kernel's walk could be wrong that changes an output
FAULTS = ("tile index restarts", "last tile wins", "enlarged latch per tile", "three rounds only",
          "rounds in order of appearance", "sample by rank among those present", "minimum of the first wavefront only",
          "strays join sample 0")


def membership_tiled(points, gt, ext, wg, tile, fault=None):
    """membership, walked as csrc/point_targets.hip walks: workgroups of `wg` points; in each, rounds on the lowest sample
    not yet served; in each round, tiles of `tile` rows of the sample's gt and enlarged boxes; idx is kept on the first
    hit, the enlarged latch is never reset.  `fault` (one of FAULTS) breaks the walk in the named way:
      tile index restarts                  the row index of a hit is min(j0, tile) + j: right in the first two tiles only
      last tile wins                       a later tile's first hit overwrites idx
      enlarged latch per tile              the enlarged latch is cleared at the start of every tile
      three rounds only                    a workgroup stops after three rounds
      rounds in order of appearance        a round serves the first lane's sample above `done`, not the lowest
      sample by rank among those present   the box rows are taken at the sample's rank among the samples the batch names
      minimum of the first wavefront only  the round's sample is not reduced across the workgroup's wavefronts
      strays join sample 0                 a point that names no sample is tested against sample 0
    -> (k, idx, ext_hit) as membership: k is the point's sample whatever the fault"""
    assert fault is None or fault in FAULTS, fault
    points = np.asarray(points, dtype=F)
    B, M, N = gt.shape[0], gt.shape[1], len(points)
    k = sample_of(points, B)
    kk = k.copy()
    if fault == "strays join sample 0" and B:
        kk[k < 0] = 0
    named = np.unique(kk[kk >= 0])
    idx = np.full(N, -1, dtype=np.int64)
    hit = np.zeros(N, dtype=bool)
    for w0 in range(0, N if M else 0, wg):
        lanes = np.arange(w0, min(w0 + wg, N))
        kw = kk[lanes]
        done, rounds = -1, 0
        while True:
            left = kw > done
            pool = kw[:64][left[:64]] if fault == "minimum of the first wavefront only" else kw[left]
            if len(pool) == 0 or (fault == "three rounds only" and rounds == 3):
                break
            s = int(pool[0] if fault == "rounds in order of appearance" else pool.min())
            rounds += 1
            row = int(np.searchsorted(named, s)) if fault == "sample by rank among those present" else s
            mine = lanes[kw == s]
            xyz = points[mine, 1:4]
            for j0 in range(0, M, tile):
                cnt = min(tile, M - j0)
                if fault == "enlarged latch per tile":
                    hit[mine] = False
                g = roipool_seq.inside_mask(xyz, np.ascontiguousarray(gt[row, j0:j0 + cnt, :7]))
                e = roipool_seq.inside_mask(xyz, np.ascontiguousarray(ext[row, j0:j0 + cnt, :7]))
                take = g.any(axis=0)
                if fault != "last tile wins":
                    take &= idx[mine] < 0
                base = min(j0, tile) if fault == "tile index restarts" else j0
                idx[mine[take]] = base + g.argmax(axis=0)[take]
                hit[mine] |= e.any(axis=0)
            done = s
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


def assign(points, gt, ext, num_class, mean_size=None, want_box=False, want_part=False, member=None):
    """-> dict(point_cls_labels (N) int64, point_box_labels (N, 8) float32 or None, point_part_labels (N, 3) or None);
    `member`: the (k, idx, ext_hit) to label from in place of membership's (what membership_tiled returns)"""
    points, gt, ext = (np.asarray(a, dtype=F) for a in (points, gt, ext))
    N = len(points)
    k, idx, hit = membership(points, gt, ext) if member is None else member
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


def crowd_cases(rec, tile):
    """name -> bool for what the scene `crowd` (tests/golden/point_targets_crowd.npz) promises past one tile of `tile` rows,
    read from its recorded arrays alone"""
    cfg, pts, gt, ext, _ = scene_inputs(rec, "crowd")
    lab = recorded(rec, "crowd")["point_cls_labels"]
    k, idx, hit = membership(pts, gt, ext)
    M = gt.shape[1]
    last = (M - 1) // tile * tile              # the first row of the last tile
    got = {"idx in each of three tiles": last == 2 * tile and set(idx[idx >= 0] // tile) == {0, 1, 2},
           "rows of two tiles hold a point, the lower row wins": False,
           "ignored, the only enlarged hit in the last tile": False,
           "point of no sample": bool((k < 0).any()) and bool((lab[k < 0] == 0).all())}
    for s in range(gt.shape[0]):
        sel = np.flatnonzero(k == s)
        g = roipool_seq.inside_mask(pts[sel, 1:4], np.ascontiguousarray(gt[s, :, :7]))
        e = roipool_seq.inside_mask(pts[sel, 1:4], np.ascontiguousarray(ext[s, :, :7]))
        tiles = np.stack([g[t:t + tile].any(axis=0) for t in range(0, M, tile)])
        two = tiles.sum(axis=0) >= 2
        first = g.argmax(axis=0)
        got["rows of two tiles hold a point, the lower row wins"] |= bool(two.any()) and bool(
            (idx[sel][two] == first[two]).all() and (lab[sel][two] == gt[s, first[two], 7].astype(np.int64)).all()
            and (first[two] // tile == tiles[:, two].argmax(axis=0)).all())
        only = (idx[sel] < 0) & e[last:].any(axis=0) & ~e[:last].any(axis=0)
        got["ignored, the only enlarged hit in the last tile"] |= bool(only.any()) and bool((lab[sel][only] == -1).all())
    return got
