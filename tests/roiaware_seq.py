"""numpy restatement of ``roiaware_pool3d_cuda.forward`` / ``backward`` (the RoI-aware voxel pooling of PartA2) under the
contract of DESIGN.md section 7j (not a test module; tests/test_roiaware_pool_cpu.py, tests/test_gpu_roiaware_pool.py,
tools/make_golden_roiaware_pool.py and tools/roiaware_pool_bench.py import it).

Inside test: the predicate of section 7e, ``roipool_seq.inside_mask``.  The voxel of an inside point, box
[cx, cy, cz, dx, dy, dz, rz], grid (out_x, out_y, out_z), everything float32 with one rounding per operation:
  * res_x = dx / float32(out_x),  q_x = (lx + dx / 2.0f) / res_x; the same for y; for z with lz = z - cz;
  * index = min(max((unsigned)(int)q, 0), out - 1), the int cast to unsigned, conversions saturating and NaN -> 0:
    NaN -> 0;  q <= -1 -> out - 1 (a negative int is a huge unsigned);  q >= out -> out - 1;  otherwise truncation
    toward zero, so -1 < q < 0 -> 0.  +-inf and a zero extent (res = 0, q = +-inf or NaN) fall under these rules.
Lists ``(N, out_x, out_y, out_z, max_pts)`` int32: word 0 is the count, capped at max_pts - 1 and WRITTEN whatever was
given; words 1..count the voxel's points in ascending index, later ones dropped; words beyond count as given.
max: slot order, strictly greater than the best so far from -inf (first of equal maxima; -inf and NaN never win);
argmax written everywhere (-1 for none), pooled only where argmax != -1.  avg: float32 sum in slot order from +0,
divided by float32(count), written only where count > 0; argmax untouched.
Backward, starting from grad_in as given, boxes in ascending index: avg adds grad_out * (1.0f / max(float32(count), 1))
(one rounding for the product) to every listed point; max adds grad_out to argmax, if that point is in the voxel's list.
"""
import numpy as np

from roipool_seq import cos_sin_f32, inside_mask

F = np.float32


def voxel_index(q, out):
    """the index rule on float32 q (any shape) -> int64, 0 <= index < out"""
    q = np.asarray(q, dtype=F)
    with np.errstate(invalid="ignore"):
        trunc = np.trunc(np.where(np.isfinite(q) & (q > -1) & (q < out), q, 0)).astype(np.int64)
        idx = np.where(np.isnan(q), 0, np.where(q <= F(-1), out - 1, np.where(q >= F(out), out - 1, trunc)))
    return idx.astype(np.int64)


def local_q(pts, rois, out):
    """(q_x, q_y, q_z), each (N, P) float32: the quotients the index rule is applied to"""
    p = np.ascontiguousarray(pts, dtype=F).reshape(-1, 3)
    bx = np.ascontiguousarray(rois, dtype=F).reshape(-1, 7)
    cosa, sina = cos_sin_f32(bx[:, 6])
    x, y, z = p[None, :, 0], p[None, :, 1], p[None, :, 2]
    with np.errstate(all="ignore"):
        sx, sy = x - bx[:, None, 0], y - bx[:, None, 1]
        lx = sx * cosa[:, None] + sy * (-sina)[:, None]
        ly = sx * sina[:, None] + sy * cosa[:, None]
        lz = z - bx[:, None, 2]
        qs = []
        for l, d, o in ((lx, bx[:, None, 3], out[0]), (ly, bx[:, None, 4], out[1]), (lz, bx[:, None, 5], out[2])):
            res = d / F(o)
            q = (l + d / F(2.0)) / res
            assert q.dtype == F
            qs.append(q)
    return qs


def voxel_ids(pts, rois, out):
    """-> (mask (N, P) bool, flat voxel id (N, P) int64: (ix * out_y + iy) * out_z + iz, meaningful where mask)"""
    n, p = len(np.reshape(rois, (-1, 7))), len(np.reshape(pts, (-1, 3)))
    if n == 0 or p == 0:
        return np.zeros((n, p), dtype=bool), np.zeros((n, p), dtype=np.int64)
    mask = inside_mask(pts, rois)
    qx, qy, qz = local_q(pts, rois, out)
    ix, iy, iz = voxel_index(qx, out[0]), voxel_index(qy, out[1]), voxel_index(qz, out[2])
    return mask, (ix * out[1] + iy) * out[2] + iz


def build_lists(pts, rois, out, max_pts, lists_given):
    """-> (lists, full): lists a copy of lists_given with counts and points written; full[b] = {voxel: all inside point
    indices, uncapped} for the tests that want to know what was dropped"""
    n = len(np.reshape(rois, (-1, 7)))
    nvox = out[0] * out[1] * out[2]
    lists = np.array(lists_given, dtype=np.int32).reshape(n, nvox, max_pts)
    lists[:, :, 0] = 0
    mask, vid = voxel_ids(pts, rois, out)
    full = []
    for b in range(n):
        k = np.flatnonzero(mask[b])
        v = vid[b, k]
        order = np.argsort(v, kind="stable")
        k, v = k[order], v[order]
        cuts = np.flatnonzero(np.diff(v)) + 1
        groups = {}
        for ks, vv in zip(np.split(k, cuts), v[np.r_[0, cuts]] if len(v) else []):
            groups[int(vv)] = ks
            take = ks[: max_pts - 1]
            lists[b, vv, 0] = len(take)
            lists[b, vv, 1:1 + len(take)] = take
        full.append(groups)
    return lists.reshape(n, out[0], out[1], out[2], max_pts), full


def pool(lists, feat, method, pooled_given, argmax_given):
    """-> (pooled, argmax), copies of the given arrays with what the pooling writes"""
    n = lists.shape[0]
    max_pts = lists.shape[-1]
    feat = np.ascontiguousarray(feat, dtype=F)
    c = feat.shape[1]
    shape = np.shape(pooled_given)
    l = lists.reshape(n, -1, max_pts)
    nvox = l.shape[1]
    pooled = np.array(pooled_given, dtype=F).reshape(n, nvox, c)
    argmax = np.array(argmax_given, dtype=np.int32).reshape(n, nvox, c)
    if method == 0:
        argmax[:] = -1
    if c == 0:
        return pooled.reshape(shape), argmax.reshape(shape)
    for b, v in np.argwhere(l[:, :, 0] > 0):
        idx = l[b, v, 1:1 + l[b, v, 0]]
        vals = feat[idx]                                            # (count, C) in slot order
        if method == 0:
            with np.errstate(invalid="ignore"):
                cand = vals > F(-np.inf)                            # NaN and -inf never win
            key = np.where(cand, vals, F(-np.inf))
            first = np.argmax(key, axis=0)                          # the first of equal maxima
            won = cand.any(axis=0)
            argmax[b, v] = np.where(won, idx[first], -1)
            pooled[b, v, won] = vals[first, np.arange(c)][won]
        else:
            with np.errstate(all="ignore"):
                total = np.cumsum(np.concatenate([np.zeros((1, c), dtype=F), vals]), axis=0, dtype=F)[-1]
                pooled[b, v] = total / F(len(idx))
    return pooled.reshape(shape), argmax.reshape(shape)


def forward(rois, pts, feat, out, max_pts, method, lists_given, pooled_given, argmax_given):
    """-> (lists, pooled, argmax)"""
    lists, _ = build_lists(pts, rois, out, max_pts, lists_given)
    pooled, argmax = pool(lists, feat, method, pooled_given, argmax_given)
    return lists, pooled, argmax


def backward(lists, argmax, grad_out, grad_in_given, method):
    """-> grad_in, a copy of grad_in_given with the gradients added box after box"""
    n = lists.shape[0]
    max_pts = lists.shape[-1]
    g = np.array(grad_in_given, dtype=F)
    npts, c = g.shape
    if c == 0 or npts == 0:
        return g
    l = lists.reshape(n, -1, max_pts)
    go = np.ascontiguousarray(grad_out, dtype=F).reshape(n, l.shape[1], c)
    am = np.asarray(argmax).reshape(n, l.shape[1], c)
    cols = np.arange(c)
    with np.errstate(all="ignore"):
        for b in range(n):
            voxel_of = np.full(npts, -1, dtype=np.int64)
            filled = np.flatnonzero(l[b, :, 0] > 0)
            for v in filled:
                voxel_of[l[b, v, 1:1 + l[b, v, 0]]] = v
            if method == 1:
                for v in filled:
                    w = F(1.0) / max(F(l[b, v, 0]), F(1.0))
                    term = go[b, v] * w
                    assert term.dtype == F
                    idx = l[b, v, 1:1 + l[b, v, 0]]
                    g[idx] = g[idx] + term[None, :]
            else:
                for v in filled:
                    p = am[b, v]
                    ok = (p >= 0) & (p < npts)
                    ok[ok] = voxel_of[p[ok]] == v
                    g[p[ok], cols[ok]] = g[p[ok], cols[ok]] + go[b, v, ok]
    return g


# ---- what the fixture must contain (tools/make_golden_roiaware_pool.py and tests/test_roiaware_pool_cpu.py assert every entry)
def scene_names(rec):
    return sorted(k[:-5] for k in rec if k.endswith("_rois"))


def fixture_cases(rec):
    """name -> bool for every case the fixture promises, read from its recorded arrays alone"""
    rel, max_ptss, grids, cs, nboxes = set(), set(), set(), set(), set()
    odd_n = cap_max = cap_avg = q_int = q_high = q_low = rotated = shared3 = False
    equal_max = none_wins = sent_pooled = sent_argmax = sent_lists = grad_given = count_given_zero = False
    for sc in scene_names(rec):
        rois, pts, feat = rec[sc + "_rois"], rec[sc + "_pts"], rec[sc + "_feat"]
        out = tuple(int(v) for v in rec[sc + "_out"])
        lists, lists_given = rec[sc + "_lists"], rec[sc + "_lists_given"]
        max_pts = lists.shape[-1]
        n, c = len(rois), feat.shape[1]
        max_ptss.add(max_pts), grids.add(out), cs.add(c), nboxes.add(n)
        odd_n |= len(pts) % 64 != 0
        mask, vid = voxel_ids(pts, rois, out)
        qs = local_q(pts, rois, out)
        _, full = build_lists(pts, rois, out, max_pts, lists_given)
        l = lists.reshape(n, -1, max_pts)
        lg = lists_given.reshape(n, -1, max_pts)
        count_given_zero |= bool((lg[:, :, 0] == 0).all())
        am_max, am_avg = rec[sc + "_argmax_max"].reshape(n, -1, c), rec[sc + "_argmax_avg"].reshape(n, -1, c)
        p_max, p_avg = rec[sc + "_pooled_max"].reshape(n, -1, c), rec[sc + "_pooled_avg"].reshape(n, -1, c)
        p_given = rec[sc + "_pooled_given"].reshape(n, -1, c)
        am_given = rec[sc + "_argmax_given"].reshape(n, -1, c)
        grad_given |= bool((rec[sc + "_grad_in_given"] != 0).any())
        sent_argmax |= bool(am_given.size and (am_given != 0).all() and np.array_equal(am_avg, am_given))
        shared3 |= bool(mask.size and (mask.sum(axis=0) >= 3).any())
        for b in range(n):
            rotated |= bool(mask[b].any() and abs(np.sin(2 * float(rois[b, 6]))) > 0.1)
            for q, o in zip(qs, out):
                qi = q[b][mask[b]]
                q_int |= bool(((qi == np.trunc(qi)) & (qi > 0) & (qi < o)).any())
                q_high |= bool((qi >= o).any())
                q_low |= bool(((qi > -1) & (qi < 0)).any())
            for v in range(l.shape[1]):
                allk = full[b].get(v, np.zeros(0, dtype=np.int64))
                cnt = len(allk)
                if max_pts >= 5:
                    rel.add("0" if cnt == 0 else "1" if cnt == 1 else "M-2" if cnt == max_pts - 2 else
                            "M-1" if cnt == max_pts - 1 else ">M-1" if cnt > max_pts - 1 else "other")
                kept = l[b, v, 1:1 + l[b, v, 0]]
                beyond = slice(1 + l[b, v, 0], None)
                sent_lists |= bool(max_pts > 1 + l[b, v, 0] and (lg[b, v, beyond] != 0).all()
                                   and np.array_equal(l[b, v, beyond], lg[b, v, beyond]))
                if cnt == 0:
                    sent_pooled |= bool(c and (p_given[b, v] != 0).all() and np.array_equal(p_max[b, v], p_given[b, v])
                                        and np.array_equal(p_avg[b, v], p_given[b, v]) and (am_max[b, v] == -1).all())
                    continue
                if cnt > max_pts - 1 and len(kept) and c:
                    dropped = allk[max_pts - 1:]
                    with np.errstate(invalid="ignore"):
                        top_dropped = feat[dropped].max(axis=0) > feat[kept].max(axis=0)
                    cap_max |= bool(top_dropped.any())
                    cap_avg |= bool(top_dropped.any() and l[b, v, 0] == max_pts - 1)
                if len(kept) and c:
                    vals = feat[kept]
                    for ch in range(c):
                        col = vals[:, ch]
                        with np.errstate(invalid="ignore"):
                            live = col > F(-np.inf)
                        if not live.any():
                            none_wins |= bool(am_max[b, v, ch] == -1 and p_max[b, v, ch] == p_given[b, v, ch]
                                              and (np.isnan(col).any() or np.isinf(col).any()))
                        elif (col[live] == col[live].max()).sum() >= 2:
                            first = kept[np.flatnonzero(live & (col == col[live].max()))[0]]
                            equal_max |= bool(am_max[b, v, ch] == first)
    return {
        "count 0": "0" in rel, "count 1": "1" in rel, "count max_pts - 2": "M-2" in rel,
        "count max_pts - 1": "M-1" in rel, "count > max_pts - 1": ">M-1" in rel,
        "the largest value is among the dropped points (max)": cap_max,
        "the largest value is among the dropped points (avg)": cap_avg,
        "max_pts 1, 2, 5, 128": max_ptss >= {1, 2, 5, 128},
        "grids (1,1,1), (3,5,2) and a cubic one": {(1, 1, 1), (3, 5, 2)} <= grids
        and any(g[0] == g[1] == g[2] > 1 for g in grids),
        "C = 1, 4, 5": cs >= {1, 4, 5}, "npoints not a multiple of 64": odd_n,
        "one box and several boxes": 1 in nboxes and any(k > 1 for k in nboxes),
        "q exactly an integer": q_int, "q >= out on the high face (clamped)": q_high, "-1 < q < 0 in the low margin": q_low,
        "a rotated box": rotated, "a point shared by >= 3 boxes": shared3, "equal maxima in one voxel": equal_max,
        "a voxel whose only values are -inf or NaN": none_wins, "sentinel in pooled": sent_pooled,
        "sentinel in argmax for avg": sent_argmax, "sentinel in the list words beyond the count": sent_lists,
        "non-zero grad_in as given": grad_given, "recorded count words start at zero": count_given_zero,
    }
