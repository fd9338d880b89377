"""numpy restatement of the seven stacked-batch PointNet++ ops with the contract of DESIGN.md section 7h
(the GPU machine has neither the reference nor the fixture generator).  tests/test_pointnet2_stack_cpu.py shows
that it reproduces every recorded output of tests/golden/pointnet2_stack.npz: indices, float32 distances,
grouped rows and interpolations bit for bit, gradients to the derived bound.

All scans of a batch are rows of one tensor; cnt (B,) holds the rows per scan.  Row p belongs to the first scan b
with p < cnt[0] + ... + cnt[b], rows past the total to scan B - 1, negative counts count as 0; the other tensor's
rows of that scan are [start_b, start_b + cnt_b) clipped to its real row count.
"""
import numpy as np

from pointnet2_seq import _d2, _scatter, check_grad  # noqa: F401  (check_grad: for the callers)

F = np.float32


def _counts(cnt):
    return np.maximum(np.asarray(cnt, dtype=np.int64), 0)


def scan_of_rows(m, cnt):
    """-> (m,) the scan of rows 0 .. m - 1"""
    cum = np.cumsum(_counts(cnt))
    return np.minimum(np.searchsorted(cum, np.arange(m), side="right"), len(cum) - 1)


def scan_ranges(cnt, rows):
    """-> (start (B,) unclipped, lo (B,), n (B,)): the scan's first row as the counts say, and its rows clipped to
    a tensor of `rows` rows as [lo, lo + n)"""
    c = _counts(cnt)
    start = np.cumsum(c) - c
    lo = np.minimum(start, rows)
    return start, lo, np.minimum(c, rows - lo)


def _first_hits(hit, cols, nsample, out):
    """hit (Q, K) bool in visiting order, cols (K,) or (Q, K) the index a hit stands for; fills out (Q, nsample) rows:
    the first nsample hits, padded with the first; a row without a hit gets out[0] = -1 and is otherwise left"""
    cnt = hit.sum(axis=1)
    rows, k = np.nonzero(hit)
    pos = (np.cumsum(hit, axis=1) - 1)[rows, k]
    keep = pos < nsample
    vals = cols[k] if cols.ndim == 1 else cols[rows, k]
    out[rows[keep], pos[keep]] = vals[keep]
    pad = (np.arange(nsample)[None, :] >= cnt[:, None]) & (cnt[:, None] > 0)
    out[pad] = np.broadcast_to(out[:, :1], out.shape)[pad]
    out[cnt == 0, 0] = -1


def ball_query(radius, nsample, xyz, xyz_cnt, new_xyz, new_cnt, idx=None, chunk=128):
    """new_xyz (M, 3), xyz (N, 3) -> idx (M, nsample) int32: per centre the first nsample rows of its scan with
    d2 < radius*radius (float32 product, strict) in index order as scan-local indices, short rows padded with the first
    hit; a row without a hit gets idx[0] = -1 and is otherwise as given (zero)."""
    xyz, new_xyz = np.asarray(xyz, dtype=F).reshape(-1, 3), np.asarray(new_xyz, dtype=F).reshape(-1, 3)
    M = len(new_xyz)
    out = np.zeros((M, nsample), dtype=np.int32) if idx is None else np.array(idx, dtype=np.int32)
    r2 = F(radius) * F(radius)
    scan = scan_of_rows(M, new_cnt)
    _, lo, n = scan_ranges(xyz_cnt, len(xyz))
    for b in np.unique(scan):
        rows = np.flatnonzero(scan == b)
        pts = xyz[lo[b]:lo[b] + n[b]]
        cols = np.arange(len(pts), dtype=np.int32)
        for c0 in range(0, len(rows), chunk):
            r = rows[c0:c0 + chunk]
            blk = out[r]
            _first_hits(_d2(new_xyz[r][:, None, :], pts[None, :, :]) < r2, cols, nsample, blk)
            out[r] = blk
    return out


def voxel_query(max_range, radius, nsample, xyz, new_xyz, new_coords, point_indices, idx=None):
    """new_xyz (M, 3), new_coords (M, 4) [batch, z, y, x], point_indices (B, R1, R2, R3): a row of xyz or negative
    -> idx (M, nsample) int32 global rows of xyz.  Cells in dz, dy, dx order over [-range, +range] per axis; outside the
    grid, negative entries, entries >= len(xyz) and a batch index outside [0, B) are skipped; a cell is rejected only if
    d2 > radius*radius, d2 = ((p - c)_x^2 + (p - c)_y^2) + (p - c)_z^2."""
    xyz, new_xyz = np.asarray(xyz, dtype=F).reshape(-1, 3), np.asarray(new_xyz, dtype=F).reshape(-1, 3)
    coords, table = np.asarray(new_coords, dtype=np.int64), np.asarray(point_indices)
    B, R1, R2, R3 = table.shape
    M = len(new_xyz)
    out = np.zeros((M, nsample), dtype=np.int32) if idx is None else np.array(idx, dtype=np.int32)
    r2 = F(radius) * F(radius)
    rz, ry, rx = (int(v) for v in max_range)
    for q in range(M):
        b, z, y, x = (int(v) for v in coords[q])
        cells = np.zeros(0, dtype=np.int64)
        if 0 <= b < B:
            cells = table[b, max(z - rz, 0):max(min(z + rz, R1 - 1) + 1, 0), max(y - ry, 0):max(min(y + ry, R2 - 1) + 1, 0),
                          max(x - rx, 0):max(min(x + rx, R3 - 1) + 1, 0)].reshape(-1).astype(np.int64)
        cells = cells[(cells >= 0) & (cells < len(xyz))]
        hit = ~(_d2(xyz[cells], new_xyz[q][None, :]) > r2)
        row = out[q:q + 1]
        _first_hits(hit[None, :], cells.astype(np.int32), nsample, row)
    return out


def three_nn(unknown, unknown_cnt, known, known_cnt, chunk=512):
    """unknown (N, 3), known (M, 3) -> dist2 (N, 3) float32 squared distances ascending, idx (N, 3) int32 global rows of
    known: the three smallest (distance, index) pairs within the row's scan; unused slots are inf / start_b."""
    unknown, known = np.asarray(unknown, dtype=F).reshape(-1, 3), np.asarray(known, dtype=F).reshape(-1, 3)
    N = len(unknown)
    dist2 = np.full((N, 3), np.inf, dtype=F)
    idx = np.zeros((N, 3), dtype=np.int32)
    scan = scan_of_rows(N, unknown_cnt)
    start, lo, n = scan_ranges(known_cnt, len(known))
    for b in np.unique(scan):
        rows = np.flatnonzero(scan == b)
        kn = known[lo[b]:lo[b] + n[b]]
        idx[rows] = start[b]
        for c0 in range(0, len(rows), chunk):
            r = rows[c0:c0 + chunk]
            d = _d2(unknown[r][:, None, :], kn[None, :, :])
            D = d.astype(np.float64)
            ar = np.arange(len(r))
            for j in range(min(3, len(kn))):
                i = np.nanargmin(D, axis=1)       # the first occurrence of the minimum: the lower index
                dist2[r, j] = d[ar, i]
                idx[r, j] = start[b] + i
                D[ar, i] = np.nan
    return dist2, idx


def _global_rows(idx, idx_cnt, feat_cnt, n_rows):
    """idx (M, S) scan-local -> (global feature row (M, S) int64, valid (M, S))"""
    idx = np.asarray(idx, dtype=np.int64)
    scan = scan_of_rows(len(idx), idx_cnt)
    _, lo, n = scan_ranges(feat_cnt, n_rows)
    valid = (idx >= 0) & (idx < n[scan][:, None])
    return np.where(valid, lo[scan][:, None] + idx, 0), valid


def group(features, feat_cnt, idx, idx_cnt):
    """features (N, C), idx (M, S) scan-local -> (M, C, S); an index outside [0, cnt_b) of its scan reads as 0"""
    features = np.asarray(features, dtype=F)
    rows, valid = _global_rows(idx, idx_cnt, feat_cnt, len(features))
    if len(features) == 0:
        return np.zeros((rows.shape[0], features.shape[1], rows.shape[1]), dtype=F)
    g = np.where(valid[:, :, None], features[rows], F(0))          # (M, S, C)
    return np.ascontiguousarray(g.transpose(0, 2, 1))


def three_interpolate(features, idx, weight):
    """features (M, C), idx / weight (N, 3) global -> (N, C) = (w0*f0 + w1*f1) + w2*f2 in float32; an index outside
    [0, M) reads as 0"""
    features, weight = np.asarray(features, dtype=F), np.asarray(weight, dtype=F)
    idx = np.asarray(idx, dtype=np.int64)
    valid = (idx >= 0) & (idx < len(features))
    f = [np.where(valid[:, j, None], features[np.where(valid[:, j], idx[:, j], 0)], F(0)) for j in range(3)]
    w = [weight[:, j, None] for j in range(3)]
    return (w[0] * f[0] + w[1] * f[1]) + w[2] * f[2]


def _scatter_rows(n_rows, rows, valid, terms):
    """rows / valid (K,), terms (C, K) float64 -> exact (sum, sum|term|, count), each (n_rows, C)"""
    C = terms.shape[0]
    s, a, k = _scatter(1, C, n_rows, rows[valid][None, :], terms[:, valid][None, :, :])
    return tuple(np.ascontiguousarray(v[0].T) for v in (s, a, k))


def group_grad(grad_out, idx, idx_cnt, feat_cnt, n_rows):
    """grad_out (M, C, S), idx (M, S) scan-local -> exact float64 (sum, sum|term|, count) over (n_rows, C)"""
    g = np.asarray(grad_out, dtype=np.float64)
    M, C, S = g.shape
    rows, valid = _global_rows(idx, idx_cnt, feat_cnt, n_rows)
    return _scatter_rows(n_rows, rows.reshape(-1), valid.reshape(-1), g.transpose(1, 0, 2).reshape(C, M * S))


def three_interpolate_grad(grad_out, idx, weight, m_rows):
    """grad_out (N, C), idx / weight (N, 3): the terms are the exact products grad_out * weight -> over (m_rows, C)"""
    g = np.asarray(grad_out, dtype=np.float64)
    N, C = g.shape
    idx = np.asarray(idx, dtype=np.int64)
    valid = (idx >= 0) & (idx < m_rows)
    t = (g.T[:, :, None] * np.asarray(weight, dtype=np.float64)[None, :, :]).reshape(C, N * 3)
    return _scatter_rows(m_rows, np.where(valid, idx, 0).reshape(-1), valid.reshape(-1), t)
