"""numpy restatement of the nine PointNet++ set-abstraction ops with the contract of DESIGN.md section 7d
(the GPU machine has neither the reference nor the fixture generator).  tests/test_pointnet2_cpu.py shows
that it reproduces every recorded output of tests/golden/pointnet2_batch.npz: indices, temp, float32
distances and interpolations bit for bit, gradients to the derived bound.

Every float32 expression is evaluated as written, one rounding per operation (numpy ufuncs on float32
arrays): (dx*dx + dy*dy) + dz*dz and (w0*p0 + w1*p1) + w2*p2.
"""
import numpy as np

F = np.float32


def _d2(a, b):
    """a (..., 3), b (..., 3) float32, broadcast -> (a - b) squared, summed left to right in float32"""
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def fps_block_size(n):
    """the reference's thread count for n points: the largest power of two <= n, at most 1024"""
    return min(1024, 1 << (int(n).bit_length() - 1))


def fps_rank(n):
    """rank of each of the n points in the reference's tie order (its reduction tree prefers the smaller
    bitreverse(k mod bs), then, inside one thread, the smaller k); unique per point, smaller wins"""
    bs = fps_block_size(n)
    L = bs.bit_length() - 1
    k = np.arange(n, dtype=np.int64)
    low = k % bs
    rev = np.zeros(n, dtype=np.int64)
    for bit in range(L):
        rev |= ((low >> bit) & 1) << (L - 1 - bit)
    return rev * ((n + bs - 1) // bs + 1) + k // bs


def furthest_point_sample(xyz, m, temp=None, tie="tree"):
    """xyz (B, N, 3) float32 -> idx (B, m) int32, temp (B, N) float32 as the kernel leaves it.
    tie = "tree": the contract; "lowest": the lowest index at the maximum (what the contract is NOT)."""
    xyz = np.ascontiguousarray(xyz, dtype=F)
    B, N, _ = xyz.shape
    temp = np.full((B, N), 1e10, dtype=F) if temp is None else np.array(temp, dtype=F)
    idx = np.zeros((B, m), dtype=np.int32)
    rank = fps_rank(N) if tie == "tree" else np.arange(N, dtype=np.int64)
    for b in range(B):
        old = 0
        for j in range(1, m):
            t = np.minimum(_d2(xyz[b], xyz[b, old]), temp[b])
            temp[b] = t
            cand = np.flatnonzero(t == t.max())
            old = int(cand[0]) if len(cand) == 1 else int(cand[np.argmin(rank[cand])])
            idx[b, j] = old
    return idx, temp


def fps_tie_steps(xyz, m):
    """per cloud: (rounds whose maximum is shared by points of different k mod bs, rounds whose maximum is
    shared inside one residue class) along the contract's own path"""
    xyz = np.ascontiguousarray(xyz, dtype=F)
    B, N, _ = xyz.shape
    bs = fps_block_size(N)
    rank = fps_rank(N)
    out = []
    for b in range(B):
        temp = np.full(N, 1e10, dtype=F)
        old, across, inside = 0, 0, 0
        for j in range(1, m):
            temp = np.minimum(_d2(xyz[b], xyz[b, old]), temp)
            cand = np.flatnonzero(temp == temp.max())
            if len(cand) > 1:
                res = cand % bs
                across += len(np.unique(res)) > 1
                inside += len(np.unique(res)) < len(res)
            old = int(cand[np.argmin(rank[cand])])
        out.append((int(across), int(inside)))
    return out


def gather(points, idx):
    """points (B, C, N), idx (B, m) -> (B, C, m)"""
    return np.take_along_axis(np.asarray(points, dtype=F), np.asarray(idx, dtype=np.int64)[:, None, :], axis=2)


def group(points, idx):
    """points (B, C, N), idx (B, P, S) -> (B, C, P, S)"""
    B, P, S = idx.shape
    return gather(points, np.asarray(idx).reshape(B, P * S)).reshape(B, points.shape[1], P, S)


def ball_query(radius, nsample, xyz, new_xyz, idx=None, chunk=128):
    """new_xyz (B, M, 3), xyz (B, N, 3) -> idx (B, M, nsample) int32: the first nsample points with
    d2 < radius*radius (float32 product, strict) in index order, short rows padded with the first hit,
    rows without a hit as given (zero)."""
    xyz, new_xyz = np.asarray(xyz, dtype=F), np.asarray(new_xyz, dtype=F)
    B, N, _ = xyz.shape
    M = new_xyz.shape[1]
    out = np.zeros((B, M, nsample), dtype=np.int32) if idx is None else np.array(idx, dtype=np.int32)
    r2 = F(radius) * F(radius)
    ar = np.arange(nsample)
    for b in range(B):
        for c0 in range(0, M, chunk):
            cen = new_xyz[b, c0:c0 + chunk]
            hit = _d2(cen[:, None, :], xyz[b][None, :, :]) < r2
            cnt = hit.sum(axis=1)
            rows, cols = np.nonzero(hit)
            pos = (np.cumsum(hit, axis=1) - 1)[rows, cols]
            keep = pos < nsample
            blk = out[b, c0:c0 + chunk]
            blk[rows[keep], pos[keep]] = cols[keep]
            pad = (ar[None, :] >= cnt[:, None]) & (cnt[:, None] > 0)
            blk[pad] = np.broadcast_to(blk[:, :1], blk.shape)[pad]
    return out


def three_nn(unknown, known, chunk=512):
    """unknown (B, n, 3), known (B, m, 3) -> dist2 (B, n, 3) float32 squared distances ascending, idx (B, n, 3)
    int32; equal distances keep the lower index first; with m < 3 the unused slots are inf / 0."""
    unknown, known = np.asarray(unknown, dtype=F), np.asarray(known, dtype=F)
    B, n, _ = unknown.shape
    m = known.shape[1]
    dist2 = np.full((B, n, 3), np.inf, dtype=F)
    idx = np.zeros((B, n, 3), dtype=np.int32)
    for b in range(B):
        for c0 in range(0, n, chunk):
            d = _d2(unknown[b, c0:c0 + chunk, None, :], known[b][None, :, :])
            D = d.astype(np.float64)
            rows = np.arange(len(D))
            for j in range(min(3, m)):
                i = np.nanargmin(D, axis=1)       # the first occurrence of the minimum: the lower index
                dist2[b, c0:c0 + chunk, j] = d[rows, i]
                idx[b, c0:c0 + chunk, j] = i
                D[rows, i] = np.nan
    return dist2, idx


def three_interpolate(points, idx, weight):
    """points (B, C, m), idx / weight (B, n, 3) -> (B, C, n) = (w0*p0 + w1*p1) + w2*p2 in float32"""
    points, weight = np.asarray(points, dtype=F), np.asarray(weight, dtype=F)
    p = [gather(points, np.asarray(idx)[:, :, j]) for j in range(3)]
    w = [weight[:, None, :, j] for j in range(3)]
    return (w[0] * p[0] + w[1] * p[1]) + w[2] * p[2]


def _scatter(B, C, N, idx, terms):
    """idx (B, K) -> for terms (B, C, K) float64: (sum, sum of magnitudes, number of terms) per (B, C, N) element"""
    K = idx.shape[1]
    flat = ((np.arange(B)[:, None, None] * C + np.arange(C)[None, :, None]) * N + np.asarray(idx, dtype=np.int64)[:, None, :]).ravel()
    size = B * C * N
    s = np.bincount(flat, weights=terms.ravel(), minlength=size).reshape(B, C, N)
    a = np.bincount(flat, weights=np.abs(terms).ravel(), minlength=size).reshape(B, C, N)
    k = np.bincount(flat, minlength=size).reshape(B, C, N)
    return s, a, k


def gather_grad(grad_out, idx, n):
    """grad_out (B, C, m), idx (B, m) -> exact float64 (sum, sum|term|, count) over (B, C, n)"""
    g = np.asarray(grad_out, dtype=np.float64)
    return _scatter(g.shape[0], g.shape[1], n, np.asarray(idx), g)


def group_grad(grad_out, idx, n):
    """grad_out (B, C, P, S), idx (B, P, S)"""
    g = np.asarray(grad_out, dtype=np.float64)
    B, C, P, S = g.shape
    return _scatter(B, C, n, np.asarray(idx).reshape(B, P * S), g.reshape(B, C, P * S))


def three_interpolate_grad(grad_out, idx, weight, m):
    """grad_out (B, C, n), idx / weight (B, n, 3): the terms are the exact products grad_out * weight"""
    g = np.asarray(grad_out, dtype=np.float64)
    B, C, n = g.shape
    t = (g[:, :, :, None] * np.asarray(weight, dtype=np.float64)[:, None, :, :]).reshape(B, C, n * 3)
    return _scatter(B, C, m, np.asarray(idx).reshape(B, n * 3), t)


def check_grad(got, given, exact):
    """the derived bound: |got - (given + sum)| <= k * 2^-23 * sum|term| per element, k = terms added into it, a
    non-zero initial value counted as one more term; an element no term reaches is exactly as given.
    Returns the number of elements that miss it."""
    s, a, k = exact
    given = np.zeros_like(s) if given is None else np.asarray(given, dtype=np.float64)
    kk = k + (given != 0)
    bound = kk * 2.0 ** -23 * (a + np.abs(given))
    bad = np.abs(np.asarray(got, dtype=np.float64) - (given + s)) > bound
    untouched = k == 0
    bad |= untouched & (np.asarray(got, dtype=np.float64) != given)
    return int(bad.sum())
