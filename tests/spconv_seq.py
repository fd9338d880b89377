"""Sequential restatement of the sparse 3-D convolution contract.  Pure numpy, not a test module,
imports nothing of modest_amd.

Sites are a dict from (b, z, y, x) to the row.  Offset k = (kz_i * ky + ky_i) * kx + kx_i.  The float32 functions add in
the stated order -- k ascending, absent neighbours skipped, channel ascending, product and sum rounded separately --
vectorised over the rows and the output channels only, which the order does not concern.  The weight and bias gradients
add the rows of a segment in ascending order and then the segments (wgrad_segments).  The float64 functions return
the same sums in float64 together with S = sum |a| |b| per element, for the bound gamma_n * S.
"""
import itertools

import numpy as np

F = np.float32
U = 2.0 ** -24


def triple(v):
    return (int(v),) * 3 if np.isscalar(v) else tuple(int(a) for a in v)


def gamma(n):
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def out_shape(shape, kernel, stride, padding, subm):
    shape, k, s, p = triple(shape), triple(kernel), triple(stride), triple(padding)
    if subm:
        return list(shape)
    out = [(shape[j] + 2 * p[j] - k[j]) // s[j] + 1 for j in range(3)]
    if min(out) <= 0:
        raise ValueError(f"output shape {out}")
    return out


def offsets(kernel):
    k = triple(kernel)
    return list(itertools.product(range(k[0]), range(k[1]), range(k[2])))   # ascending in (kz_i * ky + ky_i) * kx + kx_i


def rulebook(indices, batch_size, shape, kernel, stride, padding, subm):
    """-> out_indices (N_out, 4) int32, out_shape, nbr (K, N_out) int32, nbr_t (K, N_in) int32"""
    indices = np.asarray(indices, dtype=np.int32).reshape(-1, 4)
    shape, k = triple(shape), triple(kernel)
    s, p = ((1, 1, 1), tuple(a // 2 for a in k)) if subm else (triple(stride), triple(padding))
    oshape = out_shape(shape, k, s, p, subm)
    rows = {}
    for i, r in enumerate(indices.tolist()):
        r = tuple(r)
        if not (0 <= r[0] < batch_size and all(0 <= r[1 + j] < shape[j] for j in range(3))):
            raise ValueError(f"row {i} = {r} lies outside the shape")
        if r in rows:
            raise ValueError(f"row {i} = {r} is a duplicate")
        rows[r] = i
    offs = offsets(k)
    if subm:
        outs = [tuple(r) for r in indices.tolist()]
    else:
        found = set()
        for (b, z, y, x) in rows:
            for kk in offs:
                t = [c + p[j] - kk[j] for j, c in enumerate((z, y, x))]
                if all(t[j] >= 0 and t[j] % s[j] == 0 and t[j] // s[j] < oshape[j] for j in range(3)):
                    found.add((b, t[0] // s[0], t[1] // s[1], t[2] // s[2]))
        outs = sorted(found)
    nbr = np.full((len(offs), len(outs)), -1, dtype=np.int32)
    nbr_t = np.full((len(offs), len(indices)), -1, dtype=np.int32)
    for o, (b, z, y, x) in enumerate(outs):
        for ki, kk in enumerate(offs):
            q = tuple(c * s[j] - p[j] + kk[j] for j, c in enumerate((z, y, x)))
            if all(0 <= q[j] < shape[j] for j in range(3)):   # axis by axis: nothing wraps
                i = rows.get((b,) + q, -1)
                nbr[ki, o] = i
                if i >= 0:
                    assert nbr_t[ki, i] == -1   # at most one output reads input i at offset k
                    nbr_t[ki, i] = o
    out_indices = indices.copy() if subm else np.asarray(outs, dtype=np.int32).reshape(-1, 4)
    return out_indices, oshape, nbr, nbr_t


def forward32(x, w, bias, nbr):
    """x (N_in, Cin), w (K, Cin, Cout), bias (Cout,) or None -> (N_out, Cout) float32 in the contract's order"""
    x, w = np.asarray(x, dtype=F), np.asarray(w, dtype=F)
    K, cin, cout = w.shape
    acc = np.zeros((nbr.shape[1], cout), dtype=F)
    for k in range(K):
        rows = np.nonzero(nbr[k] >= 0)[0]
        if not len(rows):
            continue
        src = nbr[k, rows]
        for ci in range(cin):
            acc[rows] = acc[rows] + (x[src, ci][:, None] * w[k, ci][None, :])
    if bias is not None:
        acc = acc + np.asarray(bias, dtype=F)[None, :]
    return acc


def input_grad32(dy, w, nbr_t):
    """dy (N_out, Cout) -> dx (N_in, Cin) float32: k ascending, co ascending"""
    dy, w = np.asarray(dy, dtype=F), np.asarray(w, dtype=F)
    K, cin, cout = w.shape
    acc = np.zeros((nbr_t.shape[1], cin), dtype=F)
    for k in range(K):
        rows = np.nonzero(nbr_t[k] >= 0)[0]
        if not len(rows):
            continue
        src = nbr_t[k, rows]
        for co in range(cout):
            acc[rows] = acc[rows] + (dy[src, co][:, None] * w[k, :, co][None, :])
    return acc


WG_SEG_MAX, WG_SEG_ROWS = 32, 1024


def wgrad_segments(n_out):
    """-> (segments, seg_rows): the rows of a weight or bias gradient are cut into min(32, ceil(n_out / 1024)) segments
    (at least one) of ceil(n_out / segments) rows; the last one may be shorter"""
    n_out = int(n_out)
    segments = max(1, min(WG_SEG_MAX, -(-n_out // WG_SEG_ROWS)))
    return segments, -(-n_out // segments)


def weight_grad32(x, dy, nbr):
    """x (N_in, Cin), dy (N_out, Cout), nbr (K, N_out) -> dw (K, Cin, Cout) float32 in the contract's order: per (k, ci,
    co) and segment an accumulator from +0.0f walks the segment's rows in ascending order, rows with nbr[k, o] < 0
    skipped, acc = acc + (x[nbr[k, o], ci] * dy[o, co]) with the product and the sum rounded separately; then
    dw = (((+0 + p_0) + p_1) + ...) over the segments in ascending order.

    The device stages 32 rows at a time and adds 0 * 0 = +0 for an absent row of a staged chunk.  Skipping it here is
    exact: an accumulator that starts at +0 can never become -0 (in round-to-nearest a sum is -0 only when both terms
    are -0), so acc + (+0) leaves every bit of acc unchanged.

    Vectorised over (segment, k, ci, co), which the order does not concern; the loop is over the position in the segment."""
    x, dy, nbr = np.asarray(x, dtype=F), np.asarray(dy, dtype=F), np.asarray(nbr)
    K, n_out = nbr.shape
    cin, cout = x.shape[1], dy.shape[1]
    segments, seg_rows = wgrad_segments(n_out)
    part = np.zeros((segments, K, cin, cout), dtype=F)
    starts = np.arange(segments, dtype=np.int64) * seg_rows
    for j in range(seg_rows):
        o = starts + j
        oc = np.minimum(o, n_out - 1)
        src = nbr[:, oc].T                                    # (segments, K)
        live = (src >= 0) & (o < n_out)[:, None]
        if not live.any():
            continue
        p = x[np.maximum(src, 0)][:, :, :, None] * dy[oc][:, None, None, :]
        part = np.where(live[:, :, None, None], part + p, part)
    dw = np.zeros((K, cin, cout), dtype=F)
    for s in range(segments):
        dw = dw + part[s]
    return dw


def bias_grad32(dy):
    """dy (N_out, Cout) -> db (Cout,) float32: the segments of wgrad_segments, every row added in ascending order from
    +0.0f, then the segments in ascending order from +0.0f"""
    dy = np.asarray(dy, dtype=F)
    n_out, cout = dy.shape
    segments, seg_rows = wgrad_segments(n_out)
    part = np.zeros((segments, cout), dtype=F)
    starts = np.arange(segments, dtype=np.int64) * seg_rows
    for j in range(seg_rows):
        o = starts + j
        live = o < n_out
        part = np.where(live[:, None], part + dy[np.minimum(o, n_out - 1)], part)
    db = np.zeros(cout, dtype=F)
    for s in range(segments):
        db = db + part[s]
    return db


def forward64(x, w, bias, nbr):
    """-> (exact-ish sums in float64, S = sum |x| |w| + |bias|, terms per element + 1)"""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    K, cin, cout = w.shape
    acc, S = np.zeros((nbr.shape[1], cout)), np.zeros((nbr.shape[1], cout))
    terms = np.zeros(nbr.shape[1])
    for k in range(K):
        rows = np.nonzero(nbr[k] >= 0)[0]
        src = nbr[k, rows]
        acc[rows] += x[src] @ w[k]
        S[rows] += np.abs(x[src]) @ np.abs(w[k])
        terms[rows] += cin
    if bias is not None:
        acc += np.asarray(bias, dtype=np.float64)[None, :]
        S += np.abs(np.asarray(bias, dtype=np.float64))[None, :]
    return acc, S, terms[:, None] + 1


def input_grad64(dy, w, nbr_t):
    dy, w = np.asarray(dy, dtype=np.float64), np.asarray(w, dtype=np.float64)
    K, cin, cout = w.shape
    acc, S = np.zeros((nbr_t.shape[1], cin)), np.zeros((nbr_t.shape[1], cin))
    terms = np.zeros(nbr_t.shape[1])
    for k in range(K):
        rows = np.nonzero(nbr_t[k] >= 0)[0]
        src = nbr_t[k, rows]
        acc[rows] += dy[src] @ w[k].T
        S[rows] += np.abs(dy[src]) @ np.abs(w[k]).T
        terms[rows] += cout
    return acc, S, terms[:, None] + 1


def weight_grad64(x, dy, nbr):
    """-> dw (K, Cin, Cout) float64, S, n (K, 1, 1) = contributing rows + 1; db (Cout,), S, n"""
    x, dy = np.asarray(x, dtype=np.float64), np.asarray(dy, dtype=np.float64)
    K = nbr.shape[0]
    dw, S = np.zeros((K, x.shape[1], dy.shape[1])), np.zeros((K, x.shape[1], dy.shape[1]))
    n = np.zeros((K, 1, 1))
    for k in range(K):
        rows = np.nonzero(nbr[k] >= 0)[0]
        src = nbr[k, rows]
        dw[k] = x[src].T @ dy[rows]
        S[k] = np.abs(x[src]).T @ np.abs(dy[rows])
        n[k] = len(rows) + 1
    return (dw, S, n), (dy.sum(0), np.abs(dy).sum(0), len(dy) + 1)
