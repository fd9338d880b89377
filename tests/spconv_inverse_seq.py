"""Sequential restatement of the inverse sparse convolution.  Pure numpy, not a test module,
imports nothing of modest_amd.

Written from coordinates: a dict from site to row on either side and the rule i = o * s - p + k.  It does not read the
neighbour maps of a rulebook; `pairs` is its own table, pairs[k, i] = the coarse row o that fine row i reads at offset k
(at most one), -1 where there is none.  The float32 functions add in the contract's order -- k ascending, absent pairs
skipped, channel ascending, product and sum rounded separately --, the float64 functions return the same sums with
S = sum |a| |b| and the number of terms + 1, for the bound gamma_n * S.
"""
import numpy as np

import spconv_seq as seq

F = np.float32


def classes(stride):
    s = seq.triple(stride)
    return s[0] * s[1] * s[2]


def row_classes(indices, stride, padding):
    """the mixed-radix number of ((z + p_z) mod s_z, (y + p_y) mod s_y, (x + p_x) mod s_x) per row"""
    indices = np.asarray(indices, dtype=np.int64).reshape(-1, 4)
    s, p = seq.triple(stride), seq.triple(padding)
    cls = np.zeros(len(indices), dtype=np.int64)
    for j in range(3):
        cls = cls * s[j] + (indices[:, 1 + j] + p[j]) % s[j]
    return cls


def class_order(indices, stride, padding):
    """-> perm (N,) int32: the rows stably ordered by class; class_start (C + 1,) int32: the exclusive counts"""
    cls = row_classes(indices, stride, padding)
    perm = np.argsort(cls, kind="stable").astype(np.int32)
    counts = np.bincount(cls, minlength=classes(stride))
    return perm, np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def admitted(cls, kernel, stride):
    """the offsets k (ascending) that a row of class cls can be read at: k_j = r_j, r_j + s_j, ... < K_j on every axis"""
    k, s = seq.triple(kernel), seq.triple(stride)
    r = [(cls // (s[1] * s[2])) % s[0], (cls // s[2]) % s[1], cls % s[2]]
    return [(kz * k[1] + ky) * k[2] + kx for kz in range(r[0], k[0], s[0]) for ky in range(r[1], k[1], s[1])
            for kx in range(r[2], k[2], s[2])]


def pairs(fine, coarse, shape, kernel, stride, padding):
    """pairs (K, N_fine) int32 from the coordinates alone: for coarse row o and offset k, the fine site o * s - p + k"""
    fine = np.asarray(fine, dtype=np.int64).reshape(-1, 4)
    coarse = np.asarray(coarse, dtype=np.int64).reshape(-1, 4)
    shape, s, p = seq.triple(shape), seq.triple(stride), seq.triple(padding)
    rows = {tuple(r): i for i, r in enumerate(fine.tolist())}
    assert len(rows) == len(fine)
    offs = seq.offsets(kernel)
    table = np.full((len(offs), len(fine)), -1, dtype=np.int32)
    for o, (b, z, y, x) in enumerate(coarse.tolist()):
        for k, kk in enumerate(offs):
            q = tuple(c * s[j] - p[j] + kk[j] for j, c in enumerate((z, y, x)))
            if all(0 <= q[j] < shape[j] for j in range(3)):
                i = rows.get((b,) + q)
                if i is not None:
                    assert table[k, i] == -1
                    table[k, i] = o
    return table


def forward32(x, w, bias, table):
    """x (N_coarse, Cin), w (K, Cin, Cout) -> (N_fine, Cout) float32; a fine row that nothing reads is +0.0 (or the bias)"""
    x, w = np.asarray(x, dtype=F), np.asarray(w, dtype=F)
    K, cin, cout = w.shape
    acc = np.zeros((table.shape[1], cout), dtype=F)
    for k in range(K):
        rows = np.nonzero(table[k] >= 0)[0]
        if not len(rows):
            continue
        src = table[k, rows]
        for ci in range(cin):
            acc[rows] = acc[rows] + (x[src, ci][:, None] * w[k, ci][None, :])
    if bias is not None:
        acc = acc + np.asarray(bias, dtype=F)[None, :]
    return acc


def input_grad32(dy, w, table, n_coarse):
    """dy (N_fine, Cout) -> dx (N_coarse, Cin) float32: per coarse row, k ascending over its pairs, co ascending"""
    dy, w = np.asarray(dy, dtype=F), np.asarray(w, dtype=F)
    K, cin, cout = w.shape
    acc = np.zeros((n_coarse, cin), dtype=F)
    for k in range(K):
        fine = np.nonzero(table[k] >= 0)[0]
        if not len(fine):
            continue
        o = table[k, fine]   # distinct: a coarse row writes one fine site per offset
        for co in range(cout):
            acc[o] = acc[o] + (dy[fine, co][:, None] * w[k, :, co][None, :])
    return acc


def forward64(x, w, bias, table):
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    K, cin, cout = w.shape
    acc, S = np.zeros((table.shape[1], cout)), np.zeros((table.shape[1], cout))
    terms = np.zeros(table.shape[1])
    for k in range(K):
        rows = np.nonzero(table[k] >= 0)[0]
        src = table[k, rows]
        acc[rows] += x[src] @ w[k]
        S[rows] += np.abs(x[src]) @ np.abs(w[k])
        terms[rows] += cin
    if bias is not None:
        acc += np.asarray(bias, dtype=np.float64)[None, :]
        S += np.abs(np.asarray(bias, dtype=np.float64))[None, :]
    return acc, S, terms[:, None] + 1


def input_grad64(dy, w, table, n_coarse):
    dy, w = np.asarray(dy, dtype=np.float64), np.asarray(w, dtype=np.float64)
    K, cin, cout = w.shape
    acc, S = np.zeros((n_coarse, cin)), np.zeros((n_coarse, cin))
    terms = np.zeros(n_coarse)
    for k in range(K):
        fine = np.nonzero(table[k] >= 0)[0]
        o = table[k, fine]
        acc[o] += dy[fine] @ w[k].T
        S[o] += np.abs(dy[fine]) @ np.abs(w[k]).T
        terms[o] += cout
    return acc, S, terms[:, None] + 1


def weight_grad64(x, dy, table):
    """-> (dw (K, Cin, Cout) float64, S, n (K, 1, 1) = contributing rows + 1), (db (Cout,), S, n)"""
    x, dy = np.asarray(x, dtype=np.float64), np.asarray(dy, dtype=np.float64)
    K = table.shape[0]
    dw, S = np.zeros((K, x.shape[1], dy.shape[1])), np.zeros((K, x.shape[1], dy.shape[1]))
    n = np.zeros((K, 1, 1))
    for k in range(K):
        fine = np.nonzero(table[k] >= 0)[0]
        o = table[k, fine]
        dw[k] = x[o].T @ dy[fine]
        S[k] = np.abs(x[o]).T @ np.abs(dy[fine])
        n[k] = len(fine) + 1
    return (dw, S, n), (dy.sum(0), np.abs(dy).sum(0), len(dy) + 1)
