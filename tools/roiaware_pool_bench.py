#!/usr/bin/env python
"""Time the RoI-aware voxel pooling at the shape PartA2 runs it at (partA2_head.py:138-143: 128 RoIs, 16 384 points,
12^3 voxels, 128 words per list; avg over C = 4 part features and max over C = 128 backbone features, forward and
backward) against a composition of stock PyTorch-ROCm operators, and write profiles/roiaware_pool_bench.json.

There is no earlier implementation on this hardware and the reference cannot run here, so the yardstick is written in
this file, independent of the code under test: a dense (N, npoints) mask and voxel id from elementwise torch operators
(float32 products, sums and divisions as separate operators, the three comparisons in float64, cos / sin in float64
rounded once, the index rule as `where`s), the hits sorted stably by (box, voxel), ranks from a `cummax` over the
segment starts, one scatter into the lists; max pooling by `scatter_reduce`, avg pooling slot by slot over the non-empty
voxels (the contract's sum is sequential), gradients by `index_add_` / `index_put_(accumulate=True)`.  Its gradient
sums therefore land in atomic order: they are compared with the op's by count of differing bits and largest difference,
everything else bit for bit.  `--check-cpu` runs the yardstick on the CPU against the numpy restatement
(tests/roiaware_seq.py) at a small shape, where its sums are sequential too, and needs no GPU.

Both sides run in this process on the same device; every shape is warmed up first; a window holds enough launches to
last WINDOW_MS and the two sides alternate window by window; median, minimum and maximum of the windows are written.
The op's forward time includes the zero fill of pooled_features the layer does; its backward time includes the zero
fill of grad_in, the workspace and the table step, which is also timed alone ("backward table step").

    python tools/roiaware_pool_bench.py [--out profiles/roiaware_pool_bench.json] [--windows 5] [--check-cpu]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import roiaware_seq as seq  # noqa: E402
import roipool_seq  # noqa: E402
from roipool_bench import launches_for, stats, window  # noqa: E402

I32, I64, F32, F64 = torch.int32, torch.int64, torch.float32, torch.float64
MARGIN = float(np.float32(1e-5))


# ---- the yardstick: stock PyTorch operators -----------------------------------------------------------------------------
def yard_index(q, out):
    big = torch.full_like(q, float(out - 1))
    t = torch.where(torch.isnan(q), torch.zeros_like(q),
                    torch.where(q <= -1.0, big, torch.where(q >= float(out), big, torch.trunc(q))))
    return t.to(I64)


def yard_hits(rois, pts, out):
    """-> (box, point, key = box * V + voxel) of every inside pair, sorted by key, points ascending within a key"""
    bx = rois[:, None, :]
    x, y, z = pts[None, :, 0], pts[None, :, 1], pts[None, :, 2]
    ang = -rois[:, 6].to(F64)
    cosa, sina = torch.cos(ang).to(F32)[:, None], torch.sin(ang).to(F32)[:, None]
    zout = (z - bx[..., 2]).abs().to(F64) > bx[..., 5].to(F64) / 2.0
    sx, sy = x - bx[..., 0], y - bx[..., 1]
    lx = sx * cosa + sy * (-sina)
    ly = sx * sina + sy * cosa
    lz = z - bx[..., 2]
    mask = ~zout & (lx.abs().to(F64) < bx[..., 3].to(F64) / 2.0 + MARGIN) & (ly.abs().to(F64) < bx[..., 4].to(F64) / 2.0 + MARGIN)
    idx = []
    for l, d, o in ((lx, bx[..., 3], out[0]), (ly, bx[..., 4], out[1]), (lz, bx[..., 5], out[2])):
        idx.append(yard_index((l + d / 2.0) / (d / float(o)), o))
    vid = (idx[0] * out[1] + idx[1]) * out[2] + idx[2]
    b, k = mask.nonzero(as_tuple=True)                    # row major: b ascending, k ascending
    key = b * (out[0] * out[1] * out[2]) + vid[b, k]
    key, order = torch.sort(key, stable=True)
    return b[order], k[order], key


def yard_forward(rois, pts, feat, out, max_pts, method, lists_given, pooled_given, argmax_given):
    n, c = rois.shape[0], feat.shape[1]
    nv = n * out[0] * out[1] * out[2]
    _, k, key = yard_hits(rois, pts, out)
    h = torch.arange(len(key), device=key.device)
    start = torch.ones_like(key, dtype=torch.bool)
    start[1:] = key[1:] != key[:-1]
    rank = h - torch.cummax(torch.where(start, h, torch.zeros_like(h)), dim=0).values if len(key) else h
    keep = rank < max_pts - 1
    k, key, rank = k[keep], key[keep], rank[keep]
    lists = lists_given.clone().reshape(nv, max_pts)
    counts = torch.bincount(key, minlength=nv)
    lists[:, 0] = counts.to(I32)
    lists[key, 1 + rank] = k.to(I32)
    pooled, argmax = pooled_given.clone().reshape(nv, c), argmax_given.clone().reshape(nv, c)
    if c and method == 0:
        vals = feat[k]
        live = vals > float("-inf")                       # NaN and -inf never win
        best = torch.full((nv, c), float("-inf"), dtype=F32, device=feat.device)
        best.scatter_reduce_(0, key[:, None].expand(-1, c), torch.where(live, vals, best.new_tensor(float("-inf"))), "amax")
        first = torch.full((nv, c), max_pts, dtype=I64, device=feat.device)
        wins = live & (vals == best[key])
        first.scatter_reduce_(0, key[:, None].expand(-1, c), torch.where(wins, rank[:, None].expand(-1, c), max_pts), "amin")
        won = first < max_pts
        point = lists.gather(1, (first + 1).clamp(max=max_pts - 1)).to(I32)
        argmax = torch.where(won, point, torch.full_like(point, -1))
        taken = feat.gather(0, argmax.clamp(min=0).to(I64))
        pooled = torch.where(won, taken, pooled)
    elif c:
        nz = counts.nonzero()[:, 0]
        cnt = counts[nz]
        total = torch.zeros((len(nz), c), dtype=F32, device=feat.device)
        for s in range(int(cnt.max()) if len(nz) else 0):  # the contract's sum is sequential, slot by slot
            has = (cnt > s)[:, None]
            row = feat[lists[nz, (1 + s) if max_pts > 1 + s else 0].clamp(min=0).to(I64)]
            total = torch.where(has, total + row, total)
        pooled[nz] = total / cnt.to(F32)[:, None]
    shape = tuple(lists_given.shape[:4])
    return lists.reshape(shape + (max_pts,)), pooled.reshape(shape + (c,)), argmax.reshape(shape + (c,))


def yard_backward(lists, argmax, grad_out, grad_in_given, method):
    max_pts, c = lists.shape[-1], grad_out.shape[-1]
    l = lists.reshape(-1, max_pts)
    go = grad_out.reshape(-1, c)
    grad = grad_in_given.clone()
    if method == 1:
        slot = torch.arange(1, max_pts, device=l.device)[None, :]
        v, s = (slot <= l[:, :1]).nonzero(as_tuple=True)  # voxel ascending = box ascending
        w = 1.0 / l[:, 0].to(F32).clamp(min=1.0)
        grad.index_add_(0, l[v, 1 + s].to(I64), go[v] * w[v, None])
    else:
        am = argmax.reshape(-1, c)
        v, ch = (am >= 0).nonzero(as_tuple=True)
        grad.index_put_((am[v, ch].to(I64), ch), go[v, ch], accumulate=True)
    return grad


# ---- the op under test, through the drop-in module ------------------------------------------------------------------------
def op_forward(op, rois, pts, feat, out, max_pts, method):
    shape = (rois.shape[0],) + tuple(out)
    lists = torch.empty(shape + (max_pts,), dtype=I32, device=rois.device)
    pooled = torch.empty(shape + (feat.shape[1],), dtype=F32, device=rois.device)
    argmax = torch.zeros(shape + (feat.shape[1],), dtype=I32, device=rois.device)

    def run():
        pooled.zero_()
        op.forward(rois, pts, feat, argmax, lists, pooled, method)
        return lists, pooled, argmax
    return run


def op_backward(op, lists, argmax, grad_out, npts, method):
    grad = torch.empty((npts, grad_out.shape[-1]), dtype=F32, device=grad_out.device)

    def run():
        grad.zero_()
        op.backward(lists, argmax, grad_out, grad, method)
        return grad
    return run


def op_table_step(lists, npts):
    """the backward's memset + table kernel alone: a backward with one channel less everything else"""
    from modest_amd import _lib
    n, ox, oy, oz, max_pts = lists.shape
    work = torch.empty((npts, n), dtype=I32, device=lists.device)
    go = torch.zeros((n, ox, oy, oz, 1), dtype=F32, device=lists.device)
    grad = torch.zeros((npts, 1), dtype=F32, device=lists.device)
    fn = _lib.load().modest_roiaware_pool3d_backward

    def run():   # avg with C = 1: the second kernel is one lane per point, the table step is unchanged
        rc = fn(n, npts, ox, oy, oz, 1, max_pts, lists.data_ptr(), None, go.data_ptr(), grad.data_ptr(), 1, work.data_ptr(),
                work.numel() * 4, torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        return grad
    return run


def same_bits(a, b):
    return int((a.contiguous().view(I32) != b.contiguous().view(I32)).sum()) if a.dtype == F32 else int((a != b).sum())


def scene(n_pts=16384, n_rois=128):
    xyz, feat, objs = roipool_seq.synthetic_scans()
    rs = np.random.RandomState(128)
    pts = np.concatenate([xyz[0], xyz[0][: n_pts - len(xyz[0])] + rs.normal(0, 0.02, (n_pts - len(xyz[0]), 3)).astype(np.float32)])
    rois = roipool_seq.enlarge(roipool_seq.synthetic_rois(rs, objs, n_rois)[0], (1.0, 1.0, 1.0))
    return rois, pts.astype(np.float32), rs.randn(n_pts, 128).astype(np.float32)


def check_cpu():
    """the yardstick against the numpy restatement, on the CPU, every array bit for bit"""
    rs = np.random.RandomState(3)
    rois, pts, feat = scene()
    rois, pts, feat = rois[:24], pts[:3000], feat[:3000, :5].copy()
    feat[rs.randint(0, 3000, 700)] = 1.5
    feat[rs.randint(0, 3000, 50), 0] = np.nan
    feat[rs.randint(0, 3000, 50), 1] = -np.inf
    rois[3, 3] = 0.0
    for out, max_pts in (((12, 12, 12), 6), ((3, 5, 2), 128), ((2, 2, 2), 1)):
        shape = (len(rois),) + out
        given = (np.full(shape + (max_pts,), -9, dtype=np.int32), np.full(shape + (5,), -3.5, dtype=np.float32),
                 np.full(shape + (5,), -7, dtype=np.int32))
        grad_out, grad_in = rs.randn(*(shape + (5,))).astype(np.float32), rs.randn(3000, 5).astype(np.float32)
        t = torch.from_numpy
        for method in (0, 1):
            want = seq.forward(rois, pts, feat, out, max_pts, method, *given)
            got = yard_forward(t(rois), t(pts), t(feat), out, max_pts, method, *[t(g) for g in given])
            bad = [same_bits(g, t(w)) for g, w in zip(got, want)]
            wg = seq.backward(want[0], want[2], grad_out, grad_in, method)
            bad.append(same_bits(yard_backward(got[0], got[2], t(grad_out), t(grad_in), method), t(wg)))
            print("grid", out, "max_pts", max_pts, "method", method, "largest count", int(want[0][..., 0].max()),
                  "elements that differ (lists, pooled, argmax, grad_in):", bad)
            assert bad == [0, 0, 0, 0]
    print("the yardstick reproduces the restatement on the CPU")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roiaware_pool_bench.json"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--check-cpu", action="store_true", help="compare the yardstick with the numpy restatement on the CPU and exit")
    args = ap.parse_args()
    if args.check_cpu:
        return check_cpu()
    if not torch.cuda.is_available():
        raise SystemExit("tools/roiaware_pool_bench.py needs an MI355X (or --check-cpu)")
    from modest_amd.utils import roiaware_voxel_pool_cuda as op
    dev = torch.device("cuda:0")
    out, max_pts = (12, 12, 12), 128
    rois_h, pts_h, feat_h = scene()
    rois, pts = torch.from_numpy(rois_h).to(dev), torch.from_numpy(pts_h).to(dev)
    rows = []
    with torch.no_grad():
        for method, tag, c in ((1, "avg", 4), (0, "max", 128)):
            feat = torch.from_numpy(np.ascontiguousarray(feat_h[:, :c])).to(dev)
            shape = (len(rois_h),) + out
            fwd = op_forward(op, rois, pts, feat, out, max_pts, method)
            lists, pooled, argmax = fwd()
            zl, zp = torch.zeros(shape + (max_pts,), dtype=I32, device=dev), torch.zeros(shape + (c,), dtype=F32, device=dev)
            za = torch.zeros(shape + (c,), dtype=I32, device=dev)
            yfwd = lambda: yard_forward(rois, pts, feat, out, max_pts, method, zl, zp, za)   # noqa: E731
            yl, yp, ya = yfwd()
            counts = lists[..., 0]
            used = torch.arange(max_pts, device=dev) <= counts[..., None]          # words beyond the count are not written
            info = {"N": len(rois_h), "npoints": len(pts_h), "grid": list(out), "max_pts": max_pts, "C": c, "method": tag,
                    "non-empty voxels": int((counts > 0).sum()), "full voxels": int((counts == max_pts - 1).sum()),
                    "points listed": int(counts.sum())}
            cmp = {"list words that differ": int(((lists != yl) & used).sum()), "pooled elements that differ": same_bits(pooled, yp),
                   "argmax elements that differ": same_bits(argmax, ya) if method == 0 else 0}
            grad_out = torch.randn(shape + (c,), dtype=F32, device=dev)
            bwd = op_backward(op, lists, argmax, grad_out, len(pts_h), method)
            zg = torch.zeros((len(pts_h), c), dtype=F32, device=dev)
            ybwd = lambda: yard_backward(lists, argmax, grad_out, zg, method)       # noqa: E731
            g, yg = bwd(), ybwd()
            cmp.update({"grad_in elements whose bits differ (the yardstick adds in atomic order)": same_bits(g, yg),
                        "grad_in largest difference": float((g - yg).abs().max())})
            torch.cuda.synchronize()
            for name, a, b in ((f"forward {tag} C={c}", fwd, yfwd), (f"backward {tag} C={c}", bwd, ybwd)):
                la, lb = launches_for(a), launches_for(b)
                ta, tb = [], []
                for _ in range(args.windows):
                    ta.append(window(a, la))
                    tb.append(window(b, lb))
                row = {"case": name, "shape": info, "yardstick_vs_op": cmp, "op": dict(stats(ta), launches_per_window=la),
                       "yardstick": dict(stats(tb), launches_per_window=lb)}
                row["yardstick_over_op"] = row["yardstick"]["median_ms"] / row["op"]["median_ms"]
                rows.append(row)
                print(json.dumps({"case": name, "op_ms": row["op"]["median_ms"], "yardstick_ms": row["yardstick"]["median_ms"],
                                  "yardstick_over_op": row["yardstick_over_op"], **cmp}), flush=True)
            if method == 1:
                tab = op_table_step(lists, len(pts_h))
                lt = launches_for(tab)
                tt = [window(tab, lt) for _ in range(args.windows)]
                rows.append({"case": "backward table step (memset + table kernel + one-channel sum)", "shape": info,
                             "table_bytes": len(pts_h) * len(rois_h) * 4, "op": dict(stats(tt), launches_per_window=lt)})
                print(json.dumps({"case": rows[-1]["case"], "op_ms": rows[-1]["op"]["median_ms"]}), flush=True)
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "window_ms_target": 20.0, "windows": args.windows,
           "note": "HIP-event windows, op and yardstick alternating; the op's forward includes the zero fill of pooled_features, its "
                   "backward the zero fill of grad_in, the workspace allocation and the table step; the yardstick is a composition "
                   "of stock PyTorch operators written in tools/roiaware_pool_bench.py",
           "cases": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
