#!/usr/bin/env python
"""Time the nine PointNet++ ops at the shapes PointRCNN runs them at (pointrcnn_dynamic_obj.yaml, B = 2) against a
composition of stock PyTorch-ROCm operators, and write profiles/pointnet2_bench.json.

There is no earlier implementation on this hardware and the reference cannot run here, so the yardstick is written
in this file, independent of the code under test: furthest point sampling as a Python loop of min / argmax, ball
query and three-NN from torch.cdist + topk, the gathers and their gradients by indexing + autograd.  Both run in this
process on the same device; every shape is warmed up first; a window holds enough launches to last WINDOW_MS and the
two sides alternate window by window (other people's work shares the host); median, minimum and maximum of the
windows are all written.  Before any time is reported the yardstick's outputs are compared with the op's on the timed
inputs: cdist rounds differently from the contract's expression, so index entries may differ for pairs within rounding
of the radius or of each other, and argmax breaks ties differently; their number goes into the JSON.

Per-kernel times are NOT taken here: run `rocprofv3 --kernel-trace --stats -- python tools/pointnet2_bench.py --once`
separately (profiles/pointnet2_kernel_stats.csv).

    python tools/pointnet2_bench.py [--out profiles/pointnet2_bench.json] [--windows 5] [--once]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from modest_amd import synth  # noqa: E402
from modest_amd.utils.pointnet2.pointnet2_batch import pointnet2_batch_cuda as ops  # noqa: E402

WINDOW_MS = 20.0
SA_NPOINTS = (4096, 1024, 256, 64)
SA_RADIUS = ((0.1, 0.5), (0.5, 1.0), (1.0, 2.0), (2.0, 4.0))
SA_NSAMPLE = ((16, 32), (16, 32), (16, 32), (16, 32))
GROUP_C = (3, 96, 256, 512)          # channels grouped at each level (coordinates at the first; SA outputs after)
INTERP_C = (256, 512, 512, 1024)     # channels of the known level each feature-propagation module interpolates
I32, F32 = torch.int32, torch.float32


# ---- the ops under test, on preallocated buffers (the zero fills the reference's Python side does are timed too) ----
def op_fps(xyz, m):
    B, N, _ = xyz.shape
    temp = torch.empty((B, N), dtype=F32, device=xyz.device)
    idx = torch.empty((B, m), dtype=I32, device=xyz.device)

    def run():
        temp.fill_(1e10)
        ops.furthest_point_sampling_wrapper(B, N, m, xyz, temp, idx)
        return idx
    return run


def op_ball(radius, ns, xyz, new):
    B, N, _ = xyz.shape
    M = new.shape[1]
    idx = torch.empty((B, M, ns), dtype=I32, device=xyz.device)

    def run():
        idx.zero_()
        ops.ball_query_wrapper(B, N, M, radius, ns, new, xyz, idx)
        return idx
    return run


def op_nn(unk, kn):
    B, n, _ = unk.shape
    d2 = torch.empty((B, n, 3), dtype=F32, device=unk.device)
    idx = torch.empty((B, n, 3), dtype=I32, device=unk.device)

    def run():
        ops.three_nn_wrapper(B, n, kn.shape[1], unk, kn, d2, idx)
        return d2, idx
    return run


def op_group(pts, idx):
    B, C, N = pts.shape
    _, P, S = idx.shape
    out = torch.empty((B, C, P, S), dtype=F32, device=pts.device)

    def run():
        ops.group_points_wrapper(B, C, N, P, S, pts, idx, out)
        return out
    return run


def op_group_grad(go, idx, N):
    B, C, P, S = go.shape
    grad = torch.empty((B, C, N), dtype=F32, device=go.device)

    def run():
        grad.zero_()
        ops.group_points_grad_wrapper(B, C, N, P, S, go, idx, grad)
        return grad
    return run


def op_gather(pts, idx):
    B, C, N = pts.shape
    out = torch.empty((B, C, idx.shape[1]), dtype=F32, device=pts.device)

    def run():
        ops.gather_points_wrapper(B, C, N, idx.shape[1], pts, idx, out)
        return out
    return run


def op_gather_grad(go, idx, N):
    B, C, m = go.shape
    grad = torch.empty((B, C, N), dtype=F32, device=go.device)

    def run():
        grad.zero_()
        ops.gather_points_grad_wrapper(B, C, N, m, go, idx, grad)
        return grad
    return run


def op_interp(pts, idx, w):
    B, C, m = pts.shape
    n = idx.shape[1]
    out = torch.empty((B, C, n), dtype=F32, device=pts.device)

    def run():
        ops.three_interpolate_wrapper(B, C, m, n, pts, idx, w, out)
        return out
    return run


def op_interp_grad(go, idx, w, m):
    B, C, n = go.shape
    grad = torch.empty((B, C, m), dtype=F32, device=go.device)

    def run():
        grad.zero_()
        ops.three_interpolate_grad_wrapper(B, C, n, m, go, idx, w, grad)
        return grad
    return run


# ---- the yardstick: stock operators only ----------------------------------------------------------------------------
def yard_fps(xyz, m):
    B, N, _ = xyz.shape
    rows = torch.arange(B, device=xyz.device)

    def run():
        temp = torch.full((B, N), 1e10, dtype=F32, device=xyz.device)
        idx = torch.zeros((B, m), dtype=torch.int64, device=xyz.device)
        old = torch.zeros((B,), dtype=torch.int64, device=xyz.device)
        for j in range(1, m):
            d = ((xyz - xyz[rows, old].unsqueeze(1)) ** 2).sum(dim=2)
            temp = torch.minimum(temp, d)
            old = torch.argmax(temp, dim=1)
            idx[:, j] = old
        return idx
    return run


def yard_ball(radius, ns, xyz, new):
    N = xyz.shape[1]
    ar = torch.arange(N, device=xyz.device)

    def run():
        hit = torch.cdist(new, xyz) < radius
        first = torch.where(hit, ar, N).topk(ns, dim=2, largest=False, sorted=True).values
        pad = first[:, :, :1].expand(-1, -1, ns)
        first = torch.where(first == N, pad, first)
        return torch.where(first == N, 0, first)
    return run


def yard_nn(unk, kn):
    def run():
        d, i = torch.cdist(unk, kn).topk(3, dim=2, largest=False, sorted=True)
        return d * d, i
    return run


def yard_group(pts, idx):
    B, C, N = pts.shape
    li = idx.long().reshape(B, 1, -1).expand(-1, C, -1)

    def run():
        return torch.gather(pts, 2, li).reshape(B, C, *idx.shape[1:])
    return run


def yard_scatter(go, idx, N):
    """the gradient of the gather above, as autograd computes it (go (B, C, ...), idx (B, ...))"""
    B, C = go.shape[:2]
    li = idx.long().reshape(B, 1, -1).expand(-1, C, -1)
    src = torch.zeros((B, C, N), dtype=F32, device=go.device, requires_grad=True)

    def run():
        out = torch.gather(src, 2, li)
        (g,) = torch.autograd.grad(out, src, go.reshape(B, C, -1))
        return g
    return run


def yard_interp(pts, idx, w):
    B, C, m = pts.shape
    n = idx.shape[1]
    li = idx.long().reshape(B, 1, n * 3).expand(-1, C, -1)

    def run():
        return (torch.gather(pts, 2, li).reshape(B, C, n, 3) * w.unsqueeze(1)).sum(dim=3)
    return run


def yard_interp_grad(go, idx, w, m):
    B, C, n = go.shape
    li = idx.long().reshape(B, 1, n * 3).expand(-1, C, -1)
    src = torch.zeros((B, C, m), dtype=F32, device=go.device, requires_grad=True)

    def run():
        out = (torch.gather(src, 2, li).reshape(B, C, n, 3) * w.unsqueeze(1)).sum(dim=3)
        (g,) = torch.autograd.grad(out, src, go)
        return g
    return run


# ---- comparisons (before any time is reported) -------------------------------------------------------------------------
def cmp_fps(xyz):
    def cmp(a, b):
        a, b = a.long(), b.long()
        pa = torch.gather(xyz, 1, a.unsqueeze(-1).expand(-1, -1, 3))
        pb = torch.gather(xyz, 1, b.unsqueeze(-1).expand(-1, -1, 3))
        # another index at the same coordinates is a tie between duplicates broken differently; other coordinates
        # mean a tie between distinct points or a distance rounded differently (the sequences part from there on)
        return {"index_entries_differ": int((a != b).sum()), "selected_coordinates_differ": int((pa != pb).any(dim=2).sum()),
                "entries": a.numel()}
    return cmp


def cmp_index(a, b):
    a, b = (a[1], b[1]) if isinstance(a, tuple) else (a, b)
    return {"index_entries_differ": int((a.long() != b.long()).sum()), "entries": a.numel()}


def cmp_exact(a, b):
    return {"elements_differ": int((a != b).sum()), "entries": a.numel()}


def cmp_close(a, b):
    # sums of the same float32 terms in another order (and, in the yardstick's interpolation, another association)
    tol = 1e-4 * (1.0 + torch.maximum(a.abs(), b.abs()))
    return {"elements_beyond_1e-4": int(((a - b).abs() > tol).sum()), "max_abs_difference": float((a - b).abs().max()),
            "entries": a.numel()}


# ---- timing ---------------------------------------------------------------------------------------------------------------
def window(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / launches


def launches_for(fn):
    fn()
    torch.cuda.synchronize()               # warm-up: code objects loaded, allocator settled
    t = window(fn, 1)
    return int(min(2000, max(1, np.ceil(WINDOW_MS / max(t, 1e-3)))))


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "windows_ms": [float(x) for x in ms]}


def measure(name, shape, op, yard, cmp, windows, extra=None):
    with torch.no_grad():
        got = op()
    ref = yard()
    torch.cuda.synchronize()
    row = {"case": name, "shape": shape, "yardstick_vs_op": cmp(got, ref)}
    lo, ly = launches_for(op), launches_for(yard)
    to, ty = [], []
    for _ in range(windows):               # alternating windows
        to.append(window(op, lo))
        ty.append(window(yard, ly))
    row["op"] = dict(stats(to), launches_per_window=lo)
    row["yardstick"] = dict(stats(ty), launches_per_window=ly)
    row["yardstick_over_op"] = row["yardstick"]["median_ms"] / row["op"]["median_ms"]
    if extra:
        row.update(extra(row))
    print(json.dumps({k: row[k] for k in ("case", "shape", "yardstick_over_op")} | {"op_ms": row["op"]["median_ms"],
                                                                                   "yardstick_ms": row["yardstick"]["median_ms"]}), flush=True)
    return row


def build_inputs(dev):
    rs = np.random.RandomState(7)
    clouds = []
    for s in (11, 12):
        xyz = synth.make_scan(s, n_live=9000 if s == 11 else 30000, n_trav=1, n_frames=1, n_per_frame=2000).live_xyz
        clouds.append(xyz[rs.choice(len(xyz), 12288, replace=True)])      # with repetition: exact duplicates, as sample_points pads
    levels = [torch.from_numpy(np.ascontiguousarray(np.stack(clouds), dtype=np.float32)).to(dev)]
    for m in SA_NPOINTS:
        idx = op_fps(levels[-1], m)()
        levels.append(torch.gather(levels[-1], 1, idx.long().unsqueeze(-1).expand(-1, -1, 3)).contiguous())
    cloud = np.stack(clouds).astype(np.float32)
    rois = []
    for r in range(256):                                                   # the RoI head: 256 clouds of 512 pooled points
        c = cloud[r % 2][rs.randint(12288)]
        near = cloud[r % 2][np.abs(cloud[r % 2] - c).max(axis=1) < 2.5]
        rois.append(near[rs.choice(len(near), 512, replace=True)] - c)
    return levels, torch.from_numpy(np.stack(rois).astype(np.float32)).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointnet2_bench.json"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--once", action="store_true", help="launch every op a few times and exit (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/pointnet2_bench.py needs an MI355X: there is no CPU path")
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(3)

    def rand(*shape):
        return torch.randn(*shape, generator=g).to(dev)

    levels, rois = build_inputs(dev)
    cases = []
    fps_extra = lambda m: (lambda row: {"op_us_per_round": row["op"]["median_ms"] * 1e3 / (m - 1),           # noqa: E731
                                        "yardstick_us_per_round": row["yardstick"]["median_ms"] * 1e3 / (m - 1)})
    for lv, m in enumerate(SA_NPOINTS):
        x = levels[lv]
        cases.append((f"fps {x.shape[1]}->{m}", list(x.shape), op_fps(x, m), yard_fps(x, m), cmp_fps(x), fps_extra(m)))
    roi128 = torch.gather(rois, 1, op_fps(rois, 128)().long().unsqueeze(-1).expand(-1, -1, 3)).contiguous()
    roi32 = torch.gather(roi128, 1, op_fps(roi128, 32)().long().unsqueeze(-1).expand(-1, -1, 3)).contiguous()
    cases.append(("fps 256 clouds 512->128", list(rois.shape), op_fps(rois, 128), yard_fps(rois, 128), cmp_fps(rois), fps_extra(128)))
    cases.append(("fps 256 clouds 128->32", list(roi128.shape), op_fps(roi128, 32), yard_fps(roi128, 32), cmp_fps(roi128), fps_extra(32)))
    for lv in range(4):
        x, new = levels[lv], levels[lv + 1]
        for radius, ns in zip(SA_RADIUS[lv], SA_NSAMPLE[lv]):
            cases.append((f"ball_query r={radius} ns={ns}", [2, x.shape[1], new.shape[1]], op_ball(radius, ns, x, new),
                          yard_ball(radius, ns, x, new), cmp_index, None))
    cases.append(("ball_query roi r=0.2 ns=16", [256, 512, 128], op_ball(0.2, 16, rois, roi128), yard_ball(0.2, 16, rois, roi128), cmp_index, None))
    cases.append(("ball_query roi r=0.4 ns=16", [256, 128, 32], op_ball(0.4, 16, roi128, roi32), yard_ball(0.4, 16, roi128, roi32), cmp_index, None))
    for lv in range(4):
        x, new = levels[lv], levels[lv + 1]
        N, P = x.shape[1], new.shape[1]
        bidx = op_ball(SA_RADIUS[lv][1], 32, x, new)().clone()
        C = GROUP_C[lv]
        pts, go = rand(2, C, N), rand(2, C, P, 32)
        cases.append((f"group C={C}", [2, C, N, P, 32], op_group(pts, bidx), yard_group(pts, bidx), cmp_exact, None))
        cases.append((f"group_grad C={C}", [2, C, N, P, 32], op_group_grad(go, bidx, N), yard_scatter(go, bidx, N), cmp_close, None))
    fidx = op_fps(levels[0], 4096)().clone()
    cols = levels[0].transpose(1, 2).contiguous()
    cases.append(("gather C=3", [2, 3, 12288, 4096], op_gather(cols, fidx), yard_group(cols, fidx), cmp_exact, None))
    go = rand(2, 3, 4096)
    cases.append(("gather_grad C=3", [2, 3, 12288, 4096], op_gather_grad(go, fidx, 12288), yard_scatter(go, fidx, 12288), cmp_close, None))
    for lv in range(4):
        unk, kn = levels[lv], levels[lv + 1]
        n, m = unk.shape[1], kn.shape[1]
        cases.append((f"three_nn {n}<-{m}", [2, n, m], op_nn(unk, kn), yard_nn(unk, kn), cmp_index, None))
        d2, nidx = (t.clone() for t in op_nn(unk, kn)())
        w = 1.0 / (d2.sqrt() + 1e-8)
        w = (w / w.sum(dim=2, keepdim=True)).contiguous()
        C = INTERP_C[lv]
        pts, go = rand(2, C, m), rand(2, C, n)
        cases.append((f"three_interpolate C={C}", [2, C, m, n], op_interp(pts, nidx, w), yard_interp(pts, nidx, w), cmp_close, None))
        cases.append((f"three_interpolate_grad C={C}", [2, C, n, m], op_interp_grad(go, nidx, w, m), yard_interp_grad(go, nidx, w, m), cmp_close, None))

    if args.once:
        for name, _, op, _, _, _ in cases:
            for _ in range(3):
                op()
        torch.cuda.synchronize()
        print("launched", len(cases), "cases three times each")
        return
    rows = [measure(name, shape, op, yard, cmp, args.windows, extra) for name, shape, op, yard, cmp, extra in cases]
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "window_ms_target": WINDOW_MS, "windows": args.windows,
           "note": "HIP-event windows, op and yardstick alternating; the yardstick is a composition of stock PyTorch operators "
                   "written in tools/pointnet2_bench.py; per-kernel times are in pointnet2_kernel_stats.csv (a separate run)",
           "cases": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
