#!/usr/bin/env python
"""Time the stacked-batch PointNet++ ops at the shapes PV-RCNN and Voxel R-CNN run them at (B = 2) against a composition
of stock PyTorch-ROCm operators, and write profiles/pointnet2_stack_bench.json.

There is no earlier implementation on this hardware and the reference cannot run here, so the yardstick is written in
this file, independent of the code under test: the ball and voxel queries from torch.cdist + masking + topk per scan,
three-NN from cdist + topk, grouping and interpolation by indexing, their gradients by autograd.  The yardstick knows the
per-scan counts on the host (it slices per scan); the ops read them on the device.  The method is tools/pointnet2_bench.py's
(its helpers are imported): both sides run in this process on the same device, every shape is warmed up first, a window
holds enough launches to last 20 ms, the two sides alternate window by window, median, minimum and maximum of the windows
are written.  Before any time is reported the yardstick's outputs are compared with the op's on the timed inputs and the
differing entries counted: cdist rounds differently from the contract's expression, so entries may differ for pairs within
rounding of the radius or of each other.

Per-kernel times are NOT taken here: run `rocprofv3 --kernel-trace --stats -- python tools/pointnet2_stack_bench.py --once`
separately (profiles/pointnet2_stack_kernel_stats.csv).

    python tools/pointnet2_stack_bench.py [--out profiles/pointnet2_stack_bench.json] [--windows 5] [--once]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from modest_amd import synth  # noqa: E402
from modest_amd.utils.pointnet2.pointnet2_stack import pointnet2_stack_cuda as ops  # noqa: E402
from pointnet2_bench import WINDOW_MS, cmp_close, cmp_exact, cmp_index, measure  # noqa: E402

I32, F32 = torch.int32, torch.float32


def counts(c, dev):
    return torch.tensor(list(c), dtype=I32, device=dev)


def starts(c):
    return [int(v) for v in np.cumsum(c) - np.asarray(c)]


# ---- the ops under test, on preallocated buffers (the zero fills the reference's Python side does are timed too) ----
def op_ball(radius, ns, xyz, xcnt, new, qcnt):
    B, M = len(xcnt), new.shape[0]
    xc, qc = counts(xcnt, xyz.device), counts(qcnt, xyz.device)
    idx = torch.empty((M, ns), dtype=I32, device=xyz.device)

    def run():
        idx.zero_()
        ops.ball_query_wrapper(B, M, radius, ns, new, qc, xyz, xc, idx)
        return idx
    return run


def op_voxel(ranges, radius, ns, xyz, new, coords, table):
    M = new.shape[0]
    _, R1, R2, R3 = table.shape
    idx = torch.empty((M, ns), dtype=I32, device=xyz.device)

    def run():
        idx.zero_()
        ops.voxel_query_wrapper(M, R1, R2, R3, ns, radius, *ranges, new, xyz, coords, table, idx)
        return idx
    return run


def op_nn(unk, ucnt, kn, kcnt):
    uc, kc = counts(ucnt, unk.device), counts(kcnt, unk.device)
    d2 = torch.empty((unk.shape[0], 3), dtype=F32, device=unk.device)
    idx = torch.empty((unk.shape[0], 3), dtype=I32, device=unk.device)

    def run():
        ops.three_nn_wrapper(unk, uc, kn, kc, d2, idx)
        return d2, idx
    return run


def op_group(feat, fcnt, idx, icnt):
    (M, S), C = idx.shape, feat.shape[1]
    fc, ic = counts(fcnt, feat.device), counts(icnt, feat.device)
    out = torch.empty((M, C, S), dtype=F32, device=feat.device)

    def run():
        ops.group_points_wrapper(len(fcnt), M, C, S, feat, fc, idx, ic, out)
        return out
    return run


def op_group_grad(go, idx, icnt, fcnt, N):
    M, C, S = go.shape
    fc, ic = counts(fcnt, go.device), counts(icnt, go.device)
    grad = torch.empty((N, C), dtype=F32, device=go.device)

    def run():
        grad.zero_()
        ops.group_points_grad_wrapper(len(fcnt), M, C, N, S, go, idx, ic, fc, grad)
        return grad
    return run


def op_interp(feat, idx, w):
    out = torch.empty((idx.shape[0], feat.shape[1]), dtype=F32, device=feat.device)

    def run():
        ops.three_interpolate_wrapper(feat, idx, w, out)
        return out
    return run


def op_interp_grad(go, idx, w, M):
    grad = torch.empty((M, go.shape[1]), dtype=F32, device=go.device)

    def run():
        grad.zero_()
        ops.three_interpolate_grad_wrapper(go, idx, w, grad)
        return grad
    return run


# ---- the yardstick: stock operators only ----------------------------------------------------------------------------
def _first(hit, ns, fill):
    """hit (Q, K) bool -> (Q, ns) the first ns true columns in index order, padded with the first, no hit: -1 then `fill`"""
    K = hit.shape[1]
    ar = torch.arange(K, device=hit.device)
    k = min(ns, K)
    first = torch.where(hit, ar, K).topk(k, dim=1, largest=False, sorted=True).values
    if k < ns:
        first = torch.cat([first, first.new_full((hit.shape[0], ns - k), K)], dim=1)
    first = torch.where(first == K, first[:, :1].expand(-1, ns), first)
    empty = first[:, 0] == K
    first = torch.where(empty[:, None], fill, first)
    first[empty, 0] = -1
    return first


def yard_ball(radius, ns, xyz, xcnt, new, qcnt):
    xs, qs = starts(xcnt), starts(qcnt)

    def run():
        out = []
        for b in range(len(xcnt)):
            hit = torch.cdist(new[qs[b]:qs[b] + qcnt[b]], xyz[xs[b]:xs[b] + xcnt[b]]) < radius
            out.append(_first(hit, ns, 0))
        return torch.cat(out)
    return run


def yard_voxel(ranges, radius, ns, xyz, xcnt, new, coords, qcnt, cell_of_row):
    """the rows of xyz ascend in (b, z, y, x), so the visiting order dz, dy, dx is the order of the row index"""
    xs, qs = starts(xcnt), starts(qcnt)
    r = torch.tensor(ranges, device=xyz.device)

    def run():
        out = []
        for b in range(len(xcnt)):
            q, p = slice(qs[b], qs[b] + qcnt[b]), slice(xs[b], xs[b] + xcnt[b])
            near = ((cell_of_row[p][None, :, :] - coords[q, 1:][:, None, :]).abs() <= r).all(dim=2)
            hit = near & (torch.cdist(new[q], xyz[p]) <= radius)
            first = _first(hit, ns, 0)
            out.append(torch.where(first >= 0, first + xs[b], first) if xs[b] else first)
        out = torch.cat(out)
        out[out[:, 0] < 0, 1:] = 0
        return out
    return run


def yard_nn(unk, ucnt, kn, kcnt):
    us, ks = starts(ucnt), starts(kcnt)

    def run():
        d, i = [], []
        for b in range(len(ucnt)):
            dd, ii = torch.cdist(unk[us[b]:us[b] + ucnt[b]], kn[ks[b]:ks[b] + kcnt[b]]).topk(3, dim=1, largest=False, sorted=True)
            d.append(dd * dd)
            i.append(ii + ks[b])
        return torch.cat(d), torch.cat(i)
    return run


def global_rows(idx, icnt, fcnt):
    off = torch.repeat_interleave(torch.tensor(starts(fcnt), device=idx.device), torch.tensor(list(icnt), device=idx.device))
    return idx.long() + off[:, None]


def yard_group(feat, rows):
    def run():
        return feat[rows].permute(0, 2, 1).contiguous()
    return run


def yard_group_grad(go, rows, N):
    src = torch.zeros((N, go.shape[1]), dtype=F32, device=go.device, requires_grad=True)

    def run():
        (g,) = torch.autograd.grad(src[rows].permute(0, 2, 1), src, go)
        return g
    return run


def yard_interp(feat, idx, w):
    li = idx.long()

    def run():
        return (feat[li] * w.unsqueeze(-1)).sum(dim=1)
    return run


def yard_interp_grad(go, idx, w, M):
    li = idx.long()
    src = torch.zeros((M, go.shape[1]), dtype=F32, device=go.device, requires_grad=True)

    def run():
        (g,) = torch.autograd.grad((src[li] * w.unsqueeze(-1)).sum(dim=1), src, go)
        return g
    return run


# ---- inputs -----------------------------------------------------------------------------------------------------------
def build_inputs(dev):
    """B = 2: 16 384 raw points per scan (sampled with repetition from synthetic Lyft-shape scans), 2 048 keypoints of each
    by furthest point sampling, 20 000 / 18 517 voxel centres, 16 RoIs x 216 grid points per scan; a (2, 11, 50, 44) voxel
    table of the raw clouds with the rows of its points ascending in (b, z, y, x)"""
    rs = np.random.RandomState(7)
    raw, centres = [], []
    for s, n_centres in ((11, 20000), (12, 18517)):
        xyz = synth.make_scan(s, n_live=9000 if s == 11 else 60000, n_trav=1, n_frames=1, n_per_frame=2000).live_xyz
        raw.append(xyz[rs.choice(len(xyz), 16384, replace=True)])
        dense = synth.make_scan(s, n_live=120000, n_trav=1, n_frames=1, n_per_frame=2000).live_xyz
        vs = np.array([0.2, 0.2, 0.4], dtype=np.float32)
        cells = np.unique(np.floor(dense / vs).astype(np.int64), axis=0)
        cells = cells[np.sort(rs.choice(len(cells), n_centres, replace=False))]
        centres.append(((cells.astype(np.float32) + np.float32(0.5)) * vs).astype(np.float32))
    raw = np.ascontiguousarray(np.stack(raw), dtype=np.float32)
    t = torch.from_numpy(raw).to(dev)
    temp = torch.full((2, 16384), 1e10, dtype=F32, device=dev)
    fidx = torch.empty((2, 2048), dtype=I32, device=dev)
    ops.furthest_point_sampling_wrapper(2, 16384, 2048, t, temp, fidx)
    keys = torch.gather(t, 1, fidx.long().unsqueeze(-1).expand(-1, -1, 3)).reshape(-1, 3).contiguous()
    keys_np = keys.cpu().numpy().reshape(2, 2048, 3)
    c6 = (np.arange(6, dtype=np.float32) + np.float32(0.5)) / np.float32(6) - np.float32(0.5)
    cube = np.stack(np.meshgrid(c6, c6, c6, indexing="ij"), axis=-1).reshape(-1, 3)
    grid = []
    for b in range(2):
        for r in range(16):
            c, size = keys_np[b, rs.randint(2048)], rs.uniform((3.5, 1.5, 1.4), (5.0, 2.2, 2.0)).astype(np.float32)
            a = np.float32(rs.uniform(-np.pi, np.pi))
            rot = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], dtype=np.float32)
            grid.append(((cube * size) @ rot.T + c).astype(np.float32))
    # Voxel R-CNN: the table, its points, the RoI grid points as queries with the cell each lies in
    B, R1, R2, R3 = 2, 11, 50, 44
    lo, vs = np.array([-17.6, -20, -2], dtype=np.float32), np.array([0.8, 0.8, 0.4], dtype=np.float32)
    table = np.full((B, R1, R2, R3), -1, dtype=np.int32)
    vxyz, vcell = [], []
    for b in range(B):
        c = np.floor((raw[b] - lo) / vs).astype(np.int64)
        ok = ((c >= 0) & (c < np.array([R3, R2, R1]))).all(axis=1)
        _, first = np.unique(c[ok] @ np.array([1, R3, R3 * R2]), return_index=True)   # ascending (z, y, x)
        cells = c[ok][first]
        table[b, cells[:, 2], cells[:, 1], cells[:, 0]] = sum(len(x) for x in vxyz) + np.arange(len(cells), dtype=np.int32)
        vxyz.append(raw[b][ok][first])
        vcell.append(cells[:, ::-1])
    vq = np.concatenate(grid).astype(np.float32)
    vcoords = np.floor((vq - lo) / vs).astype(np.int64)[:, ::-1]
    vcoords = np.concatenate([np.repeat(np.arange(2), 16 * 216)[:, None], vcoords], axis=1).astype(np.int32)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    return dict(raw=t.reshape(-1, 3).contiguous(), raw_cnt=(16384, 16384), keys=keys, key_cnt=(2048, 2048),
                centres=to(np.concatenate(centres)), centre_cnt=tuple(len(c) for c in centres),
                grid=to(vq), grid_cnt=(16 * 216, 16 * 216),
                vxyz=to(np.concatenate(vxyz).astype(np.float32)), vcnt=tuple(len(v) for v in vxyz), vcell=to(np.concatenate(vcell).astype(np.int64)),
                vcoords=to(vcoords), table=to(table))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointnet2_stack_bench.json"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--once", action="store_true", help="launch every op a few times and exit (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/pointnet2_stack_bench.py needs an MI355X: there is no CPU path")
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(3)

    def rand(*shape):
        return torch.randn(*shape, generator=g).to(dev)

    s = build_inputs(dev)
    cases = []
    for name, xyz, xcnt, new, qcnt, radii, ns in (("keypoints<-raw", s["raw"], s["raw_cnt"], s["keys"], s["key_cnt"], (0.4, 0.8), 16),
                                                   ("keypoints<-voxel centres", s["centres"], s["centre_cnt"], s["keys"], s["key_cnt"], (1.2, 2.4), 32),
                                                   ("roi grid<-keypoints", s["keys"], s["key_cnt"], s["grid"], s["grid_cnt"], (0.8, 1.6), 16)):
        for radius in radii:
            cases.append((f"ball_query {name} r={radius} ns={ns}", [list(qcnt), list(xcnt)], op_ball(radius, ns, xyz, xcnt, new, qcnt),
                          yard_ball(radius, ns, xyz, xcnt, new, qcnt), cmp_index, None))
    ranges = (1, 4, 4)
    cases.append(("voxel_query roi grid ranges=(1,4,4) r=0.8 ns=16", [list(s["grid_cnt"]), list(s["table"].shape)],
                  op_voxel(ranges, 0.8, 16, s["vxyz"], s["grid"], s["vcoords"], s["table"]),
                  yard_voxel(ranges, 0.8, 16, s["vxyz"], s["vcnt"], s["grid"], s["vcoords"], s["grid_cnt"], s["vcell"]), cmp_index, None))
    # grouping: the raw points' rows (C = 4) and the voxel features (C = 32, 64) at the queries above, and Voxel R-CNN's
    for name, fcnt, icnt, C, mk in (("raw r=0.8", s["raw_cnt"], s["key_cnt"], 4, lambda: op_ball(0.8, 16, s["raw"], s["raw_cnt"], s["keys"], s["key_cnt"])()),
                                    ("voxel centres r=1.2", s["centre_cnt"], s["key_cnt"], 32, lambda: op_ball(1.2, 32, s["centres"], s["centre_cnt"], s["keys"], s["key_cnt"])()),
                                    ("voxel centres r=2.4", s["centre_cnt"], s["key_cnt"], 64, lambda: op_ball(2.4, 32, s["centres"], s["centre_cnt"], s["keys"], s["key_cnt"])()),
                                    ("roi grid<-keypoints r=1.6", s["key_cnt"], s["grid_cnt"], 128, lambda: op_ball(1.6, 16, s["keys"], s["key_cnt"], s["grid"], s["grid_cnt"])())):
        idx = mk().clone()
        idx[idx[:, 0] < 0] = 0
        N = sum(fcnt)
        feat, go = rand(N, C), rand(idx.shape[0], C, idx.shape[1])
        rows = global_rows(idx, icnt, fcnt)
        cases.append((f"group {name} C={C}", [N, C, list(idx.shape)], op_group(feat, fcnt, idx, icnt), yard_group(feat, rows), cmp_exact, None))
        cases.append((f"group_grad {name} C={C}", [N, C, list(idx.shape)], op_group_grad(go, idx, icnt, fcnt, N), yard_group_grad(go, rows, N), cmp_close, None))
    cases.append(("three_nn raw<-keypoints", [list(s["raw_cnt"]), list(s["key_cnt"])], op_nn(s["raw"], s["raw_cnt"], s["keys"], s["key_cnt"]),
                  yard_nn(s["raw"], s["raw_cnt"], s["keys"], s["key_cnt"]), cmp_index, None))
    d2, nidx = (t.clone() for t in op_nn(s["raw"], s["raw_cnt"], s["keys"], s["key_cnt"])())
    w = 1.0 / (d2.sqrt() + 1e-8)
    w = (w / w.sum(dim=1, keepdim=True)).contiguous()
    C, M, N = 128, s["keys"].shape[0], s["raw"].shape[0]
    feat, go = rand(M, C), rand(N, C)
    cases.append((f"three_interpolate C={C}", [M, C, N], op_interp(feat, nidx, w), yard_interp(feat, nidx, w), cmp_close, None))
    cases.append((f"three_interpolate_grad C={C}", [N, C, M], op_interp_grad(go, nidx, w, M), yard_interp_grad(go, nidx, w, M), cmp_close, None))

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
                   "written in tools/pointnet2_stack_bench.py (it slices per scan with the counts on the host, the ops read them on "
                   "the device); per-kernel times are in pointnet2_stack_kernel_stats.csv (a separate run)",
           "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
