#!/usr/bin/env python
"""Time the RoI point pooling and points_in_boxes_gpu at the shapes PointRCNN runs them at (pointrcnn_dynamic_obj.yaml,
B = 2, 12 288 points, 128 RoIs in training and 100 in test, 512 samples, 130 feature channels; 40 padded gt boxes and
their 0.2-enlarged twins) against a composition of stock PyTorch-ROCm operators, and write profiles/roipool_bench.json.

There is no earlier implementation on this hardware and the reference cannot run here, so the yardstick is written in
this file, independent of the code under test: a dense (B, M, N) membership mask from elementwise torch operators
(float32 products and sums as separate operators, the three comparisons in float64, cos / sin in float64 rounded once),
then for the pooling cumsum ranks, a scatter of the first S indices per box, the k % cnt fill and one gather of the
rows; for the assignment the argmax of the first hit.  Both run in this process on the same device; every shape is
warmed up first; a window holds enough launches to last WINDOW_MS and the two sides alternate window by window (other
people's work shares the host); median, minimum and maximum of the windows are all written.  Before any time is
reported the yardstick's outputs are compared with the op's on the timed inputs and every differing entry is listed.

    python tools/roipool_bench.py [--out profiles/roipool_bench.json] [--windows 5] [--once]
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
import roipool_seq as seq  # noqa: E402
from modest_amd.utils import roiaware_pool3d_cuda as aware  # noqa: E402
from modest_amd.utils.roipoint_pool3d import roipoint_pool3d_cuda as pool  # noqa: E402

WINDOW_MS = 20.0
I32, F32, F64 = torch.int32, torch.float32, torch.float64
MARGIN = float(np.float32(1e-5))


# ---- the ops under test, on preallocated buffers (the zero fills the reference's Python side does are timed too) ----
def op_pool(xyz, boxes, feat, s):
    B, M = boxes.shape[:2]
    pooled = torch.empty((B, M, s, 3 + feat.shape[2]), dtype=F32, device=xyz.device)
    flag = torch.empty((B, M), dtype=I32, device=xyz.device)

    def run():
        pooled.zero_()
        flag.zero_()
        pool.forward(xyz, boxes, feat, pooled, flag)
        return pooled, flag
    return run


def op_assign(boxes, pts):
    B, N = pts.shape[:2]
    out = torch.empty((B, N), dtype=I32, device=pts.device)

    def run():
        out.fill_(-1)
        aware.points_in_boxes_gpu(boxes, pts, out)
        return out
    return run


# ---- the yardstick: stock PyTorch operators ---------------------------------------------------------------------------
def yard_mask(boxes, pts):
    """(B, M, N) bool"""
    bx = boxes[:, :, None, :]
    x, y, z = pts[:, None, :, 0], pts[:, None, :, 1], pts[:, None, :, 2]
    ang = -boxes[:, :, 6].to(F64)
    cosa, sina = torch.cos(ang).to(F32)[:, :, None], torch.sin(ang).to(F32)[:, :, None]
    zout = (z - bx[..., 2]).abs().to(F64) > bx[..., 5].to(F64) / 2.0
    sx, sy = x - bx[..., 0], y - bx[..., 1]
    lx = sx * cosa + sy * (-sina)
    ly = sx * sina + sy * cosa
    inx = lx.abs().to(F64) < bx[..., 3].to(F64) / 2.0 + MARGIN
    iny = ly.abs().to(F64) < bx[..., 4].to(F64) / 2.0 + MARGIN
    return ~zout & inx & iny


def yard_pool(xyz, boxes, feat, s):
    B, N, _ = xyz.shape
    M = boxes.shape[1]
    rows = torch.cat([xyz, feat], dim=2)
    W = rows.shape[2]
    karange = torch.arange(N, device=xyz.device).expand(B, M, N)
    sarange = torch.arange(s, device=xyz.device)

    def run():
        mask = yard_mask(boxes, xyz)
        rank = mask.cumsum(dim=2) - 1
        cnt = mask.sum(dim=2)
        slot = torch.where(mask & (rank < s), rank, s)              # everything else lands in a spare slot
        table = torch.zeros((B, M, s + 1), dtype=torch.int64, device=xyz.device)
        table.scatter_(2, slot, karange)
        taken = cnt.clamp(max=s)
        src = sarange[None, None, :] % taken.clamp(min=1)[:, :, None]
        idx = table[:, :, :s].gather(2, src)                          # (B, M, s)
        out = rows.gather(1, idx.reshape(B, M * s, 1).expand(-1, -1, W)).reshape(B, M, s, W)
        out = torch.where((cnt > 0)[:, :, None, None], out, torch.zeros((), dtype=F32, device=xyz.device))
        return out, (cnt == 0).to(I32)
    return run


def yard_assign(boxes, pts):
    M = boxes.shape[1]
    weight = torch.arange(M, 0, -1, device=pts.device, dtype=I32)[None, :, None]   # the first hit is the largest

    def run():
        mask = yard_mask(boxes, pts)
        first = (mask.to(I32) * weight).argmax(dim=1)
        return torch.where(mask.any(dim=1), first, -1).to(I32)
    return run


def cmp_pool(a, b):
    (pa, fa), (pb, fb) = a, b
    bad = ((pa.view(I32) != pb.view(I32)).any(dim=3).any(dim=2) | (fa != fb)).nonzero()
    return {"boxes_differ": int(len(bad)), "boxes": int(fa.numel()), "differing (cloud, box)": bad[:32].tolist()}


def cmp_assign(a, b):
    bad = (a != b).nonzero()
    return {"points_differ": int(len(bad)), "points": int(a.numel()), "differing (cloud, point)": bad[:32].tolist()}


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


def measure(name, shape, op, yard, cmp, windows):
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
    print(json.dumps({"case": name, "shape": shape, "yardstick_vs_op": {k: v for k, v in row["yardstick_vs_op"].items() if "differing" not in k},
                      "op_ms": row["op"]["median_ms"], "yardstick_ms": row["yardstick"]["median_ms"],
                      "yardstick_over_op": row["yardstick_over_op"]}), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roipool_bench.json"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--once", action="store_true", help="launch every op a few times and exit (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/roipool_bench.py needs an MI355X: there is no CPU path")
    dev = torch.device("cuda:0")
    xyz_h, feat_h, objs = seq.synthetic_scans()
    xyz, feat = torch.from_numpy(xyz_h).to(dev), torch.from_numpy(feat_h).to(dev)
    cases = []
    for m, what in ((128, "training"), (100, "test")):
        boxes_h = seq.enlarge(seq.synthetic_rois(np.random.RandomState(m), objs, m), (1.0, 1.0, 1.0))
        cnt = seq.inside_counts(xyz_h, boxes_h)
        boxes = torch.from_numpy(boxes_h).to(dev)
        shape = {"B": 2, "N": 12288, "M": m, "S": 512, "C": 130, "empty boxes": int((cnt == 0).sum()),
                 "boxes with fewer than S points": int(((cnt > 0) & (cnt < 512)).sum()), "boxes with S or more": int((cnt >= 512).sum())}
        cases.append((f"roipoint_pool3d {what} M={m}", shape, op_pool(xyz, boxes, feat, 512), yard_pool(xyz, boxes, feat, 512), cmp_pool))
    gt_h = seq.gt_boxes(np.random.RandomState(40), objs, 40, (23, 31))
    for name, b_h in (("gt boxes", gt_h), ("gt boxes + 0.2", seq.enlarge(gt_h.reshape(-1, 7), (0.2, 0.2, 0.2)).reshape(2, 40, 7))):
        bx = torch.from_numpy(b_h).to(dev)
        inside = int((seq.points_in_boxes(b_h, xyz_h) >= 0).sum())
        cases.append((f"points_in_boxes_gpu {name}", {"B": 2, "N": 12288, "M": 40, "points in a box": inside},
                      op_assign(bx, xyz), yard_assign(bx, xyz), cmp_assign))
    if args.once:
        for _, _, op, _, _ in cases:
            for _ in range(3):
                op()
        torch.cuda.synchronize()
        print("launched", len(cases), "cases three times each")
        return
    rows = [measure(name, shape, op, yard, cmp, args.windows) for name, shape, op, yard, cmp in cases]
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "window_ms_target": WINDOW_MS, "windows": args.windows,
           "note": "HIP-event windows, op and yardstick alternating; the op's time includes the zero fill of its outputs; the "
                   "yardstick is a composition of stock PyTorch operators written in tools/roipool_bench.py",
           "cases": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
