#!/usr/bin/env python
"""Time modest_amd.utils.target_assigner.AxisAlignedTargetAssigner.assign_targets against a PyTorch restatement of the
reference's path on the same device, and write profiles/anchor_targets_bench.json.

The yardstick is written in this file (the reference cannot run here: it needs its compiled extensions): per sample the
host loop that trims the padded gt rows reading the device once per row, per anchor class the class mask on the host, the
dense (anchors, gts) IoU matrix, its two copies to the host for numpy's argmax and the copies back, the `nonzero()` calls
and the residual encoding of the foreground rows, then the concatenation into the head's layout.  It computes the same
labels; before any time is reported its outputs are compared with ours on the timed inputs.

Shapes: the Lyft PointPillars head (B = 4, one class, 1 x 248 x 280 x 2 = 138 880 anchors, 5..25 gts) and KITTI's three-class
PointPillars head (B = 4, 1 x 248 x 216 x 2 anchors per class).  Method: both sides in this process on the same device, every
shape warmed up, a window holds enough calls to last 200 ms, the two sides alternate window by window; median, minimum and
maximum of the windows are written.  A window is timed with device events around the calls, ending in a synchronise, so the
host round trips of the yardstick are inside it.  Host synchronisations per call are counted by PyTorch itself
(`torch.cuda.set_sync_debug_mode("warn")`, one call of each side).

    python tools/anchor_targets_bench.py [--out profiles/anchor_targets_bench.json] [--windows 5] [--once]
"""
import argparse
import json
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import anchor_targets_seq as seq  # noqa: E402
from modest_amd.utils import target_assigner as ta  # noqa: E402

WINDOW_MS = 200.0


# ---- the yardstick: the reference's path in stock PyTorch operators ------------------------------------------------------
def yard_bev(boxes):
    r = boxes[:, 6]
    rot = (r - torch.floor(r / np.pi + 0.5) * np.pi).abs()
    dims = torch.where(rot[:, None] < np.pi / 4, boxes[:, [3, 4]], boxes[:, [4, 3]])
    return torch.cat((boxes[:, 0:2] - dims / 2, boxes[:, 0:2] + dims / 2), dim=1)


def yard_iou(a, b):
    x_min, x_max = torch.max(a[:, 0, None], b[None, :, 0]), torch.min(a[:, 2, None], b[None, :, 2])
    y_min, y_max = torch.max(a[:, 1, None], b[None, :, 1]), torch.min(a[:, 3, None], b[None, :, 3])
    inter = torch.clamp_min(x_max - x_min, min=0) * torch.clamp_min(y_max - y_min, min=0)
    area_a, area_b = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]), (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    return inter / torch.clamp_min(area_a[:, None] + area_b[None, :] - inter, min=1e-6)


def yard_encode(g, a, sincos):
    a, g = a.clone(), g.clone()
    a[:, 3:6] = torch.clamp_min(a[:, 3:6], min=1e-5)
    g[:, 3:6] = torch.clamp_min(g[:, 3:6], min=1e-5)
    diag = torch.sqrt(a[:, 3] ** 2 + a[:, 4] ** 2)
    cols = [(g[:, 0] - a[:, 0]) / diag, (g[:, 1] - a[:, 1]) / diag, (g[:, 2] - a[:, 2]) / a[:, 5],
            torch.log(g[:, 3] / a[:, 3]), torch.log(g[:, 4] / a[:, 4]), torch.log(g[:, 5] / a[:, 5])]
    cols += [torch.cos(g[:, 6]) - torch.cos(a[:, 6]), torch.sin(g[:, 6]) - torch.sin(a[:, 6])] if sincos else [g[:, 6] - a[:, 6]]
    cols += [g[:, e] - a[:, e] for e in range(7, min(g.shape[1], a.shape[1]))]
    return torch.stack(cols, dim=1)


def yard_single(anchors, gts, classes, matched, unmatched, sincos, code):
    n, dev = anchors.shape[0], anchors.device
    labels = torch.full((n,), -1, dtype=torch.int32, device=dev)
    if len(gts) > 0 and n > 0:
        iou = yard_iou(yard_bev(anchors), yard_bev(gts))
        arg = torch.from_numpy(iou.cpu().numpy().argmax(axis=1)).to(dev)           # host round trip 1
        row_max = iou[torch.arange(n, device=dev), arg]
        col_arg = torch.from_numpy(iou.cpu().numpy().argmax(axis=0)).to(dev)       # host round trip 2
        col_max = iou[col_arg, torch.arange(len(gts), device=dev)]
        col_max[col_max == 0] = -1
        forced = (iou == col_max).nonzero()[:, 0]
        forced_cls = classes[arg[forced]]
        labels[forced] = forced_cls
        pos = row_max >= matched
        labels[pos] = classes[arg[pos]]
        bg = (row_max < unmatched).nonzero()[:, 0]
        labels[bg] = 0
        labels[forced] = forced_cls
    else:
        labels[:] = 0
    fg = (labels > 0).nonzero()[:, 0]
    targets = anchors.new_zeros((n, code))
    if len(gts) > 0 and n > 0:
        targets[fg, :] = yard_encode(gts[arg[fg], :], anchors[fg, :], sincos)
    weights = anchors.new_zeros((n,))
    weights[labels > 0] = 1.0
    return labels, targets, weights


def yard_assign(cfg, all_anchors, gt):
    names = np.array(cfg["class_names"])
    sincos, multi = bool(cfg["sincos"]), bool(cfg["use_multihead"])
    code = 7 + int(sincos) + min(all_anchors[0].shape[-1] - 7, gt.shape[2] - 8)
    L, T, W = [], [], []
    for b in range(gt.shape[0]):
        boxes = gt[b, :, :-1]
        cnt = len(boxes) - 1
        while cnt > 0 and boxes[cnt].sum() == 0:       # reads the device once per trimmed row
            cnt -= 1
        boxes = boxes[:cnt + 1]
        classes = gt[b, :cnt + 1, -1].int()
        per = []
        for c, anchors in zip(cfg["classes"], all_anchors):
            mask = torch.from_numpy(np.atleast_1d(names[classes.cpu().numpy() - 1] == c["class_name"])).to(gt.device)
            flat = anchors.permute(3, 4, 0, 1, 2, 5).contiguous().view(-1, anchors.shape[-1]) if multi else anchors.view(-1, anchors.shape[-1])
            per.append(yard_single(flat, boxes[mask], classes[mask], c["matched_threshold"], c["unmatched_threshold"], sincos, code))
        if multi:
            lab, tar, wei = (torch.cat([p[i] for p in per], dim=0) for i in range(3))
        else:
            fm = all_anchors[0].shape[:3]
            lab = torch.cat([p[0].view(*fm, -1) for p in per], dim=-1).view(-1)
            tar = torch.cat([p[1].view(*fm, -1, code) for p in per], dim=-2).view(-1, code)
            wei = torch.cat([p[2].view(*fm, -1) for p in per], dim=-1).view(-1)
        L.append(lab), T.append(tar), W.append(wei)
    return {"box_cls_labels": torch.stack(L), "box_reg_targets": torch.stack(T), "reg_weights": torch.stack(W)}


# ---- shapes -----------------------------------------------------------------------------------------------------------------
def cls(name, size, z, m, u, grid):
    return dict(class_name=name, anchor_sizes=[size], anchor_rotations=[0, 1.57], anchor_bottom_heights=[z], align_center=False,
                matched_threshold=m, unmatched_threshold=u, grid_size=list(grid))


def shapes():
    lyft = dict(anchor_range=[-80, -80, -5, 80, 80, 3], use_multihead=False, code_size=7, sincos=False, class_names=["car"],
                classes=[cls("car", [4.75, 1.92, 1.71], -1.07, 0.5, 0.35, (280, 248))])
    kitti = dict(anchor_range=[0, -39.68, -3, 69.12, 39.68, 1], use_multihead=False, code_size=7, sincos=False,
                 class_names=["Car", "Pedestrian", "Cyclist"],
                 classes=[cls("Car", [3.9, 1.6, 1.56], -1.78, 0.6, 0.45, (216, 248)),
                          cls("Pedestrian", [0.8, 0.6, 1.73], -0.6, 0.5, 0.35, (216, 248)),
                          cls("Cyclist", [1.76, 0.6, 1.73], -0.6, 0.5, 0.35, (216, 248))])
    return [("lyft pointpillar B=4 138880x1", lyft, (5, 25, 13, 19)), ("kitti pointpillar B=4 107136x3", kitti, (6, 14, 9, 11))]


def random_gt(rs, cfg, anchors, counts, pad=5):
    gt = np.zeros((len(counts), max(counts) + pad, 8), dtype=np.float32)
    for b, n in enumerate(counts):
        for j in range(n):
            ci = rs.randint(len(anchors))
            flat = anchors[ci].reshape(-1, anchors[ci].shape[-1])
            a = flat[rs.randint(len(flat))]
            gt[b, j] = [a[0] + rs.normal(0, 0.3) * a[3], a[1] + rs.normal(0, 0.3) * a[4], a[2] + rs.normal(0, 0.2),
                        *(a[3:6] * rs.uniform(0.8, 1.25, 3)), a[6] + rs.normal(0, 0.25) + np.pi * rs.randint(-1, 2), ci + 1]
    return gt


# ---- timing -----------------------------------------------------------------------------------------------------------------
def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def calls_for(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()               # warm-up: code objects loaded, allocator settled
    t = window(fn, 3)
    return int(min(5000, max(3, np.ceil(WINDOW_MS / max(t, 1e-3)))))


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "windows_ms": [float(x) for x in ms]}


def host_syncs(fn):
    """synchronising calls PyTorch reports for one call of fn"""
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    return sum("called a synchronizing" in str(w.message) for w in seen)   # not the mode's own "prototype feature" notice


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anchor_targets_bench.json"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--once", action="store_true", help="call each side a few times and exit (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/anchor_targets_bench.py needs an MI355X: there is no CPU path")
    dev = torch.device("cuda:0")
    rows = []
    for name, cfg, counts in shapes():
        anchors_np = seq.make_anchors(cfg)
        gt_np = random_gt(np.random.RandomState(11), cfg, anchors_np, counts)
        anchors = [torch.from_numpy(a).to(dev) for a in anchors_np]
        gt = torch.from_numpy(gt_np).to(dev)
        assigner = ta.AxisAlignedTargetAssigner(seq.model_cfg(cfg), cfg["class_names"], seq.Coder(cfg))
        op = lambda: assigner.assign_targets(anchors, gt)      # noqa: E731
        yard = lambda: yard_assign(cfg, anchors, gt)           # noqa: E731
        got, ref = op(), yard()
        torch.cuda.synchronize()
        if args.once:
            continue
        tol = 1e-5 * (1.0 + ref["box_reg_targets"].abs())
        row = {"case": name, "gt_counts": list(counts), "anchors_per_sample": int(got["box_cls_labels"].shape[1]),
               "yardstick_vs_op": {"labels_differ": int((got["box_cls_labels"] != ref["box_cls_labels"]).sum()),
                                   "weights_differ": int((got["reg_weights"] != ref["reg_weights"]).sum()),
                                   "targets_beyond_1e-5": int(((got["box_reg_targets"] - ref["box_reg_targets"]).abs() > tol).sum()),
                                   "targets_bits_differ": int((got["box_reg_targets"].view(torch.int32) != ref["box_reg_targets"].view(torch.int32)).sum()),
                                   "foreground": int((ref["box_cls_labels"] > 0).sum())}}
        row["host_synchronisations_per_call"] = {"op": host_syncs(op), "yardstick": host_syncs(yard)}
        no, ny = calls_for(op), calls_for(yard)
        to, ty = [], []
        for _ in range(args.windows):       # alternating windows
            to.append(window(op, no))
            ty.append(window(yard, ny))
        row["op"] = dict(stats(to), calls_per_window=no)
        row["yardstick"] = dict(stats(ty), calls_per_window=ny)
        row["yardstick_over_op"] = row["yardstick"]["median_ms"] / row["op"]["median_ms"]
        print(json.dumps({k: row[k] for k in ("case", "yardstick_over_op", "host_synchronisations_per_call", "yardstick_vs_op")}
                         | {"op_ms": row["op"]["median_ms"], "yardstick_ms": row["yardstick"]["median_ms"]}), flush=True)
        rows.append(row)
    if args.once:
        return
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "window_ms_target": WINDOW_MS, "windows": args.windows,
           "method": "alternating windows of calls timed with device events ending in a synchronise; medians over the windows",
           "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
