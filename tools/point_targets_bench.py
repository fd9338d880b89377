#!/usr/bin/env python
"""Time modest_amd.utils.point_head_targets.assign_stack_targets against the path a point head took before it: the
reference's loop over the batch restated in stock PyTorch operators over this project's own ``points_in_boxes_gpu``
(``modest_amd.utils.roiaware_pool3d_utils``), on the same device; writes profiles/point_targets_bench.json (DESIGN.md
section 7l).

The yardstick is written in this file: per sample the boolean mask over all points and the indexing with it, two
``points_in_boxes_gpu`` calls (gt boxes, enlarged boxes), the masked assignments, ``PointResidualCoder.encode_torch`` with
its in-place clamp, the rotation as a batched matmul, and the scatters back through the mask.  On the CPU, with the numpy
membership in place of the device op, it reproduces tests/golden/point_targets.npz (tests/test_point_targets_cpu.py);
before any time is reported its outputs are compared with ours on the timed inputs.

Shape: PointRCNN's point head, B = 4, 16 384 points per sample, 40 gt rows (23-31 live), box labels (PointHeadBox); the same
with part labels as well (PartA2's PointIntraPartOffsetHead) and labels alone (PV-RCNN's PointHeadSimple).  Method: both
sides in this process on the same device, every shape warmed up.  Device time per call: a window holds enough calls to
last 200 ms and is timed with device events, ending in a synchronise; the two sides alternate window by window.  Wall time
per call: the host clock around one call and a synchronise, alternating, median of 50.  Host synchronisations per call are
counted by PyTorch itself (`torch.cuda.set_sync_debug_mode("warn")`).

    python tools/point_targets_bench.py [--out profiles/point_targets_bench.json] [--windows 5] [--once]
"""
import argparse
import json
import os
import sys
import time
import types
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WINDOW_MS = 200.0
KITTI = [[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]]


# ---- the yardstick: the reference's path in stock PyTorch operators ------------------------------------------------------
def yard_encode(gt_boxes, points, gt_classes, mean_size):
    gt_boxes[:, 3:6] = torch.clamp_min(gt_boxes[:, 3:6], min=1e-5)   # in place, on the caller's rows
    xg, yg, zg, dxg, dyg, dzg, rg = torch.split(gt_boxes, 1, dim=-1)
    xa, ya, za = torch.split(points, 1, dim=-1)
    if mean_size is not None:
        dxa, dya, dza = torch.split(mean_size[gt_classes - 1], 1, dim=-1)
        diagonal = torch.sqrt(dxa ** 2 + dya ** 2)
        xt, yt, zt = (xg - xa) / diagonal, (yg - ya) / diagonal, (zg - za) / dza
        dxt, dyt, dzt = torch.log(dxg / dxa), torch.log(dyg / dya), torch.log(dzg / dza)
    else:
        xt, yt, zt = xg - xa, yg - ya, zg - za
        dxt, dyt, dzt = torch.log(dxg), torch.log(dyg), torch.log(dzg)
    return torch.cat([xt, yt, zt, dxt, dyt, dzt, torch.cos(rg), torch.sin(rg)], dim=-1)


def yard_rotate(points, angle):
    cosa, sina = torch.cos(angle), torch.sin(angle)
    zeros, ones = angle.new_zeros(points.shape[0]), angle.new_ones(points.shape[0])
    rot = torch.stack((cosa, sina, zeros, -sina, cosa, zeros, zeros, zeros, ones), dim=1).view(-1, 3, 3).float()
    return torch.matmul(points[:, :, 0:3], rot)


def yard_assign(points, gt_boxes, extend_gt_boxes, num_class, mean_size, want_box, want_part, points_in_boxes_gpu):
    batch_size = gt_boxes.shape[0]
    bs_idx = points[:, 0]
    point_cls_labels = points.new_zeros(points.shape[0]).long()
    point_box_labels = gt_boxes.new_zeros((points.shape[0], 8)) if want_box else None
    point_part_labels = gt_boxes.new_zeros((points.shape[0], 3)) if want_part else None
    for k in range(batch_size):
        bs_mask = (bs_idx == k)
        points_single = points[bs_mask][:, 1:4]
        labels_single = point_cls_labels.new_zeros(bs_mask.sum())
        box_idxs = points_in_boxes_gpu(points_single.unsqueeze(dim=0), gt_boxes[k:k + 1, :, 0:7].contiguous()).long().squeeze(dim=0)
        fg_flag = (box_idxs >= 0)
        ext_idxs = points_in_boxes_gpu(points_single.unsqueeze(dim=0), extend_gt_boxes[k:k + 1, :, 0:7].contiguous()).long().squeeze(dim=0)
        labels_single[fg_flag ^ (ext_idxs >= 0)] = -1
        gt_of_fg = gt_boxes[k][box_idxs[fg_flag]]
        labels_single[fg_flag] = 1 if num_class == 1 else gt_of_fg[:, -1].long()
        point_cls_labels[bs_mask] = labels_single
        if want_box and gt_of_fg.shape[0] > 0:
            box_single = point_box_labels.new_zeros((bs_mask.sum(), 8))
            box_single[fg_flag] = yard_encode(gt_of_fg[:, :-1], points_single[fg_flag], gt_of_fg[:, -1].long(), mean_size)
            point_box_labels[bs_mask] = box_single
        if want_part:
            part_single = point_part_labels.new_zeros((bs_mask.sum(), 3))
            moved = points_single[fg_flag] - gt_of_fg[:, 0:3]
            moved = yard_rotate(moved.view(-1, 1, 3), -gt_of_fg[:, 6]).view(-1, 3)
            offset = torch.tensor([0.5, 0.5, 0.5]).view(1, 3).type_as(moved)
            part_single[fg_flag] = (moved / gt_of_fg[:, 3:6]) + offset
            point_part_labels[bs_mask] = part_single
    return {"point_cls_labels": point_cls_labels, "point_box_labels": point_box_labels, "point_part_labels": point_part_labels}


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def pointrcnn_inputs(B=4, n_per=16384, M=40, seed=5):
    """B samples of n_per points: 40 gt rows of which 23-31 are live (classes 1..3), three points in ten near a box"""
    import point_targets_seq as seq
    rs = np.random.RandomState(seed)
    gt = np.zeros((B, M, 8), dtype=np.float32)
    pts = np.zeros((B * n_per, 4), dtype=np.float32)
    for b in range(B):
        live = rs.randint(23, 32)
        gt[b, :live] = np.c_[rs.uniform(0, 70, live), rs.uniform(-40, 40, live), rs.uniform(-1.5, 0, live), rs.uniform(3.2, 4.6, live),
                             rs.uniform(1.4, 1.9, live), rs.uniform(1.4, 1.8, live), rs.uniform(-np.pi, np.pi, live),
                             rs.randint(1, 4, live)]
        p = np.c_[rs.uniform(0, 70.4, n_per), rs.uniform(-40, 40, n_per), rs.uniform(-3, 1, n_per)]
        near = rs.rand(n_per) < 0.3
        g = gt[b, rs.randint(0, live, n_per)]
        u = rs.uniform(-0.6, 0.6, (n_per, 3)) * g[:, 3:6]
        c, s = np.cos(g[:, 6]), np.sin(g[:, 6])
        q = np.c_[g[:, 0] + u[:, 0] * c - u[:, 1] * s, g[:, 1] + u[:, 0] * s + u[:, 1] * c, g[:, 2] + u[:, 2]]
        pts[b * n_per:(b + 1) * n_per, 0] = b
        pts[b * n_per:(b + 1) * n_per, 1:] = np.where(near[:, None], q, p)
    return pts, gt, seq.enlarge(gt)


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


def wall_once(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}


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
    return sum("called a synchronizing" in str(w.message) for w in seen)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_targets_bench.json"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--once", action="store_true", help="call each side a few times and exit (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/point_targets_bench.py needs an MI355X: there is no CPU path")
    from modest_amd.utils import point_head_targets as pht
    from modest_amd.utils.roiaware_pool3d_utils import points_in_boxes_gpu
    dev = torch.device("cuda:0")
    pts_np, gt_np, ext_np = pointrcnn_inputs()
    pts, gt, ext = (torch.from_numpy(a).to(dev) for a in (pts_np, gt_np, ext_np))
    mean = torch.tensor(KITTI, dtype=torch.float32, device=dev)
    head = pht.bind(type("Head", (), {}))()
    head.num_class, head.box_coder = 3, types.SimpleNamespace(use_mean_size=True, mean_size=mean, code_size=8)
    rows = []
    for name, want_box, want_part in (("PointHeadBox: box labels", True, False),
                                      ("PointIntraPartOffsetHead: box and part labels", True, True),
                                      ("PointHeadSimple: labels alone", False, False)):
        op = lambda: head.assign_stack_targets(pts, gt, extend_gt_boxes=ext, ret_box_labels=want_box,      # noqa: E731
                                               ret_part_labels=want_part)
        yard = lambda: yard_assign(pts, gt, ext, 3, mean, want_box, want_part, points_in_boxes_gpu)       # noqa: E731
        got, ref = op(), yard()
        torch.cuda.synchronize()
        if args.once:
            continue
        cmp = {"labels_differ": int((got["point_cls_labels"] != ref["point_cls_labels"]).sum()),
               "foreground": int((ref["point_cls_labels"] > 0).sum()), "ignored": int((ref["point_cls_labels"] < 0).sum())}
        for key in ("point_box_labels", "point_part_labels"):
            if ref[key] is not None:
                cmp[key + "_beyond_1e-5"] = int(((got[key] - ref[key]).abs() > 1e-5 * (1.0 + ref[key].abs())).sum())
                cmp[key + "_bits_differ"] = int((got[key].view(torch.int32) != ref[key].view(torch.int32)).sum())
        row = {"case": name, "points": int(pts.shape[0]), "batch": int(gt.shape[0]), "gt_rows": int(gt.shape[1]), "yardstick_vs_op": cmp,
               "host_synchronisations_per_call": {"op": host_syncs(op), "yardstick": host_syncs(yard)}}
        no, ny = calls_for(op), calls_for(yard)
        to, ty, wo, wy = [], [], [], []
        for _ in range(args.windows):       # alternating windows
            to.append(window(op, no))
            ty.append(window(yard, ny))
        for _ in range(50):                 # alternating single calls
            wo.append(wall_once(op))
            wy.append(wall_once(yard))
        row["op"] = dict(device=dict(stats(to), calls_per_window=no), wall=stats(wo))
        row["yardstick"] = dict(device=dict(stats(ty), calls_per_window=ny), wall=stats(wy))
        row["yardstick_over_op"] = {"device": row["yardstick"]["device"]["median_ms"] / row["op"]["device"]["median_ms"],
                                    "wall": row["yardstick"]["wall"]["median_ms"] / row["op"]["wall"]["median_ms"]}
        print(json.dumps({"case": name, "op_device_ms": row["op"]["device"]["median_ms"], "op_wall_ms": row["op"]["wall"]["median_ms"],
                          "yardstick_device_ms": row["yardstick"]["device"]["median_ms"],
                          "yardstick_wall_ms": row["yardstick"]["wall"]["median_ms"], "yardstick_over_op": row["yardstick_over_op"],
                          "host_synchronisations_per_call": row["host_synchronisations_per_call"], "yardstick_vs_op": cmp}), flush=True)
        rows.append(row)
    if args.once:
        return
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "window_ms_target": WINDOW_MS, "windows": args.windows,
           "method": "device: alternating windows of calls timed with device events ending in a synchronise; wall: host clock "
                     "around one call and a synchronise, alternating, 50 each; medians", "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
