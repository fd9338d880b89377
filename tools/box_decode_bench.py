"""Box decoding on one MI355X: the reference's generate_predicted_boxes -- its torch expressions, restated here with torch ops from
the semantics of tests/box_decode_seq.py, since pcdet is not importable on the GPU machine -- against the drop-in methods of
modest_amd.utils.box_decode on the same tensors, and profiles/box_decode_bench.json.

Shapes, at B = 4: the KITTI three-class anchor head (321 408 anchors, code 7, 2 bins), the Lyft PointPillars head (138 880
anchors, code 9), PointRCNN's point head (65 536 points, K = 3), PV-RCNN's 8 192 key points, RoI heads at 4 x 100 and 4 x 512.
Per shape and side: the time of a call (median over --windows windows of events on the stream, each long enough to measure,
warm, the two sides alternating), the kernel launches of a call (torch's profiler), the peak memory a call allocates, and the
largest difference between the two sides' boxes (headings modulo the period).  For the two anchor shapes also the achieved
bytes per second against the algorithmic traffic B N (code_in + bins + code_out) 4 + N cols 4, as a fraction of 8 TB/s, next
to a device-to-device copy that moves the same traffic (half of it read, half written) in the same run.

    python tools/box_decode_bench.py [--out profiles/box_decode_bench.json] [--windows 5]
    python tools/box_decode_bench.py --once --side op      (one call per shape, for a kernel trace)
"""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WINDOW_MS = 200.0
PEAK_BYTES_PER_S = 8e12     # the figure the README uses


# ---- the reference's methods as torch expressions ---------------------------------------------------------------------------
def yard_residual_decode(box_encodings, anchors, sincos):
    xa, ya, za, dxa, dya, dza, ra, *cas = torch.split(anchors, 1, dim=-1)
    if not sincos:
        xt, yt, zt, dxt, dyt, dzt, rt, *cts = torch.split(box_encodings, 1, dim=-1)
    else:
        xt, yt, zt, dxt, dyt, dzt, cost, sint, *cts = torch.split(box_encodings, 1, dim=-1)
    diagonal = torch.sqrt(dxa ** 2 + dya ** 2)
    xg = xt * diagonal + xa
    yg = yt * diagonal + ya
    zg = zt * dza + za
    dxg = torch.exp(dxt) * dxa
    dyg = torch.exp(dyt) * dya
    dzg = torch.exp(dzt) * dza
    if sincos:
        rg = torch.atan2(sint + torch.sin(ra), cost + torch.cos(ra))
    else:
        rg = rt + ra
    cgs = [t + a for t, a in zip(cts, cas)]
    return torch.cat([xg, yg, zg, dxg, dyg, dzg, rg, *cgs], dim=-1)


def yard_anchor(head, batch_size, cls_preds, box_preds, dir_cls_preds=None):
    anchors = head.anchors
    num_anchors = anchors.view(-1, anchors.shape[-1]).shape[0]
    batch_anchors = anchors.view(1, -1, anchors.shape[-1]).repeat(batch_size, 1, 1)
    batch_cls_preds = cls_preds.view(batch_size, num_anchors, -1).float()
    batch_box_preds = box_preds.view(batch_size, num_anchors, -1)
    batch_box_preds = yard_residual_decode(batch_box_preds, batch_anchors, head.box_coder.encode_angle_by_sincos)
    if dir_cls_preds is not None:
        dir_offset, dir_limit_offset = head.model_cfg["DIR_OFFSET"], head.model_cfg["DIR_LIMIT_OFFSET"]
        dir_cls_preds = dir_cls_preds.view(batch_size, num_anchors, -1)
        dir_labels = torch.max(dir_cls_preds, dim=-1)[1]
        period = 2 * np.pi / head.model_cfg["NUM_DIR_BINS"]
        val = batch_box_preds[..., 6] - dir_offset
        dir_rot = val - torch.floor(val / period + dir_limit_offset) * period
        batch_box_preds[..., 6] = dir_rot + dir_offset + period * dir_labels.to(batch_box_preds.dtype)
    return batch_cls_preds, batch_box_preds


def yard_point(head, points, point_cls_preds, point_box_preds):
    _, pred_classes = point_cls_preds.max(dim=-1)
    pred_classes = pred_classes + 1
    xt, yt, zt, dxt, dyt, dzt, cost, sint, *cts = torch.split(point_box_preds, 1, dim=-1)
    xa, ya, za = torch.split(points, 1, dim=-1)
    if head.box_coder.use_mean_size:
        point_anchor_size = head.box_coder.mean_size[pred_classes - 1]
        dxa, dya, dza = torch.split(point_anchor_size, 1, dim=-1)
        diagonal = torch.sqrt(dxa ** 2 + dya ** 2)
        xg = xt * diagonal + xa
        yg = yt * diagonal + ya
        zg = zt * dza + za
        dxg = torch.exp(dxt) * dxa
        dyg = torch.exp(dyt) * dya
        dzg = torch.exp(dzt) * dza
    else:
        xg, yg, zg = xt + xa, yt + ya, zt + za
        dxg, dyg, dzg = torch.split(torch.exp(point_box_preds[..., 3:6]), 1, dim=-1)
    rg = torch.atan2(sint, cost)
    return point_cls_preds, torch.cat([xg, yg, zg, dxg, dyg, dzg, rg, *cts], dim=-1)


def yard_roi(head, batch_size, rois, cls_preds, box_preds):
    code_size = head.box_coder.code_size
    batch_cls_preds = cls_preds.view(batch_size, -1, cls_preds.shape[-1])
    batch_box_preds = box_preds.view(batch_size, -1, code_size)
    roi_ry = rois[:, :, 6].view(-1)
    roi_xyz = rois[:, :, 0:3].view(-1, 3)
    local_rois = rois.clone().detach()
    local_rois[:, :, 0:3] = 0
    batch_box_preds = yard_residual_decode(batch_box_preds, local_rois, False).view(-1, code_size)
    points = batch_box_preds.unsqueeze(dim=1)
    cosa, sina = torch.cos(roi_ry), torch.sin(roi_ry)
    zeros, ones = roi_ry.new_zeros(points.shape[0]), roi_ry.new_ones(points.shape[0])
    rot_matrix = torch.stack((cosa, sina, zeros, -sina, cosa, zeros, zeros, zeros, ones), dim=1).view(-1, 3, 3).float()
    points_rot = torch.matmul(points[:, :, 0:3], rot_matrix)
    batch_box_preds = torch.cat((points_rot, points[:, :, 3:]), dim=-1).squeeze(dim=1)
    batch_box_preds[:, 0:3] += roi_xyz
    return batch_cls_preds, batch_box_preds.view(batch_size, -1, code_size)


YARD = {"anchor": yard_anchor, "point": yard_point, "roi": yard_roi}


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


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = int(torch.cuda.max_memory_allocated() - base)
    del out
    return peak


def launches(fn):
    """kernel launches and device copies of one call, from torch's profiler; None where it is not available"""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return int(sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")))
    except Exception as err:      # noqa: BLE001
        print("launch count not available:", err, file=sys.stderr)
        return None


# (name, kind, settings)
SHAPES = (("KITTI 3-class anchor head, B = 4", "anchor", dict(B=4, N=321408, extra=0, bins=2)),
          ("Lyft PointPillars anchor head, B = 4", "anchor", dict(B=4, N=138880, extra=2, bins=2)),
          ("PointRCNN point head, 4 x 16384 points", "point", dict(N=65536, K=3)),
          ("PV-RCNN key points, 4 x 2048", "point", dict(N=8192, K=3)),
          ("RoI head, 4 x 100", "roi", dict(B=4, M=100)),
          ("RoI head, 4 x 512", "roi", dict(B=4, M=512)))


def make(kind, cfg, dev):
    """-> (stand-in head with both methods' attributes, the arguments, the case)"""
    import box_decode_seq as seq
    if kind == "anchor":
        case = seq.make_anchor(1, cfg["B"], cfg["N"], extra=cfg["extra"], bins=cfg["bins"])
    elif kind == "point":
        case = seq.make_point(2, cfg["N"], K=cfg["K"])
    else:
        case = seq.make_roi(3, cfg["B"], cfg["M"])
    head, args = seq.bare_head(case, device=dev)
    args = tuple(a.detach() if torch.is_tensor(a) else a for a in args)
    return head, args, case


def difference(kind, case, a, b):
    """the largest |a - b| over finite elements, headings modulo their period"""
    a, b = a.detach().double().reshape(-1, a.shape[-1]), b.detach().double().reshape(-1, b.shape[-1])
    d = (a - b).abs()
    period = None
    if kind == "anchor" and case.get("dir") is not None:
        period = 2 * np.pi / case["dir"].shape[-1]
    elif kind == "point":
        period = 2 * np.pi
    if period is not None:
        w = d[:, 6] % period
        d[:, 6] = torch.minimum(w, period - w)
    d = d[torch.isfinite(d)]
    return float(d.max()) if d.numel() else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_decode_bench.json"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--once", action="store_true", help="run --steps calls of --side per shape and exit (for a kernel trace)")
    ap.add_argument("--side", choices=("both", "op", "yardstick"), default="both", help="with --once: the side to run")
    ap.add_argument("--steps", type=int, default=1, help="with --once: calls per side and shape")
    ap.add_argument("--shapes", type=int, default=len(SHAPES), help="the first so many shapes")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "box_decode_bench needs an MI355X: there is no CPU fallback"
    dev = torch.device("cuda:0")
    rows = []
    for name, kind, cfg in SHAPES[:args.shapes]:
        head, call_args, case = make(kind, cfg, dev)
        ours = lambda: head.generate_predicted_boxes(*call_args)      # noqa: E731
        yard = lambda: YARD[kind](head, *call_args)                   # noqa: E731
        if args.once:
            for _ in range(args.steps):
                if args.side in ("both", "op"):
                    ours()
                if args.side in ("both", "yardstick"):
                    yard()
            torch.cuda.synchronize()
            continue
        diff = difference(kind, case, ours()[1], yard()[1])
        assert diff < 1e-3, (name, diff)
        n_ours, n_yard = calls_for(ours), calls_for(yard)
        t_ours, t_yard = [], []
        for _ in range(args.windows):                                  # alternating: both sides see the same neighbours
            t_ours.append(window(ours, n_ours))
            t_yard.append(window(yard, n_yard))
        row = {"case": name, "kind": kind, "settings": cfg, "op": stats(t_ours), "yardstick": stats(t_yard),
               "yardstick_over_op": float(np.median(t_yard) / np.median(t_ours)),
               "launches": {"op": launches(ours), "yardstick": launches(yard)},
               "peak_bytes": {"op": peak_bytes(ours), "yardstick": peak_bytes(yard)},
               "largest_difference": diff}
        if kind == "anchor":
            B, N, code = case["box"].shape
            cols, bins = case["anchors"].shape[1], case["dir"].shape[-1]
            traffic = B * N * (code + bins + cols) * 4 + N * cols * 4
            src = torch.empty((traffic // 2,), dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            copy = lambda: dst.copy_(src)                              # noqa: E731  (a device-to-device memcpy on the stream)
            n_copy = calls_for(copy)
            t_copy = [window(copy, n_copy) for _ in range(args.windows)]
            row["traffic_bytes"] = traffic
            row["op_bytes_per_s"] = traffic / (np.median(t_ours) * 1e-3)
            row["op_fraction_of_8TBps"] = row["op_bytes_per_s"] / PEAK_BYTES_PER_S
            row["copy"] = dict(stats(t_copy), bytes_copied=traffic // 2, bytes_per_s=traffic / (np.median(t_copy) * 1e-3))
            row["op_over_copy_rate"] = row["op_bytes_per_s"] / row["copy"]["bytes_per_s"]
        rows.append(row)
        print(json.dumps({k: row[k] for k in row if k not in ("op", "yardstick", "settings", "copy")}
                         | {"op_ms": row["op"]["median_ms"], "yardstick_ms": row["yardstick"]["median_ms"]}), flush=True)
    if args.once:
        return
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "window_ms": WINDOW_MS, "windows": args.windows,
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
