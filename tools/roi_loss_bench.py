#!/usr/bin/env python
"""Time modest_amd.utils.roi_head_loss.get_loss with its backward against a PyTorch restatement of the reference's path on the
same device, and write profiles/roi_loss_bench.json.

The yardstick is written in this file (``yard_get_loss``: the reference's head cannot be constructed here, it needs its
compiled extensions): the binary cross entropy of the sigmoid with its valid mask, the cloned rois encoded against with the
sizes clamped in place, the smooth-L1 loss over all rows times the 0 / 1 mask, the boolean-indexed foreground rows decoded,
rotated by a batched matmul and moved, three sets of corners each through another rotation matmul, two norms, the ``min``, the
smooth L1 with beta 1 and the means, and the five host reads (``fg_sum.item()`` and four loss ``.item()``) -- stock PyTorch
operators in the reference's order (plus one clamp of the hard labels' -1, without which torch 2.10's device kernel aborts), so on the CPU it gives the recorded reference bit for bit (tests/test_roi_loss_cpu.py).
A step of either side is the forward, ``backward()`` into the two leaf predictions and the Python floats of ``tb_dict``.
Before any time is reported the two sides' outputs are compared on the timed inputs, and ours with the numpy restatement.

Shapes: PointRCNN's training head (B = 4 and B = 16, 128 rois per sample, hard ``cls`` labels with ignored rows) and a
PV-RCNN-like head (B = 4, soft ``roi_iou`` labels), the inputs from this library's RoI target assignment on the scenes of
tools/roi_targets_bench.py.  Method: both sides in this process on the same device, every shape warmed up, a window holds
enough steps to last 200 ms, the two sides alternate window by window; median, minimum and maximum of the windows are
written.  A window is timed with device events around the steps, ending in a synchronise, so the host waits of either side are
inside it.  Host synchronisations per step are counted by PyTorch itself (``torch.cuda.set_sync_debug_mode("warn")``), the
peak memory of a step by ``torch.cuda.max_memory_allocated`` above what is allocated when the step begins.  The launches of a
step are not counted here: they are the difference of the kernel calls of two traced ``--once`` runs of one side with
different ``--steps`` (profiles/README.md).

    python tools/roi_loss_bench.py [--out profiles/roi_loss_bench.json] [--windows 5]
    python tools/roi_loss_bench.py --once [--side op|yardstick|both] [--steps 1] [--shapes 3]
"""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as nnf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import roi_loss_seq as seq  # noqa: E402

WINDOW_MS = 200.0


# ---- the yardstick: the reference's path in stock PyTorch operators ------------------------------------------------------
def yard_rotate_z(points, angle):
    """(n, k, 3) points about z by (n) angles: a batched matmul with the (n, 3, 3) matrices"""
    c, s = torch.cos(angle), torch.sin(angle)
    zero, one = angle.new_zeros(points.shape[0]), angle.new_ones(points.shape[0])
    rot = torch.stack((c, s, zero, -s, c, zero, zero, zero, one), dim=1).view(-1, 3, 3).float()
    return torch.matmul(points[:, :, 0:3], rot)


def yard_corners(boxes):
    """(n, 7) -> (n, 8, 3)"""
    template = boxes.new_tensor(([1, 1, -1], [1, -1, -1], [-1, -1, -1], [-1, 1, -1],
                                 [1, 1, 1], [1, -1, 1], [-1, -1, 1], [-1, 1, 1])) / 2
    corners = boxes[:, None, 3:6].repeat(1, 8, 1) * template[None, :, :]
    corners = yard_rotate_z(corners.view(-1, 8, 3), boxes[:, 6]).view(-1, 8, 3)
    corners += boxes[:, None, 0:3]
    return corners


def yard_smooth_l1(n, beta):
    return torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta)


def yard_encode(boxes, anchors):
    """the residual encoding; both sets of sizes clamped IN PLACE"""
    anchors[:, 3:6] = torch.clamp_min(anchors[:, 3:6], min=1e-5)
    boxes[:, 3:6] = torch.clamp_min(boxes[:, 3:6], min=1e-5)
    a = [anchors[:, k:k + 1] for k in range(anchors.shape[1])]
    g = [boxes[:, k:k + 1] for k in range(boxes.shape[1])]
    diagonal = torch.sqrt(a[3] ** 2 + a[4] ** 2)
    cols = [(g[0] - a[0]) / diagonal, (g[1] - a[1]) / diagonal, (g[2] - a[2]) / a[5], torch.log(g[3] / a[3]), torch.log(g[4] / a[4]),
            torch.log(g[5] / a[5]), g[6] - a[6]]
    cols += [gk - ak for gk, ak in zip(g[7:], a[7:])]
    return torch.cat(cols, dim=-1)


def yard_decode(enc, anchors):
    a = [anchors[..., k:k + 1] for k in range(anchors.shape[-1])]
    t = [enc[..., k:k + 1] for k in range(enc.shape[-1])]
    diagonal = torch.sqrt(a[3] ** 2 + a[4] ** 2)
    cols = [t[0] * diagonal + a[0], t[1] * diagonal + a[1], t[2] * a[5] + a[2], torch.exp(t[3]) * a[3], torch.exp(t[4]) * a[4],
            torch.exp(t[5]) * a[5], t[6] + a[6]]
    cols += [tk + ak for tk, ak in zip(t[7:], a[7:])]
    return torch.cat(cols, dim=-1)


def yard_cls_loss(head, clamp_labels=None):
    ret = head.forward_ret_dict
    x = ret['rcnn_cls'].view(-1)
    labels = ret['rcnn_cls_labels'].view(-1)
    target = labels.float()
    # hard labels hold -1 for the ignored rows.  torch 2.10 refuses such a target: its CPU kernel raises, its device kernel
    # asserts 0 <= target <= 1 and the assertion aborts the process (measured: a hardware exception in
    # binary_cross_entropy_out_cuda).  The reference as it stands cannot run on this torch with ignored rows; the yardstick
    # therefore clamps the target of hard labels at 0, one element-wise kernel more, as tools/make_golden_roi_loss.py does
    # for the recording.  The valid mask below comes from the unclamped labels, so those rows still enter as finite * 0.
    if clamp_labels is None:
        clamp_labels = not labels.is_floating_point()
    if clamp_labels:
        target = target.clamp(min=0)
    batch = nnf.binary_cross_entropy(torch.sigmoid(x), target, reduction='none')
    valid = (labels >= 0).float()
    loss = (batch * valid).sum() / torch.clamp(valid.sum(), min=1.0)
    loss = loss * head.model_cfg.LOSS_CONFIG.LOSS_WEIGHTS['rcnn_cls_weight']
    return loss, {'rcnn_loss_cls': loss.item()}


def yard_reg_loss(head):
    ret, cfg = head.forward_ret_dict, head.model_cfg.LOSS_CONFIG
    code = head.box_coder.code_size
    mask = ret['reg_valid_mask'].view(-1)
    gt_ct = ret['gt_of_rois'][..., 0:code]
    gt_src = ret['gt_of_rois_src'][..., 0:code].view(-1, code)
    reg, rois = ret['rcnn_reg'], ret['rois']
    R = gt_ct.view(-1, code).shape[0]
    fg = mask > 0
    fg_sum = fg.long().sum().item()
    tb = {}
    anchor = rois.clone().detach().view(-1, code)
    anchor[:, 0:3] = 0
    anchor[:, 6] = 0
    target = yard_encode(gt_ct.view(R, code), anchor)
    inp = reg.view(R, -1).unsqueeze(dim=0)
    target = target.unsqueeze(dim=0)
    target = torch.where(torch.isnan(target), inp, target)
    diff = (inp - target) * head.reg_loss_func.code_weights.view(1, 1, -1)
    loss = yard_smooth_l1(torch.abs(diff), head.reg_loss_func.beta)
    loss = (loss.view(R, -1) * fg.unsqueeze(dim=-1).float()).sum() / max(fg_sum, 1)
    loss = loss * cfg.LOSS_WEIGHTS['rcnn_reg_weight']
    tb['rcnn_loss_reg'] = loss.item()
    if cfg.CORNER_LOSS_REGULARIZATION and fg_sum > 0:
        fg_reg = reg.view(R, -1)[fg]
        fg_rois = rois.view(-1, code)[fg].view(1, -1, code)
        anchors = fg_rois.clone().detach()
        ry, xyz = fg_rois[:, :, 6].view(-1), fg_rois[:, :, 0:3].view(-1, 3)
        anchors[:, :, 0:3] = 0
        boxes = yard_decode(fg_reg.view(anchors.shape[0], -1, code), anchors).view(-1, code)
        moved = yard_rotate_z(boxes.unsqueeze(dim=1), ry)
        boxes = torch.cat((moved, boxes.unsqueeze(dim=1)[:, :, 3:]), dim=-1).squeeze(dim=1)
        boxes[:, 0:3] += xyz
        pred, gt = boxes[:, 0:7], gt_src[fg][:, 0:7]
        pc, gc = yard_corners(pred), yard_corners(gt)
        flip = gt.clone()
        flip[:, 6] += np.pi
        fc = yard_corners(flip)
        dist = torch.min(torch.norm(pc - gc, dim=2), torch.norm(pc - fc, dim=2))
        corner = yard_smooth_l1(torch.abs(dist), 1.0).mean(dim=1).mean()
        corner = corner * cfg.LOSS_WEIGHTS['rcnn_corner_weight']
        loss += corner
        tb['rcnn_loss_corner'] = corner.item()
    return loss, tb


def yard_get_loss(head, tb_dict=None, clamp_labels=None):
    tb_dict = {} if tb_dict is None else tb_dict
    loss = 0
    cls, tb = yard_cls_loss(head, clamp_labels)
    loss += cls
    tb_dict.update(tb)
    reg, tb = yard_reg_loss(head)
    loss += reg
    tb_dict.update(tb)
    tb_dict['rcnn_loss'] = loss.item()
    return loss, tb_dict


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


def peak_bytes(fn, clear):
    """the most a step allocates above what is allocated when it begins, the gradients of the step before released"""
    clear()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def host_syncs(fn):
    import warnings
    mode = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    return sum("called a synchronizing" in str(w.message) for w in seen)


SHAPES = (("PointRCNN train, B = 4", 4, "cls"), ("PointRCNN train, B = 16", 16, "cls"), ("PV-RCNN-like train, B = 4 (roi_iou)", 4, "roi_iou"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roi_loss_bench.json"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--once", action="store_true", help="run --steps steps of --side per shape and exit (for a kernel trace)")
    ap.add_argument("--side", choices=("both", "op", "yardstick"), default="both", help="with --once: the side to run")
    ap.add_argument("--steps", type=int, default=1, help="with --once: steps per side and shape")
    ap.add_argument("--shapes", type=int, default=len(SHAPES), help="with --once: the first so many shapes")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/roi_loss_bench.py needs an MI355X: there is no CPU path")
    import roi_targets_bench as rtb
    from modest_amd.utils import roi_head_loss, roi_targets as rt
    dev = torch.device("cuda:0")
    rows = []
    for name, B, score_type in (SHAPES[:args.shapes] if args.once else SHAPES):
        tcfg = rtb.POINTRCNN if score_type == "cls" else rtb.PVRCNN
        r, s, l, g = (torch.from_numpy(a).to(dev) for a in rtb.inputs(B, 40 + B))
        assigner = rt.bind(type("RoIHead", (), {}))()
        assigner.model_cfg = types.SimpleNamespace(TARGET_CONFIG=types.SimpleNamespace(**tcfg))
        np.random.seed(1), torch.manual_seed(2)
        targets = assigner.assign_targets(dict(batch_size=B, rois=r, roi_scores=s, roi_labels=l, gt_boxes=g))
        M = int(targets["rois"].shape[1])
        R = B * M
        cfg = seq.base_cfg(B=B, M=M, code=7, gt_cols=int(targets["gt_of_rois"].shape[-1]), labels="cls" if score_type == "cls" else "iou",
                           label_dtype=str(targets["rcnn_cls_labels"].dtype).split(".")[-1],
                           mask_dtype=str(targets["reg_valid_mask"].dtype).split(".")[-1])
        gen = torch.Generator(device="cpu").manual_seed(7)
        preds = {"cls": (torch.randn((R, 1), generator=gen) * 2.0).to(dev).requires_grad_(True),
                 "reg": (torch.randn((R, 7), generator=gen) * 0.3).to(dev).requires_grad_(True)}
        head = type("Head", (), {})()
        head.model_cfg = seq.model_cfg(cfg)
        head.box_coder = seq.loss_stub("ResidualCoder", code_size=7, encode_angle_by_sincos=False)
        head.reg_loss_func = seq.loss_stub("WeightedSmoothL1Loss", beta=1.0 / 9.0, code_weights=torch.ones(7, device=dev))
        keys = ("rcnn_cls_labels", "reg_valid_mask", "gt_of_rois", "gt_of_rois_src", "rois")
        head.forward_ret_dict = dict(rcnn_cls=preds["cls"], rcnn_reg=preds["reg"], **{k: targets[k] for k in keys})
        inp = dict(cls=preds["cls"].detach().view(-1).cpu().numpy(), reg=preds["reg"].detach().cpu().numpy(),
                   labels=targets["rcnn_cls_labels"].view(-1).cpu().numpy(), mask=targets["reg_valid_mask"].view(-1).cpu().numpy(),
                   gt=targets["gt_of_rois"].reshape(R, -1).cpu().numpy(), src=targets["gt_of_rois_src"].reshape(R, -1).cpu().numpy(),
                   rois=targets["rois"].reshape(R, 7).cpu().numpy(), cw=np.ones(7, dtype=np.float32))

        def clear():
            for p in preds.values():
                p.grad = None

        def step(fn):
            clear()
            loss, tb = fn(head)
            loss.backward()
            return tb

        op = lambda: step(roi_head_loss.get_loss)      # noqa: E731
        yard = lambda: step(yard_get_loss)             # noqa: E731
        if args.once:          # the launches of a step: the difference of two traced runs with different --steps
            for _ in range(args.steps):
                if args.side != "yardstick":
                    op()
                if args.side != "op":
                    yard()
            torch.cuda.synchronize()
            continue
        tb_o = op()
        grads_o = {k: p.grad.clone() for k, p in preds.items()}
        tb_y = yard()          # after ours: it clamps the sizes in the dict's gt_of_rois in place
        grads_y = {k: p.grad.clone() for k, p in preds.items()}
        torch.cuda.synchronize()
        want = seq.restate(inp, cfg)
        table = head._modest_roi_loss_table
        got = dict(table=np.array([tb_o["rcnn_loss_cls"], tb_o["rcnn_loss_reg"], tb_o.get("rcnn_loss_corner", 0.0), tb_o["rcnn_loss"],
                                   float(table[4]), float(table[5])], dtype=np.float32),
                   grad_cls=grads_o["cls"].view(-1).cpu().numpy(), grad_reg=grads_o["reg"].cpu().numpy())
        why = seq.report(got, want, "the device")
        row = {"case": name, "batch": B, "rows": R, "fg_sum": int(got["table"][4]), "valid_class_rows": int(got["table"][5]),
               "score_type": score_type, "op_vs_restatement": why or "bit for bit",
               "yardstick_vs_op": {k: float(abs(tb_y[k] - tb_o[k]) / max(abs(tb_y[k]), 1e-30)) for k in tb_y} | {
                   f"grad_{k}_max_abs_diff": float((grads_y[k] - grads_o[k]).abs().max()) for k in preds} | {
                   f"grad_{k}_max_abs": float(grads_y[k].abs().max()) for k in preds}}
        assert sorted(tb_y) == sorted(tb_o), (sorted(tb_y), sorted(tb_o))
        assert all(v < 1e-4 for k, v in row["yardstick_vs_op"].items() if k.startswith("rcnn")), row
        assert all(row["yardstick_vs_op"][f"grad_{k}_max_abs_diff"] <= 1e-4 * row["yardstick_vs_op"][f"grad_{k}_max_abs"] for k in preds), row
        row["host_synchronisations_per_step"] = {"op": host_syncs(op), "yardstick": host_syncs(yard)}
        row["peak_bytes_of_a_step"] = {"op": peak_bytes(op, clear), "yardstick": peak_bytes(yard, clear)}
        no, ny = calls_for(op), calls_for(yard)
        to, ty = [], []
        for _ in range(args.windows):       # alternating windows
            to.append(window(op, no))
            ty.append(window(yard, ny))
        row["op"] = dict(stats(to), calls_per_window=no)
        row["yardstick"] = dict(stats(ty), calls_per_window=ny)
        row["yardstick_over_op"] = row["yardstick"]["median_ms"] / row["op"]["median_ms"]
        print(json.dumps({k: row[k] for k in ("case", "rows", "fg_sum", "yardstick_over_op", "host_synchronisations_per_step",
                                              "peak_bytes_of_a_step", "op_vs_restatement", "yardstick_vs_op")}
                         | {"op_ms": row["op"], "yardstick_ms": row["yardstick"]}), flush=True)
        rows.append(row)
    if args.once:
        return
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "window_ms_target": WINDOW_MS, "windows": args.windows,
           "method": "a step = forward, backward() into the two leaf predictions and tb_dict's floats; alternating windows of steps "
                     "timed with device events ending in a synchronise; medians over the windows", "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
