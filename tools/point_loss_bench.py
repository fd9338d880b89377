#!/usr/bin/env python
"""Time modest_amd.utils.point_head_loss.get_loss with its backward against a PyTorch restatement of the reference's path on
the same device, and write profiles/point_loss_bench.json.

The yardstick is written in this file (``yard_get_loss``: the reference's heads cannot be constructed here, they need their
compiled extensions): the weights from the labels, the ``(N, num_class + 1)`` one-hot tensor by ``scatter_`` and its slice, the
focal loss as its chain of element-wise operators, ``binary_cross_entropy`` of the sigmoid of the part predictions times the
0 / 1 mask, the weighted smooth L1 over all rows times a weight that is zero off the positives, and the host reads
(``.item()`` of every loss, of the positive count, and the ``(pos_mask > 0).sum().item()`` of the part term) -- stock PyTorch
operators in the reference's order, so on the CPU it gives the recorded reference bit for bit (tests/test_point_loss_cpu.py).
A step of either side is the forward, ``backward()`` into the leaf predictions and the Python floats of ``tb_dict``.  Before
any time is reported the two sides' outputs are compared on the timed inputs, and ours with the numpy restatement.

Shapes: PointRCNN's point head (B = 4 and B = 16, 16 384 points per sample, one class, cls + box), a PartA2-like head (B = 4,
20 000 voxel centres per sample, three classes, cls + part + box) and PV-RCNN's key-point head (B = 4, 2 048 key points per
sample, three classes, cls alone); the labels come from this library's ``assign_stack_targets`` on the scenes of
tools/point_targets_bench.py, the part labels clamped into [0, 1] (torch's ``binary_cross_entropy`` refuses what lies
outside).  Method: both sides in this process on the same device, every shape warmed up, a window holds enough steps to last
200 ms, the two sides alternate window by window; median, minimum and maximum of the windows are written.  A window is timed
with device events around the steps, ending in a synchronise, so the host waits of either side are inside it.  Host
synchronisations per step are counted by PyTorch itself (``torch.cuda.set_sync_debug_mode("warn")``), the peak memory of a
step by ``torch.cuda.max_memory_allocated`` above what is allocated when the step begins.  The launches of a step are not
counted here: they are the difference of the kernel calls of two traced ``--once`` runs of one side with different
``--steps`` (profiles/README.md).

    python tools/point_loss_bench.py [--out profiles/point_loss_bench.json] [--windows 5]
    python tools/point_loss_bench.py --once [--side op|yardstick|both] [--steps 1] [--shapes 4]
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
import point_loss_seq as seq  # noqa: E402

WINDOW_MS = 200.0


# ---- the yardstick: the reference's path in stock PyTorch operators ------------------------------------------------------
def yard_cls_loss(head):
    ret = head.forward_ret_dict
    labels = ret['point_cls_labels'].view(-1)
    x = ret['point_cls_preds'].view(-1, head.num_class)
    pos = labels > 0
    weights = ((labels == 0) * 1.0 + 1.0 * pos).float()
    count = pos.sum(dim=0).float()
    weights /= torch.clamp(count, min=1.0)
    onehot = x.new_zeros(*list(labels.shape), head.num_class + 1)
    onehot.scatter_(-1, (labels * (labels >= 0).long()).unsqueeze(dim=-1).long(), 1.0)
    t = onehot[..., 1:]
    s = torch.sigmoid(x)
    alpha_w = t * 0.25 + (1 - t) * (1 - 0.25)
    pt = t * (1.0 - s) + (1.0 - t) * s
    focal = alpha_w * torch.pow(pt, 2.0)
    bce = torch.clamp(x, min=0) - x * t + torch.log1p(torch.exp(-torch.abs(x)))
    loss = (focal * bce * weights.unsqueeze(-1)).sum()
    loss = loss * head.model_cfg.LOSS_CONFIG.LOSS_WEIGHTS['point_cls_weight']
    return loss, {'point_loss_cls': loss.item(), 'point_pos_num': count.item()}


def yard_part_loss(head):
    ret = head.forward_ret_dict
    pos = ret['point_cls_labels'] > 0
    count = max(1, (pos > 0).sum().item())
    loss = nnf.binary_cross_entropy(torch.sigmoid(ret['point_part_preds']), ret['point_part_labels'], reduction='none')
    loss = (loss.sum(dim=-1) * pos.float()).sum() / (3 * count)
    loss = loss * head.model_cfg.LOSS_CONFIG.LOSS_WEIGHTS['point_part_weight']
    return loss, {'point_loss_part': loss.item()}


def yard_box_loss(head):
    ret = head.forward_ret_dict
    pos = ret['point_cls_labels'] > 0
    weights = pos.float()
    weights /= torch.clamp(pos.sum().float(), min=1.0)
    a, b = ret['point_box_preds'][None, ...], ret['point_box_labels'][None, ...]
    b = torch.where(torch.isnan(b), a, b)
    diff = (a - b) * head.reg_loss_func.code_weights.view(1, 1, -1)
    beta = head.reg_loss_func.beta
    n = torch.abs(diff)
    loss = n if beta < 1e-5 else torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta)
    loss = (loss * weights[None, ...].unsqueeze(-1)).sum()
    loss = loss * head.model_cfg.LOSS_CONFIG.LOSS_WEIGHTS['point_box_weight']
    return loss, {'point_loss_box': loss.item()}


def yard_get_loss(head, tb_dict=None):
    """the three heads' get_loss: the terms follow the head's class name and box_layers"""
    tb_dict = {} if tb_dict is None else tb_dict
    kind = type(head).__name__
    loss, tb = yard_cls_loss(head)
    tb_dict.update(tb)
    if kind == "PointIntraPartOffsetHead":
        part, tb = yard_part_loss(head)
        tb_dict.update(tb)
        loss = loss + part
    if kind == "PointHeadBox" or (kind == "PointIntraPartOffsetHead" and head.box_layers is not None):
        box, tb = yard_box_loss(head)
        tb_dict.update(tb)
        loss = loss + box
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


# (name, head, B, points per sample, num_class)
SHAPES = (("PointRCNN, B = 4", "PointHeadBox", 4, 16384, 1), ("PointRCNN, B = 16", "PointHeadBox", 16, 16384, 1),
          ("PartA2-like, B = 4", "PointIntraPartOffsetHead", 4, 20000, 3), ("PV-RCNN, B = 4", "PointHeadSimple", 4, 2048, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_loss_bench.json"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--once", action="store_true", help="run --steps steps of --side per shape and exit (for a kernel trace)")
    ap.add_argument("--side", choices=("both", "op", "yardstick"), default="both", help="with --once: the side to run")
    ap.add_argument("--steps", type=int, default=1, help="with --once: steps per side and shape")
    ap.add_argument("--shapes", type=int, default=len(SHAPES), help="with --once: the first so many shapes")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/point_loss_bench.py needs an MI355X: there is no CPU path")
    import point_targets_bench as ptb
    from modest_amd.utils import point_head_targets as pht
    dev = torch.device("cuda:0")
    mean = torch.tensor(ptb.KITTI, dtype=torch.float32, device=dev)
    rows = []
    for name, kind, B, n_per, C in (SHAPES[:args.shapes] if args.once else SHAPES):
        cfg = seq.base_cfg(head=kind, B=B, N=n_per, num_class=C, code=8)
        terms = seq.terms_of(cfg)
        pts, gt, ext = (torch.from_numpy(a).to(dev) for a in ptb.pointrcnn_inputs(B=B, n_per=n_per, seed=5 + B))
        assigner = pht.bind(type("Head", (), {}))()
        assigner.num_class, assigner.box_coder = C, types.SimpleNamespace(use_mean_size=True, mean_size=mean, code_size=8)
        targets = assigner.assign_stack_targets(pts, gt, extend_gt_boxes=ext, ret_box_labels="box" in terms,
                                                ret_part_labels="part" in terms)
        R = B * n_per
        gen = torch.Generator(device="cpu").manual_seed(7)
        preds = {"cls": (torch.randn((R, C), generator=gen) * 3.0).to(dev).requires_grad_(True)}
        if "part" in terms:
            preds["part"] = (torch.randn((R, 3), generator=gen) * 2.0).to(dev).requires_grad_(True)
        if "box" in terms:
            preds["box"] = (torch.randn((R, 8), generator=gen) * 0.5).to(dev).requires_grad_(True)
        head = seq.bound_class(kind)()
        head.model_cfg, head.num_class = seq.model_cfg(cfg), C
        if kind == "PointIntraPartOffsetHead":
            head.box_layers = object()
        head.cls_loss_func = seq.loss_stub("SigmoidFocalClassificationLoss", alpha=seq.ALPHA, gamma=seq.GAMMA)
        head.reg_loss_func = seq.loss_stub("WeightedSmoothL1Loss", beta=1.0 / 9.0, code_weights=torch.ones(8, device=dev))
        head.forward_ret_dict = dict(point_cls_preds=preds["cls"], point_cls_labels=targets["point_cls_labels"])
        inp = dict(cls=preds["cls"].detach().cpu().numpy(), labels=targets["point_cls_labels"].cpu().numpy())
        if "part" in terms:
            part_t = targets["point_part_labels"].clamp(0.0, 1.0)
            head.forward_ret_dict.update(point_part_preds=preds["part"], point_part_labels=part_t)
            inp.update(part=preds["part"].detach().cpu().numpy(), part_t=part_t.cpu().numpy())
        if "box" in terms:
            head.forward_ret_dict.update(point_box_preds=preds["box"], point_box_labels=targets["point_box_labels"])
            inp.update(box=preds["box"].detach().cpu().numpy(), box_t=targets["point_box_labels"].cpu().numpy(),
                       cw=np.ones(8, dtype=np.float32))
        cfg["int64"] = targets["point_cls_labels"].dtype == torch.int64

        def clear():
            for p in preds.values():
                p.grad = None

        def step(fn):
            clear()
            loss, tb = fn(head)
            loss.backward()
            return loss, tb

        op = lambda: step(type(head).get_loss)         # noqa: E731
        yard = lambda: step(yard_get_loss)             # noqa: E731
        if args.once:          # the launches of a step: the difference of two traced runs with different --steps
            for _ in range(args.steps):
                if args.side != "yardstick":
                    op()
                if args.side != "op":
                    yard()
            torch.cuda.synchronize()
            continue
        loss_o, tb_o = op()
        got = seq.outputs_of(loss_o.item(), tb_o, preds)
        grads_o = {k: p.grad.clone() for k, p in preds.items()}
        loss_y, tb_y = yard()
        grads_y = {k: p.grad.clone() for k, p in preds.items()}
        torch.cuda.synchronize()
        why = seq.report(got, seq.restate(inp, cfg), "the device")
        tb_y["point_loss"], tb_o["point_loss"] = loss_y.item(), loss_o.item()
        row = {"case": name, "head": kind, "terms": list(terms), "batch": B, "rows": R, "num_class": C,
               "positives": int(tb_o["point_pos_num"]), "ignored": int((targets["point_cls_labels"] < 0).sum()),
               "op_vs_restatement": why or "bit for bit",
               "yardstick_vs_op": {k: float(abs(tb_y[k] - tb_o[k]) / max(abs(tb_y[k]), 1e-30)) for k in tb_y} | {
                   f"grad_{k}_max_abs_diff": float((grads_y[k] - grads_o[k]).abs().max()) for k in preds} | {
                   f"grad_{k}_max_abs": float(grads_y[k].abs().max()) for k in preds}}
        assert list(tb_y) == list(tb_o), (list(tb_y), list(tb_o))
        assert all(v < 1e-4 for k, v in row["yardstick_vs_op"].items() if k.startswith("point")), row
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
        print(json.dumps({k: row[k] for k in ("case", "rows", "positives", "yardstick_over_op", "host_synchronisations_per_step",
                                              "peak_bytes_of_a_step", "op_vs_restatement", "yardstick_vs_op")}
                         | {"op_ms": row["op"], "yardstick_ms": row["yardstick"]}), flush=True)
        rows.append(row)
    if args.once:
        return
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "window_ms_target": WINDOW_MS, "windows": args.windows,
           "method": "a step = forward, backward() into the leaf predictions and tb_dict's floats; alternating windows of steps "
                     "timed with device events ending in a synchronise; medians over the windows", "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
