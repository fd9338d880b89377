#!/usr/bin/env python
"""Time modest_amd.utils.anchor_head_loss.get_loss with its backward against a PyTorch restatement of the reference's path on
the same device, and write profiles/anchor_loss_bench.json.

The yardstick is written in this file (``yard_get_loss``: the reference's head cannot be constructed here, it needs its
compiled extensions): the weights from the labels, the one-hot scatter, the focal loss, the anchors repeated over the batch,
the two box tensors rebuilt with ``torch.cat`` for the sine difference, the smooth-L1 loss, the direction target with its
one-hot scatter, the cross entropy, and the four ``.item()`` reads -- stock PyTorch operators in the reference's order, so on
the CPU it gives the recorded reference bit for bit (tests/test_anchor_loss_cpu.py).  A step of either side is the forward,
``backward()`` and the Python floats of ``tb_dict``.  Before any time is reported the two sides' outputs are compared on the
timed inputs, and ours with the numpy restatement.

Shapes: the Lyft PointPillars head (B = 4, one class, 138 880 anchors, 7 columns, 2 bins) and KITTI's three-class head (B = 4,
321 408 anchors), labels and targets from this library's assigner for 5 to 25 gts per sample.  Method: both sides in this
process on the same device, every shape warmed up, a window holds enough steps to last 200 ms, the two sides alternate window
by window; median, minimum and maximum of the windows are written.  A window is timed with device events around the steps,
ending in a synchronise, so the host waits of either side are inside it.  Host synchronisations per step are counted by
PyTorch itself (``torch.cuda.set_sync_debug_mode("warn")``), the peak memory of a step by
``torch.cuda.max_memory_allocated`` above what is allocated when the step begins.

    python tools/anchor_loss_bench.py [--out profiles/anchor_loss_bench.json] [--windows 5] [--once]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as nnf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import anchor_loss_seq as seq  # noqa: E402

WINDOW_MS = 200.0


# ---- the yardstick: the reference's path in stock PyTorch operators ------------------------------------------------------
def yard_weights(labels):
    pos = labels > 0
    norm = torch.clamp(pos.sum(1, keepdim=True).float(), min=1.0)
    cls_w = ((labels == 0) * 1.0 + 1.0 * pos).float()
    reg_w = pos.float()
    reg_w /= norm
    cls_w /= norm
    return pos, cls_w, reg_w


def yard_cls_loss(head):
    x = head.forward_ret_dict['cls_preds']
    labels = head.forward_ret_dict['box_cls_labels'].clone()      # the reference writes into the dict's own tensor
    B = int(x.shape[0])
    pos, cls_w, _ = yard_weights(labels)
    if head.num_class == 1:
        labels[pos] = 1
    target = labels * (labels >= 0).type_as(labels)
    onehot = torch.zeros(*target.shape, head.num_class + 1, dtype=x.dtype, device=x.device)
    onehot.scatter_(-1, target.unsqueeze(-1).long(), 1.0)
    x = x.view(B, -1, head.num_class)
    t = onehot[..., 1:]
    s = torch.sigmoid(x)
    alpha_w = t * 0.25 + (1 - t) * (1 - 0.25)
    pt = t * (1.0 - s) + (1.0 - t) * s
    focal = alpha_w * torch.pow(pt, 2.0)
    bce = torch.clamp(x, min=0) - x * t + torch.log1p(torch.exp(-torch.abs(x)))
    loss = (focal * bce * cls_w.unsqueeze(-1)).sum() / B
    loss = loss * head.model_cfg.LOSS_CONFIG.LOSS_WEIGHTS['cls_weight']
    return loss, {'rpn_loss_cls': loss.item()}


def yard_box_loss(head):
    ret = head.forward_ret_dict
    box, dirs, tg, labels = ret['box_preds'], ret.get('dir_cls_preds', None), ret['box_reg_targets'], ret['box_cls_labels']
    B = int(box.shape[0])
    pos, _, reg_w = yard_weights(labels)
    anchors = torch.cat(head.anchors, dim=-3) if isinstance(head.anchors, list) else head.anchors
    anchors = anchors.view(1, -1, anchors.shape[-1]).repeat(B, 1, 1)
    box = box.view(B, -1, box.shape[-1] // head.num_anchors_per_location)
    enc_p = torch.sin(box[..., 6:7]) * torch.cos(tg[..., 6:7])
    enc_t = torch.cos(box[..., 6:7]) * torch.sin(tg[..., 6:7])
    a = torch.cat([box[..., :6], enc_p, box[..., 7:]], dim=-1)
    b = torch.cat([tg[..., :6], enc_t, tg[..., 7:]], dim=-1)
    b = torch.where(torch.isnan(b), a, b)
    diff = (a - b) * head.reg_loss_func.code_weights.view(1, 1, -1)
    beta = getattr(head.reg_loss_func, "beta", 0.0)
    n = torch.abs(diff)
    loc = n if beta < 1e-5 else torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta)
    loc = (loc * reg_w.unsqueeze(-1)).sum() / B
    loc = loc * head.model_cfg.LOSS_CONFIG.LOSS_WEIGHTS['loc_weight']
    total, tb = loc, {'rpn_loss_loc': loc.item()}
    if dirs is not None:
        bins = head.model_cfg.NUM_DIR_BINS
        rot = tg[..., 6] + anchors[..., 6]
        val = rot - head.model_cfg.DIR_OFFSET
        val = val - torch.floor(val / (2 * np.pi) + 0) * (2 * np.pi)
        which = torch.clamp(torch.floor(val / (2 * np.pi / bins)).long(), min=0, max=bins - 1)
        onehot = torch.zeros(*which.shape, bins, dtype=anchors.dtype, device=which.device)
        onehot.scatter_(-1, which.unsqueeze(-1).long(), 1.0)
        w = pos.type_as(dirs)
        w /= torch.clamp(w.sum(-1, keepdim=True), min=1.0)
        logits = dirs.view(B, -1, bins)
        ce = nnf.cross_entropy(logits.permute(0, 2, 1), onehot.argmax(dim=-1), reduction='none') * w
        dl = ce.sum() / B
        dl = dl * head.model_cfg.LOSS_CONFIG.LOSS_WEIGHTS['dir_weight']
        total = total + dl
        tb['rpn_loss_dir'] = dl.item()
    return total, tb


def yard_get_loss(head):
    cls, tb = yard_cls_loss(head)
    box, tb_box = yard_box_loss(head)
    tb.update(tb_box)
    loss = cls + box
    tb['rpn_loss'] = loss.item()
    return loss, tb


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anchor_loss_bench.json"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--once", action="store_true", help="run each side a few times and exit (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/anchor_loss_bench.py needs an MI355X: there is no CPU path")
    import anchor_targets_bench as atb
    import anchor_targets_seq as tseq
    from modest_amd.utils import anchor_head_loss, target_assigner as ta
    dev = torch.device("cuda:0")
    rows = []
    for (name, acfg, counts), num_class in zip(atb.shapes(), (1, 3)):
        anchors_np = tseq.make_anchors(acfg)
        gt = torch.from_numpy(atb.random_gt(np.random.RandomState(11), acfg, anchors_np, counts)).to(dev)
        anchors = [torch.from_numpy(a).to(dev) for a in anchors_np]
        assigner = ta.AxisAlignedTargetAssigner(tseq.model_cfg(acfg), acfg["class_names"], tseq.Coder(acfg))
        targets = assigner.assign_targets(anchors, gt)
        B, N = (int(v) for v in targets["box_cls_labels"].shape)
        per_loc = sum(int(a.shape[3]) * int(a.shape[4]) for a in anchors)
        H, W = int(anchors[0].shape[1]), int(anchors[0].shape[2])
        cfg = seq.base_cfg(B=B, N=N, num_class=num_class, code=7, bins=2, dir_offset=0.78539, cls_weight=1.0, loc_weight=2.0,
                           dir_weight=0.2)
        g = torch.Generator(device="cpu").manual_seed(7)
        preds = {k: (torch.randn((B, H, W, per_loc * c), generator=g) * s).to(dev).requires_grad_(True)
                 for k, c, s in (("cls", num_class, 3.0), ("box", 7, 0.5), ("dir", 2, 2.0))}
        head = type("Head", (), {})()
        head.model_cfg = seq.model_cfg(cfg)
        head.num_class, head.num_anchors_per_location, head.use_multihead, head.anchors = num_class, per_loc, False, anchors
        head.cls_loss_func = seq.loss_stub("SigmoidFocalClassificationLoss", alpha=0.25, gamma=2.0)
        head.reg_loss_func = seq.loss_stub("WeightedSmoothL1Loss", beta=1.0 / 9.0, code_weights=torch.ones(7, device=dev))
        head.dir_loss_func = seq.loss_stub("WeightedCrossEntropyLoss")
        head.forward_ret_dict = dict(cls_preds=preds["cls"], box_preds=preds["box"], dir_cls_preds=preds["dir"],
                                     box_cls_labels=targets["box_cls_labels"], box_reg_targets=targets["box_reg_targets"])

        def clear():
            for p in preds.values():
                p.grad = None

        def step(fn):
            clear()
            loss, tb = fn(head)
            loss.backward()
            return tb

        op = lambda: step(anchor_head_loss.get_loss)      # noqa: E731
        yard = lambda: step(yard_get_loss)                # noqa: E731
        tb_o = op()
        grads_o = {k: p.grad.clone() for k, p in preds.items()}
        tb_y = yard()
        grads_y = {k: p.grad.clone() for k, p in preds.items()}
        torch.cuda.synchronize()
        if args.once:
            continue
        inp = dict(cls=preds["cls"].detach().view(B, N, -1).cpu().numpy(), box=preds["box"].detach().view(B, N, 7).cpu().numpy(),
                   dir=preds["dir"].detach().view(B, N, 2).cpu().numpy(), labels=targets["box_cls_labels"].cpu().numpy(),
                   tg=targets["box_reg_targets"].cpu().numpy(), anchors=anchor_head_loss._flat_anchors(head).cpu().numpy(),
                   cw=np.ones(7, dtype=np.float32))
        want = seq.restate(inp, cfg)
        got = dict(losses=np.array([tb_o["rpn_loss_cls"], tb_o["rpn_loss_loc"], tb_o["rpn_loss_dir"], tb_o["rpn_loss"]], dtype=np.float32),
                   grad_cls=grads_o["cls"].view(B, N, -1).cpu().numpy(), grad_box=grads_o["box"].view(B, N, 7).cpu().numpy(),
                   grad_dir=grads_o["dir"].view(B, N, 2).cpu().numpy())
        why = seq.report(got, want, "the device")
        row = {"case": name, "anchors_per_sample": N, "positives": [int(v) for v in (targets["box_cls_labels"] > 0).sum(1).tolist()],
               "op_vs_restatement": why or "bit for bit",
               "yardstick_vs_op": {k: float(abs(tb_y[k] - tb_o[k]) / max(abs(tb_y[k]), 1e-30)) for k in tb_y} | {
                   f"grad_{k}_max_abs_diff": float((grads_y[k] - grads_o[k]).abs().max()) for k in preds} | {
                   f"grad_{k}_max_abs": float(grads_y[k].abs().max()) for k in preds}}
        assert all(v < 1e-4 for k, v in row["yardstick_vs_op"].items() if k.startswith("rpn")), row
        assert all(row["yardstick_vs_op"][f"grad_{k}_max_abs_diff"] <= 1e-4 * row["yardstick_vs_op"][f"grad_{k}_max_abs"] for k in preds), row
        row["host_synchronisations_per_step"] = {"op": atb.host_syncs(op), "yardstick": atb.host_syncs(yard)}
        row["peak_bytes_of_a_step"] = {"op": peak_bytes(op, clear), "yardstick": peak_bytes(yard, clear)}
        no, ny = calls_for(op), calls_for(yard)
        to, ty = [], []
        for _ in range(args.windows):       # alternating windows
            to.append(window(op, no))
            ty.append(window(yard, ny))
        row["op"] = dict(stats(to), calls_per_window=no)
        row["yardstick"] = dict(stats(ty), calls_per_window=ny)
        row["yardstick_over_op"] = row["yardstick"]["median_ms"] / row["op"]["median_ms"]
        print(json.dumps({k: row[k] for k in ("case", "yardstick_over_op", "host_synchronisations_per_step", "peak_bytes_of_a_step",
                                              "op_vs_restatement", "yardstick_vs_op")}
                         | {"op_ms": row["op"]["median_ms"], "yardstick_ms": row["yardstick"]["median_ms"]}), flush=True)
        rows.append(row)
    if args.once:
        return
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "window_ms_target": WINDOW_MS, "windows": args.windows,
           "method": "a step = forward, backward() and tb_dict's floats; alternating windows of steps timed with device events "
                     "ending in a synchronise; medians over the windows", "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
