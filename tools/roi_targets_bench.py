#!/usr/bin/env python
"""Time modest_amd.utils.roi_targets.assign_targets (through bind()) against the path a two-stage head took before it: the
reference's RoIHeadTemplate.assign_targets over ProposalTargetLayer.forward, restated in this file over torch and this
project's own ``iou3d_nms_utils.boxes_iou3d_gpu`` shim, on the same device; writes profiles/roi_targets_bench.json
(DESIGN.md section 7n).

Three shapes: PointRCNN train (B = 4, 512 rois, 30 gts padded with 20 zero rows, M = 128, cls, by class), the same with
roi_iou and PV-RCNN's thresholds, and B = 16.  Both sides draw from the same global generators, seeded alike before the one
comparison of their outputs, which is reported, not required: the path before evaluates its trig, its division by a scalar
and its matmul with PyTorch's device kernels.

Method (tools/proposals_bench.py): both sides in this process on the same device, every shape warmed up.  Device time per
call: a window holds enough calls to last 200 ms and is timed with device events, ending in a synchronise; the two sides
alternate window by window.  Wall time per call: the host clock around one call and a synchronise, alternating, median of
50.  Host synchronisations per call: those PyTorch reports plus, for the op, the one inside modest_roi_targets_match.

    python tools/roi_targets_bench.py [--out profiles/roi_targets_bench.json] [--windows 5]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from point_targets_bench import calls_for, host_syncs, stats, wall_once, window  # noqa: E402

POINTRCNN = dict(ROI_PER_IMAGE=128, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True, CLS_SCORE_TYPE="cls", CLS_FG_THRESH=0.6,
                 CLS_BG_THRESH=0.45, CLS_BG_THRESH_LO=0.1, HARD_BG_RATIO=0.8, REG_FG_THRESH=0.55)
PVRCNN = dict(POINTRCNN, CLS_SCORE_TYPE="roi_iou", CLS_FG_THRESH=0.75, CLS_BG_THRESH=0.25)
CONFIGS = (("PointRCNN train", 4, POINTRCNN), ("PV-RCNN / PartA2 train (roi_iou)", 4, PVRCNN), ("PointRCNN train, B = 16", 16, POINTRCNN))
N_ROIS, N_GT, N_PAD = 512, 30, 20


def yard_sample_bg(hard, easy, n, ratio):
    if hard.numel() > 0 and easy.numel() > 0:
        hn = min(int(n * ratio), len(hard))
        h = hard[torch.randint(low=0, high=hard.numel(), size=(hn,)).long()]
        e = easy[torch.randint(low=0, high=easy.numel(), size=(n - hn,)).long()]
        return torch.cat([h, e], dim=0)
    src = hard if hard.numel() > 0 else easy
    return src[torch.randint(low=0, high=src.numel(), size=(n,)).long()]


def yard_assign_targets(rois, roi_scores, roi_labels, gt_boxes, cfg):
    """the path before, sample by sample and class by class -> the eight tensors"""
    from modest_amd.utils.iou3d_nms import iou3d_nms_utils
    B, M, cols = rois.shape[0], cfg["ROI_PER_IMAGE"], rois.shape[-1]
    o_rois, o_gt = rois.new_zeros(B, M, cols), rois.new_zeros(B, M, cols + 1)
    o_iou, o_scores, o_labels = rois.new_zeros(B, M), rois.new_zeros(B, M), rois.new_zeros((B, M), dtype=torch.long)
    for i in range(B):
        cur_roi, cur_gt, cur_lab = rois[i], gt_boxes[i], roi_labels[i]
        k = len(cur_gt) - 1
        while k > 0 and cur_gt[k].sum() == 0:
            k -= 1
        cur_gt = cur_gt[:k + 1]
        gt_lab = cur_gt[:, -1].long()
        best, at = cur_roi.new_zeros(cur_roi.shape[0]), cur_lab.new_zeros(cur_lab.shape[0])
        for c in range(gt_lab.min().item(), gt_lab.max().item() + 1):
            rm, gm = cur_lab == c, gt_lab == c
            if rm.sum() > 0 and gm.sum() > 0:
                origin = gm.nonzero().view(-1)
                v, a = torch.max(iou3d_nms_utils.boxes_iou3d_gpu(cur_roi[rm][:, :7], cur_gt[gm][:, :7]), dim=1)
                best[rm], at[rm] = v, origin[a]
        fg = (best >= min(cfg["REG_FG_THRESH"], cfg["CLS_FG_THRESH"])).nonzero().view(-1)
        easy = (best < cfg["CLS_BG_THRESH_LO"]).nonzero().view(-1)
        hard = ((best < cfg["REG_FG_THRESH"]) & (best >= cfg["CLS_BG_THRESH_LO"])).nonzero().view(-1)
        nf, nb = fg.numel(), hard.numel() + easy.numel()
        per = int(np.round(cfg["FG_RATIO"] * M))
        if nf > 0 and nb > 0:
            take = min(per, nf)
            fg = fg[torch.from_numpy(np.random.permutation(nf)).type_as(best).long()[:take]]
            picked = torch.cat((fg, yard_sample_bg(hard, easy, M - take, cfg["HARD_BG_RATIO"])), dim=0)
        elif nf > 0:
            picked = fg[torch.from_numpy(np.floor(np.random.rand(M) * nf)).type_as(best).long()]
        else:
            picked = yard_sample_bg(hard, easy, M, cfg["HARD_BG_RATIO"])
        o_rois[i], o_labels[i], o_iou[i], o_scores[i], o_gt[i] = cur_roi[picked], cur_lab[picked], best[picked], roi_scores[i][picked], cur_gt[at[picked]]
    reg_valid = (o_iou > cfg["REG_FG_THRESH"]).long()
    if cfg["CLS_SCORE_TYPE"] == "cls":
        cls = (o_iou > cfg["CLS_FG_THRESH"]).long()
        cls[(o_iou > cfg["CLS_BG_THRESH"]) & (o_iou < cfg["CLS_FG_THRESH"])] = -1
    else:
        fgm, bgm = o_iou > cfg["CLS_FG_THRESH"], o_iou < cfg["CLS_BG_THRESH"]
        mid = (fgm == 0) & (bgm == 0)
        cls = (fgm > 0).float()
        cls[mid] = (o_iou[mid] - cfg["CLS_BG_THRESH"]) / (cfg["CLS_FG_THRESH"] - cfg["CLS_BG_THRESH"])
    src = o_gt.clone()
    ry = o_rois[:, :, 6] % (2 * np.pi)
    o_gt[:, :, 0:3] = o_gt[:, :, 0:3] - o_rois[:, :, 0:3]
    o_gt[:, :, 6] = o_gt[:, :, 6] - ry
    a = -ry.view(-1)
    cosa, sina, zeros, ones = torch.cos(a), torch.sin(a), a.new_zeros(a.shape[0]), a.new_ones(a.shape[0])
    rot = torch.stack((cosa, sina, zeros, -sina, cosa, zeros, zeros, zeros, ones), dim=1).view(-1, 3, 3)
    flat = o_gt.view(-1, 1, cols + 1)
    o_gt = torch.cat((torch.matmul(flat[:, :, 0:3], rot), flat[:, :, 3:]), dim=-1).view(B, -1, cols + 1)
    h = o_gt[:, :, 6] % (2 * np.pi)
    opp = (h > np.pi * 0.5) & (h < np.pi * 1.5)
    h[opp] = (h[opp] + np.pi) % (2 * np.pi)
    h[h > np.pi] = h[h > np.pi] - np.pi * 2
    o_gt[:, :, 6] = torch.clamp(h, min=-np.pi / 2, max=np.pi / 2)
    return {"rois": o_rois, "gt_of_rois": o_gt, "gt_iou_of_rois": o_iou, "roi_scores": o_scores, "roi_labels": o_labels,
            "reg_valid_mask": reg_valid, "rcnn_cls_labels": cls, "gt_of_rois_src": src}


def inputs(B, seed):
    """B samples: 30 gts of classes 1 - 3 in a 70 m x 80 m scene padded with 20 zero rows; 512 rois, moved copies of the gts
    at three distances (a third near, a third half a metre off, a third well off)"""
    rng = np.random.default_rng(seed)
    gt = np.zeros((B, N_GT + N_PAD, 8), np.float32)
    rois = np.zeros((B, N_ROIS, 7), np.float32)
    labels = np.zeros((B, N_ROIS), np.int64)
    for b in range(B):
        g = np.c_[rng.uniform(0, 70, N_GT), rng.uniform(-40, 40, N_GT), rng.uniform(-1.5, 0, N_GT), rng.uniform(3.2, 4.8, N_GT),
                  rng.uniform(1.5, 2.0, N_GT), rng.uniform(1.4, 1.7, N_GT), rng.uniform(-3.2, 3.2, N_GT), rng.integers(1, 4, N_GT)]
        gt[b, :N_GT] = g
        k = rng.integers(0, N_GT, N_ROIS)
        p = g[k, :7].copy()
        p[:, :2] += rng.normal(0, 1, (N_ROIS, 2)) * rng.choice([0.08, 0.45, 1.5], N_ROIS)[:, None]
        p[:, 3:6] *= rng.normal(1, 0.04, (N_ROIS, 3))
        p[:, 6] += rng.normal(0, 0.06, N_ROIS) + np.pi * (rng.random(N_ROIS) < 0.2)
        rois[b], labels[b] = p, g[k, 7]
    return rois, rng.random((B, N_ROIS)).astype(np.float32), labels, gt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roi_targets_bench.json"))
    ap.add_argument("--windows", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/roi_targets_bench.py needs an MI355X: there is no CPU path")
    from modest_amd.utils import roi_targets as rt
    dev = torch.device("cuda:0")
    rows = []
    for name, B, cfg in CONFIGS:
        r, s, l, g = (torch.from_numpy(a).to(dev) for a in inputs(B, 40 + B))
        head = rt.bind(type("RoIHead", (), {}))()
        head.model_cfg = types.SimpleNamespace(TARGET_CONFIG=types.SimpleNamespace(**cfg))

        def op():
            return head.assign_targets(dict(batch_size=B, rois=r, roi_scores=s, roi_labels=l, gt_boxes=g))

        def yard():
            return yard_assign_targets(r, s, l, g, cfg)

        np.random.seed(1), torch.manual_seed(2)
        got = op()
        np.random.seed(1), torch.manual_seed(2)
        ref = yard()
        torch.cuda.synchronize()
        view = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t      # noqa: E731
        equal = {k: bool(torch.equal(view(got[k]), view(ref[k]))) for k in got}
        differing = {k: int((view(got[k]) != view(ref[k])).sum()) for k in got if not equal[k]}
        row = {"case": name, "batch": B, "rois_per_sample": N_ROIS, "gts": N_GT, "zero_rows": N_PAD, "roi_per_image": cfg["ROI_PER_IMAGE"],
               "score_type": cfg["CLS_SCORE_TYPE"], "outputs_equal_bit_for_bit": equal, "elements_differing": differing,
               "host_synchronisations_per_call": {"op": host_syncs(op) + 1, "yardstick": host_syncs(yard)}}
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
        print(json.dumps(row), flush=True)
        rows.append(row)
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "window_ms_target": 200.0, "windows": args.windows,
           "method": "device: alternating windows of calls timed with device events ending in a synchronise; wall: host clock "
                     "around one call and a synchronise, alternating, 50 each; medians with their ranges", "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
