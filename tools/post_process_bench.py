#!/usr/bin/env python
"""Time modest_amd.utils.post_processing.post_processing against the path a detector took before it: the reference's
Detector3DTemplate.post_processing over class_agnostic_nms and generate_recall_record, restated in this file over torch and
this project's own ``iou3d_nms_utils`` shims as they were (nms_gpu: tile mask on the device, walk on the host;
boxes_iou3d_gpu), on the same device; writes profiles/post_process_bench.json.

Three shapes at B = 4, taken from the reference's configs:
  PointRCNN test      dense 4 x 100 rois, K = 1 raw logits, roi_labels and rois given, 30 gts of 40 rows,
                      SCORE_THRESH 0.1, NMS 0.1 / 4096 / 500 (kitti_models/pointrcnn.yaml);
  PointPillars        dense 4 x 138 880 anchors (lyft_models/pointpillar_dynamic_obj.yaml: 280 x 248 cells, 2 rotations),
                      K = 3 raw logits, 30 gts, SCORE_THRESH 0.1, NMS 0.01 / 4096 / 500: about 660 rows a sample pass;
  PointPillars PRE    the same with SCORE_THRESH 0.001: about 13 000 rows a sample pass and NMS_PRE_MAXSIZE = 4096 binds.
Boxes are clustered like tests/iou3d_cases.py:proposals.  The logits are pairwise distinct and their sigmoids at least
fifty float32 steps apart, so torch's float32 sigmoid (the path before) and the double rule (the op) rank alike: boxes,
labels, counts and the recall dict must be equal bit for bit, which is checked and recorded (results_equal) before any
time is reported; the largest distance of two scores is recorded in ulp (scores_ulp).

Method (tools/proposals_bench.py): both sides in this process on the same device, every shape warmed up.  Device time per
call: a window holds enough calls to last 200 ms and is timed with device events, ending in a synchronise; the two sides
alternate window by window; median of 5 with range.  Wall time per call: the host clock around one call and a synchronise,
alternating, median of 50.  Host synchronisations per call: those PyTorch reports (`torch.cuda.set_sync_debug_mode("warn")`)
plus the ones inside the library that PyTorch cannot see: one per nms_gpu call for the path before, the one stream
synchronise of modest_post_process for the op.

    python tools/post_process_bench.py [--out profiles/post_process_bench.json] [--windows 5] [--once]
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

B = 4
ANCHORS = 280 * 248 * 2      # lyft_models/pointpillar_dynamic_obj.yaml: range 89.6 x 79.36 m, voxel 0.16, stride 2, 2 rotations
RECALL = [0.3, 0.5, 0.7]
CONFIGS = (
    # name, rows per sample, K, score threshold, NMS threshold, two-stage
    ("PointRCNN test", 100, 1, 0.1, 0.1, True),
    ("PointPillars", ANCHORS, 3, 0.1, 0.01, False),
    ("PointPillars PRE binds", ANCHORS, 3, 0.001, 0.01, False),
)
PRE, POST = 4096, 500


def yard_post_processing(d, cfg, num_class):
    """the reference's loop (detector3d_template.py:175-325, model_nms_utils.py:6-25) over the shims
    -> pred_dicts, recall_dict, nms calls"""
    from modest_amd.utils.iou3d_nms import iou3d_nms_utils
    nms_cfg = cfg.NMS_CONFIG
    recall_dict, pred_dicts, calls = {}, [], 0
    for index in range(d['batch_size']):
        box_preds = d['batch_box_preds'][index]
        src_box_preds = box_preds
        cls_preds = d['batch_cls_preds'][index]
        src_cls_preds = cls_preds
        assert cls_preds.shape[1] in [1, num_class]
        if not d['cls_preds_normalized']:
            cls_preds = torch.sigmoid(cls_preds)
        cls_preds, label_preds = torch.max(cls_preds, dim=-1)
        if d.get('has_class_labels', False):
            label_preds = d['roi_labels'][index]
        else:
            label_preds = label_preds + 1
        # class_agnostic_nms
        box_scores, boxes = cls_preds, box_preds
        scores_mask = (box_scores >= cfg.SCORE_THRESH)
        box_scores, boxes = box_scores[scores_mask], boxes[scores_mask]
        selected = []
        if box_scores.shape[0] > 0:
            top, indices = torch.topk(box_scores, k=min(nms_cfg.NMS_PRE_MAXSIZE, box_scores.shape[0]))
            keep, _ = iou3d_nms_utils.nms_gpu(boxes[indices][:, 0:7], top, nms_cfg.NMS_THRESH)
            calls += 1
            selected = indices[keep[:nms_cfg.NMS_POST_MAXSIZE]]
        selected = scores_mask.nonzero().view(-1)[selected]
        final_scores, final_labels, final_boxes = cls_preds[selected], label_preds[selected], box_preds[selected]
        # generate_recall_record
        if 'gt_boxes' in d:
            rois = d['rois'][index] if 'rois' in d else None
            rcnn = final_boxes if rois is None else src_box_preds
            if not recall_dict:
                recall_dict = {'gt': 0}
                for t in cfg.RECALL_THRESH_LIST:
                    recall_dict['roi_%s' % str(t)] = 0
                    recall_dict['rcnn_%s' % str(t)] = 0
            cur_gt = d['gt_boxes'][index]
            k = cur_gt.__len__() - 1
            while k > 0 and cur_gt[k].sum() == 0:
                k -= 1
            cur_gt = cur_gt[:k + 1]
            if cur_gt.shape[0] > 0:
                iou3d_rcnn = iou3d_nms_utils.boxes_iou3d_gpu(rcnn[:, 0:7], cur_gt[:, 0:7]) if rcnn.shape[0] > 0 else torch.zeros((0, cur_gt.shape[0]))
                if rois is not None:
                    iou3d_roi = iou3d_nms_utils.boxes_iou3d_gpu(rois[:, 0:7], cur_gt[:, 0:7])
                for t in cfg.RECALL_THRESH_LIST:
                    if iou3d_rcnn.shape[0] > 0:
                        recall_dict['rcnn_%s' % str(t)] += (iou3d_rcnn.max(dim=0)[0] > t).sum().item()
                    if rois is not None:
                        recall_dict['roi_%s' % str(t)] += (iou3d_roi.max(dim=0)[0] > t).sum().item()
                recall_dict['gt'] += cur_gt.shape[0]
        pred_dicts.append({'pred_boxes': final_boxes, 'pred_scores': final_scores, 'pred_labels': final_labels})
    return pred_dicts, recall_dict, calls


def inputs(n_per, K, seed):
    """B samples of n_per clustered boxes (jittered copies of max(30, n_per / 128) objects in a 70 m x 80 m scene, a fifth
    turned by pi); K raw class values per row, the row maxima pairwise distinct, dense towards low scores (the fourth root
    spreads 0.5 % of the rows above sigmoid 0.1 and 10 % above 0.001); 30 gts of 40 rows near the first objects"""
    rng = np.random.default_rng(seed)
    box = np.zeros((B, n_per, 7), np.float32)
    gt = np.zeros((B, 40, 8), np.float32)
    for b in range(B):
        nobj = max(30, n_per // 128)
        obj = np.c_[rng.uniform(0, 70, nobj), rng.uniform(-40, 40, nobj), rng.uniform(-1.5, 0, nobj), rng.uniform(3.2, 4.8, nobj),
                    rng.uniform(1.5, 2.0, nobj), rng.uniform(1.4, 1.7, nobj), rng.uniform(-3.2, 3.2, nobj)]
        p = obj[rng.integers(0, nobj, n_per)]
        p[:, :2] += rng.normal(0, 0.25, (n_per, 2))
        p[:, 3:5] *= rng.normal(1, 0.06, (n_per, 2))
        p[:, 6] += rng.normal(0, 0.08, n_per) + np.pi * (rng.random(n_per) < 0.2)
        box[b] = p
        g = obj[:30].copy()
        g[:, :2] += rng.normal(0, 0.3, (30, 2))
        gt[b, :30, :7], gt[b, :30, 7] = g, rng.integers(1, 4, 30)
    total = B * n_per
    u = (rng.permutation(total) + 0.5) / total
    top = (2.0 - 16.0 * u ** 0.25).astype(np.float32).reshape(B, n_per) if n_per > 1000 else (8.0 * u - 4.0).astype(np.float32).reshape(B, n_per)
    assert len(np.unique(top)) == total
    cls = np.stack([top - np.float32(1.5 * k) for k in range(K)], 2)
    if K > 1:      # the maximum in a column of its own per row
        shift = rng.integers(0, K, (B, n_per))
        cls = np.take_along_axis(cls, (np.arange(K)[None, None, :] + shift[..., None]) % K, 2)
    return box, np.ascontiguousarray(cls, np.float32), gt


def equal_results(got, ref):
    """-> (boxes, labels, counts and recall equal bit for bit, the largest distance of two scores in ulp: torch's float32
    sigmoid on the device against the double rule)"""
    (gp, gr), (rp, rr) = got, ref
    if gr != rr or list(gr) != list(rr) or len(gp) != len(rp):
        return False, 0
    worst = 0
    for g, r in zip(gp, rp):
        if g['pred_boxes'].shape != r['pred_boxes'].shape or not torch.equal(g['pred_boxes'].view(torch.int32), r['pred_boxes'].view(torch.int32)):
            return False, 0
        if not torch.equal(g['pred_labels'], r['pred_labels'].reshape(-1)):
            return False, 0
        if len(g['pred_scores']):
            worst = max(worst, int((g['pred_scores'].view(torch.int32) - r['pred_scores'].view(torch.int32)).abs().max()))
    return True, worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "post_process_bench.json"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--once", action="store_true", help="call each side a few times and exit (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/post_process_bench.py needs an MI355X: there is no CPU path")
    from modest_amd.utils import post_processing as pp
    dev = torch.device("cuda:0")
    rows, made = [], {}
    for name, n_per, K, score_thresh, nms_thresh, two_stage in CONFIGS:
        if (n_per, K) not in made:
            made[(n_per, K)] = inputs(n_per, K, 17 + n_per)
        box_np, cls_np, gt_np = made[(n_per, K)]
        box, cls, gt = (torch.from_numpy(a).to(dev) for a in (box_np, cls_np, gt_np))
        batch = dict(batch_size=B, batch_box_preds=box, batch_cls_preds=cls, cls_preds_normalized=False, gt_boxes=gt)
        if two_stage:
            rng = np.random.default_rng(5)
            rois = box_np.copy()
            rois[..., :2] += rng.normal(0, 0.1, rois[..., :2].shape).astype(np.float32)
            batch.update(rois=torch.from_numpy(rois).to(dev), has_class_labels=True,
                         roi_labels=torch.from_numpy(rng.integers(1, 4, (B, n_per))).to(dev))
        post_cfg = types.SimpleNamespace(RECALL_THRESH_LIST=RECALL, SCORE_THRESH=score_thresh, OUTPUT_RAW_SCORE=False,
                                         NMS_CONFIG=types.SimpleNamespace(MULTI_CLASSES_NMS=False, NMS_TYPE="nms_gpu", NMS_THRESH=nms_thresh,
                                                                          NMS_PRE_MAXSIZE=PRE, NMS_POST_MAXSIZE=POST))
        det = pp.bind(type("Detector", (), {}))()
        det.model_cfg, det.num_class = types.SimpleNamespace(POST_PROCESSING=post_cfg), 3

        def op():
            return det.post_processing(dict(batch))

        def yard():
            return yard_post_processing(dict(batch), post_cfg, 3)

        got, ref = op(), yard()
        torch.cuda.synchronize()
        if args.once:
            continue
        same, ulp = equal_results(got, ref[:2])
        sig = torch.sigmoid(cls.max(-1)[0])
        passing = [int(v) for v in (sig >= score_thresh).sum(1).tolist()]
        row = {"case": name, "rows_per_sample": n_per, "batch": B, "K": K, "score_thresh": score_thresh, "nms_thresh": nms_thresh,
               "pre": PRE, "post": POST, "passing_per_sample": passing, "final_per_sample": [len(p['pred_boxes']) for p in got[0]],
               "recall": got[1], "results_equal": bool(same), "scores_ulp": ulp,
               "host_synchronisations_per_call": {"op": host_syncs(op) + 1, "yardstick": host_syncs(yard) + ref[2]}}
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
        print(json.dumps({k: row[k] for k in ("case", "passing_per_sample", "final_per_sample", "results_equal", "scores_ulp",
                                              "host_synchronisations_per_call", "op", "yardstick", "yardstick_over_op")}), flush=True)
        rows.append(row)
    if args.once:
        return
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "window_ms_target": 200.0, "windows": args.windows,
           "method": "device: alternating windows of calls timed with device events ending in a synchronise; wall: host clock "
                     "around one call and a synchronise, alternating, 50 each; medians", "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
