"""numpy restatement of modest_post_process and of the drop-in modest_amd.utils.post_processing (csrc/post_process.hip,
DESIGN.md section 7o): Detector3DTemplate.post_processing (detector3d_template.py:175-325) over class_agnostic_nms
(model_nms_utils.py:6-25) and generate_recall_record, with MULTI_CLASSES_NMS off, the reference's loop line by line.  The
keys, the candidates and the two walks are those of tests/proposals_seq.py, the trim and the 3-D IoU those of
tests/roi_targets_seq.py.  Where the reference leaves the result open the library's rule stands: equal scores by ascending
row, the lowest class among equal maxima, and the sigmoid is the double function rounded once.

FAULTS names deliberately wrong variants; each must change the expected result of a named case of
tests/post_process_cases.py (tests/test_post_process_cpu.py holds them to that).
"""
import json

import numpy as np

import proposals_seq as ps
import roi_targets_seq as rs

F = np.float32
POST_MAX, BATCH_MAX, THRESH_MAX = ps.POST_MAX, ps.BATCH_MAX, 16      # csrc/post_process.hip

# fault -> the case of tests/post_process_cases.py whose expected result it changes
FAULTS = {
    "thresh_strict": "score equal to SCORE_THRESH",        # > where the threshold has >=
    "thresh_after_pre": "PRE cuts after the threshold",    # topk over all rows first, the threshold on what is left
    "nan_kept": "non-finite scores",                       # a NaN score passes the threshold
    "key_from_logit": "saturating logits",                 # the sort key from the logit instead of its sigmoid
    "raw_not_taken": "OUTPUT_RAW_SCORE",                   # the normalised score although OUTPUT_RAW_SCORE is set
    "label_from_argmax": "given labels",                   # argmax + 1 although labels are given
    "gt_row_0_trimmed": "all-zero gts",                    # the trim may drop row 0
    "recall_from_final": "rois present",                   # "rcnn" from the final boxes although rois are present
    "recall_ge": "recall tie",                             # >= in the recall comparison
}


def sigmoid(x):
    """torch.sigmoid by the library's rule: the double function, rounded once"""
    with np.errstate(over="ignore"):
        return np.asarray(1.0 / (1.0 + np.exp(-np.asarray(x, F).astype(np.float64)))).astype(F)


def trim(gt, fault=None):
    """valid rows of one sample's (G, 7 + C + 1) gts as generate_recall_record trims them: none of no rows, else row 0
    always stays"""
    if len(gt) == 0:
        return 0
    n = rs.trim(gt)
    if fault == "gt_row_0_trimmed" and n == 1:
        with np.errstate(all="ignore"):
            s = F(0)
            for v in np.asarray(gt[0], F):
                s = F(s + v)
        return 0 if s == 0 else 1
    return n


def recalled(boxes, gt, thresholds, fault=None):
    """per threshold the gts whose maximum 3-D IoU over `boxes` is > it: torch's max hands a NaN on, which is not recalled;
    no box, none recalled"""
    if len(boxes) == 0 or len(gt) == 0:
        return [0] * len(thresholds)
    iou = rs.iou3d(boxes[:, :7], gt[:, :7])
    with np.errstate(all="ignore"):
        best = np.max(iou, axis=0)            # numpy's max hands a NaN on, as torch's
        return [int((best >= F(t)).sum()) if fault == "recall_ge" else int((best > F(t)).sum()) for t in thresholds]


def max_iou(boxes, gt):
    """the maxima `recalled` compares, for the tests' margins"""
    with np.errstate(all="ignore"):
        return np.max(rs.iou3d(boxes[:, :7], gt[:, :7]), axis=0)


def post_process(box, cls, B, pre, post, nms_thresh, rotated=True, score_thresh=None, normalized=True,
                 output_raw_score=False, labels=None, batch_index=None, gt_boxes=None, rois=None, recall_thresh=(),
                 walk=ps.parent_walk, fault=None, **walk_kw):
    """-> (preds, recall): preds a list of B tuples (pred_boxes (n_b, 7 + C) float32, pred_scores (n_b,) float32, pred_labels
    (n_b,) int64); recall None without gt_boxes, else {"gt": int, "rcnn": [..], "roi": [..]} (roi zeros without rois)"""
    assert fault is None or fault in FAULTS, fault
    box, cls, per = ps._flat(box, cls, batch_index)
    src_max, arg = ps.score_label(cls)                       # torch.max(cls_preds, dim=-1)
    sample = ps.sample_of(batch_index, len(box), B, per)
    by_sample = np.argsort(sample, kind="stable")
    cut = np.searchsorted(sample[by_sample], np.arange(B + 1))
    given = None if labels is None else np.asarray(labels, np.int64).reshape(B, -1)
    T = len(recall_thresh)
    recall = None if gt_boxes is None else {"gt": 0, "rcnn": [0] * T, "roi": [0] * T}
    preds = []
    for index in range(B):
        rows = by_sample[cut[index]:cut[index + 1]]          # batch_mask, in row order
        box_preds, src_cls = box[rows], src_max[rows]
        cls_preds = src_cls if normalized else sigmoid(src_cls)
        label_preds = given[index] if given is not None and fault != "label_from_argmax" else arg[rows] + 1
        # class_agnostic_nms
        if score_thresh is not None:
            t = F(score_thresh)                              # torch compares a float32 tensor with the scalar in float32
            with np.errstate(invalid="ignore"):
                mask = (cls_preds > t) if fault == "thresh_strict" else (cls_preds >= t)
            if fault == "nan_kept":
                mask = mask | np.isnan(cls_preds)
        else:
            mask = np.ones(len(rows), bool)
        key = src_cls if fault == "key_from_logit" else cls_preds
        zeros = np.zeros(len(rows), np.int64)
        if fault == "thresh_after_pre":
            top = ps.candidates(key, zeros, 1, pre)[0]
            top = top[mask[top]]
        else:
            original = np.flatnonzero(mask)
            top = original[ps.candidates(key[original], zeros[:len(original)], 1, pre)[0]]      # torch.topk
        keep = walk(box_preds[top], nms_thresh, rotated, post, **walk_kw) if len(top) else np.zeros(0, np.int64)
        selected = top[keep]
        final_scores = cls_preds[selected]
        if output_raw_score and fault != "raw_not_taken":
            final_scores = src_cls[selected]
        final_boxes = box_preds[selected]
        preds.append((np.ascontiguousarray(final_boxes, F), np.ascontiguousarray(final_scores, F),
                      np.ascontiguousarray(label_preds[selected], np.int64)))
        # generate_recall_record
        if gt_boxes is not None:
            cur_gt = np.asarray(gt_boxes[index], F)
            cur_gt = cur_gt[:trim(cur_gt, fault)]
            if len(cur_gt) > 0:
                rcnn_list = final_boxes if rois is None or fault == "recall_from_final" else box_preds
                for k, v in enumerate(recalled(rcnn_list, cur_gt, recall_thresh, fault)):
                    recall["rcnn"][k] += v
                if rois is not None:
                    for k, v in enumerate(recalled(np.asarray(rois[index], F), cur_gt, recall_thresh, fault)):
                        recall["roi"][k] += v
                recall["gt"] += len(cur_gt)
    return preds, recall


def recall_dict(recall, thresh_list):
    """the reference's dict, in its key order"""
    if recall is None:
        return {}
    out = {"gt": recall["gt"]}
    for k, t in enumerate(thresh_list):
        out["roi_%s" % str(t)] = recall["roi"][k]
        out["rcnn_%s" % str(t)] = recall["rcnn"][k]
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def describe(got, want):
    """differences of (preds, recall) pairs, bit for bit"""
    out = []
    (gp, gr), (wp, wr) = got, want
    if len(gp) != len(wp):
        return [f"{len(gp)} samples against {len(wp)}"]
    for b, (g3, w3) in enumerate(zip(gp, wp)):
        for name, g, w in zip(("pred_boxes", "pred_scores", "pred_labels"), g3, w3):
            g, w = np.asarray(g), np.asarray(w)
            if g.shape != w.shape or g.dtype != w.dtype:
                out.append(f"sample {b} {name}: {g.dtype}{g.shape} against {w.dtype}{w.shape}")
                continue
            bad = np.argwhere(bits(g) != bits(w))
            if len(bad):
                i = tuple(bad[0])
                out.append(f"sample {b} {name}: {len(bad)} of {g.size} differ, first at {i}: {g[i]!r} against {w[i]!r}")
    if gr != wr:
        out.append(f"recall: {gr} against {wr}")
    return out


def same(got, want):
    return not describe(got, want)


# ------------------------------------------------------------------------------------------------ the recorded fixture
ARRAYS = ("box", "cls", "batch_index", "labels", "gt_boxes", "rois")


def scenes(rec):
    return json.loads(str(rec["scenes"]))


def scene_inputs(rec, name):
    """-> (cfg dict, {name: array or None})"""
    cfg = json.loads(str(rec[name + "_cfg"]))
    return cfg, {k: (rec[f"{name}_{k}"] if f"{name}_{k}" in rec else None) for k in ARRAYS}


def recorded(rec, name):
    """-> (preds, recall dict in the reference's form)"""
    B = json.loads(str(rec[name + "_cfg"]))["batch_size"]
    preds = [(rec[f"{name}_pred_boxes_{b}"], rec[f"{name}_pred_scores_{b}"], rec[f"{name}_pred_labels_{b}"]) for b in range(B)]
    return preds, json.loads(str(rec[name + "_recall"]))
