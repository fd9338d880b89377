"""The refusals of the detector ops of ``modest_amd.ops`` -- anchor_targets, point_targets, proposals, roi_targets*, post_process,
the three head losses with their backward calls, the three decodes -- pinned call by call: for each bad call the exception
TYPE, its full TEXT, and, where a call is bad in two ways, WHICH argument is refused first.  One table; a call of the "cpu" part
is refused on host tensors or non-tensors at the first check, a call of the "gpu" part on the smallest device tensors that reach
its check.  Every call is refused before any kernel is launched.  Not in the table: what needs two devices (the "is on ..., ...
on ..." texts) and the texts other test files already pin with ``match=``."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from modest_amd import ops  # noqa: E402
from modest_amd._lib import ModestHipError  # noqa: E402

F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
DEVICE = "must be a device tensor (PyTorch-ROCm 'cuda')"
HOST = torch.device("cpu")


def z(d, *shape, dtype=F32):
    return torch.zeros(shape, dtype=dtype, device=d)


def cfg(**kw):
    base = dict(ROI_PER_IMAGE=2, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True, CLS_SCORE_TYPE="roi_iou", CLS_FG_THRESH=0.75,
                CLS_BG_THRESH=0.25, CLS_BG_THRESH_LO=0.1, HARD_BG_RATIO=0.8, REG_FG_THRESH=0.55)
    base.update(kw)
    return base


# ---- the good arguments of each op on device d, as a dict by parameter name; a case replaces some of them
def anchor_targets(d, **kw):
    a = dict(gt=z(d, 1, 2, 8), anchors=z(d, 4, 7), cls_table=z(d, 1, 5, dtype=I64), thresholds=z(d, 1, 2),
             name_match=z(d, 1, 1, dtype=U8), max_cls_rows=4, n_out=4)
    a.update(kw)
    return ops.anchor_targets(**a)


def point_targets(d, **kw):
    a = dict(points=z(d, 2, 4), gt_boxes=z(d, 1, 1, 8), extend_gt_boxes=z(d, 1, 1, 8), num_class=1)
    a.update(kw)
    return ops.point_targets(**a)


def proposals(d, **kw):
    a = dict(box_preds=z(d, 1, 2, 7), cls_preds=z(d, 1, 2, 1), batch_size=1, pre_maxsize=2, post_maxsize=2, thresh=0.5)
    a.update(kw)
    return ops.proposals(**a)


def post_process(d, **kw):
    a = dict(box_preds=z(d, 1, 2, 7), cls_preds=z(d, 1, 2, 1), batch_size=1, pre_maxsize=2, post_maxsize=2, nms_thresh=0.5)
    a.update(kw)
    return ops.post_process(**a)


def stacked(d, **kw):
    a = dict(box_preds=z(d, 2, 7), cls_preds=z(d, 2, 1), batch_index=z(d, 2))
    a.update(kw)
    return a


def roi_targets(d, cfg_=None, **kw):
    a = dict(rois=z(d, 1, 2, 7), roi_scores=z(d, 1, 2), roi_labels=z(d, 1, 2, dtype=I64), gt_boxes=z(d, 1, 1, 8))
    a.update(kw)
    return ops.roi_targets(a["rois"], a["roi_scores"], a["roi_labels"], a["gt_boxes"], cfg() if cfg_ is None else cfg_)


def roi_targets_match(d, **kw):
    a = dict(rois=z(d, 1, 2, 7), roi_labels=z(d, 1, 2, dtype=I64), gt_boxes=z(d, 1, 1, 8), fg_thresh=0.55, bg_thresh_lo=0.1,
             reg_fg_thresh=0.55, by_class=True, workspace=z(d, 1 << 16, dtype=U8), counts_pinned=z(HOST, 16, dtype=I32))
    a.update(kw)
    return ops.roi_targets_match(**a)


def roi_targets_sample(d, **kw):
    a = dict(picks=z(d, 1, 2, 2, dtype=I32), rois=z(d, 1, 2, 7), roi_scores=z(d, 1, 2), roi_labels=z(d, 1, 2, dtype=I64),
             gt_boxes=z(d, 1, 1, 8), reg_fg_thresh=0.55, cls_fg_thresh=0.75, cls_bg_thresh=0.25, score_type="roi_iou",
             workspace=z(d, 1 << 16, dtype=U8))
    a.update(kw)
    return ops.roi_targets_sample(**a)


def anchor_loss(d, **kw):
    a = dict(cls_preds=z(d, 1, 2, 1), box_preds=z(d, 1, 2, 7), dir_preds=None, labels=z(d, 1, 2, dtype=I32),
             reg_targets=z(d, 1, 2, 7), anchors=z(d, 2, 7), code_weights=z(d, 7))
    a.update(kw)
    return ops.anchor_loss(**a)


def roi_loss(d, **kw):
    a = dict(rcnn_cls=z(d, 2), rcnn_reg=z(d, 2, 7), rcnn_cls_labels=z(d, 2, dtype=I64), reg_valid_mask=z(d, 2, dtype=I64),
             gt_of_rois=z(d, 2, 8), gt_of_rois_src=z(d, 2, 8), rois=z(d, 2, 7), code_weights=z(d, 7))
    a.update(kw)
    return ops.roi_loss(**a)


def point_loss(d, **kw):
    a = dict(cls_preds=z(d, 2, 1), labels=z(d, 2, dtype=I64))
    a.update(kw)
    return ops.point_loss(**a)


def anchor_decode(d, **kw):
    a = dict(box_preds=z(d, 1, 2, 7), anchors=z(d, 2, 7))
    a.update(kw)
    return ops.anchor_decode(**a)


def point_decode(d, **kw):
    a = dict(point_box_preds=z(d, 2, 8), points=z(d, 2, 3), point_cls_preds=z(d, 2, 1))
    a.update(kw)
    return ops.point_decode(**a)


def roi_decode(d, **kw):
    a = dict(rois=z(d, 2, 7), box_preds=z(d, 2, 7))
    a.update(kw)
    return ops.roi_decode(**a)


WS_TEXT = "workspace must be torch.uint8, got torch.float32"


def big_f32(d):
    """a float32 tensor with more elements than any of these calls needs bytes: large enough to be kept, and so to be refused"""
    return z(d, 1 << 20)


# (part, name, call(d), exception type, full text); "{d}" in a text is the device's name
CASES = [
    # ------------------------------------------------------------------------------------------------ anchor_targets
    ("cpu", "anchor_targets: gt on the host", lambda d: anchor_targets(HOST), ValueError, "gt must be a (B, M, 8 + C) float32 device tensor"),
    ("gpu", "anchor_targets: gt float64", lambda d: anchor_targets(d, gt=z(d, 1, 2, 8, dtype=F64)), ValueError,
     "gt must be a (B, M, 8 + C) float32 device tensor"),
    ("gpu", "anchor_targets: anchors on the host", lambda d: anchor_targets(d, anchors=z(HOST, 4, 7), cls_table=z(d, 1, 5, dtype=I32)),
     ValueError, f"anchors {DEVICE}"),
    ("gpu", "anchor_targets: cls_table int32", lambda d: anchor_targets(d, cls_table=z(d, 1, 5, dtype=I32), thresholds=z(HOST, 1, 2)),
     TypeError, "cls_table must be torch.int64, got torch.int32"),
    ("gpu", "anchor_targets: anchors of 6 columns", lambda d: anchor_targets(d, anchors=z(d, 4, 6)), ValueError,
     "anchors has shape (4, 6) and gt (1, 2, 8): expected (N, 7 + Ca) and (B, M, 7 + Cg + 1)"),
    ("gpu", "anchor_targets: tables disagree", lambda d: anchor_targets(d, thresholds=z(d, 2, 2)), ValueError,
     "cls_table (n_cls, 5), thresholds (n_cls, 2) and name_match (n_cls, n_names) disagree"),
    ("gpu", "anchor_targets: out of two", lambda d: anchor_targets(d, out=(z(d, 1, 4, dtype=I32), z(d, 1, 4, 7))), ValueError,
     "out must be (labels, targets, weights)"),
    ("gpu", "anchor_targets: out labels int64", lambda d: anchor_targets(d, out=(z(d, 1, 4, dtype=I64), z(d, 1, 4, 8), z(d, 1, 4))),
     TypeError, "out labels must be torch.int32, got torch.int64"),
    ("gpu", "anchor_targets: out labels on the host", lambda d: anchor_targets(d, out=(z(HOST, 1, 4, dtype=I32), z(d, 1, 4, 7), z(d, 1, 4))),
     ValueError, f"out labels {DEVICE}"),
    ("gpu", "anchor_targets: out targets shape", lambda d: anchor_targets(d, out=(z(d, 1, 4, dtype=I32), z(d, 1, 4, 8), z(d, 1, 5))),
     ValueError, "out targets has shape (1, 4, 8), expected (1, 4, 7)"),
    ("gpu", "anchor_targets: workspace float32", lambda d: anchor_targets(d, workspace=big_f32(d)), TypeError, WS_TEXT),
    # ------------------------------------------------------------------------------------------------ point_targets
    ("cpu", "point_targets: points None", lambda d: point_targets(HOST, points=None), ValueError, f"points {DEVICE}"),
    ("cpu", "point_targets: points on the host", lambda d: point_targets(HOST), ValueError, f"points {DEVICE}"),
    ("gpu", "point_targets: points float64 before gt_boxes on the host", lambda d: point_targets(d, points=z(d, 2, 4, dtype=F64), gt_boxes=z(HOST, 1, 1, 8)),
     ValueError, "points must be float32, got torch.float64"),
    ("gpu", "point_targets: gt_boxes on the host", lambda d: point_targets(d, gt_boxes=z(HOST, 1, 1, 8)), ValueError, f"gt_boxes {DEVICE}"),
    ("gpu", "point_targets: extend_gt_boxes float64", lambda d: point_targets(d, extend_gt_boxes=z(d, 1, 1, 8, dtype=F64)), ValueError,
     "extend_gt_boxes must be float32, got torch.float64"),
    ("gpu", "point_targets: points of 3 columns", lambda d: point_targets(d, points=z(d, 2, 3)), ValueError, "points has shape (2, 3), expected (N, 4)"),
    ("gpu", "point_targets: boxes disagree", lambda d: point_targets(d, extend_gt_boxes=z(d, 1, 2, 8)), ValueError,
     "gt_boxes has shape (1, 1, 8) and extend_gt_boxes (1, 2, 8): expected (B, M, 8) twice"),
    ("gpu", "point_targets: mean_size on the host", lambda d: point_targets(d, mean_size=z(HOST, 1, 3)), ValueError,
     "mean_size must be a device tensor on the points' device"),
    ("gpu", "point_targets: mean_size of 2 columns", lambda d: point_targets(d, mean_size=z(d, 1, 2)), ValueError,
     "mean_size must be a contiguous (n_cls, 3) float32 tensor with n_cls >= 1"),
    ("gpu", "point_targets: num_class 0", lambda d: point_targets(d, num_class=0), ValueError, "num_class is 0"),
    ("gpu", "point_targets: out of two", lambda d: point_targets(d, out=(z(d, 2, dtype=I64), None)), ValueError,
     "out must be (point_cls_labels, point_box_labels, point_part_labels)"),
    ("gpu", "point_targets: out box not asked for", lambda d: point_targets(d, out=(z(d, 2, dtype=I64), z(d, 2, 8), None)), ValueError,
     "out point_box_labels is given but not asked for"),
    ("gpu", "point_targets: out box missing", lambda d: point_targets(d, want_box=True, out=(z(d, 2, dtype=I64), None, None)), ValueError,
     "out point_box_labels is missing"),
    ("gpu", "point_targets: out box shape before part missing", lambda d: point_targets(d, want_box=True, want_part=True, out=(z(d, 2, dtype=I64), z(d, 2, 7), None)),
     ValueError, "out point_box_labels has shape (2, 7), expected (2, 8)"),
    ("gpu", "point_targets: out labels int32", lambda d: point_targets(d, out=(z(d, 2, dtype=I32), None, None)), TypeError,
     "out point_cls_labels must be torch.int64, got torch.int32"),
    ("gpu", "point_targets: out labels shape", lambda d: point_targets(d, out=(z(d, 3, dtype=I64), None, None)), ValueError,
     "out point_cls_labels has shape (3,), expected (2,)"),
    # ------------------------------------------------------------------------------------------------ proposals
    ("cpu", "proposals: box_preds None", lambda d: proposals(HOST, box_preds=None), ValueError, f"box_preds {DEVICE}"),
    ("cpu", "proposals: box_preds on the host", lambda d: proposals(HOST), ValueError, f"box_preds {DEVICE}"),
    ("gpu", "proposals: box_preds float64 before cls_preds on the host", lambda d: proposals(d, box_preds=z(d, 1, 2, 7, dtype=F64), cls_preds=z(HOST, 1, 2, 1)),
     ValueError, "box_preds must be float32, got torch.float64"),
    ("gpu", "proposals: cls_preds on the host", lambda d: proposals(d, cls_preds=z(HOST, 1, 2, 1)), ValueError, f"cls_preds {DEVICE}"),
    ("gpu", "proposals: cls_preds float64", lambda d: proposals(d, cls_preds=z(d, 1, 2, 1, dtype=F64)), ValueError,
     "cls_preds must be float32, got torch.float64"),
    ("gpu", "proposals: dense form", lambda d: proposals(d, batch_size=2), ValueError,
     "dense form: box_preds (1, 2, 7) and cls_preds (1, 2, 1) must be (batch_size = 2, N, 7 + C) and (batch_size, N, K)"),
    ("gpu", "proposals: stacked form", lambda d: proposals(d, **stacked(d, batch_index=z(d, 3))), ValueError,
     "stacked form: box_preds (2, 7), cls_preds (2, 1) and batch_index must be (N, 7 + C), (N, K) and (N)"),
    ("gpu", "proposals: batch_index a list", lambda d: proposals(d, **stacked(d, batch_index=[0, 0])), ValueError,
     "stacked form: box_preds (2, 7), cls_preds (2, 1) and batch_index must be (N, 7 + C), (N, K) and (N)"),
    ("gpu", "proposals: 6 columns", lambda d: proposals(d, box_preds=z(d, 1, 2, 6), post_maxsize=-1), ValueError,
     "box_preds needs 7 + C columns and cls_preds K >= 1, got 6 and 1"),
    ("gpu", "proposals: stacked, no class column", lambda d: proposals(d, **stacked(d, cls_preds=z(d, 2, 0))), ValueError,
     "box_preds needs 7 + C columns and cls_preds K >= 1, got 7 and 0"),
    ("gpu", "proposals: negative post_maxsize", lambda d: proposals(d, post_maxsize=-1, out=()), ValueError,
     "batch_size, pre_maxsize and post_maxsize must not be negative"),
    ("gpu", "proposals: negative pre_maxsize", lambda d: proposals(d, pre_maxsize=-1), ValueError,
     "batch_size, pre_maxsize and post_maxsize must not be negative"),
    ("gpu", "proposals: out of two", lambda d: proposals(d, out=(z(d, 1, 2, 7), z(d, 1, 2)), workspace=big_f32(d)), ValueError,
     "out must be (rois, roi_scores, roi_labels)"),
    ("gpu", "proposals: out roi_labels int32", lambda d: proposals(d, out=(z(d, 1, 2, 7), z(d, 1, 2), z(d, 1, 2, dtype=I32))), TypeError,
     "out roi_labels must be torch.int64, got torch.int32"),
    ("gpu", "proposals: out rois shape before roi_scores float64", lambda d: proposals(d, out=(z(d, 1, 3, 7), z(d, 1, 2, dtype=F64), z(d, 1, 2, dtype=I64))),
     ValueError, "out rois has shape (1, 3, 7), expected (1, 2, 7)"),
    ("gpu", "proposals: out roi_scores on the host", lambda d: proposals(d, out=(z(d, 1, 2, 7), z(HOST, 1, 2), z(d, 1, 2, dtype=I64))),
     ValueError, f"out roi_scores {DEVICE}"),
    ("gpu", "proposals: workspace float32", lambda d: proposals(d, workspace=big_f32(d)), TypeError, WS_TEXT),
    # ------------------------------------------------------------------------------------------------ roi_targets*
    ("cpu", "roi_targets: rois on the host", lambda d: roi_targets(HOST), ValueError, f"rois {DEVICE}"),
    ("cpu", "roi_targets: rois None", lambda d: roi_targets(HOST, rois=None), ValueError, f"rois {DEVICE}"),
    ("gpu", "roi_targets: roi_labels on the host", lambda d: roi_targets(d, roi_labels=z(HOST, 1, 2, dtype=I64), gt_boxes=None), ValueError,
     f"roi_labels {DEVICE}"),
    ("gpu", "roi_targets: gt_boxes on the host", lambda d: roi_targets(d, gt_boxes=z(HOST, 1, 1, 8)), ValueError, f"gt_boxes {DEVICE}"),
    ("gpu", "roi_targets: shapes", lambda d: roi_targets(d, roi_scores=z(d, 1, 3)), ValueError,
     "rois (1, 2, 7), roi_scores (1, 3), roi_labels (1, 2) and gt_boxes (1, 1, 8) must be (B, N, 7 + C), (B, N), (B, N) and (B, G, 7 + C + 1)"),
    ("gpu", "roi_targets: CLS_SCORE_TYPE", lambda d: roi_targets(d, cfg(CLS_SCORE_TYPE="x")), NotImplementedError, "CLS_SCORE_TYPE 'x'"),
    ("gpu", "roi_targets_match: rois float64", lambda d: roi_targets_match(d, rois=z(d, 1, 2, 7, dtype=F64)), TypeError,
     "rois must be torch.float32, got torch.float64"),
    ("gpu", "roi_targets_match: gt_boxes float64", lambda d: roi_targets_match(d, gt_boxes=z(d, 1, 1, 8, dtype=F64)), ValueError,
     "gt_boxes must be a float32 device tensor"),
    ("gpu", "roi_targets_match: counts not pinned", lambda d: roi_targets_match(d), ValueError,
     "counts_pinned must be a pinned int32 tensor of at least 3 * B words"),
    ("gpu", "roi_targets_sample: picks", lambda d: roi_targets_sample(d, picks=z(d, 1, 2, 2, dtype=I64)), ValueError,
     "picks must be a contiguous (B, M, 2) int32 tensor in pinned host or device memory"),
    ("gpu", "roi_targets_sample: score type", lambda d: roi_targets_sample(d, score_type="x"), NotImplementedError, "CLS_SCORE_TYPE 'x'"),
    ("gpu", "roi_targets_sample: roi_scores float64", lambda d: roi_targets_sample(d, roi_scores=z(d, 1, 2, dtype=F64)), TypeError,
     "roi_scores must be torch.float32, got torch.float64"),
    # ------------------------------------------------------------------------------------------------ post_process
    ("cpu", "post_process: box_preds None", lambda d: post_process(HOST, box_preds=None), ValueError, f"box_preds {DEVICE}"),
    ("cpu", "post_process: box_preds on the host", lambda d: post_process(HOST), ValueError, f"box_preds {DEVICE}"),
    ("gpu", "post_process: box_preds float64 before cls_preds on the host", lambda d: post_process(d, box_preds=z(d, 1, 2, 7, dtype=F64), cls_preds=z(HOST, 1, 2, 1)),
     ValueError, "box_preds must be float32, got torch.float64"),
    ("gpu", "post_process: cls_preds on the host", lambda d: post_process(d, cls_preds=z(HOST, 1, 2, 1)), ValueError, f"cls_preds {DEVICE}"),
    ("gpu", "post_process: cls_preds float64", lambda d: post_process(d, cls_preds=z(d, 1, 2, 1, dtype=F64)), ValueError,
     "cls_preds must be float32, got torch.float64"),
    ("gpu", "post_process: dense form", lambda d: post_process(d, batch_size=2), ValueError,
     "dense form: box_preds (1, 2, 7) and cls_preds (1, 2, 1) must be (batch_size = 2, N, 7 + C) and (batch_size, N, K)"),
    ("gpu", "post_process: stacked form before given labels", lambda d: post_process(d, **stacked(d, batch_index=z(d, 3)), labels=z(d, 2, dtype=I64)),
     ValueError, "stacked form: box_preds (2, 7), cls_preds (2, 1) and batch_index must be (N, 7 + C), (N, K) and (N)"),
    ("gpu", "post_process: given labels with batch_index before the columns", lambda d: post_process(d, **stacked(d, box_preds=z(d, 2, 6)), labels=z(d, 2, dtype=I64)),
     NotImplementedError, "given labels or rois together with batch_index: no head produces that combination"),
    ("gpu", "post_process: rois with batch_index", lambda d: post_process(d, **stacked(d), rois=z(d, 1, 2, 7)), NotImplementedError,
     "given labels or rois together with batch_index: no head produces that combination"),
    ("gpu", "post_process: 6 columns", lambda d: post_process(d, box_preds=z(d, 1, 2, 6), post_maxsize=-1), ValueError,
     "box_preds needs 7 + C columns and cls_preds K >= 1, got 6 and 1"),
    ("gpu", "post_process: negative batch_size", lambda d: post_process(d, **stacked(d), batch_size=-1, labels=None), ValueError,
     "batch_size, pre_maxsize and post_maxsize must not be negative"),
    ("gpu", "post_process: negative pre_maxsize before labels", lambda d: post_process(d, pre_maxsize=-1, labels=z(d, 3, dtype=I64)), ValueError,
     "batch_size, pre_maxsize and post_maxsize must not be negative"),
    ("gpu", "post_process: labels of 3", lambda d: post_process(d, labels=z(d, 3, dtype=I64)), ValueError,
     "labels must be a device tensor of (batch_size, N) = (1, 2) elements"),
    ("gpu", "post_process: labels on the host", lambda d: post_process(d, labels=z(HOST, 1, 2, dtype=I64)), ValueError,
     "labels must be a device tensor of (batch_size, N) = (1, 2) elements"),
    ("gpu", "post_process: 17 thresholds", lambda d: post_process(d, recall_thresh=[0.5] * 17), ValueError,
     "RECALL_THRESH_LIST has 17 thresholds, above the limit of 16"),
    ("gpu", "post_process: gt_boxes float64", lambda d: post_process(d, gt_boxes=z(d, 1, 1, 8, dtype=F64)), ValueError,
     "gt_boxes must be a float32 device tensor on the boxes' device"),
    ("gpu", "post_process: gt_boxes of 7 columns", lambda d: post_process(d, gt_boxes=z(d, 1, 1, 7)), ValueError,
     "gt_boxes (1, 1, 7) must be (batch_size = 1, G, 7 + C + 1 = 8)"),
    ("gpu", "post_process: rois on the host", lambda d: post_process(d, gt_boxes=z(d, 1, 1, 8), rois=z(HOST, 1, 2, 7)), ValueError,
     "rois must be a float32 device tensor on the boxes' device"),
    ("gpu", "post_process: rois of 2 samples", lambda d: post_process(d, gt_boxes=z(d, 1, 1, 8), rois=z(d, 2, 1, 7)), ValueError,
     "rois (2, 1, 7) must be (batch_size = 1, R, 7 + C)"),
    ("gpu", "post_process: out of two", lambda d: post_process(d, out=(z(d, 1, 2, 7), z(d, 1, 2)), workspace=big_f32(d)), ValueError,
     "out must be (pred_boxes, pred_scores, pred_labels)"),
    ("gpu", "post_process: out pred_scores float64", lambda d: post_process(d, out=(z(d, 1, 2, 7), z(d, 1, 2, dtype=F64), z(d, 1, 3, dtype=I64))),
     TypeError, "out pred_scores must be torch.float32, got torch.float64"),
    ("gpu", "post_process: out pred_labels shape", lambda d: post_process(d, out=(z(d, 1, 2, 7), z(d, 1, 2), z(d, 1, 3, dtype=I64))), ValueError,
     "out pred_labels has shape (1, 3), expected (1, 2)"),
    ("gpu", "post_process: workspace float32 before the table", lambda d: post_process(d, workspace=big_f32(d), table=z(HOST, 64, dtype=I32)), TypeError, WS_TEXT),
    ("gpu", "post_process: table not pinned", lambda d: post_process(d, table=z(HOST, 64, dtype=I32)), ValueError,
     "table must be a contiguous pinned int32 tensor"),
    # ------------------------------------------------------------------------------------------------ anchor_loss
    ("cpu", "anchor_loss: cls_preds on the host", lambda d: anchor_loss(HOST), ValueError, f"cls_preds {DEVICE}"),
    ("cpu", "anchor_loss: cls_preds None", lambda d: anchor_loss(HOST, cls_preds=None), ValueError, f"cls_preds {DEVICE}"),
    ("gpu", "anchor_loss: cls_preds float64 before box_preds on the host", lambda d: anchor_loss(d, cls_preds=z(d, 1, 2, 1, dtype=F64), box_preds=z(HOST, 1, 2, 7)),
     TypeError, "cls_preds must be float32, got torch.float64"),
    ("gpu", "anchor_loss: dir_preds on the host", lambda d: anchor_loss(d, dir_preds=z(HOST, 1, 2, 2)), ValueError, f"dir_preds {DEVICE}"),
    ("gpu", "anchor_loss: labels None", lambda d: anchor_loss(d, labels=None), ValueError, f"labels {DEVICE}"),
    ("gpu", "anchor_loss: labels float32", lambda d: anchor_loss(d, labels=z(d, 1, 2)), TypeError, "labels must be int32 or int64, got torch.float32"),
    ("gpu", "anchor_loss: code_weights float64", lambda d: anchor_loss(d, code_weights=z(d, 7, dtype=F64)), TypeError,
     "code_weights must be float32, got torch.float64"),
    ("gpu", "anchor_loss: shapes", lambda d: anchor_loss(d, box_preds=z(d, 1, 3, 7)), ValueError,
     "cls_preds (1, 2, 1) and box_preds (1, 3, 7) must be (B, N, C) and (B, N, code)"),
    ("gpu", "anchor_loss: gamma", lambda d: anchor_loss(d, gamma=3), ValueError,
     "gamma = 3: only gamma = 2 is provided (the focal power is the product pt * pt)"),
    ("gpu", "anchor_loss: labels not contiguous", lambda d: anchor_loss(d, labels=z(d, 1, 4, dtype=I32)[:, ::2]), ValueError, "labels must be contiguous"),
    ("gpu", "anchor_loss: out of three", lambda d: anchor_loss(d, out=(z(d, 4), z(d, 1, 2, 1), z(d, 1, 2, 7))), ValueError,
     "out must be (losses, grad_cls, grad_box, grad_dir)"),
    ("gpu", "anchor_loss: out grad_dir without dir_preds", lambda d: anchor_loss(d, out=(z(d, 4), z(d, 1, 2, 1), z(d, 1, 2, 7), z(d, 1, 2, 0))), ValueError,
     "out grad_dir must be None"),
    ("gpu", "anchor_loss: out grad_cls None", lambda d: anchor_loss(d, out=(z(d, 4), None, z(d, 1, 2, 7), None)), ValueError, "out grad_cls must be a tensor"),
    ("gpu", "anchor_loss: out losses float64", lambda d: anchor_loss(d, out=(z(d, 4, dtype=F64), z(d, 1, 2, 1), z(d, 1, 2, 7), None)), TypeError,
     "out losses must be torch.float32, got torch.float64"),
    ("gpu", "anchor_loss: out losses on the host", lambda d: anchor_loss(d, out=(z(HOST, 4), z(d, 1, 2, 1), z(d, 1, 2, 7), None)), ValueError,
     f"out losses {DEVICE}"),
    ("gpu", "anchor_loss: out losses shape", lambda d: anchor_loss(d, out=(z(d, 5), z(d, 1, 2, 1), z(d, 1, 2, 7), None)), ValueError,
     "out losses has shape (5,) on {d}, expected (4,) on {d}"),
    ("gpu", "anchor_loss: workspace float32", lambda d: anchor_loss(d, workspace=big_f32(d)), TypeError, WS_TEXT),
    # ------------------------------------------------------------------------------------------------ roi_loss
    ("cpu", "roi_loss: rcnn_cls on the host", lambda d: roi_loss(HOST), ValueError, f"rcnn_cls {DEVICE}"),
    ("gpu", "roi_loss: rcnn_cls_labels float64", lambda d: roi_loss(d, rcnn_cls_labels=z(d, 2, dtype=F64), reg_valid_mask=z(HOST, 2, dtype=I64)), TypeError,
     "rcnn_cls_labels must be int32, int64 or float32, got torch.float64"),
    ("gpu", "roi_loss: reg_valid_mask float32", lambda d: roi_loss(d, reg_valid_mask=z(d, 2)), TypeError, "reg_valid_mask must be int32 or int64, got torch.float32"),
    ("gpu", "roi_loss: rois float64", lambda d: roi_loss(d, rois=z(d, 2, 7, dtype=F64)), TypeError, "rois must be float32, got torch.float64"),
    ("gpu", "roi_loss: code_weights on the host", lambda d: roi_loss(d, code_weights=z(HOST, 7)), ValueError, f"code_weights {DEVICE}"),
    ("gpu", "roi_loss: rcnn_reg of one dimension", lambda d: roi_loss(d, rcnn_reg=z(d, 2)), ValueError, "rcnn_reg (2,) must be (R, code)"),
    ("gpu", "roi_loss: out of two", lambda d: roi_loss(d, out=(z(d, 6), z(d, 2))), ValueError, "out must be (table, grad_cls, grad_reg)"),
    ("gpu", "roi_loss: out grad_cls without want_grad", lambda d: roi_loss(d, want_grad=False, out=(z(d, 6), z(d, 2), None)), ValueError,
     "out grad_cls must be None"),
    ("gpu", "roi_loss: out table shape", lambda d: roi_loss(d, out=(z(d, 5), z(d, 2), z(d, 2, 7))), ValueError,
     "out table has shape (5,) on {d}, expected (6,) on {d}"),
    ("gpu", "roi_loss: out grad_reg float64", lambda d: roi_loss(d, out=(z(d, 6), z(d, 2), z(d, 2, 7, dtype=F64))), TypeError,
     "out grad_reg must be torch.float32, got torch.float64"),
    ("gpu", "roi_loss: workspace float32", lambda d: roi_loss(d, workspace=big_f32(d)), TypeError, WS_TEXT),
    # ------------------------------------------------------------------------------------------------ point_loss
    ("cpu", "point_loss: part_preds alone", lambda d: point_loss(HOST, part_preds=z(HOST, 2, 3)), ValueError, "part_preds and part_labels come together"),
    ("cpu", "point_loss: box_preds without code_weights", lambda d: point_loss(HOST, box_preds=z(HOST, 2, 8), box_labels=z(HOST, 2, 8)), ValueError,
     "box_preds, box_labels and code_weights come together"),
    ("cpu", "point_loss: cls_preds on the host", lambda d: point_loss(HOST), ValueError, f"cls_preds {DEVICE}"),
    ("gpu", "point_loss: labels None", lambda d: point_loss(d, labels=None), ValueError, f"labels {DEVICE}"),
    ("gpu", "point_loss: labels float32", lambda d: point_loss(d, labels=z(d, 2)), TypeError, "labels must be int32 or int64, got torch.float32"),
    ("gpu", "point_loss: part_preds float64 before part_labels on the host", lambda d: point_loss(d, part_preds=z(d, 2, 3, dtype=F64), part_labels=z(HOST, 2, 3)),
     TypeError, "part_preds must be float32, got torch.float64"),
    ("gpu", "point_loss: part_labels on the host", lambda d: point_loss(d, part_preds=z(d, 2, 3), part_labels=z(HOST, 2, 3)), ValueError,
     f"part_labels {DEVICE}"),
    ("gpu", "point_loss: cls_preds of one dimension", lambda d: point_loss(d, cls_preds=z(d, 2)), ValueError,
     "cls_preds (2,) must be (N, num_class) or (B, n, num_class)"),
    ("gpu", "point_loss: out of three", lambda d: point_loss(d, out=(z(d, 5), z(d, 2, 1), None)), ValueError,
     "out must be (table, grad_cls, grad_part, grad_box)"),
    ("gpu", "point_loss: out grad_part without part_preds", lambda d: point_loss(d, out=(z(d, 5), z(d, 2, 1), z(d, 2, 3), None)), ValueError,
     "out grad_part must be None"),
    ("gpu", "point_loss: out grad_cls shape", lambda d: point_loss(d, out=(z(d, 5), z(d, 3, 1), None, None)), ValueError,
     "out grad_cls has shape (3, 1) on {d}, expected (2, 1) on {d}"),
    ("gpu", "point_loss: workspace float32", lambda d: point_loss(d, workspace=big_f32(d)), TypeError, WS_TEXT),
    # ------------------------------------------------------------------------------------------------ the backward calls
    ("cpu", "anchor_loss_backward: upstream on the host", lambda d: ops.anchor_loss_backward((None, None, None), z(HOST, 1)), ValueError,
     "upstream must be a float32 device tensor of one element"),
    ("gpu", "anchor_loss_backward: upstream of two", lambda d: ops.anchor_loss_backward((None, None, None), z(d, 2)), ValueError,
     "upstream must be a float32 device tensor of one element"),
    ("gpu", "anchor_loss_backward: two grads", lambda d: ops.anchor_loss_backward((z(d, 2), z(d, 2)), z(d, 1)), ValueError,
     "grads must be (grad_cls, grad_box, grad_dir)"),
    ("gpu", "anchor_loss_backward: a float64 gradient", lambda d: ops.anchor_loss_backward((z(d, 2), z(d, 2, dtype=F64), None), z(d, 1)), TypeError,
     "a gradient buffer must be torch.float32, got torch.float64"),
    ("gpu", "roi_loss_backward: three grads", lambda d: ops.roi_loss_backward((z(d, 2), z(d, 2), z(d, 2)), z(d, 1)), ValueError,
     "grads must be (grad_cls, grad_reg)"),
    ("gpu", "roi_loss_backward: a gradient on the host", lambda d: ops.roi_loss_backward((z(d, 2), z(HOST, 2)), z(d, 1)), ValueError,
     f"a gradient buffer {DEVICE}"),
    ("gpu", "point_loss_backward: two grads", lambda d: ops.point_loss_backward((z(d, 2), z(d, 2)), z(d, 1)), ValueError,
     "grads must be (grad_cls, grad_part, grad_box)"),
    ("gpu", "point_loss_backward: upstream float64", lambda d: ops.point_loss_backward((z(d, 2), None, None), z(d, 1, dtype=F64)), ValueError,
     "upstream must be a float32 device tensor of one element"),
    # ------------------------------------------------------------------------------------------------ the decodes
    ("cpu", "anchor_decode: box_preds on the host", lambda d: anchor_decode(HOST), ValueError, f"box_preds {DEVICE}"),
    ("cpu", "anchor_decode: box_preds a list", lambda d: anchor_decode(HOST, box_preds=[1.0]), ValueError, f"box_preds {DEVICE}"),
    ("gpu", "anchor_decode: box_preds float64 before anchors on the host", lambda d: anchor_decode(d, box_preds=z(d, 1, 2, 7, dtype=F64), anchors=z(HOST, 2, 7)),
     TypeError, "box_preds must be float32, got torch.float64"),
    ("gpu", "anchor_decode: anchors on the host", lambda d: anchor_decode(d, anchors=z(HOST, 2, 7)), ValueError, f"anchors {DEVICE}"),
    ("gpu", "anchor_decode: dir_cls_preds float64", lambda d: anchor_decode(d, dir_cls_preds=z(d, 1, 2, 2, dtype=F64)), TypeError,
     "dir_cls_preds must be float32, got torch.float64"),
    ("gpu", "anchor_decode: anchors of three dimensions", lambda d: anchor_decode(d, anchors=z(d, 2, 7, 1)), ValueError,
     "box_preds (1, 2, 7) must be (B, N, code) and anchors (2, 7, 1) (N, 7 + C)"),
    ("gpu", "anchor_decode: out shape", lambda d: anchor_decode(d, out=z(d, 1, 2, 8)), ValueError, "out must be a contiguous float32 (1, 2, 7) tensor on {d}"),
    ("gpu", "anchor_decode: out float64", lambda d: anchor_decode(d, out=z(d, 1, 2, 7, dtype=F64)), ValueError,
     "out must be a contiguous float32 (1, 2, 7) tensor on {d}"),
    ("gpu", "anchor_decode: out on the host", lambda d: anchor_decode(d, out=z(HOST, 1, 2, 7)), ValueError,
     "out must be a contiguous float32 (1, 2, 7) tensor on {d}"),
    ("gpu", "anchor_decode: out a list", lambda d: anchor_decode(d, out=[]), ValueError, "out must be a contiguous float32 (1, 2, 7) tensor on {d}"),
    ("cpu", "point_decode: point_box_preds on the host", lambda d: point_decode(HOST), ValueError, f"point_box_preds {DEVICE}"),
    ("gpu", "point_decode: points on the host", lambda d: point_decode(d, points=z(HOST, 2, 3), point_cls_preds=z(d, 2, 1, dtype=F64)), ValueError,
     f"points {DEVICE}"),
    ("gpu", "point_decode: mean_size float64", lambda d: point_decode(d, mean_size=z(d, 1, 3, dtype=F64)), TypeError,
     "mean_size must be float32, got torch.float64"),
    ("gpu", "point_decode: out not contiguous", lambda d: point_decode(d, out=z(d, 2, 14)[:, ::2]), ValueError,
     "out must be a contiguous float32 (2, 7) tensor on {d}"),
    ("cpu", "roi_decode: rois on the host", lambda d: roi_decode(HOST), ValueError, f"rois {DEVICE}"),
    ("gpu", "roi_decode: box_preds float64", lambda d: roi_decode(d, box_preds=z(d, 2, 7, dtype=F64)), TypeError,
     "box_preds must be float32, got torch.float64"),
    ("gpu", "roi_decode: out shape", lambda d: roi_decode(d, out=z(d, 2, 8)), ValueError, "out must be a contiguous float32 (2, 7) tensor on {d}"),
]


def refused(call, d, exc, text):
    with pytest.raises(Exception) as e:
        call(d)
    assert type(e.value) is exc, (type(e.value), str(e.value))
    assert str(e.value) == text.replace("{d}", str(d))


def test_the_table_names_every_detector_op():
    names = {name.split(":")[0] for _, name, _, _, _ in CASES}
    assert names == {"anchor_targets", "point_targets", "proposals", "roi_targets", "roi_targets_match", "roi_targets_sample",
                     "post_process", "anchor_loss", "roi_loss", "point_loss", "anchor_loss_backward", "roi_loss_backward",
                     "point_loss_backward", "anchor_decode", "point_decode", "roi_decode"}
    assert len({name for _, name, _, _, _ in CASES}) == len(CASES)


@pytest.mark.parametrize("name,call,exc,text", [c[1:] for c in CASES if c[0] == "cpu"], ids=[c[1] for c in CASES if c[0] == "cpu"])
def test_refused_on_the_host(name, call, exc, text):
    refused(call, HOST, exc, text)


# the six *_workspace_bytes wrappers hand a refusal of the library on as ModestHipError, with its name in front
WORKSPACE_BYTES = [
    ("proposals_workspace_bytes", (-1,), "modest_proposals_workspace_bytes: requirement failed: 0 <= n_rows <= 2147483647 (the row count of a call)"),
    ("post_process_workspace_bytes", (-1, 1), "modest_post_process_workspace_bytes: requirement failed: 0 <= n_rows <= 2147483647 and 0 <= batch_size <= 65535"),
    ("post_process_workspace_bytes", (1, 65536), "modest_post_process_workspace_bytes: requirement failed: 0 <= n_rows <= 2147483647 and 0 <= batch_size <= 65535"),
    ("anchor_targets_workspace_bytes", (-1, 1, 1), None),
    ("roi_targets_workspace_bytes", (-1, 1), None),
    ("anchor_loss_workspace_bytes", (-1, 1), None),
    ("roi_loss_workspace_bytes", (-1,), None),
    ("point_loss_workspace_bytes", (-1,), None),
]


@pytest.mark.parametrize("fn,args,text", WORKSPACE_BYTES, ids=[f"{fn}{args}" for fn, args, _ in WORKSPACE_BYTES])
def test_workspace_bytes_refusals(fn, args, text):
    with pytest.raises(ModestHipError) as e:
        getattr(ops, fn)(*args)
    head, _, tail = str(e.value).partition("): ")
    assert head.startswith(f"modest_{fn} failed (rc=-") and head[len(f"modest_{fn} failed (rc=-"):].isdigit()
    assert tail.startswith(f"modest_{fn}: ") if text is None else tail == text


@pytest.mark.gpu
@pytest.mark.parametrize("name,call,exc,text", [c[1:] for c in CASES if c[0] == "gpu"], ids=[c[1] for c in CASES if c[0] == "gpu"])
def test_refused_on_the_device(gpu, name, call, exc, text):
    refused(call, gpu, exc, text)
