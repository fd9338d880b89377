"""Drop-in for ``Detector3DTemplate.post_processing`` of OpenPCDet's detectors
(``pcdet/models/detectors/detector3d_template.py``, over ``class_agnostic_nms`` and ``generate_recall_record``) on the GPU
(DESIGN.md section 7o): what closes every test-time forward of PointRCNN, PointPillars, SECOND, PartA2, PV-RCNN and
Voxel R-CNN.

One library call (``modest_amd.ops.post_process``, csrc/post_process.hip) on PyTorch's current stream takes the whole batch:
the score threshold, the sigmoid, the cut at ``NMS_PRE_MAXSIZE``, the greedy NMS up to ``NMS_POST_MAXSIZE`` and the recall
counters, with no loop over the samples, no suppression mask and ONE host wait (the library's stream synchronise), after
which the survivors per sample and the counters lie in a small pinned table.  ``pred_dicts`` are views ``buf[b, :n_b]`` of
three padded buffers allocated per call; no kernel is launched for them.  The workspace and the pinned table are kept on the
detector, grow with the largest call and serve one stream at a time.

Provided: ``MULTI_CLASSES_NMS: False`` with ``NMS_TYPE`` ``nms_gpu`` or ``nms_normal_gpu`` and ``batch_cls_preds`` as one
tensor; the multi-class branch and a list of class predictions (the multihead configs) raise ``NotImplementedError``, and
so do ``has_class_labels`` or ``rois`` together with ``batch_index``, which no head produces.  Where the reference leaves
the order open: equal scores (equal after the sigmoid) go by ascending row, equal class maxima to the lowest class, and
the sigmoid is the double function rounded once.  The limits (``ValueError``): ``NMS_POST_MAXSIZE`` <= ``POST_MAX``, batch <=
``BATCH_MAX``, at most ``THRESH_MAX`` recall thresholds, 4096 columns, 2^31 - 1 rows.  ``bind(cls)`` sets the method on a
detector class; ``pcdet_bind.bind_post_processing()`` does that for the reference's ``Detector3DTemplate``.
"""
import torch

from ._head_loss import _get, device_workspace, pinned_table

POST_MAX = 1024       # survivors per sample: the kept list is held in LDS (csrc/prop_walk.h)
BATCH_MAX = 65535     # samples per call: 16 sample bits of the sort key
THRESH_MAX = 16       # len(RECALL_THRESH_LIST): the thresholds travel in a kernel's arguments
NMS_TYPES = {"nms_gpu": True, "nms_normal_gpu": False}   # name -> rotated


def _buffers(detector, dev, rows, B, T):
    """the workspace and the pinned table kept on `detector`: they grow with the largest call.  Every call ends in a
    stream synchronise, so no kernel of an earlier call can still write a table that is replaced here."""
    from .. import ops
    return (device_workspace(detector, "_modest_post_process_workspace", ops.post_process_workspace_bytes(rows, B), dev),
            pinned_table(detector, "_modest_post_process_table", ops.post_process_table_words(B, T)))


@torch.no_grad()
def post_processing(self, batch_dict):
    """
    Args:
        batch_dict:
            batch_size:
            batch_cls_preds: (B, num_boxes, num_classes | 1) or (N1+N2+..., num_classes | 1)
            batch_box_preds: (B, num_boxes, 7+C) or (N1+N2+..., 7+C)
            cls_preds_normalized: indicate whether batch_cls_preds is normalized
            batch_index: optional (N1+N2+...)
            has_class_labels: True/False
            roi_labels: (B, num_rois)  1 .. num_classes
            batch_pred_labels: (B, num_boxes, 1)
            gt_boxes: optional (B, G, 7+C+1);  rois: optional (B, num_rois, 7+C)
    Returns:
        pred_dicts: B dicts of pred_boxes (n_b, 7+C), pred_scores (n_b), pred_labels (n_b) int64
        recall_dict: {} without gt_boxes, else 'gt' and 'roi_%s' / 'rcnn_%s' per threshold, Python ints
    """
    from .. import ops
    from .._lib import ModestHipError
    model_cfg = self.model_cfg
    cfg = model_cfg["POST_PROCESSING"] if isinstance(model_cfg, dict) else model_cfg.POST_PROCESSING
    nms_cfg = _get(cfg, "NMS_CONFIG")
    batch_size = int(batch_dict['batch_size'])
    cls_preds = batch_dict['batch_cls_preds']
    box_preds = batch_dict['batch_box_preds']
    if isinstance(cls_preds, (list, tuple)):
        raise NotImplementedError("batch_cls_preds as a list (the multihead configs) is not provided")
    if _get(nms_cfg, "MULTI_CLASSES_NMS"):
        raise NotImplementedError("MULTI_CLASSES_NMS: True is not provided")
    nms_type = _get(nms_cfg, "NMS_TYPE")
    if nms_type not in NMS_TYPES:
        raise ValueError(f"NMS_TYPE {nms_type!r} is not provided: one of {sorted(NMS_TYPES)}")
    batch_index = batch_dict.get('batch_index', None)
    if batch_index is not None:
        assert box_preds.shape.__len__() == 2
    else:
        assert box_preds.shape.__len__() == 3
    assert cls_preds.shape[-1] in [1, self.num_class]
    has_labels = bool(batch_dict.get('has_class_labels', False))
    if batch_index is not None and (has_labels or 'rois' in batch_dict):
        raise NotImplementedError("has_class_labels or rois together with batch_index: no head produces that combination")
    post, pre = int(_get(nms_cfg, "NMS_POST_MAXSIZE")), int(_get(nms_cfg, "NMS_PRE_MAXSIZE"))
    thresh_list = list(_get(cfg, "RECALL_THRESH_LIST"))
    if post > POST_MAX:
        raise ValueError(f"NMS_POST_MAXSIZE = {post} is above the limit of {POST_MAX} survivors per sample")
    if batch_size > BATCH_MAX:
        raise ValueError(f"batch_size = {batch_size} is above the limit of {BATCH_MAX} samples per call")
    if len(thresh_list) > THRESH_MAX:
        raise ValueError(f"RECALL_THRESH_LIST has {len(thresh_list)} thresholds, above the limit of {THRESH_MAX}")
    for t, name in ((box_preds, "batch_box_preds"), (cls_preds, "batch_cls_preds")):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError(f"{name} must be a device tensor (PyTorch-ROCm 'cuda')")
    labels = None
    if has_labels:
        labels = batch_dict['roi_labels' if 'roi_labels' in batch_dict else 'batch_pred_labels']
    gt_boxes = batch_dict.get('gt_boxes', None)
    rois = batch_dict.get('rois', None) if gt_boxes is not None else None
    for t, name in ((labels, "the given labels"), (gt_boxes, "gt_boxes"), (rois, "rois")):
        if t is not None and (not torch.is_tensor(t) or not t.is_cuda):
            raise ValueError(f"{name} must be a device tensor (PyTorch-ROCm 'cuda')")
    f32 = lambda t: t if t is None or t.dtype == torch.float32 else t.float()      # noqa: E731
    box, cls = f32(box_preds), f32(cls_preds)
    try:
        ws, table = _buffers(self, box.device, box.numel() // box.shape[-1], batch_size, len(thresh_list) if gt_boxes is not None else 0)
        boxes, scores, labs, counts, recall = ops.post_process(
            box, cls, batch_size, pre, post, float(_get(nms_cfg, "NMS_THRESH")), rotated=NMS_TYPES[nms_type],
            score_thresh=_get(cfg, "SCORE_THRESH", None), normalized=bool(batch_dict['cls_preds_normalized']),
            output_raw_score=bool(_get(cfg, "OUTPUT_RAW_SCORE", False)), labels=labels, batch_index=batch_index,
            gt_boxes=f32(gt_boxes), rois=f32(rois), recall_thresh=thresh_list if gt_boxes is not None else (),
            workspace=ws, table=table)
    except ModestHipError as e:
        if "requirement failed" in str(e):
            raise ValueError(str(e)) from e   # a limit of the library, named in its message
        raise
    if box_preds.dtype != torch.float32:
        boxes = boxes.to(box_preds.dtype)
    if cls_preds.dtype != torch.float32:
        scores = scores.to(cls_preds.dtype)
    pred_dicts = []
    for index in range(batch_size):
        n = int(counts[index])
        pred_dicts.append({'pred_boxes': boxes[index, :n], 'pred_scores': scores[index, :n], 'pred_labels': labs[index, :n]})
    recall_dict = {}
    if recall is not None and batch_size > 0:
        recall_dict['gt'] = recall["gt"]
        for k, cur_thresh in enumerate(thresh_list):
            recall_dict['roi_%s' % (str(cur_thresh))] = recall["roi"][k]
            recall_dict['rcnn_%s' % (str(cur_thresh))] = recall["rcnn"][k]
    return pred_dicts, recall_dict


def bind(cls):
    """set post_processing on a detector class (Detector3DTemplate or a subclass) -> cls"""
    cls.post_processing = post_processing
    return cls
