"""Drop-in for ``RoIHeadTemplate.proposal_layer`` of OpenPCDet's two-stage detectors
(``pcdet/models/roi_heads/roi_head_template.py``, over ``class_agnostic_nms``) on the GPU: the
proposal selection of PointRCNN, PartA2 and PV-RCNN, in training and at test time.

One library call (``modest_amd.ops.proposals``, csrc/proposals.hip) selects the proposals of the whole batch on PyTorch's
current stream: no loop over the samples, no suppression mask, nothing is copied to the host, nothing synchronises.  The
workspace is kept on the head and grows with the largest call.

Provided: ``MULTI_CLASSES_NMS: False`` with ``NMS_TYPE`` ``nms_gpu`` or ``nms_normal_gpu``; the multi-class branch raises
``NotImplementedError`` as the reference does.  Where the reference leaves the order open, equal scores go by ascending
row, equal class maxima to the lowest class, and a NaN score ranks above every number.  ``NMS_POST_MAXSIZE`` above
``POST_MAX`` or a batch above ``BATCH_MAX`` raises ``ValueError``.  ``bind(cls)`` sets the method on a head class;
``pcdet_bind.install(proposal_layer=True)`` does that for the reference's ``RoIHeadTemplate``.
"""
import torch

from ._head_loss import _get, device_workspace

POST_MAX = 1024       # survivors per sample: the kept list is held in LDS (csrc/prop_walk.h)
BATCH_MAX = 65535     # samples per call: 16 sample bits of the sort key
NMS_TYPES = {"nms_gpu": True, "nms_normal_gpu": False}   # name -> rotated


@torch.no_grad()
def proposal_layer(self, batch_dict, nms_config):
    """
    Args:
        batch_dict:
            batch_size:
            batch_cls_preds: (B, num_boxes, num_classes | 1) or (N1+N2+..., num_classes | 1)
            batch_box_preds: (B, num_boxes, 7+C) or (N1+N2+..., 7+C)
            batch_index: optional (N1+N2+...)
        nms_config:
    Returns:
        batch_dict:
            rois: (B, num_rois, 7+C)
            roi_scores: (B, num_rois)
            roi_labels: (B, num_rois)
    """
    from .. import ops
    from .._lib import ModestHipError
    if _get(nms_config, "MULTI_CLASSES_NMS"):
        raise NotImplementedError
    nms_type = _get(nms_config, "NMS_TYPE")
    if nms_type not in NMS_TYPES:
        raise ValueError(f"NMS_TYPE {nms_type!r} is not provided: one of {sorted(NMS_TYPES)}")
    batch_size = int(batch_dict['batch_size'])
    post, pre = int(_get(nms_config, "NMS_POST_MAXSIZE")), int(_get(nms_config, "NMS_PRE_MAXSIZE"))
    if post > POST_MAX:
        raise ValueError(f"NMS_POST_MAXSIZE = {post} is above the limit of {POST_MAX} survivors per sample")
    if batch_size > BATCH_MAX:
        raise ValueError(f"batch_size = {batch_size} is above the limit of {BATCH_MAX} samples per call")
    box_preds = batch_dict['batch_box_preds']
    cls_preds = batch_dict['batch_cls_preds']
    batch_index = batch_dict.get('batch_index', None)
    if batch_index is not None:
        assert cls_preds.shape.__len__() == 2
    else:
        assert cls_preds.shape.__len__() == 3
    if not box_preds.is_cuda or not cls_preds.is_cuda:
        raise ValueError("batch_box_preds and batch_cls_preds must be device tensors (PyTorch-ROCm 'cuda')")
    box = box_preds if box_preds.dtype == torch.float32 else box_preds.float()
    cls = cls_preds if cls_preds.dtype == torch.float32 else cls_preds.float()
    try:
        ws = device_workspace(self, '_modest_proposals_workspace', ops.proposals_workspace_bytes(box.numel() // box.shape[-1]), box.device)
        rois, roi_scores, roi_labels = ops.proposals(box, cls, batch_size, pre, post, float(_get(nms_config, "NMS_THRESH")),
                                                     rotated=NMS_TYPES[nms_type], batch_index=batch_index, workspace=ws)
    except ModestHipError as e:
        if "requirement failed" in str(e):
            raise ValueError(str(e)) from e   # a limit of the library, named in its message
        raise
    if box_preds.dtype != torch.float32:
        rois, roi_scores = rois.to(box_preds.dtype), roi_scores.to(box_preds.dtype)
    batch_dict['rois'] = rois
    batch_dict['roi_scores'] = roi_scores
    batch_dict['roi_labels'] = roi_labels
    batch_dict['has_class_labels'] = True if cls_preds.shape[-1] > 1 else False
    batch_dict.pop('batch_index', None)
    return batch_dict


def bind(cls):
    """set proposal_layer on a head class (RoIHeadTemplate or a subclass) -> cls"""
    cls.proposal_layer = proposal_layer
    return cls
