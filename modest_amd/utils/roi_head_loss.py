"""Drop-in for ``RoIHeadTemplate.get_loss`` of OpenPCDet's RoI heads (``pcdet/models/roi_heads/roi_head_template.py``, over
``ResidualCoder`` of ``pcdet/utils/box_coder_utils.py``, ``WeightedSmoothL1Loss`` and ``get_corner_loss_lidar`` of
``pcdet/utils/loss_utils.py``) on the GPU: what closes every training step of PointRCNN, PartA2,
PV-RCNN and Voxel R-CNN.  It consumes the dict that ``modest_amd.utils.roi_targets.assign_targets`` produces.

One library call (``modest_amd.ops.roi_loss``, csrc/roi_loss.hip) on PyTorch's current stream computes the classification,
regression and corner losses and, where a prediction requires a gradient, the two gradients of ``rcnn_loss`` in the same pass:
no encoded targets, no foreground subset, no rotation matrices, no corner tensors, nothing kept for autograd but the two
gradient buffers.  ``backward`` is one more library call, which scales those buffers in place by the upstream gradient read
from the device.  ``tb_dict``'s floats and ``fg_sum`` are read through a small pinned table after ONE stream synchronise (the
reference waits five times); the table decides whether ``rcnn_loss_corner`` is reported.  The workspace and the pinned table
are kept on the head.

Provided: ``CLS_LOSS: BinaryCrossEntropy`` (hard labels with -1 = ignore, or soft ``roi_iou`` labels), ``REG_LOSS: smooth-l1``
with ``WeightedSmoothL1Loss``, ``CORNER_LOSS_REGULARIZATION`` on or off, ``ResidualCoder`` without ``encode_angle_by_sincos``,
float32 predictions.  ``CLS_LOSS: CrossEntropy``, another ``REG_LOSS``, another box coder, another ``reg_loss_func`` and
predictions of another type raise ``NotImplementedError`` naming the option; the limits (``ValueError``): code size 7 .. 16,
at most 2^20 rows.  A head whose class overrides ``get_box_reg_layer_loss`` or ``get_box_cls_layer_loss`` is handed to the
method this one replaced; a head class with a ``get_loss`` of its own (``SECONDHead``) keeps it.

One visible difference: the reference clamps the sizes inside ``forward_ret_dict['gt_of_rois']`` at 1e-5 IN PLACE
(``encode_torch``); this method leaves the dict as it found it.

``bind(cls)`` sets the method on a head class; ``pcdet_bind.bind_roi_loss()`` does that for the reference's
``RoIHeadTemplate``.
"""
import torch

from ._head_loss import HeadLossFunction, _get, buffers, code_weights_tensor, read_table, replaced_get_loss

CLS_LOSS = "BinaryCrossEntropy"
REG_LOSS = "smooth-l1"
REG_LOSS_FUNC = "WeightedSmoothL1Loss"
BOX_CODER = "ResidualCoder"
PARTS = ("get_box_reg_layer_loss", "get_box_cls_layer_loss")   # an override of either: the head computes another loss

_ORIGINAL = {}   # class -> the get_loss that bind() replaced on it (None: it had none of its own)


class RoiLossFunction(HeadLossFunction):
    """(rcnn_cls, rcnn_reg, labels, mask, gt_of_rois, gt_of_rois_src, rois, code_weights, scalars, workspace) -> table (6):
    [rcnn_loss_cls, rcnn_loss_reg, rcnn_loss_corner, rcnn_loss, fg_sum, cls_valid]"""
    OPS, PREDS, WORD = ("roi_loss", "roi_loss_backward"), (0, 1), "RoI"


def _rows(t, code, name):
    """(..., >= code) -> (R, C) with unit column stride, a view wherever the rows are evenly strided"""
    if t.shape[-1] < code:
        raise ValueError(f"{name} has {t.shape[-1]} columns, fewer than the code size {code}")
    if t.dtype != torch.float32:
        t = t.float()
    flat = t.reshape(-1, t.shape[-1])      # a view wherever the strides allow it
    if flat.stride(1) == 1 and (flat.shape[0] <= 1 or flat.stride(0) >= code):
        return flat
    return flat[:, 0:code].contiguous()


def get_loss(self, tb_dict=None):
    """-> (rcnn_loss, tb_dict): rcnn_loss a 0-dim device tensor with its gradient function; tb_dict the dict passed in (or a
    new one) updated with the Python floats rcnn_loss_cls, rcnn_loss_reg, rcnn_loss and, iff the corner term is on and there
    is a foreground row, rcnn_loss_corner"""
    from .. import ops
    _, original = replaced_get_loss(type(self), _ORIGINAL, PARTS)
    if original is not None:
        return original(self, tb_dict)
    tb_dict = {} if tb_dict is None else tb_dict
    loss_cfg = _get(self.model_cfg, "LOSS_CONFIG")
    cls_loss, reg_loss = _get(loss_cfg, "CLS_LOSS"), _get(loss_cfg, "REG_LOSS")
    if cls_loss != CLS_LOSS:
        raise NotImplementedError(f"CLS_LOSS: {cls_loss} is not provided by modest_amd's RoI loss: {CLS_LOSS} only")
    if reg_loss != REG_LOSS:
        raise NotImplementedError(f"REG_LOSS: {reg_loss} is not provided by modest_amd's RoI loss: {REG_LOSS} only")
    coder = self.box_coder
    if type(coder).__name__ != BOX_CODER:
        raise NotImplementedError(f"BOX_CODER: {type(coder).__name__} is not provided: {BOX_CODER} only")
    if getattr(coder, "encode_angle_by_sincos", False):
        raise NotImplementedError("BOX_CODER with encode_angle_by_sincos is not provided")
    reg_fn = self.reg_loss_func
    if type(reg_fn).__name__ != REG_LOSS_FUNC:
        raise NotImplementedError(f"reg_loss_func = {type(reg_fn).__name__} is not provided: {REG_LOSS_FUNC} only")
    ret = self.forward_ret_dict
    rcnn_cls, rcnn_reg = ret['rcnn_cls'], ret['rcnn_reg']
    for t, name in ((rcnn_cls, "rcnn_cls"), (rcnn_reg, "rcnn_reg")):
        if torch.is_tensor(t) and t.dtype != torch.float32:
            raise NotImplementedError(f"{name} of {t.dtype} (mixed precision) is not provided: float32 predictions only")
    code = int(coder.code_size)
    if code < ops.ROI_LOSS_MIN_CODE or code > ops.ROI_LOSS_MAX_CODE:
        raise ValueError(f"code size = {code} is outside the limit of {ops.ROI_LOSS_MIN_CODE} .. {ops.ROI_LOSS_MAX_CODE}")
    labels, mask = ret['rcnn_cls_labels'], ret['reg_valid_mask']
    gt, src, rois = ret['gt_of_rois'], ret['gt_of_rois_src'], ret['rois']
    R = int(mask.numel())
    if R > ops.ROI_LOSS_MAX_ROWS:
        raise ValueError(f"reg_valid_mask has {R} rows, above the limit of {ops.ROI_LOSS_MAX_ROWS}")
    if rcnn_cls.numel() != R:
        raise ValueError(f"rcnn_cls has {rcnn_cls.numel()} elements, reg_valid_mask {R} rows")
    if rcnn_reg.numel() != R * code:
        raise ValueError(f"rcnn_reg has {rcnn_reg.numel()} elements, expected {R} rows of code size {code}")
    for t, name in ((rcnn_cls, "rcnn_cls"), (rcnn_reg, "rcnn_reg"), (labels, "rcnn_cls_labels"), (mask, "reg_valid_mask"),
                    (gt, "gt_of_rois"), (src, "gt_of_rois_src"), (rois, "rois")):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError(f"{name} must be a device tensor (PyTorch-ROCm 'cuda')")
    dev = rcnn_cls.device
    cls, reg = rcnn_cls.reshape(R), rcnn_reg.reshape(R, code)
    if labels.dtype not in (torch.int32, torch.int64, torch.float32):
        labels = labels.float() if labels.is_floating_point() else labels.long()
    labels = labels.reshape(R).contiguous()
    if mask.dtype not in (torch.int32, torch.int64):
        mask = mask.long()
    mask = mask.reshape(R).contiguous()
    gt, src = _rows(gt, code, "gt_of_rois"), _rows(src, code, "gt_of_rois_src")
    rois = rois.detach().float().reshape(R, code).contiguous()
    code_weights = code_weights_tensor(reg_fn, code, dev)
    weights = _get(loss_cfg, "LOSS_WEIGHTS")
    corner = bool(_get(loss_cfg, "CORNER_LOSS_REGULARIZATION", False))
    scalars = dict(beta=float(getattr(reg_fn, "beta", 1.0 / 9.0)), cls_weight=float(weights['rcnn_cls_weight']),
                   reg_weight=float(weights['rcnn_reg_weight']),
                   corner_weight=float(weights['rcnn_corner_weight']) if corner else 0.0, corner=corner)
    ws, table = buffers(self, "_modest_roi_loss", ops.roi_loss_workspace_bytes(R), 6, dev)
    if torch.is_grad_enabled() and (cls.requires_grad or reg.requires_grad):
        out = RoiLossFunction.apply(cls, reg, labels, mask, gt.detach(), src.detach(), rois, code_weights, scalars, ws)
    else:
        out, _ = ops.roi_loss(cls.detach(), reg.detach(), labels, mask, gt.detach(), src.detach(), rois, code_weights,
                              want_grad=False, workspace=ws, **scalars)
    values = read_table(table, out, dev)
    tb_dict['rcnn_loss_cls'] = values[0]
    tb_dict['rcnn_loss_reg'] = values[1]
    if corner and values[4] > 0:
        tb_dict['rcnn_loss_corner'] = values[2]
    tb_dict['rcnn_loss'] = values[3]
    return out[3], tb_dict


def bind(cls):
    """set get_loss on a head class (RoIHeadTemplate or a subclass) -> cls; the method it had is kept for the heads that
    override a part of the loss.  Idempotent."""
    if cls.__dict__.get("get_loss") is get_loss:
        return cls
    _ORIGINAL[cls] = cls.__dict__.get("get_loss")
    cls.get_loss = get_loss
    return cls
