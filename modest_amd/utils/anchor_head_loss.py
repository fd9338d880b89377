"""Drop-in for ``AnchorHeadTemplate.get_loss`` of OpenPCDet's anchor heads
(``pcdet/models/dense_heads/anchor_head_template.py``, over ``SigmoidFocalClassificationLoss``, ``WeightedSmoothL1Loss`` /
``WeightedL1Loss`` and ``WeightedCrossEntropyLoss`` of ``pcdet/utils/loss_utils.py``) on the GPU:
what closes every training step of PointPillars, SECOND, PV-RCNN, Voxel R-CNN and PartA2.

One library call (``modest_amd.ops.anchor_loss``, csrc/anchor_loss.hip) on PyTorch's current stream computes the three losses
and, where a prediction requires a gradient, the three gradients of ``rpn_loss`` in the same pass: no one-hot tensor, no
repeated anchors, no concatenated box tensors, nothing kept for autograd but the three gradient buffers.  ``backward`` is one
more library call, which scales those buffers in place by the upstream gradient read from the device.  ``tb_dict``'s floats
are read through a small pinned table after ONE stream synchronise (the reference waits four times).  The flattened anchors,
the workspace and the pinned table are kept on the head.

Provided: a single head (``USE_MULTIHEAD: False``), the reference's three loss classes (the focal loss with alpha = 0.25 and
gamma = 2), float32 predictions.  ``USE_MULTIHEAD: True``, another ``cls_loss_func`` / ``reg_loss_func`` / ``dir_loss_func`` and
predictions of another type raise ``NotImplementedError`` naming the option; the limits (``ValueError``): ``num_class`` <= 32,
code size <= 16, ``NUM_DIR_BINS`` <= 8, batch <= 65535.  A head whose class overrides ``get_cls_layer_loss`` or
``get_box_reg_layer_loss`` (``AnchorHeadMulti``) is handed to the method this one replaced.

One visible difference: with ``num_class == 1`` the reference overwrites the positive labels in
``forward_ret_dict['box_cls_labels']`` with 1; this method leaves the dict as it found it.

``bind(cls)`` sets the method on a head class; ``pcdet_bind.bind_anchor_loss()`` does that for the reference's
``AnchorHeadTemplate``.
"""
import torch

from ._anchors import flat_anchors as _flat_anchors
from ._head_loss import HeadLossFunction, _get, buffers, code_weights_tensor, read_table, replaced_get_loss

CLS_LOSS = "SigmoidFocalClassificationLoss"
REG_LOSSES = ("WeightedSmoothL1Loss", "WeightedL1Loss")
DIR_LOSS = "WeightedCrossEntropyLoss"
PARTS = ("get_cls_layer_loss", "get_box_reg_layer_loss")   # an override of either: the head computes another loss

_ORIGINAL = {}   # class -> the get_loss that bind() replaced on it (None: it had none of its own)


class AnchorLossFunction(HeadLossFunction):
    """(cls_preds, box_preds, dir_preds or None, labels, reg_targets, anchors, code_weights, scalars, workspace) -> losses (4):
    [rpn_loss_cls, rpn_loss_loc, rpn_loss_dir, rpn_loss]"""
    OPS, PREDS, WORD = ("anchor_loss", "anchor_loss_backward"), (0, 1, 2), "anchor"


def get_loss(self):
    """-> (rpn_loss, tb_dict): rpn_loss a 0-dim device tensor with its gradient function, tb_dict the Python floats
    rpn_loss_cls, rpn_loss_loc, rpn_loss_dir (only with a direction head) and rpn_loss"""
    from .. import ops
    _, original = replaced_get_loss(type(self), _ORIGINAL, PARTS)
    if original is not None:
        return original(self)
    model_cfg = self.model_cfg
    if _get(model_cfg, "USE_MULTIHEAD", False) or getattr(self, "use_multihead", False):
        raise NotImplementedError("USE_MULTIHEAD: True is not provided by modest_amd's anchor loss")
    cls_fn, reg_fn, dir_fn = self.cls_loss_func, self.reg_loss_func, self.dir_loss_func
    if type(cls_fn).__name__ != CLS_LOSS:
        raise NotImplementedError(f"cls_loss_func = {type(cls_fn).__name__} is not provided: {CLS_LOSS} only")
    alpha, gamma = float(getattr(cls_fn, "alpha", 0.25)), float(getattr(cls_fn, "gamma", 2.0))
    if alpha != 0.25 or gamma != 2.0:
        raise NotImplementedError(f"cls_loss_func with alpha = {alpha}, gamma = {gamma} is not provided: alpha = 0.25, gamma = 2.0 only")
    if type(reg_fn).__name__ not in REG_LOSSES:
        raise NotImplementedError(f"reg_loss_func = {type(reg_fn).__name__} (REG_LOSS_TYPE) is not provided: one of {REG_LOSSES}")
    ret = self.forward_ret_dict
    cls_preds, box_preds = ret['cls_preds'], ret['box_preds']
    dir_preds = ret.get('dir_cls_preds', None)
    if dir_preds is not None and type(dir_fn).__name__ != DIR_LOSS:
        raise NotImplementedError(f"dir_loss_func = {type(dir_fn).__name__} is not provided: {DIR_LOSS} only")
    for t, name in ((cls_preds, "cls_preds"), (box_preds, "box_preds"), (dir_preds, "dir_cls_preds")):
        if t is not None and t.dtype != torch.float32:
            raise NotImplementedError(f"{name} of {t.dtype} (mixed precision) is not provided: float32 predictions only")
    labels, targets = ret['box_cls_labels'], ret['box_reg_targets']
    loss_cfg = _get(model_cfg, "LOSS_CONFIG")
    weights = _get(loss_cfg, "LOSS_WEIGHTS")
    batch_size = int(cls_preds.shape[0])
    num_class = int(self.num_class)
    cls = cls_preds.reshape(batch_size, -1, num_class)
    box = box_preds.reshape(batch_size, -1, box_preds.shape[-1] // int(self.num_anchors_per_location))
    N, code = int(box.shape[1]), int(box.shape[2])
    bins = 0
    dirp = None
    if dir_preds is not None:
        bins = int(_get(model_cfg, "NUM_DIR_BINS"))
        dirp = dir_preds.reshape(batch_size, -1, bins)
    for value, limit, name in ((num_class, ops.ANCHOR_LOSS_MAX_CLASS, "num_class"), (code, ops.ANCHOR_LOSS_MAX_CODE, "code size"),
                               (bins, ops.ANCHOR_LOSS_MAX_BINS, "NUM_DIR_BINS"), (batch_size, ops.ANCHOR_LOSS_MAX_BATCH, "batch_size")):
        if value > limit:
            raise ValueError(f"{name} = {value} is above the limit of {limit}")
    for t, name in ((cls_preds, "cls_preds"), (box_preds, "box_preds"), (dir_preds, "dir_cls_preds"),
                    (labels, "box_cls_labels"), (targets, "box_reg_targets")):
        if t is not None and (not torch.is_tensor(t) or not t.is_cuda):
            raise ValueError(f"{name} must be a device tensor (PyTorch-ROCm 'cuda')")
    if labels.dtype not in (torch.int32, torch.int64):
        labels = labels.long()
    labels = labels.reshape(batch_size, -1).contiguous()
    targets = targets.float().reshape(batch_size, -1, targets.shape[-1]).contiguous()
    anchors = _flat_anchors(self)
    code_weights = code_weights_tensor(reg_fn, code, cls.device)
    scalars = dict(beta=float(getattr(reg_fn, "beta", 0.0)), dir_offset=float(_get(model_cfg, "DIR_OFFSET", 0.0)) if dirp is not None else 0.0,
                   cls_weight=float(weights['cls_weight']), loc_weight=float(weights['loc_weight']),
                   dir_weight=float(weights['dir_weight']) if dirp is not None else 0.0, alpha=alpha, gamma=gamma)
    ws, table = buffers(self, "_modest_anchor_loss", ops.anchor_loss_workspace_bytes(batch_size, N), 4, cls.device)
    wants = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (cls, box, dirp))
    if wants:
        losses = AnchorLossFunction.apply(cls, box, dirp, labels, targets, anchors, code_weights, scalars, ws)
    else:
        losses, _ = ops.anchor_loss(cls, box, dirp, labels, targets, anchors, code_weights, want_grad=False, workspace=ws, **scalars)
    values = read_table(table, losses, cls.device)
    tb_dict = {'rpn_loss_cls': values[0], 'rpn_loss_loc': values[1]}
    if dirp is not None:
        tb_dict['rpn_loss_dir'] = values[2]
    tb_dict['rpn_loss'] = values[3]
    return losses[3], tb_dict


def bind(cls):
    """set get_loss on a head class (AnchorHeadTemplate or a subclass) -> cls; the method it had is kept for the heads
    that override a part of the loss.  Idempotent."""
    if cls.__dict__.get("get_loss") is get_loss:
        return cls
    _ORIGINAL[cls] = cls.__dict__.get("get_loss")
    cls.get_loss = get_loss
    return cls
