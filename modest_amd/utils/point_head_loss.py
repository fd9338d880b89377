"""Drop-in for the ``get_loss`` of OpenPCDet's point heads (``PointHeadBox``, ``PointIntraPartOffsetHead`` and
``PointHeadSimple`` of ``pcdet/models/dense_heads``, over ``get_cls_layer_loss``, ``get_part_layer_loss`` and
``get_box_layer_loss`` of ``point_head_template.py``) on the GPU: what closes every training step of
PointRCNN's, PartA2's and PV-RCNN's point head.  It consumes what ``modest_amd.utils.point_head_targets.assign_stack_targets``
leaves in ``forward_ret_dict``.

One library call (``modest_amd.ops.point_loss``, csrc/point_loss.hip) on PyTorch's current stream computes the classification,
part and box losses and, where a prediction requires a gradient, the gradients of ``point_loss`` in the same pass: no one-hot
tensor, no element-wise chain, nothing kept for autograd but the gradient buffers, and the part and box tensors are read for
positive points only.  ``backward`` is one more library call, which scales those buffers in place by the upstream gradient
read from the device.  ``tb_dict``'s floats are read through a small pinned table after ONE stream synchronise (the reference
waits two to five times).  The workspace and the pinned table are kept on the head and serve one stream at a time.

The terms follow the class the method is bound on: ``PointHeadSimple`` cls; ``PointHeadBox`` cls + box;
``PointIntraPartOffsetHead`` cls + part, plus box iff the head has ``box_layers``.  The number of positives is counted over the
whole stacked batch and the class target is strictly ``label == c + 1``, as in the reference.

Provided: ``SigmoidFocalClassificationLoss`` with alpha 0.25 and gamma 2, ``WeightedSmoothL1Loss`` for the box term, float32
predictions.  Another ``cls_loss_func``, another ``reg_loss_func`` with the box term on (the reference itself cannot run
``F.smooth_l1_loss`` there: it passes ``weights=``) and predictions of another type raise ``NotImplementedError`` naming the
option; the limits (``ValueError``): 1 .. 32 classes, code size 1 .. 16, at most 2^24 points.  A head whose class overrides
``get_cls_layer_loss``, ``get_part_layer_loss`` or ``get_box_layer_loss`` below the bound class is handed to the method this
one replaced.  The dict in ``forward_ret_dict`` is left as found.

``bind(cls, terms)`` sets the method on a head class; ``pcdet_bind.bind_point_loss()`` does that for the reference's three.
"""
import torch

from ._head_loss import HeadLossFunction, _get, buffers, code_weights_tensor, read_table, replaced_get_loss

CLS_LOSS_FUNC = "SigmoidFocalClassificationLoss"
REG_LOSS_FUNC = "WeightedSmoothL1Loss"
ALPHA, GAMMA = 0.25, 2.0
TERMS = {"PointHeadSimple": ("cls",), "PointHeadBox": ("cls", "box"), "PointIntraPartOffsetHead": ("cls", "part", "box?")}
PARTS = ("get_cls_layer_loss", "get_part_layer_loss", "get_box_layer_loss")   # an override of any: the head computes another loss

_ORIGINAL = {}   # class -> the get_loss that bind() replaced on it (None: it had none of its own)
_TERMS = {}      # class -> its terms: "cls", "part", "box", or "box?" (iff the head has box_layers)


class PointLossFunction(HeadLossFunction):
    """(cls_preds, labels, part_preds | None, part_labels, box_preds | None, box_labels, code_weights, scalars, workspace) ->
    table (5): [point_loss_cls, point_loss_part, point_loss_box, point_loss, point_pos_num]"""
    OPS, PREDS, WORD = ("point_loss", "point_loss_backward"), (0, 2, 4), "point-head"


def get_loss(self, tb_dict=None):
    """-> (point_loss, tb_dict): point_loss a 0-dim device tensor with its gradient function; tb_dict the dict passed in (or a
    new one) updated with the Python floats point_loss_cls, point_pos_num and, for the terms of the head, point_loss_part and
    point_loss_box -- the reference's keys in the reference's order; no key for the total"""
    from .. import ops
    base, original = replaced_get_loss(type(self), _ORIGINAL, PARTS)
    if original is not None:
        return original(self, tb_dict)
    tb_dict = {} if tb_dict is None else tb_dict
    terms = _TERMS[base] if base is not None else TERMS[type(self).__name__]      # called unbound: by the class's name
    with_part = "part" in terms
    with_box = "box" in terms or ("box?" in terms and getattr(self, "box_layers", None) is not None)
    cls_fn = self.cls_loss_func
    if type(cls_fn).__name__ != CLS_LOSS_FUNC:
        raise NotImplementedError(f"cls_loss_func = {type(cls_fn).__name__} is not provided by modest_amd's point-head loss: "
                                  f"{CLS_LOSS_FUNC} only")
    alpha, gamma = float(getattr(cls_fn, "alpha", ALPHA)), float(getattr(cls_fn, "gamma", GAMMA))
    if alpha != ALPHA or gamma != GAMMA:
        raise NotImplementedError(f"cls_loss_func with alpha = {alpha}, gamma = {gamma} is not provided: alpha {ALPHA}, gamma {GAMMA} only")
    reg_fn = getattr(self, "reg_loss_func", None)
    if with_box and type(reg_fn).__name__ != REG_LOSS_FUNC:
        name = getattr(reg_fn, "__name__", type(reg_fn).__name__)
        raise NotImplementedError(f"reg_loss_func = {name} is not provided for the box term: LOSS_REG: {REG_LOSS_FUNC} only")
    ret = self.forward_ret_dict
    keys = [("point_cls_preds", True), ("point_cls_labels", False)]
    if with_part:
        keys += [("point_part_preds", True), ("point_part_labels", False)]
    if with_box:
        keys += [("point_box_preds", True), ("point_box_labels", False)]
    for key, pred in keys:
        t = ret[key]
        if pred and torch.is_tensor(t) and t.dtype != torch.float32:
            raise NotImplementedError(f"{key} of {t.dtype} (mixed precision) is not provided: float32 predictions only")
    labels, cls = ret["point_cls_labels"], ret["point_cls_preds"]
    K = int(self.num_class)
    if K < 1 or K > ops.POINT_LOSS_MAX_CLASS:
        raise ValueError(f"num_class = {K} is outside the limit of 1 .. {ops.POINT_LOSS_MAX_CLASS}")
    N = int(labels.numel())
    if N > ops.POINT_LOSS_MAX_ROWS:
        raise ValueError(f"point_cls_labels has {N} rows, above the limit of {ops.POINT_LOSS_MAX_ROWS}")
    if cls.numel() != N * K:
        raise ValueError(f"point_cls_preds has {cls.numel()} elements, expected {N} rows of num_class = {K}")
    part = part_t = box = box_t = code_weights = None
    if with_part:
        part, part_t = ret["point_part_preds"], ret["point_part_labels"]
        for t, name in ((part, "point_part_preds"), (part_t, "point_part_labels")):
            if t.numel() != N * ops.POINT_LOSS_PART:
                raise ValueError(f"{name} has {t.numel()} elements, expected {N} rows of {ops.POINT_LOSS_PART} columns")
    code = 0
    if with_box:
        box, box_t = ret["point_box_preds"], ret["point_box_labels"]
        code = int(box.shape[-1])
        if code < 1 or code > ops.POINT_LOSS_MAX_CODE:
            raise ValueError(f"code size = {code} is outside the limit of 1 .. {ops.POINT_LOSS_MAX_CODE}")
        for t, name in ((box, "point_box_preds"), (box_t, "point_box_labels")):
            if t.numel() != N * code:
                raise ValueError(f"{name} has {t.numel()} elements, expected {N} rows of code size {code}")
    for key, _ in keys:
        if not torch.is_tensor(ret[key]) or not ret[key].is_cuda:
            raise ValueError(f"{key} must be a device tensor (PyTorch-ROCm 'cuda')")
    dev = cls.device
    if labels.dtype not in (torch.int32, torch.int64):
        labels = labels.long()
    labels = labels.reshape(N).contiguous()
    cls = cls.reshape(-1, K)                         # a view wherever the strides allow it
    if with_part:
        part, part_t = part.reshape(-1, ops.POINT_LOSS_PART), part_t.detach().float().reshape(-1, ops.POINT_LOSS_PART)
    if with_box:
        box, box_t = box.reshape(-1, code), box_t.detach().float().reshape(-1, code)
        code_weights = code_weights_tensor(reg_fn, code, dev)
        if code_weights.numel() != code:
            raise ValueError(f"code_weights has {code_weights.numel()} elements, the code size is {code}")
    weights = _get(_get(self.model_cfg, "LOSS_CONFIG"), "LOSS_WEIGHTS")
    scalars = dict(beta=float(getattr(reg_fn, "beta", 1.0 / 9.0)) if with_box else 1.0 / 9.0,
                   cls_weight=float(weights["point_cls_weight"]),
                   part_weight=float(weights["point_part_weight"]) if with_part else 0.0,
                   box_weight=float(weights["point_box_weight"]) if with_box else 0.0)
    ws, table = buffers(self, "_modest_point_loss", ops.point_loss_workspace_bytes(N), 5, dev)
    preds = [t for t in (cls, part, box) if t is not None]
    if torch.is_grad_enabled() and any(t.requires_grad for t in preds):
        out = PointLossFunction.apply(cls, labels, part, part_t, box, box_t, code_weights, scalars, ws)
    else:
        out, _ = ops.point_loss(cls.detach(), labels, None if part is None else part.detach(), part_t,
                                None if box is None else box.detach(), box_t, code_weights, want_grad=False, workspace=ws,
                                **scalars)
    values = read_table(table, out, dev)
    tb_dict["point_loss_cls"] = values[0]
    tb_dict["point_pos_num"] = values[4]
    if with_part:
        tb_dict["point_loss_part"] = values[1]
    if with_box:
        tb_dict["point_loss_box"] = values[2]
    return out[3], tb_dict


def bind(cls, terms=None):
    """set get_loss on a point head class -> cls; `terms` its terms ("cls", "part", "box", or "box?": the box term iff the head
    has box_layers), by default those of the reference class of that name.  The method it had is kept for the heads that
    override a part of the loss.  Idempotent."""
    if cls.__dict__.get("get_loss") is get_loss:
        return cls
    if terms is None:
        terms = TERMS.get(cls.__name__)
        if terms is None:
            raise ValueError(f"bind({cls.__name__}) needs its terms: {cls.__name__} is none of {sorted(TERMS)}")
    terms = tuple(terms)
    if "cls" not in terms or any(t not in ("cls", "part", "box", "box?") for t in terms):
        raise ValueError(f"terms = {terms}: 'cls' and any of 'part', 'box', 'box?'")
    _ORIGINAL[cls] = cls.__dict__.get("get_loss")
    _TERMS[cls] = terms
    cls.get_loss = get_loss
    return cls
