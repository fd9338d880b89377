"""Drop-ins for ``generate_predicted_boxes`` of OpenPCDet's three kinds of head on the GPU:
``AnchorHeadTemplate`` (pcdet/models/dense_heads/anchor_head_template.py), ``PointHeadTemplate``
(pcdet/models/dense_heads/point_head_template.py) and ``RoIHeadTemplate`` (pcdet/models/roi_heads/roi_head_template.py), over
``ResidualCoder`` / ``PointResidualCoder`` ``.decode_torch``, ``limit_period`` and ``rotate_points_along_z``.  It is what stands
between a head's raw predictions and ``proposal_layer`` / ``post_processing``: every test-time forward of every detector, and
every training step of the two-stage models (``predict_boxes_when_training``).

Each method is ONE library call (``modest_amd.ops.anchor_decode`` / ``point_decode`` / ``roi_decode``, csrc/box_decode.hip) on
PyTorch's current stream: it only enqueues, allocates nothing but the output and never waits for the device.  The anchors are
one (N, 7 + C) table (``_anchors.flat_anchors``, shared with the anchor loss) read once per row for every sample: no
``(B, N, 7)`` repeat; no ``local_rois`` clone, rotation matrices or ``matmul`` on the RoI head; ``points`` is read through its
row stride, so the view ``point_coords[:, 1:4]`` is not copied.

Signatures and return values are the reference's:
  anchor head  (batch_cls_preds, batch_box_preds): ``cls_preds.view(B, N, -1).float()`` -- a view, its graph is kept -- and a new
               (B, N, 7 + C) tensor;
  point head   (point_cls_preds, point_box_preds): the class predictions as given and a new (N, 7 + C) tensor;
  RoI head     (batch_cls_preds, batch_box_preds), both reshaped to (B, -1, .).
THE ONE DIFFERENCE: the decoded boxes are computed from detached inputs and carry no ``grad_fn``.  Every consumer in the
reference rebuilds its tensors from them without a graph (``proposal_layer``, ``post_processing``).  Inputs are left untouched.

Not provided (``NotImplementedError`` before anything is launched): list-valued ``cls_preds`` / ``box_preds``
(``USE_MULTIHEAD``), ``PreviousResidualDecoder`` / ``PreviousResidualRoIDecoder``, a coder class that is none of
``ResidualCoder`` (anchor and RoI heads) / ``PointResidualCoder`` (point heads), ``encode_angle_by_sincos`` on a RoI head (the
reference's own ``view`` fails there), predictions that are not float32.  Limits (``ValueError``): code size at most 16,
1 .. 8 direction bins, 1 .. 32 classes, at most 2^31 - 1 rows per call (B * N for the anchor head: the kernels count rows in an
int and element offsets in int64).

``bind(cls, kind)`` sets the method on a head class; ``pcdet_bind.bind_box_decode()`` does that for the reference's three
templates.  A head that overrides ``generate_predicted_boxes`` itself keeps its own, as Python's MRO gives.
"""
import torch

from ._anchors import flat_anchors
from ._head_loss import _get

METHOD = "generate_predicted_boxes"
PREVIOUS = ("PreviousResidualDecoder", "PreviousResidualRoIDecoder")

_ORIGINAL = {}   # class -> the generate_predicted_boxes that bind() replaced on it (None: it had none of its own)


def _coder(head, wanted):
    name = type(head.box_coder).__name__
    if name in PREVIOUS:
        raise NotImplementedError(f"box_coder = {name} is not provided by modest_amd's box decoding: {wanted} only")
    if name != wanted:
        raise NotImplementedError(f"box_coder = {name} is not provided by modest_amd's box decoding: {wanted} only")
    return head.box_coder


def _float32(named):
    for name, t in named:
        if t is not None and t.dtype != torch.float32:
            raise NotImplementedError(f"{name} of {t.dtype} (mixed precision) is not provided: float32 predictions only")


def anchor_generate_predicted_boxes(self, batch_size, cls_preds, box_preds, dir_cls_preds=None):
    """-> (batch_cls_preds (B, N, num_class) -- cls_preds viewed, as float32 --, batch_box_preds (B, N, 7 + C) without a graph)"""
    from .. import ops
    if isinstance(cls_preds, (list, tuple)) or isinstance(box_preds, (list, tuple)) or isinstance(dir_cls_preds, (list, tuple)) \
            or getattr(self, "use_multihead", False):
        raise NotImplementedError("USE_MULTIHEAD: True (list-valued predictions) is not provided by modest_amd's box decoding")
    coder = _coder(self, "ResidualCoder")
    _float32((("box_preds", box_preds), ("dir_cls_preds", dir_cls_preds)))
    sincos = bool(getattr(coder, "encode_angle_by_sincos", False))
    batch_size = int(batch_size)
    anchors = flat_anchors(self)
    N, cols = int(anchors.shape[0]), int(anchors.shape[1])
    if box_preds.numel() % max(batch_size * N, 1) or batch_size * N == 0:
        raise ValueError(f"box_preds has {box_preds.numel()} elements, which is no multiple of batch_size * anchors = {batch_size} * {N}")
    code = box_preds.numel() // (batch_size * N)
    if code > ops.BOX_DECODE_MAX_CODE:
        raise ValueError(f"code size = {code} is outside the limit of {8 if sincos else 7} .. {ops.BOX_DECODE_MAX_CODE} box columns")
    if code != cols + (1 if sincos else 0):
        raise ValueError(f"code size = {code} does not go with anchors of {cols} columns" + (" and encode_angle_by_sincos" if sincos else ""))
    if batch_size * N > ops.BOX_DECODE_MAX_ROWS:
        raise ValueError(f"box_preds has {batch_size * N} rows, above the limit of {ops.BOX_DECODE_MAX_ROWS} rows per call")
    scalars = {}
    dirp = None
    if dir_cls_preds is not None:
        bins = int(_get(self.model_cfg, "NUM_DIR_BINS"))
        if bins < 1 or bins > ops.BOX_DECODE_MAX_BINS:
            raise ValueError(f"NUM_DIR_BINS = {bins} is outside the limit of 1 .. {ops.BOX_DECODE_MAX_BINS} direction bins")
        if dir_cls_preds.numel() != batch_size * N * bins:
            raise ValueError(f"dir_cls_preds has {dir_cls_preds.numel()} elements, expected {batch_size} * {N} rows of NUM_DIR_BINS = {bins}")
        dirp = dir_cls_preds.detach().reshape(batch_size, N, bins).contiguous()
        scalars = dict(dir_offset=float(_get(self.model_cfg, "DIR_OFFSET")), dir_limit_offset=float(_get(self.model_cfg, "DIR_LIMIT_OFFSET")))
    batch_cls_preds = cls_preds.view(batch_size, N, -1).float()
    box = box_preds.detach().reshape(batch_size, N, code).contiguous()
    return batch_cls_preds, ops.anchor_decode(box, anchors, dirp, sincos=sincos, **scalars)


def point_generate_predicted_boxes(self, points, point_cls_preds, point_box_preds):
    """-> (point_cls_preds as given, point_box_preds (N, 7 + C) without a graph)"""
    from .. import ops
    if isinstance(point_cls_preds, (list, tuple)) or isinstance(point_box_preds, (list, tuple)):
        raise NotImplementedError("list-valued predictions are not provided by modest_amd's box decoding")
    coder = _coder(self, "PointResidualCoder")
    _float32((("point_cls_preds", point_cls_preds), ("point_box_preds", point_box_preds), ("points", points)))
    if point_box_preds.ndim != 2 or point_cls_preds.ndim != 2:
        raise ValueError(f"point_box_preds {tuple(point_box_preds.shape)} and point_cls_preds {tuple(point_cls_preds.shape)} must be "
                         f"(N, 8 + C) and (N, num_class)")
    N, code = int(point_box_preds.shape[0]), int(point_box_preds.shape[1])
    K = int(point_cls_preds.shape[1])
    if code < 8 or code > ops.BOX_DECODE_MAX_CODE:
        raise ValueError(f"code size = {code} is outside the limit of 8 .. {ops.BOX_DECODE_MAX_CODE} box columns")
    if K < 1 or K > ops.BOX_DECODE_MAX_CLASS:
        raise ValueError(f"num_class = {K} is outside the limit of 1 .. {ops.BOX_DECODE_MAX_CLASS} class columns")
    if N > ops.BOX_DECODE_MAX_ROWS:
        raise ValueError(f"point_box_preds has {N} rows, above the limit of {ops.BOX_DECODE_MAX_ROWS} rows per call")
    mean = None
    if getattr(coder, "use_mean_size", True):
        mean = coder.mean_size
        if mean.ndim != 2 or mean.shape[1] != 3 or mean.shape[0] < K:
            raise ValueError(f"mean_size {tuple(mean.shape)} has no row for each of the {K} classes")
        mean = mean.detach().float()[:K].contiguous()
    pts = points.detach()
    if pts.ndim == 2 and pts.shape[0] > 0 and pts.stride(1) != 1:
        pts = pts.contiguous()
    boxes = ops.point_decode(point_box_preds.detach().contiguous(), pts, point_cls_preds.detach().contiguous(), mean)
    return point_cls_preds, boxes


def roi_generate_predicted_boxes(self, batch_size, rois, cls_preds, box_preds):
    """-> (batch_cls_preds (B, M, num_class or 1) -- cls_preds viewed --, batch_box_preds (B, M, code) without a graph)"""
    from .. import ops
    if isinstance(cls_preds, (list, tuple)) or isinstance(box_preds, (list, tuple)):
        raise NotImplementedError("list-valued predictions are not provided by modest_amd's box decoding")
    coder = _coder(self, "ResidualCoder")
    if getattr(coder, "encode_angle_by_sincos", False):
        raise NotImplementedError("encode_angle_by_sincos on a RoI head is not provided (the reference's own view fails there)")
    _float32((("box_preds", box_preds), ("rois", rois)))
    code = int(coder.code_size)
    if code < 7 or code > ops.BOX_DECODE_MAX_CODE:
        raise ValueError(f"code size = {code} is outside the limit of 7 .. {ops.BOX_DECODE_MAX_CODE} box columns")
    batch_size = int(batch_size)
    if box_preds.numel() % code or int(rois.shape[-1]) != code or rois.numel() != box_preds.numel():
        raise ValueError(f"rois {tuple(rois.shape)} and box_preds {tuple(box_preds.shape)} must hold the same rows of the code size {code}")
    R = box_preds.numel() // code
    if R > ops.BOX_DECODE_MAX_ROWS:
        raise ValueError(f"box_preds has {R} rows, above the limit of {ops.BOX_DECODE_MAX_ROWS} rows per call")
    batch_cls_preds = cls_preds.view(batch_size, -1, cls_preds.shape[-1])
    boxes = ops.roi_decode(rois.detach().contiguous(), box_preds.detach().reshape(-1, code).contiguous())
    return batch_cls_preds, boxes.view(batch_size, -1, code)


KINDS = {"AnchorHeadTemplate": anchor_generate_predicted_boxes, "PointHeadTemplate": point_generate_predicted_boxes,
         "RoIHeadTemplate": roi_generate_predicted_boxes}


def bind(cls, kind=None):
    """set generate_predicted_boxes on a head class -> cls; `kind` one of KINDS' names, by default the class's own name.  The
    method it had is kept in _ORIGINAL.  Idempotent."""
    kind = cls.__name__ if kind is None else kind
    method = KINDS.get(kind)
    if method is None:
        raise ValueError(f"bind({cls.__name__}) needs its kind: one of {sorted(KINDS)}")
    if cls.__dict__.get(METHOD) is method:
        return cls
    _ORIGINAL[cls] = cls.__dict__.get(METHOD)
    setattr(cls, METHOD, method)
    return cls


def unbind(cls):
    """put back what bind() replaced on cls -> cls"""
    if cls in _ORIGINAL:
        original = _ORIGINAL.pop(cls)
        if original is None:
            delattr(cls, METHOD)
        else:
            setattr(cls, METHOD, original)
    return cls
