"""Drop-in for ``PointHeadTemplate.assign_stack_targets`` of OpenPCDet's point heads
(``pcdet/models/dense_heads/point_head_template.py``) on the GPU: the target assignment of
``PointHeadBox`` (PointRCNN), ``PointIntraPartOffsetHead`` (PartA2) and ``PointHeadSimple`` (PV-RCNN).

One library call (``modest_amd.ops.point_targets``, csrc/point_targets.hip) assigns the whole stacked batch on PyTorch's
current stream: no loop over the samples, no boolean-mask indexing, nothing is copied to the host, nothing synchronises.
The coder's ``mean_size`` is uploaded at the first call and kept on the device.

Provided: ``set_ignore_flag=True, use_ball_constraint=False``, what all three heads pass.  The ball-constraint branch
raises ``NotImplementedError``.  ``bind(cls)`` sets the method on a head class; ``pcdet_bind.install(point_targets=True)``
does that for the reference's ``PointHeadTemplate``.
"""
import numpy as np
import torch


def _mean_size(coder, device):
    """the coder's (n_cls, 3) table as a float32 device tensor, uploaded once per coder, table and device; None without"""
    if not getattr(coder, 'use_mean_size', False):
        return None
    table = coder.mean_size
    cached = getattr(coder, '_modest_mean_size', None)
    version = table._version if torch.is_tensor(table) else None
    if cached is not None and cached[0] is table and cached[1] == version and cached[2].device == device:
        return cached[2]
    if torch.is_tensor(table):
        dev = table.detach().to(device=device, dtype=torch.float32).contiguous()
    else:
        dev = torch.from_numpy(np.ascontiguousarray(np.array(table, dtype=np.float32))).to(device)
    dev = dev.reshape(-1, 3)
    coder._modest_mean_size = (table, version, dev)
    return dev


def assign_stack_targets(self, points, gt_boxes, extend_gt_boxes=None, ret_box_labels=False, ret_part_labels=False,
                         set_ignore_flag=True, use_ball_constraint=False, central_radius=2.0):
    """
    Args:
        points: (N1 + N2 + N3 + ..., 4) [bs_idx, x, y, z]
        gt_boxes: (B, M, 8)
        extend_gt_boxes: (B, M, 8)
    Returns:
        point_cls_labels: (N1 + N2 + N3 + ...) int64, 0: background, -1: ignored
        point_box_labels: (N1 + N2 + N3 + ..., 8) or None
        point_part_labels: (N1 + N2 + N3 + ..., 3) or None
    """
    from .. import ops
    assert len(points.shape) == 2 and points.shape[1] == 4, 'points.shape=%s' % str(points.shape)
    assert len(gt_boxes.shape) == 3 and gt_boxes.shape[2] == 8, 'gt_boxes.shape=%s' % str(gt_boxes.shape)
    assert extend_gt_boxes is None or len(extend_gt_boxes.shape) == 3 and extend_gt_boxes.shape[2] == 8, \
        'extend_gt_boxes.shape=%s' % str(extend_gt_boxes.shape)
    assert set_ignore_flag != use_ball_constraint, 'Choose one only!'
    if use_ball_constraint:
        raise NotImplementedError("use_ball_constraint=True (central_radius) is not provided by modest_amd: the three "
                                  "point heads of the reference pass set_ignore_flag=True")
    if extend_gt_boxes is None:
        raise ValueError("set_ignore_flag=True needs extend_gt_boxes")
    mean_size = None
    if ret_box_labels:
        mean_size = _mean_size(self.box_coder, points.device if torch.is_tensor(points) else None)
    gt = gt_boxes if gt_boxes.dtype == torch.float32 else gt_boxes.float()
    ext = extend_gt_boxes if extend_gt_boxes.dtype == torch.float32 else extend_gt_boxes.float()
    pts = points if points.dtype == torch.float32 else points.float()
    labels, box, part = ops.point_targets(pts, gt, ext, int(self.num_class), mean_size=mean_size,
                                          want_box=bool(ret_box_labels), want_part=bool(ret_part_labels))
    return {'point_cls_labels': labels, 'point_box_labels': box, 'point_part_labels': part}


def bind(cls):
    """set assign_stack_targets on a head class (PointHeadTemplate or a subclass) -> cls"""
    cls.assign_stack_targets = assign_stack_targets
    return cls
