"""Drop-in for OpenPCDet's ``pcdet.models.dense_heads.target_assigner.axis_aligned_target_assigner`` on the GPU
(DESIGN.md section 7i): ``AxisAlignedTargetAssigner(model_cfg, class_names, box_coder, match_height=False)`` with
``assign_targets(all_anchors, gt_boxes_with_classes)`` returning the same dict.

One library call (``modest_amd.ops.anchor_targets``, csrc/anchor_targets.hip) assigns the whole batch and all anchor
classes on PyTorch's current stream: nothing is copied to the host, nothing synchronises, the (anchors, gts) IoU matrix
is never formed.  The flattened anchors and the class table are built at the first call and kept on the device, keyed
on the anchor tensors handed in (they are constants of the head).

Provided: the branch every config of the reference takes -- ``POS_FRACTION < 0``, ``NORM_BY_NUM_EXAMPLES: False``,
``MATCH_HEIGHT: False`` -- with ``ResidualCoder`` (7 + C columns, optionally ``encode_angle_by_sincos``), single head
and ``USE_MULTIHEAD``.  Each other option raises ``NotImplementedError`` in the constructor.  ``bind`` it under the
reference's name with ``pcdet_bind.install(anchor_targets=True)``.
"""
import numpy as np
import torch


def output_layout(anchor_shapes, use_multihead):
    """anchor_shapes: per class the (z, y, x, sizes, rotations, ...) shape of its anchors.
    -> (rows per class, [(first row, rows, k, stride, offset)], rows per sample): row i of a class, in the order the
    reference flattens that class, goes to output row (i // k) * stride + offset + i % k."""
    rows = [int(np.prod(s[:5])) for s in anchor_shapes]
    table, first = [], 0
    if use_multihead:   # classes concatenated
        for n in rows:
            table.append((first, n, max(n, 1), 0, first))
            first += n
        return rows, table, first
    per_loc = [int(s[3]) * int(s[4]) for s in anchor_shapes]
    locs = {int(np.prod(s[:3])) for s in anchor_shapes}
    if len(locs) > 1:
        raise ValueError(f"the anchor classes of a single head must share one feature map, got {[tuple(s[:3]) for s in anchor_shapes]}")
    stride, off = sum(per_loc), 0
    for n, k in zip(rows, per_loc):   # location-major, the classes' anchors interleaved
        table.append((first, n, max(k, 1), stride, off))
        first += n
        off += k
    return rows, table, first


class AxisAlignedTargetAssigner(object):
    def __init__(self, model_cfg, class_names, box_coder, match_height=False):
        super().__init__()
        anchor_generator_cfg = model_cfg.ANCHOR_GENERATOR_CONFIG
        anchor_target_cfg = model_cfg.TARGET_ASSIGNER_CONFIG
        if anchor_target_cfg.POS_FRACTION >= 0:
            raise NotImplementedError("POS_FRACTION >= 0 samples with torch's random generator: not provided by modest_amd "
                                      "(every config of the reference sets -1.0)")
        if match_height:
            raise NotImplementedError("MATCH_HEIGHT: True (3-D IoU matching) is not provided by modest_amd")
        if anchor_target_cfg.NORM_BY_NUM_EXAMPLES:
            raise NotImplementedError("NORM_BY_NUM_EXAMPLES: True is not provided by modest_amd")
        self.box_coder = box_coder
        self.match_height = match_height
        self.class_names = np.array(class_names)
        self.anchor_class_names = [config['class_name'] for config in anchor_generator_cfg]
        self.pos_fraction = None
        self.sample_size = anchor_target_cfg.SAMPLE_SIZE
        self.norm_by_num_examples = anchor_target_cfg.NORM_BY_NUM_EXAMPLES
        self.matched_thresholds = {}
        self.unmatched_thresholds = {}
        for config in anchor_generator_cfg:
            self.matched_thresholds[config['class_name']] = config['matched_threshold']
            self.unmatched_thresholds[config['class_name']] = config['unmatched_threshold']
        self.use_multihead = model_cfg.get('USE_MULTIHEAD', False)
        self.sincos = bool(getattr(box_coder, 'encode_angle_by_sincos', False))
        self._key = None
        self._tables = None

    def _device_tables(self, all_anchors):
        """flattened anchors + class table on the device, built once per list of anchor tensors"""
        key = self._key
        if key is not None and len(key) == len(all_anchors) and all(a is b and a._version == v for a, (b, v) in zip(all_anchors, key)):
            return self._tables
        if len(all_anchors) != len(self.anchor_class_names):
            raise ValueError(f"{len(all_anchors)} anchor tensors for {len(self.anchor_class_names)} anchor classes")
        for a in all_anchors:
            if not a.is_cuda or a.dtype != torch.float32 or a.ndim != 6 or a.shape[-1] < 7:
                raise ValueError("anchors must be float32 device tensors of shape (z, y, x, sizes, rotations, 7 + C)")
        cols = int(all_anchors[0].shape[-1])
        dev = all_anchors[0].device
        if any(a.shape[-1] != cols or a.device != dev for a in all_anchors):
            raise ValueError("the anchor tensors must share their last dimension and their device")
        rows, table, n_out = output_layout([tuple(a.shape) for a in all_anchors], self.use_multihead)
        if self.use_multihead:
            flat = [a.permute(3, 4, 0, 1, 2, 5).contiguous().view(-1, cols) for a in all_anchors]
        else:
            flat = [a.reshape(-1, cols) for a in all_anchors]
        anchors = torch.cat(flat, dim=0).contiguous() if len(flat) > 1 else flat[0].contiguous().clone()
        thr = np.array([[self.matched_thresholds[n], self.unmatched_thresholds[n]] for n in self.anchor_class_names],
                       dtype=np.float32).reshape(-1, 2)
        match = np.array([[n == a for n in self.class_names] for a in self.anchor_class_names], dtype=np.uint8)
        match = match.reshape(len(self.anchor_class_names), len(self.class_names))
        self._tables = dict(
            anchors=anchors, cols=cols, n_out=n_out, max_rows=max(rows) if rows else 0,
            cls=torch.from_numpy(np.array(table, dtype=np.int64).reshape(-1, 5)).to(dev),
            thr=torch.from_numpy(thr).to(dev), match=torch.from_numpy(match).to(dev))
        self._key = [(a, a._version) for a in all_anchors]
        return self._tables

    def assign_targets(self, all_anchors, gt_boxes_with_classes):
        """
        Args:
            all_anchors: [(z, y, x, sizes, rotations, 7 + C), ...], one tensor per anchor class
            gt_boxes_with_classes: (B, M, 7 + C + 1), zero rows as padding, the class id last; any strides
        Returns:
            box_cls_labels (B, N) int32, box_reg_targets (B, N, code_size) float32, reg_weights (B, N) float32
        """
        from .. import ops
        t = self._device_tables(all_anchors)
        gt = gt_boxes_with_classes
        if not torch.is_tensor(gt) or not gt.is_cuda:
            raise ValueError("gt_boxes_with_classes must be a device tensor (PyTorch-ROCm 'cuda')")
        if gt.ndim != 3 or gt.shape[2] < 8:
            raise ValueError(f"gt_boxes_with_classes has shape {tuple(gt.shape)}, expected (B, M, 7 + C + 1)")
        code = 7 + int(self.sincos) + min(t["cols"] - 7, int(gt.shape[2]) - 8)   # encode_torch zips the extra columns
        if int(self.box_coder.code_size) != code:
            raise ValueError(f"box_coder.code_size is {self.box_coder.code_size}: anchors of {t['cols']} and gt boxes of "
                             f"{int(gt.shape[2]) - 1} columns encode to {code}")
        if gt.device != t["anchors"].device:
            raise ValueError("anchors and gt boxes are on different devices")
        if gt.dtype != torch.float32:
            gt = gt.float()
        labels, targets, weights = ops.anchor_targets(gt, t["anchors"], t["cls"], t["thr"], t["match"], t["max_rows"],
                                                      t["n_out"], self.sincos)
        return {'box_cls_labels': labels, 'box_reg_targets': targets, 'reg_weights': weights}
