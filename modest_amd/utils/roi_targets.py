"""Drop-in for ``RoIHeadTemplate.assign_targets`` of OpenPCDet's two-stage detectors
(``pcdet/models/roi_heads/roi_head_template.py``, over ``ProposalTargetLayer.forward`` of
``roi_heads/target_assigner/proposal_target_layer.py``) on the GPU: the RoI sampling and the
regression / classification targets of PointRCNN, PartA2, PV-RCNN, SECOND-IoU and Voxel R-CNN in training.

Two library calls (``modest_amd.ops.roi_targets``, csrc/roi_targets.hip) on PyTorch's current stream: the match call trims
the padded gts, matches every roi and builds the fg / hard / easy lists of the whole batch in one launch and hands their
lengths to the host -- the call's one synchronise; the reference's draws follow, the same calls in the same order on
numpy's and torch's global CPU generators, so a seeded run samples the rois the reference samples; the sample call gathers
the picks, the labels and the canonical transform.  No loop of device work over the samples or the classes.  The workspace
and the two pinned tables are kept on the head and grow with the largest call.

Where the reference leaves the result to ``torch.max``: equal maxima go to the lowest gt row and a NaN IoU is the maximum
(the first one).  A sample all of whose maxima are NaN raises ``NotImplementedError`` as the reference does; so does an
unknown ``CLS_SCORE_TYPE``.  The limits (``ValueError``): 7 + C <= ``COLS_MAX``, batch <= ``BATCH_MAX``, ``ROI_PER_IMAGE``
>= 1, at most 2^31 - 1 rows.  ``bind(cls)`` sets ``assign_targets`` on a head class; ``pcdet_bind.bind_roi_targets()`` does
that for the reference's ``RoIHeadTemplate``.  ``forward`` has ``ProposalTargetLayer.forward``'s contract.
"""
import torch

from ._head_loss import device_workspace, pinned_table

BATCH_MAX = 65535     # samples per call
COLS_MAX = 4096       # 7 + C
KEYS = ("rois", "gt_of_rois", "gt_iou_of_rois", "roi_scores", "roi_labels", "reg_valid_mask", "rcnn_cls_labels",
        "gt_of_rois_src")
GT_TILE = 64          # gts the match kernel stages in LDS at a time: modest_roi_targets_gt_tile() (a test holds them equal)
WORKGROUP = 512       # rois a match workgroup takes at a time


def _config(head):
    cfg = getattr(head, "model_cfg", None)
    if cfg is not None:
        return cfg["TARGET_CONFIG"] if isinstance(cfg, dict) else cfg.TARGET_CONFIG
    layer = head if hasattr(head, "roi_sampler_cfg") else head.proposal_target_layer
    return layer.roi_sampler_cfg


def _buffers(head, dev, B, N, M):
    """the workspace and the two pinned tables kept on `head`: they grow with the largest call"""
    from .. import ops
    ws = device_workspace(head, "_modest_roi_targets_workspace", ops.roi_targets_workspace_bytes(B, N), dev)
    counts = pinned_table(head, "_modest_roi_targets_counts", 3 * B)
    picks = getattr(head, "_modest_roi_targets_picks", None)
    if picks is not None and picks.numel() < 2 * B * M:
        # The sample kernel reads this table where it lies, through a pointer PyTorch's host allocator does not see.  The
        # host writes it in every call only after that call's match has synchronised the stream, so the sample kernel of
        # the call before has read it.  A table that is replaced goes back to the allocator at once, though, and could be
        # handed out and overwritten while that kernel still waits: so the stream is synchronised before it is dropped (on
        # growth only; a steady shape never comes here).  A head is used on one stream at a time.
        torch.cuda.current_stream(dev).synchronize()
    return ws, counts, pinned_table(head, "_modest_roi_targets_picks", 2 * B * M)


def _run(head, batch_dict, cfg):
    from .. import ops
    from .._lib import ModestHipError
    rois, gt_boxes = batch_dict['rois'], batch_dict['gt_boxes']
    roi_scores, roi_labels = batch_dict['roi_scores'], batch_dict['roi_labels']
    for t, name in ((rois, "rois"), (roi_scores, "roi_scores"), (roi_labels, "roi_labels"), (gt_boxes, "gt_boxes")):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError(f"{name} must be a device tensor (PyTorch-ROCm 'cuda')")
    if ops._cfg_get(cfg, "CLS_SCORE_TYPE") not in ops.ROI_SCORE_TYPES:
        raise NotImplementedError
    B, N, cols = int(rois.shape[0]), int(rois.shape[1]), int(rois.shape[2])
    M = int(ops._cfg_get(cfg, "ROI_PER_IMAGE"))
    ops.roi_targets_limits(B, cols, M, N, int(gt_boxes.shape[1]))
    try:
        ws, counts, picks = _buffers(head, rois.device, B, N, M)
        return ops.roi_targets(rois, roi_scores, roi_labels, gt_boxes, cfg, workspace=ws, counts_pinned=counts,
                               picks_pinned=picks)
    except ModestHipError as e:
        if "requirement failed" in str(e):
            raise ValueError(str(e)) from e   # a limit of the library, named in its message
        raise


@torch.no_grad()
def forward(self, batch_dict):
    """
    ProposalTargetLayer.forward
    Args:
        batch_dict:
            batch_size:
            rois: (B, num_rois, 7 + C)
            roi_scores: (B, num_rois)
            gt_boxes: (B, N, 7 + C + 1)
            roi_labels: (B, num_rois)
    Returns:
        batch_dict:
            rois: (B, M, 7 + C)
            gt_of_rois: (B, M, 7 + C + 1)
            gt_iou_of_rois: (B, M)
            roi_scores: (B, M)
            roi_labels: (B, M)
            reg_valid_mask: (B, M)
            rcnn_cls_labels: (B, M)
    """
    out = _run(self, batch_dict, _config(self))
    out["gt_of_rois"] = out.pop("gt_of_rois_src")
    return {k: out[k] for k in KEYS[:7]}


def assign_targets(self, batch_dict):
    """RoIHeadTemplate.assign_targets: forward's dict with gt_of_rois in the roi's canonical frame and gt_of_rois_src"""
    with torch.no_grad():
        out = _run(self, batch_dict, _config(self))
    return {k: out[k] for k in KEYS}


def bind(cls):
    """set assign_targets on a head class (RoIHeadTemplate or a subclass) -> cls"""
    cls.assign_targets = assign_targets
    return cls
