"""The anchors of a single anchor head as one (N, columns) table, shared by the head's loss (anchor_head_loss) and its box
decoding (box_decode)."""
import torch


def flat_anchors(head):
    """(N, cols) anchors of a single head on the device, flattened as the reference flattens them, built once per list of
    anchor tensors (keyed as modest_amd.utils.target_assigner keys its tables)"""
    anchors = head.anchors
    given = list(anchors) if isinstance(anchors, (list, tuple)) else [anchors]
    key = getattr(head, "_modest_anchor_loss_key", None)
    if key is not None and len(key) == len(given) and all(a is b and a._version == v for a, (b, v) in zip(given, key)):
        return head._modest_anchor_loss_anchors
    if isinstance(anchors, (list, tuple)):
        flat = torch.cat(given, dim=-3) if len(given) > 1 else given[0]
    else:
        flat = anchors
    flat = flat.reshape(-1, flat.shape[-1]).float().contiguous()
    head._modest_anchor_loss_anchors = flat
    head._modest_anchor_loss_key = [(a, a._version) for a in given]
    return flat
