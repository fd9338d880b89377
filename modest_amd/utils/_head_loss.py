"""What the ``get_loss`` drop-ins of the anchor, RoI and point heads share (``anchor_head_loss``, ``roi_head_loss``,
``point_head_loss``; DESIGN.md sections 7p - 7r): the config lookup, the hand-back of a head that overrides a part of the loss
to the method ``bind`` replaced, the buffers kept on the head, the code weights, the autograd function around the fused
forward + gradient call, and the one host wait.  The config lookup and the two grow-only buffers (``device_workspace``,
``pinned_table``) also serve the other drop-ins that keep buffers on a head or a detector (``proposal_layer``, ``roi_targets``,
``post_processing``)."""
import torch
from torch.autograd.function import once_differentiable


from ..ops import _cfg_get as _get      # noqa: F401  the config lookup of every drop-in: cfg[name] or cfg.name, with a default


def device_workspace(owner, attr, nbytes, dev):
    """the uint8 device workspace kept on `owner` as `attr`: replaced when it is too small or on another device, never shrunk"""
    ws = getattr(owner, attr, None)
    if ws is None or ws.numel() < nbytes or ws.device != dev:
        ws = torch.empty((max(nbytes, 256),), dtype=torch.uint8, device=dev)
        setattr(owner, attr, ws)
    return ws


def pinned_table(owner, attr, words):
    """the pinned int32 table kept on `owner` as `attr`: replaced when it is too small, never shrunk"""
    table = getattr(owner, attr, None)
    if table is None or table.numel() < words:
        table = torch.zeros((max(words, 16),), dtype=torch.int32).pin_memory()
        setattr(owner, attr, table)
    return table


def replaced_get_loss(head_type, original, parts):
    """-> (base, method): base the class of `head_type`'s MRO that `bind` was called on (`original`: class -> the get_loss it
    had of its own, or None), method the get_loss that `bind` replaced iff `head_type` overrides one of `parts` below base
    (the head computes another loss), else None"""
    base = next((c for c in head_type.__mro__ if c in original), None)
    if base is None or all(getattr(head_type, part, None) is getattr(base, part, None) for part in parts):
        return base, None
    method = original[base]
    if method is None:
        method = next(c.__dict__["get_loss"] for c in base.__mro__[1:] if "get_loss" in c.__dict__)
    return base, method


def buffers(head, prefix, workspace_bytes, table_len, dev):
    """the workspace and the pinned table kept on `head` as `prefix`_workspace and `prefix`_table; a table serves one stream
    at a time"""
    ws = device_workspace(head, prefix + "_workspace", workspace_bytes, dev)
    table = getattr(head, prefix + "_table", None)
    if table is None:
        table = torch.zeros((table_len,), dtype=torch.float32).pin_memory()
        setattr(head, prefix + "_table", table)
    return ws, table


def code_weights_tensor(reg_fn, code, dev):
    """`reg_fn.code_weights` (a tensor, a sequence or absent: ones) as a contiguous float32 vector on `dev`"""
    code_weights = getattr(reg_fn, "code_weights", None)
    if code_weights is None:
        return torch.ones((code,), dtype=torch.float32, device=dev)
    if not torch.is_tensor(code_weights):
        return torch.tensor([float(v) for v in code_weights], dtype=torch.float32, device=dev)
    return code_weights.to(device=dev, dtype=torch.float32).reshape(-1).contiguous()


def read_table(table, out, dev):
    """the device table `out` as Python floats through the pinned `table`, after the one host wait of a step"""
    table.copy_(out.detach(), non_blocking=True)
    torch.cuda.current_stream(dev).synchronize()      # the one host wait
    return table.tolist()


class HeadLossFunction(torch.autograd.Function):
    """(the tensors of ``ops.<OPS[0]>`` in its order, scalars, workspace) -> its table.  Only element 3, the total, carries a
    gradient: backward scales the unit gradients kept by forward with the upstream gradient of that element, in place
    (``ops.<OPS[1]>``), so it runs once.  A subclass names OPS, PREDS (the positions of the predictions among the tensors)
    and WORD (the loss, in the message of a second backward)."""
    OPS = PREDS = WORD = None

    @staticmethod
    def forward(ctx, *args):
        from .. import ops
        fn = ctx._forward_cls
        *tensors, scalars, workspace = args
        table, grads = getattr(ops, fn.OPS[0])(*tensors, want_grad=True, workspace=workspace, **scalars)
        ctx.unit_grads = grads
        ctx.shapes = tuple(None if tensors[i] is None else tensors[i].shape for i in fn.PREDS)
        ctx.n_inputs = len(args)
        return table

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_table):
        from .. import ops
        fn = ctx._forward_cls
        grads = ctx.unit_grads
        if grads is None:
            raise RuntimeError(f"the {fn.WORD} loss was differentiated a second time: its gradient buffers were scaled in place")
        ctx.unit_grads = None
        upstream = grad_table.contiguous()[3:4]
        if upstream.dtype != torch.float32:
            upstream = upstream.float()
        getattr(ops, fn.OPS[1])(grads, upstream)
        out = [None] * ctx.n_inputs
        for i, g, s in zip(fn.PREDS, grads, ctx.shapes):
            out[i] = None if g is None else g.view(s)
        return tuple(out)
