"""Drop-ins for ``PillarVFE.forward`` (pcdet/models/backbones_3d/vfe/pillar_vfe.py) and ``PointPillarScatter.forward``
(pcdet/models/backbones_2d/map_to_bev/pointpillar_scatter.py) on the GPU: PointPillars' front end
between the voxeliser and the 2-D backbone.

``pillar_vfe_forward`` builds the point features, runs the one PFN layer (Linear without bias, BatchNorm1d, ReLU) and takes
the maximum over a pillar's slots inside the library (``modest_amd.ops.pillar_vfe``, csrc/pillar_vfe.hip): the
``(P, S, K)`` feature tensor and the three ``(P, S, C)`` tensors of the reference never exist.  Its backward
(``ops.pillar_vfe_backward``) visits the winning slot of every (pillar, channel) only.  ``pillar_scatter_forward`` writes the
BEV canvas in one call, without the reference's ``coords[:, 0].max().item()`` and its per-sample masks; the batch size is
``batch_dict['batch_size']``.  Every call enqueues on PyTorch's current stream and never waits for the device.

Only ``forward`` is replaced: the module keeps ``pfn_layers[0].linear.weight``, ``.norm.weight``, ``.norm.bias``,
``.running_mean``, ``.running_var`` and ``.num_batches_tracked``, so checkpoints, optimiser parameter groups and
``state_dict`` are unchanged.  In training mode the running buffers are updated in place by the library, with the module's own
``eps`` and ``momentum``.  ``voxel_num_points`` and ``voxel_coords`` are read as float32, int32 or int64, as they arrive.

THE ONE DIFFERENCE from the reference: one pillar (P = 1) gives ``pillar_features`` of (1, C); the reference's ``squeeze()``
gives (C,) there, and its scatter then fails.

Not provided (``NotImplementedError`` before anything is launched): more than one PFN layer, ``USE_NORM: False``, voxels that
require grad, gradients in eval mode, voxels or parameters that are not float32, ``nz != 1``.  Limits (``ValueError``): 1 .. 64
output channels, 1 .. 16 features of a point, 1 .. 255 slots, at most 2^31 - 1 rows (P * S), a batch of at most 65 535.
A row of the scatter whose b, z, y or x is out of range is skipped (its gradient is zero); two rows of one cell are a
precondition not to occur, as in the reference.

``bind(cls, kind)`` sets ``forward`` on a class; ``pcdet_bind.bind_pillar_vfe()`` does that for the reference's two.  A subclass
that overrides ``forward`` keeps its own, as Python's MRO gives.
"""
import torch

METHOD = "forward"

_ORIGINAL = {}   # class -> the forward that bind() replaced on it (None: it had none of its own)


def _geometry(module):
    return ((module.voxel_x, module.voxel_y, module.voxel_z), (module.x_offset, module.y_offset, module.z_offset))


class PillarVFEFunction(torch.autograd.Function):
    """out (P, C) = max over the slots of relu(norm(linear(features))); gradients for weight, gamma and beta"""

    @staticmethod
    def forward(ctx, voxels, num_points, coords, weight, gamma, beta, running_mean, running_var, tracked, geometry, parts, eps,
                momentum, training):
        from .. import ops
        out, winner, sums, stat = ops.pillar_vfe(voxels, num_points, coords, weight, gamma, beta, running_mean, running_var,
                                                 tracked, voxel_size=geometry[0], offsets=geometry[1], parts=parts, eps=eps,
                                                 momentum=momentum, training=training)
        ctx.training = training
        if training:
            ctx.geometry, ctx.parts = geometry, parts
            ctx.save_for_backward(voxels, num_points, coords, weight, gamma, out, winner, sums, stat)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        from .. import ops
        if not ctx.training:
            raise NotImplementedError("gradients of PillarVFE in eval mode are not provided by modest_amd")
        voxels, num_points, coords, weight, gamma, out, winner, sums, stat = ctx.saved_tensors
        dW, dg, db = ops.pillar_vfe_backward(voxels, num_points, coords, weight, gamma, out, winner, grad_out.contiguous(), sums,
                                             stat, voxel_size=ctx.geometry[0], offsets=ctx.geometry[1], parts=ctx.parts)
        return (None, None, None, dW, dg, db) + (None,) * 8


class PillarScatterFunction(torch.autograd.Function):
    """canvas (B, C, ny, nx) from pillar features (P, C); the gradient of the features"""

    @staticmethod
    def forward(ctx, features, coords, batch_size, ny, nx):
        from .. import ops
        ctx.save_for_backward(coords)
        return ops.pillar_scatter(features, coords, batch_size, ny, nx)

    @staticmethod
    def backward(ctx, grad_canvas):
        from .. import ops
        (coords,) = ctx.saved_tensors
        return ops.pillar_scatter_backward(grad_canvas.contiguous(), coords), None, None, None, None


def pillar_vfe_forward(self, batch_dict, **kwargs):
    """PillarVFE.forward: batch_dict['pillar_features'] (P, C) from 'voxels', 'voxel_num_points', 'voxel_coords' -> batch_dict"""
    from .. import ops
    if len(self.pfn_layers) != 1:
        raise NotImplementedError(f"{len(self.pfn_layers)} PFN layers are not provided by modest_amd's PillarVFE: one layer only")
    pfn = self.pfn_layers[0]
    if not getattr(pfn, "use_norm", True) or getattr(pfn, "norm", None) is None:
        raise NotImplementedError("USE_NORM: False is not provided by modest_amd's PillarVFE")
    voxels, num_points, coords = batch_dict["voxels"], batch_dict["voxel_num_points"], batch_dict["voxel_coords"]
    weight, norm = pfn.linear.weight, pfn.norm
    if voxels.requires_grad:
        raise NotImplementedError("voxels that require grad are not provided by modest_amd's PillarVFE")
    for name, t in (("voxels", voxels), ("linear.weight", weight), ("norm.weight", norm.weight), ("norm.bias", norm.bias),
                    ("norm.running_mean", norm.running_mean), ("norm.running_var", norm.running_var)):
        if t is not None and t.dtype != torch.float32:
            raise NotImplementedError(f"{name} of {t.dtype} (mixed precision) is not provided: float32 only")
    if norm.weight is None or norm.bias is None:
        raise NotImplementedError("a norm without affine parameters is not provided by modest_amd's PillarVFE")
    training = bool(self.training and pfn.training) or norm.running_mean is None
    grads = torch.is_grad_enabled() and (weight.requires_grad or norm.weight.requires_grad or norm.bias.requires_grad)
    if grads and not training:
        raise NotImplementedError("gradients of PillarVFE in eval mode are not provided by modest_amd")
    parts = ops.PILLAR_CLUSTER | ops.PILLAR_CENTER | (ops.PILLAR_XYZ if self.use_absolute_xyz else 0) \
        | (ops.PILLAR_DIST if self.with_distance else 0)
    update = bool(self.training and pfn.training) and norm.running_mean is not None
    features = PillarVFEFunction.apply(voxels.contiguous(), num_points.contiguous(), coords.contiguous(), weight.contiguous(),
                                       norm.weight, norm.bias, norm.running_mean if update or not training else None,
                                       norm.running_var if update or not training else None,
                                       norm.num_batches_tracked if update else None, _geometry(self), parts, float(norm.eps),
                                       norm.momentum, training)
    batch_dict["pillar_features"] = features
    return batch_dict


def pillar_scatter_forward(self, batch_dict, **kwargs):
    """PointPillarScatter.forward: batch_dict['spatial_features'] (B, C, ny, nx) from 'pillar_features' and 'voxel_coords'
    -> batch_dict"""
    if int(self.nz) != 1:
        raise NotImplementedError(f"nz = {self.nz} is not provided by modest_amd's PointPillarScatter: nz = 1 only")
    features, coords = batch_dict["pillar_features"], batch_dict["voxel_coords"]
    if features.dtype != torch.float32:
        raise NotImplementedError(f"pillar_features of {features.dtype} (mixed precision) is not provided: float32 only")
    if features.ndim != 2 or int(features.shape[1]) != int(self.num_bev_features):
        raise ValueError(f"pillar_features {tuple(features.shape)} must be (P, NUM_BEV_FEATURES) = (P, {self.num_bev_features})")
    batch_dict["spatial_features"] = PillarScatterFunction.apply(features.contiguous(), coords.contiguous(),
                                                                 int(batch_dict["batch_size"]), int(self.ny), int(self.nx))
    return batch_dict


KINDS = {"PillarVFE": pillar_vfe_forward, "PointPillarScatter": pillar_scatter_forward}


def bind(cls, kind=None):
    """set forward on a class -> cls; `kind` one of KINDS' names, by default the class's own name.  The method it had is kept in
    _ORIGINAL.  Idempotent."""
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
