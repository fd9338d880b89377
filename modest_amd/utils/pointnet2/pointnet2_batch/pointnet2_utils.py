"""The public names of OpenPCDet's ``pcdet/ops/pointnet2/pointnet2_batch/pointnet2_utils.py`` on
top of the HIP ops (``pointnet2_batch_cuda`` in this package), for callers without OpenPCDet and
for the gradient tests: six ``torch.autograd.Function``s with the reference's signatures and the
same differentiable arguments (features only; every index-producing function returns no gradient),
``QueryAndGroup`` and ``GroupAll``.  Written from the interface.
"""
import torch
from torch import nn

from . import pointnet2_batch_cuda as _ops


def _f32(t):
    return t.contiguous() if t.dtype == torch.float32 else t.float().contiguous()


class _FurthestPointSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz, npoint):
        """xyz (B, N, 3) float32, npoint -> (B, npoint) int32 indices, the first one 0"""
        xyz = xyz.contiguous()
        b, n = xyz.shape[0], xyz.shape[1]
        idx = torch.empty((b, npoint), dtype=torch.int32, device=xyz.device)
        temp = torch.full((b, n), 1e10, dtype=torch.float32, device=xyz.device)
        _ops.furthest_point_sampling_wrapper(b, n, int(npoint), xyz, temp, idx)
        ctx.mark_non_differentiable(idx)
        return idx

    @staticmethod
    def backward(ctx, grad=None):
        return None, None


class _Gather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, idx):
        """features (B, C, N), idx (B, npoint) int32 -> (B, C, npoint)"""
        features, idx = features.contiguous(), idx.contiguous()
        b, c, n = features.shape
        m = idx.shape[1]
        out = torch.empty((b, c, m), dtype=torch.float32, device=features.device)
        _ops.gather_points_wrapper(b, c, n, m, features, idx, out)
        ctx.save_for_backward(idx)
        ctx.n = n
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        g = _f32(grad_out)
        b, c, m = g.shape
        grad = torch.zeros((b, c, ctx.n), dtype=torch.float32, device=g.device)
        _ops.gather_points_grad_wrapper(b, c, ctx.n, m, g, idx, grad)
        return grad, None


class _ThreeNN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, unknown, known):
        """unknown (B, n, 3), known (B, m, 3) -> (distances (B, n, 3), NOT squared; idx (B, n, 3) int32)"""
        unknown, known = unknown.contiguous(), known.contiguous()
        b, n = unknown.shape[0], unknown.shape[1]
        m = known.shape[1]
        dist2 = torch.empty((b, n, 3), dtype=torch.float32, device=unknown.device)
        idx = torch.empty((b, n, 3), dtype=torch.int32, device=unknown.device)
        _ops.three_nn_wrapper(b, n, m, unknown, known, dist2, idx)
        dist = torch.sqrt(dist2)
        ctx.mark_non_differentiable(dist, idx)
        return dist, idx

    @staticmethod
    def backward(ctx, a=None, b=None):
        return None, None


class _ThreeInterpolate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, idx, weight):
        """features (B, C, m), idx / weight (B, n, 3) -> (B, C, n)"""
        features, idx, weight = features.contiguous(), idx.contiguous(), weight.contiguous()
        b, c, m = features.shape
        n = idx.shape[1]
        out = torch.empty((b, c, n), dtype=torch.float32, device=features.device)
        _ops.three_interpolate_wrapper(b, c, m, n, features, idx, weight, out)
        ctx.save_for_backward(idx, weight)
        ctx.m = m
        return out

    @staticmethod
    def backward(ctx, grad_out):
        idx, weight = ctx.saved_tensors
        g = _f32(grad_out)
        b, c, n = g.shape
        grad = torch.zeros((b, c, ctx.m), dtype=torch.float32, device=g.device)
        _ops.three_interpolate_grad_wrapper(b, c, n, ctx.m, g, idx, weight, grad)
        return grad, None, None


class _Grouping(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, idx):
        """features (B, C, N), idx (B, npoint, nsample) int32 -> (B, C, npoint, nsample)"""
        features, idx = features.contiguous(), idx.contiguous()
        b, c, n = features.shape
        p, s = idx.shape[1], idx.shape[2]
        out = torch.empty((b, c, p, s), dtype=torch.float32, device=features.device)
        _ops.group_points_wrapper(b, c, n, p, s, features, idx, out)
        ctx.save_for_backward(idx)
        ctx.n = n
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        g = _f32(grad_out)
        b, c, p, s = g.shape
        grad = torch.zeros((b, c, ctx.n), dtype=torch.float32, device=g.device)
        _ops.group_points_grad_wrapper(b, c, ctx.n, p, s, g, idx, grad)
        return grad, None


class _BallQuery(torch.autograd.Function):
    @staticmethod
    def forward(ctx, radius, nsample, xyz, new_xyz):
        """xyz (B, N, 3), new_xyz (B, npoint, 3) -> idx (B, npoint, nsample) int32, rows without a hit all 0"""
        xyz, new_xyz = xyz.contiguous(), new_xyz.contiguous()
        b, n = xyz.shape[0], xyz.shape[1]
        p = new_xyz.shape[1]
        idx = torch.zeros((b, p, int(nsample)), dtype=torch.int32, device=xyz.device)
        _ops.ball_query_wrapper(b, n, p, float(radius), int(nsample), new_xyz, xyz, idx)
        ctx.mark_non_differentiable(idx)
        return idx

    @staticmethod
    def backward(ctx, grad=None):
        return None, None, None, None


furthest_point_sample = _FurthestPointSample.apply
gather_operation = _Gather.apply
three_nn = _ThreeNN.apply
three_interpolate = _ThreeInterpolate.apply
grouping_operation = _Grouping.apply
ball_query = _BallQuery.apply


class QueryAndGroup(nn.Module):
    """ball query around new_xyz, the neighbours' coordinates relative to their centre (+ their features)"""

    def __init__(self, radius, nsample, use_xyz=True):
        super().__init__()
        self.radius, self.nsample, self.use_xyz = radius, nsample, use_xyz

    def forward(self, xyz, new_xyz, features=None):
        """xyz (B, N, 3), new_xyz (B, npoint, 3), features (B, C, N) -> (B, 3 + C, npoint, nsample)"""
        idx = ball_query(self.radius, self.nsample, xyz, new_xyz)
        rel = grouping_operation(xyz.transpose(1, 2).contiguous(), idx) - new_xyz.transpose(1, 2).unsqueeze(-1)
        if features is None:
            if not self.use_xyz:
                raise ValueError("QueryAndGroup without features needs use_xyz")
            return rel
        grouped = grouping_operation(features, idx)
        return torch.cat([rel, grouped], dim=1) if self.use_xyz else grouped


class GroupAll(nn.Module):
    """one group of all points: (B, 3 + C, 1, N)"""

    def __init__(self, use_xyz=True):
        super().__init__()
        self.use_xyz = use_xyz

    def forward(self, xyz, new_xyz, features=None):
        g = xyz.transpose(1, 2).unsqueeze(2)
        if features is None:
            return g
        f = features.unsqueeze(2)
        return torch.cat([g, f], dim=1) if self.use_xyz else f
