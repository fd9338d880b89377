"""The public names of OpenPCDet's ``pcdet/ops/pointnet2/pointnet2_stack/pointnet2_utils.py`` on
top of the HIP ops (``pointnet2_stack_cuda`` in this package), for callers without OpenPCDet and
for the gradient tests: the five ``torch.autograd.Function``s with the reference's signatures and
returns (features are the only differentiable argument), their ``.apply`` aliases and
``QueryAndGroup``.  All scans of a batch are rows of one tensor, ``*_batch_cnt`` are int32 ``(B,)``
device tensors.  Written from the interface.
"""
import torch
from torch import nn

from . import pointnet2_stack_cuda as pointnet2


def _f32(t):
    return t.contiguous() if t.dtype == torch.float32 else t.float().contiguous()


def _cnt(t):
    return t.contiguous() if t.dtype == torch.int32 else t.int().contiguous()


class BallQuery(torch.autograd.Function):
    @staticmethod
    def forward(ctx, radius, nsample, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt):
        """xyz (N1 + N2 ..., 3), new_xyz (M1 + M2 ..., 3) -> idx (M1 + M2 ..., nsample) int32 scan-local, rows without
        a hit zeroed; empty_ball_mask (M1 + M2 ...) bool"""
        xyz, new_xyz = _f32(xyz), _f32(new_xyz)
        xyz_batch_cnt, new_xyz_batch_cnt = _cnt(xyz_batch_cnt), _cnt(new_xyz_batch_cnt)
        B, M = xyz_batch_cnt.shape[0], new_xyz.shape[0]
        idx = torch.zeros((M, nsample), dtype=torch.int32, device=new_xyz.device)
        pointnet2.ball_query_wrapper(B, M, radius, nsample, new_xyz, new_xyz_batch_cnt, xyz, xyz_batch_cnt, idx)
        empty_ball_mask = idx[:, 0] == -1
        idx[empty_ball_mask] = 0
        ctx.mark_non_differentiable(idx, empty_ball_mask)
        return idx, empty_ball_mask

    @staticmethod
    def backward(ctx, a=None, b=None):
        return None, None, None, None, None, None


ball_query = BallQuery.apply


class GroupingOperation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, features_batch_cnt, idx, idx_batch_cnt):
        """features (N1 + N2 ..., C), idx (M1 + M2 ..., nsample) scan-local -> (M1 + M2 ..., C, nsample)"""
        features, idx = _f32(features), idx.contiguous()
        features_batch_cnt, idx_batch_cnt = _cnt(features_batch_cnt), _cnt(idx_batch_cnt)
        M, nsample = idx.shape
        N, C = features.shape
        B = idx_batch_cnt.shape[0]
        out = torch.empty((M, C, nsample), dtype=torch.float32, device=features.device)
        pointnet2.group_points_wrapper(B, M, C, nsample, features, features_batch_cnt, idx, idx_batch_cnt, out)
        ctx.for_backwards = (B, N, idx, features_batch_cnt, idx_batch_cnt)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        B, N, idx, features_batch_cnt, idx_batch_cnt = ctx.for_backwards
        g = _f32(grad_out)
        M, C, nsample = g.shape
        grad_features = torch.zeros((N, C), dtype=torch.float32, device=g.device)
        pointnet2.group_points_grad_wrapper(B, M, C, N, nsample, g, idx, idx_batch_cnt, features_batch_cnt, grad_features)
        return grad_features, None, None, None


grouping_operation = GroupingOperation.apply


class QueryAndGroup(nn.Module):
    def __init__(self, radius, nsample, use_xyz=True):
        super().__init__()
        self.radius, self.nsample, self.use_xyz = radius, nsample, use_xyz

    def forward(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features=None):
        """-> new_features (M1 + M2 ..., [3 +] C, nsample): the grouped coordinates relative to their centre, then the
        grouped features; rows of an empty ball are zero; idx (M1 + M2 ..., nsample)"""
        assert xyz.shape[0] == xyz_batch_cnt.sum(), f"xyz: {tuple(xyz.shape)}, xyz_batch_cnt: {xyz_batch_cnt}"
        assert new_xyz.shape[0] == new_xyz_batch_cnt.sum(), \
            f"new_xyz: {tuple(new_xyz.shape)}, new_xyz_batch_cnt: {new_xyz_batch_cnt}"
        idx, empty_ball_mask = ball_query(self.radius, self.nsample, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt)
        grouped_xyz = grouping_operation(xyz, xyz_batch_cnt, idx, new_xyz_batch_cnt)
        grouped_xyz = grouped_xyz - new_xyz.unsqueeze(-1)
        grouped_xyz = grouped_xyz.masked_fill(empty_ball_mask[:, None, None], 0)
        if features is not None:
            grouped_features = grouping_operation(features, xyz_batch_cnt, idx, new_xyz_batch_cnt)
            grouped_features = grouped_features.masked_fill(empty_ball_mask[:, None, None], 0)
            new_features = torch.cat([grouped_xyz, grouped_features], dim=1) if self.use_xyz else grouped_features
        else:
            assert self.use_xyz, "Cannot have not features and not use xyz as a feature!"
            new_features = grouped_xyz
        return new_features, idx


class FurthestPointSampling(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz, npoint):
        """xyz (B, N, 3), npoint -> (B, npoint) int32 indices, the first one 0"""
        xyz = _f32(xyz)
        B, N = xyz.shape[0], xyz.shape[1]
        idx = torch.empty((B, npoint), dtype=torch.int32, device=xyz.device)
        temp = torch.full((B, N), 1e10, dtype=torch.float32, device=xyz.device)
        pointnet2.furthest_point_sampling_wrapper(B, N, int(npoint), xyz, temp, idx)
        ctx.mark_non_differentiable(idx)
        return idx

    @staticmethod
    def backward(ctx, a=None):
        return None, None


furthest_point_sample = FurthestPointSampling.apply


class ThreeNN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, unknown, unknown_batch_cnt, known, known_batch_cnt):
        """unknown (N1 + N2 ..., 3), known (M1 + M2 ..., 3) -> (distances (N1 + N2 ..., 3), NOT squared;
        idx (N1 + N2 ..., 3) int32 global rows of known)"""
        assert unknown.dim() == 2 and unknown.shape[1] == 3
        assert known.dim() == 2 and known.shape[1] == 3
        assert len(unknown_batch_cnt) == len(known_batch_cnt)
        unknown, known = _f32(unknown), _f32(known)
        dist2 = torch.empty(unknown.shape, dtype=torch.float32, device=unknown.device)
        idx = torch.empty(unknown.shape, dtype=torch.int32, device=unknown.device)
        pointnet2.three_nn_wrapper(unknown, _cnt(unknown_batch_cnt), known, _cnt(known_batch_cnt), dist2, idx)
        dist = torch.sqrt(dist2)
        ctx.mark_non_differentiable(dist, idx)
        return dist, idx

    @staticmethod
    def backward(ctx, a=None, b=None):
        return None, None, None, None


three_nn = ThreeNN.apply


class ThreeInterpolate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, idx, weight):
        """features (M1 + M2 ..., C), idx / weight (N1 + N2 ..., 3) -> (N1 + N2 ..., C)"""
        assert idx.shape[0] == weight.shape[0] and idx.shape[1] == weight.shape[1] == 3
        features, idx, weight = _f32(features), idx.contiguous(), _f32(weight)
        ctx.three_interpolate_for_backward = (idx, weight, features.shape[0])
        out = torch.empty((idx.shape[0], features.shape[1]), dtype=torch.float32, device=features.device)
        pointnet2.three_interpolate_wrapper(features, idx, weight, out)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        idx, weight, M = ctx.three_interpolate_for_backward
        g = _f32(grad_out)
        grad_features = torch.zeros((M, g.shape[1]), dtype=torch.float32, device=g.device)
        pointnet2.three_interpolate_grad_wrapper(g, idx, weight, grad_features)
        return grad_features, None, None


three_interpolate = ThreeInterpolate.apply
