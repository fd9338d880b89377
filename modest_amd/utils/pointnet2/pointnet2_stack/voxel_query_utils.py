"""The public names of OpenPCDet's ``pcdet/ops/pointnet2/pointnet2_stack/voxel_query_utils.py`` on
top of the HIP ops: ``VoxelQuery`` / ``voxel_query`` and ``VoxelQueryAndGrouping`` (Voxel R-CNN's
RoI-grid pooling), with the reference's signatures and returns.  Written from the interface.
"""
import torch
from torch import nn

from . import pointnet2_stack_cuda as pointnet2
from . import pointnet2_utils


class VoxelQuery(torch.autograd.Function):
    @staticmethod
    def forward(ctx, max_range, radius, nsample, xyz, new_xyz, new_coords, point_indices):
        """max_range (z, y, x) cells, xyz (N1 + N2 ..., 3), new_xyz (M1 + M2 ..., 3), new_coords (M1 + M2 ..., 4)
        int32 [batch, z, y, x], point_indices (B, Z, Y, X) int32: the row of xyz in a cell or -1
        -> idx (M1 + M2 ..., nsample) int32 GLOBAL rows of xyz, rows without a hit zeroed; empty_ball_mask"""
        xyz, new_xyz = pointnet2_utils._f32(xyz), pointnet2_utils._f32(new_xyz)
        new_coords, point_indices = pointnet2_utils._cnt(new_coords), pointnet2_utils._cnt(point_indices)
        M = new_coords.shape[0]
        _, Z, Y, X = point_indices.shape
        idx = torch.zeros((M, nsample), dtype=torch.int32, device=new_xyz.device)
        z_range, y_range, x_range = max_range
        pointnet2.voxel_query_wrapper(M, Z, Y, X, nsample, radius, int(z_range), int(y_range), int(x_range), new_xyz, xyz,
                                      new_coords, point_indices, idx)
        empty_ball_mask = idx[:, 0] == -1
        idx[empty_ball_mask] = 0
        ctx.mark_non_differentiable(idx, empty_ball_mask)
        return idx, empty_ball_mask

    @staticmethod
    def backward(ctx, a=None, b=None):
        return None, None, None, None, None, None, None


voxel_query = VoxelQuery.apply


class VoxelQueryAndGrouping(nn.Module):
    def __init__(self, max_range, radius, nsample):
        super().__init__()
        self.max_range, self.radius, self.nsample = max_range, radius, nsample

    def forward(self, new_coords, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features, voxel2point_indices):
        """-> grouped_features (M1 + M2 ..., C, nsample), grouped_xyz (M1 + M2 ..., 3, nsample), empty_ball_mask.
        As in the reference every scan holds the same number of queries (the RoI grid)."""
        assert xyz.shape[0] == xyz_batch_cnt.sum(), f"xyz: {tuple(xyz.shape)}, xyz_batch_cnt: {xyz_batch_cnt}"
        assert new_coords.shape[0] == new_xyz_batch_cnt.sum(), \
            f"new_coords: {tuple(new_coords.shape)}, new_xyz_batch_cnt: {new_xyz_batch_cnt}"
        batch_size = xyz_batch_cnt.shape[0]
        idx, empty_ball_mask = voxel_query(self.max_range, self.radius, self.nsample, xyz, new_xyz, new_coords,
                                           voxel2point_indices)
        # global rows -> scan-local: minus the scan's first row, for all scans at once
        start = (torch.cumsum(xyz_batch_cnt, 0) - xyz_batch_cnt).to(idx.dtype)
        idx = (idx.view(batch_size, -1, self.nsample) - start.view(batch_size, 1, 1)).view(-1, self.nsample)
        idx = idx.masked_fill(empty_ball_mask[:, None], 0)
        grouped_xyz = pointnet2_utils.grouping_operation(xyz, xyz_batch_cnt, idx, new_xyz_batch_cnt)
        grouped_features = pointnet2_utils.grouping_operation(features, xyz_batch_cnt, idx, new_xyz_batch_cnt)
        return grouped_features, grouped_xyz, empty_ball_mask
