"""``RoIPointPool3d`` / ``RoIPointPool3dFunction`` of OpenPCDet's ops/roipoint_pool3d/roipoint_pool3d_utils.py:9-63, stated
on ``roipoint_pool3d_cuda.forward`` of this package: the same constructor and call signature, the boxes enlarged by
``pool_extra_width`` here (``box_utils.enlarge_box3d``: dx, dy, dz grow by the extra width, centre and heading stay),
zero-filled outputs, no backward.  For callers without OpenPCDet; with it, bind the extension module and use its own
file unchanged."""
import torch
import torch.nn as nn
from torch.autograd import Function

from . import roipoint_pool3d_cuda


def enlarge_box3d(boxes3d, extra_width=(0, 0, 0)):
    """boxes3d (N, 7) [x, y, z, dx, dy, dz, heading] -> a copy with the three sizes grown by extra_width (one number
    or one per size)"""
    large = boxes3d.clone()
    large[:, 3:6] += boxes3d.new_tensor(extra_width).reshape(1, -1)
    return large


class RoIPointPool3d(nn.Module):
    def __init__(self, num_sampled_points=512, pool_extra_width=1.0):
        super().__init__()
        self.num_sampled_points = num_sampled_points
        self.pool_extra_width = pool_extra_width

    def forward(self, points, point_features, boxes3d):
        """
        Args:
            points: (B, N, 3)
            point_features: (B, N, C)
            boxes3d: (B, M, 7), [x, y, z, dx, dy, dz, heading]

        Returns:
            pooled_features: (B, M, num_sampled_points, 3 + C)
            pooled_empty_flag: (B, M) int32, 1 for a box without a point
        """
        return RoIPointPool3dFunction.apply(points, point_features, boxes3d, self.pool_extra_width,
                                            self.num_sampled_points)


class RoIPointPool3dFunction(Function):
    @staticmethod
    def forward(ctx, points, point_features, boxes3d, pool_extra_width, num_sampled_points=512):
        assert points.shape.__len__() == 3 and points.shape[2] == 3
        batch_size, boxes_num, feature_len = points.shape[0], boxes3d.shape[1], point_features.shape[2]
        pooled_boxes3d = enlarge_box3d(boxes3d.reshape(-1, 7), pool_extra_width).view(batch_size, -1, 7)

        pooled_features = point_features.new_zeros((batch_size, boxes_num, num_sampled_points, 3 + feature_len))
        pooled_empty_flag = point_features.new_zeros((batch_size, boxes_num)).int()

        roipoint_pool3d_cuda.forward(points.contiguous(), pooled_boxes3d.contiguous(), point_features.contiguous(),
                                     pooled_features, pooled_empty_flag)
        return pooled_features, pooled_empty_flag

    @staticmethod
    def backward(ctx, *grad_outs):
        # one gradient per output (pooled_features, pooled_empty_flag): the reference's one-argument statement raises
        # TypeError before it reaches its NotImplementedError
        raise NotImplementedError
