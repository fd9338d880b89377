"""``points_in_boxes_cpu`` and ``points_in_boxes_gpu`` of OpenPCDet's ops/roiaware_pool3d/roiaware_pool3d_utils.py:9-41
(whose compiled half is a CUDA extension), both on the GPU.

``points_in_boxes_cpu`` is the dense (num_boxes, num_points) int32 membership mask that ``create_groundtruth_database``,
the ``gt_sampling`` augmentor and users' scripts ask for.  Same predicate, bit for bit, as
ops/roiaware_pool3d/src/roiaware_pool3d.cpp:121-168; computed by csrc/kitti_infos.hip (``ops.infos_count``).

``points_in_boxes_gpu`` is the batched (B, num_points) index of the first box that holds each point, the point head's
target assignment (csrc/roipool.hip).  The RoI point pooling is ``utils/roipoint_pool3d``, the
PointNet++ ops are ``utils/pointnet2``.

``RoIAwarePool3d`` / ``RoIAwarePool3dFunction`` are the RoI-aware voxel pooling of PartA2 (the same file, lines 44-107)
on ``modest_amd.utils.roiaware_voxel_pool_cuda`` (csrc/roiaware_pool.hip): the reference's
signature, its ``out_size`` int-or-triple rule and its assertions."""
import numpy as np
import torch
import torch.nn as nn
from torch.autograd import Function


def points_in_boxes_cpu(points, boxes):
    """
    Args:
        points: (num_points, 3)
        boxes: (N, 7) [x, y, z, dx, dy, dz, heading], (x, y, z) is the box centre; boxes may overlap
    Returns:
        point_indices: (N, num_points) int32 -- numpy in, numpy out; tensor in, tensor out (on the input's device)
    """
    from .. import ops
    from ..kitti_infos import host_cos_sin_f32
    assert boxes.shape[1] == 7
    assert points.shape[1] == 3
    is_numpy = isinstance(points, np.ndarray)
    pts = torch.from_numpy(points).float() if is_numpy else points.float()
    bx = torch.from_numpy(boxes).float() if isinstance(boxes, np.ndarray) else boxes.float()
    out_dev = pts.device
    n, nb = pts.shape[0], bx.shape[0]
    if n == 0 or nb == 0:
        out = torch.zeros((nb, n), dtype=torch.int32, device=out_dev)
        return out.numpy() if is_numpy else out
    dev = pts.device if pts.is_cuda else torch.device("cuda", torch.cuda.current_device())
    rows = torch.zeros((n, 4), dtype=torch.float32, device=dev)
    rows[:, :3] = pts.to(dev)
    b32 = bx.detach().cpu().numpy().astype(np.float32)
    fr = np.zeros(1, dtype=ops.INFOS_FRAME)
    fr["n"], fr["box_count"] = n, nb
    tab = np.zeros(nb, dtype=ops.INFOS_BOX)
    tab["b"], tab["bf"] = b32.astype(np.float64), b32
    tab["cosa"], tab["sina"] = host_cos_sin_f32(b32[:, 6])
    tab["reject"] = np.inf          # (no early reject: any float32 input, NaN and huge boxes included, takes the exact path)
    tab["tau"] = 0.0
    st = ops.infos_count(rows, n, fr, tab, und_cap=0, dense_stride=n)
    out = st.dense[:nb].to(out_dev)
    return out.numpy() if is_numpy else out


def points_in_boxes_gpu(points, boxes):
    """
    :param points: (B, M, 3)
    :param boxes: (B, T, 7), num_valid_boxes <= T
    :return box_idxs_of_pts: (B, M) int32, the lowest index of a box that holds the point, background = -1
    """
    from . import roiaware_pool3d_cuda
    assert boxes.shape[0] == points.shape[0]
    assert boxes.shape[2] == 7 and points.shape[2] == 3
    batch_size, num_points, _ = points.shape

    box_idxs_of_pts = points.new_zeros((batch_size, num_points), dtype=torch.int).fill_(-1)
    roiaware_pool3d_cuda.points_in_boxes_gpu(boxes.contiguous(), points.contiguous(), box_idxs_of_pts)
    return box_idxs_of_pts


class RoIAwarePool3d(nn.Module):
    def __init__(self, out_size, max_pts_each_voxel=128):
        super().__init__()
        self.out_size = out_size
        self.max_pts_each_voxel = max_pts_each_voxel

    def forward(self, rois, pts, pts_feature, pool_method='max'):
        assert pool_method in ['max', 'avg']
        return RoIAwarePool3dFunction.apply(rois, pts, pts_feature, self.out_size, self.max_pts_each_voxel, pool_method)


class RoIAwarePool3dFunction(Function):
    @staticmethod
    def forward(ctx, rois, pts, pts_feature, out_size, max_pts_each_voxel, pool_method):
        """
        Args:
            rois: (N, 7) [x, y, z, dx, dy, dz, heading] (x, y, z) is the box centre
            pts: (npoints, 3)
            pts_feature: (npoints, C)
            out_size: int or a triple of ints, like 7 or (7, 7, 7)
            max_pts_each_voxel: words per voxel list, the count word included
            pool_method: 'max' or 'avg'
        Returns:
            pooled_features: (N, out_x, out_y, out_z, C), zero where nothing is pooled
        """
        from . import roiaware_voxel_pool_cuda
        assert rois.shape[1] == 7 and pts.shape[1] == 3
        if isinstance(out_size, int):
            out_x = out_y = out_z = out_size
        else:
            assert len(out_size) == 3
            for k in range(3):
                assert isinstance(out_size[k], int)
            out_x, out_y, out_z = out_size

        num_rois = rois.shape[0]
        num_channels = pts_feature.shape[-1]
        num_pts = pts.shape[0]
        pool_method = {'max': 0, 'avg': 1}[pool_method]

        # the kernels write every count word and read list words only below the count, and max pooling writes every
        # argmax: those two are not zero-filled; pooled_features is, it is written only where
        # something is pooled
        shape = (num_rois, out_x, out_y, out_z)
        pooled_features = pts_feature.new_zeros(shape + (num_channels,))
        pts_idx_of_voxels = pts_feature.new_empty(shape + (max_pts_each_voxel,), dtype=torch.int)
        if pool_method == 0:
            argmax = pts_feature.new_empty(shape + (num_channels,), dtype=torch.int)
        else:
            argmax = pts_feature.new_zeros(shape + (num_channels,), dtype=torch.int)
        roiaware_voxel_pool_cuda.forward(rois.contiguous(), pts.contiguous(), pts_feature.contiguous(), argmax,
                                         pts_idx_of_voxels, pooled_features, pool_method)

        ctx.roiaware_pool3d_for_backward = (pts_idx_of_voxels, argmax, pool_method, num_pts, num_channels)
        return pooled_features

    @staticmethod
    def backward(ctx, grad_out):
        """
        :param grad_out: (N, out_x, out_y, out_z, C)
        :return: grad_in: (npoints, C) for pts_feature
        """
        from . import roiaware_voxel_pool_cuda
        pts_idx_of_voxels, argmax, pool_method, num_pts, num_channels = ctx.roiaware_pool3d_for_backward

        grad_in = grad_out.new_zeros((num_pts, num_channels))
        roiaware_voxel_pool_cuda.backward(pts_idx_of_voxels, argmax, grad_out.contiguous(), grad_in, pool_method)

        return None, None, grad_in, None, None, None
