"""``VoxelizeOnDevice``: the point-to-voxel grouping of PointPillars as a module ahead of the VFE.

With ``transform_points_to_voxels`` replaced by ``calculate_grid_size`` in the data pipeline a batch reaches the GPU as
its stacked points only; this module fills ``voxels``, ``voxel_coords`` and ``voxel_num_points`` from
``batch_dict['points']`` with ``modest_amd.ops.voxelize``, bit for bit what the host generator and
``collate_batch`` produce.
"""
import torch

from .. import ops


class VoxelizeOnDevice(torch.nn.Module):
    def __init__(self, voxel_size, point_cloud_range, max_num_points, max_voxels):
        """max_voxels: an int, or {'train': ..., 'test': ...} chosen by ``self.training``"""
        super().__init__()
        self.geometry = ops.VoxelizeGeometry(voxel_size, point_cloud_range)
        self.max_num_points = int(max_num_points)
        if isinstance(max_voxels, dict):
            self.max_voxels = {"train": int(max_voxels["train"]), "test": int(max_voxels["test"])}
        else:
            self.max_voxels = {"train": int(max_voxels), "test": int(max_voxels)}
        self._workspace = None   # grow-only scratch and the pinned counts, reused from batch to batch
        self._counts = None

    @property
    def grid_size(self):
        return self.geometry.grid_size

    def forward(self, batch_dict):
        points = batch_dict["points"]
        if not isinstance(points, torch.Tensor) or not points.is_cuda:
            raise ValueError("batch_dict['points'] must be a device tensor (after load_data_to_gpu)")
        if points.dtype != torch.float32 or points.ndim != 2 or points.shape[1] < 4:
            raise ValueError(f"batch_dict['points'] must be (N, 1 + C) float32, got {tuple(points.shape)} {points.dtype}")
        points = points.contiguous()
        batch_size = batch_dict.get("batch_size")
        m = self.max_voxels["train" if self.training else "test"]
        pl = ops.voxelize_plan(points, None, None, self.max_num_points, m, None if batch_size is None else int(batch_size),
                               self._workspace, self._counts, self.geometry)
        self._workspace, self._counts = pl.workspace, pl.counts_pinned
        voxels, coords, num, mask = ops.voxelize_fill(pl)
        batch_dict["voxels"] = voxels
        # load_data_to_gpu hands the models float tensors for these two
        batch_dict["voxel_coords"] = coords.float()
        batch_dict["voxel_num_points"] = num.float()
        batch_dict["voxel_point_mask"] = mask
        return batch_dict
