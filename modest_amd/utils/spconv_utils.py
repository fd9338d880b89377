"""Drop-in for ``spconv.utils`` as far as PointPillars needs it: ``VoxelGenerator`` / ``VoxelGeneratorV2`` of
spconv 1.2 (hard voxelisation, first come first served), on the host.

``pcdet/datasets/processor/data_processor.py:47-80`` constructs one generator per dataset and calls ``generate`` for
every sample inside DataLoader workers, so nothing here opens the GPU: the walk is ``modest_voxelize_host`` of
libmodest_hip.so, pure host code.  What it computes is DESIGN.md section 7f.  Bound as ``sys.modules["spconv.utils"]``
by ``modest_amd.utils.pcdet_bind.install`` when no real spconv is installed.

A generator owns its cell table and output staging and is not re-entrant: one generator per thread (forked workers
each have their own copy).
"""
import numpy as np

from .. import _lib

MAX_CELLS = 2147483647


def grid_size_f32(voxel_size, point_cloud_range):
    """(lo, vs, grid): the float32 lower corner and voxel size, and round((hi - lo) / vs) taken in float32 as int64"""
    rng = np.asarray(point_cloud_range, dtype=np.float32).reshape(-1)
    vs = np.asarray(voxel_size, dtype=np.float32).reshape(-1)
    if rng.shape != (6,) or vs.shape != (3,):
        raise ValueError("point_cloud_range must have 6 values and voxel_size 3")
    if not (np.all(np.isfinite(rng)) and np.all(np.isfinite(vs)) and np.all(vs > 0)):
        raise ValueError("point_cloud_range and voxel_size must be finite, voxel_size positive")
    grid = np.round((rng[3:] - rng[:3]) / vs).astype(np.int64)
    if np.any(grid < 1):
        raise ValueError(f"the grid {grid.tolist()} has no cells")
    if int(grid[0]) * int(grid[1]) * int(grid[2]) > MAX_CELLS:
        raise ValueError(f"the grid {grid.tolist()} has more than 2^31 - 1 cells")
    return np.ascontiguousarray(rng[:3]), vs, grid


class VoxelGenerator:
    """spconv 1.2's ``VoxelGeneratorV2`` (and ``VoxelGenerator``: one class here, both return the dict)"""

    def __init__(self, voxel_size, point_cloud_range, max_num_points, max_voxels=20000, full_mean=False,
                 block_filtering=False, block_factor=8, block_size=3, height_threshold=0.1, height_high_threshold=2.0):
        if full_mean or block_filtering:
            raise NotImplementedError("full_mean / block_filtering are not provided by modest_amd")
        if (block_factor, block_size, height_threshold, height_high_threshold) != (8, 3, 0.1, 2.0):
            raise NotImplementedError("the block filtering parameters are accepted at their defaults only")
        self._lo, self._voxel_size, self._grid_size = grid_size_f32(voxel_size, point_cloud_range)
        self._point_cloud_range = np.asarray(point_cloud_range, dtype=np.float32).reshape(-1)
        self._max_num_points = int(max_num_points)
        self._max_voxels = int(max_voxels)
        if self._max_num_points < 1 or self._max_voxels < 1:
            raise ValueError("max_num_points and max_voxels must be positive")
        self._grid32 = np.ascontiguousarray(self._grid_size, dtype=np.int32)
        self._table = None    # cell -> voxel number, dense as spconv's; allocated at the first call, left all -1 by every call
        self._stage = None    # (capacity, C) -> output staging

    def generate(self, points, max_voxels=None):
        """points (N, C) float32, C >= 3 -> {'voxels', 'coordinates', 'num_points_per_voxel', 'voxel_point_mask', 'voxel_num'}"""
        pts = np.ascontiguousarray(points, dtype=np.float32)
        if pts.ndim != 2 or pts.shape[1] < 3:
            raise ValueError(f"points has shape {pts.shape}, expected (N, C) with C >= 3")
        m = self._max_voxels if max_voxels is None else int(max_voxels)
        if m < 1:
            raise ValueError("max_voxels must be positive")
        n, c = pts.shape
        p = self._max_num_points
        if self._table is None:
            self._table = np.full(int(np.prod(self._grid_size)), -1, dtype=np.int32)
        # fresh arrays per call, as spconv hands out: the caller keeps what it is given
        voxels = np.empty((m, p, c), dtype=np.float32)
        coords = np.empty((m, 3), dtype=np.int32)
        num = np.empty((m,), dtype=np.int32)
        mask = np.empty((m, p), dtype=np.int32)
        v = _lib.load().modest_voxelize_host(pts.ctypes.data, n, c, self._lo.ctypes.data, self._voxel_size.ctypes.data,
                                             self._grid32.ctypes.data, p, m, self._table.ctypes.data, voxels.ctypes.data,
                                             coords.ctypes.data, num.ctypes.data, mask.ctypes.data)
        if v < 0:
            _lib.check(int(v), "modest_voxelize_host")
        return {"voxels": voxels[:v], "coordinates": coords[:v], "num_points_per_voxel": num[:v],
                "voxel_point_mask": mask[:v], "voxel_num": int(v)}

    @property
    def voxel_size(self):
        return self._voxel_size

    @property
    def max_num_points_per_voxel(self):
        return self._max_num_points

    @property
    def point_cloud_range(self):
        return self._point_cloud_range

    @property
    def grid_size(self):
        return self._grid_size


VoxelGeneratorV2 = VoxelGenerator
