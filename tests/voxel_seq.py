"""The contract of the point-to-voxel grouping, restated sequentially in numpy: spconv 1.2's hard
voxelisation, first come first served.  The yardstick of the host path and of the device path; not a test module.

    grid = round((hi - lo) / vs) in float32
    for every point in order:  c_j = floorf((p_j - lo_j) / vs_j) in float32 (numpy's float32 division is the correctly
    rounded one); dropped unless 0 <= c_j < float(grid_j) on the FLOAT for all three axes; cell (z, y, x) = (c_2, c_1, c_0);
    a cell no earlier point opened becomes voxel V unless max_voxels are open (then the point is dropped and the walk
    goes on); the point takes the voxel's next slot unless max_num_points are taken.
"""
import numpy as np

KEYS = ("voxels", "coordinates", "num_points_per_voxel", "voxel_point_mask")


def grid_size(point_cloud_range, voxel_size):
    rng = np.asarray(point_cloud_range, dtype=np.float32)
    vs = np.asarray(voxel_size, dtype=np.float32)
    return np.round((rng[3:] - rng[:3]) / vs).astype(np.int64)


def cells(points, point_cloud_range, voxel_size):
    """(c (N, 3) float32 = floorf((p - lo) / vs) per axis x, y, z; kept (N,) bool)"""
    rng = np.asarray(point_cloud_range, dtype=np.float32)
    vs = np.asarray(voxel_size, dtype=np.float32)
    g = grid_size(point_cloud_range, voxel_size)
    p = np.asarray(points, dtype=np.float32)[:, :3]
    with np.errstate(invalid="ignore", over="ignore"):
        d = p - rng[None, :3]                 # one rounding
        c = np.floor(d / vs[None, :])         # one correctly rounded division, then floor
        kept = np.all((c >= np.float32(0)) & (c < g.astype(np.float32)[None, :]), axis=1)   # NaN compares false
    assert d.dtype == np.float32 and c.dtype == np.float32
    return c, kept


def voxelize(points, voxel_size, point_cloud_range, max_num_points, max_voxels):
    points = np.ascontiguousarray(points, dtype=np.float32)
    n, width = points.shape
    P, M = int(max_num_points), int(max_voxels)
    c, kept = cells(points, point_cloud_range, voxel_size)
    raw = points.view(np.uint32)
    voxels, coords, num, mask, opened = [], [], [], [], {}
    for i in np.nonzero(kept)[0]:
        x, y, z = int(c[i, 0]), int(c[i, 1]), int(c[i, 2])   # to integer only after the test on the float
        v = opened.get((z, y, x))
        if v is None:
            if len(coords) >= M:
                continue                      # the walk continues
            v = opened[(z, y, x)] = len(coords)
            coords.append((z, y, x))
            num.append(0)
            voxels.append(np.zeros((P, width), dtype=np.uint32))      # +0.0
            mask.append(np.full((P,), -1, dtype=np.int32))
        if num[v] >= P:
            continue
        voxels[v][num[v]] = raw[i]            # raw 32-bit words
        mask[v][num[v]] = i
        num[v] += 1
    V = len(coords)
    return {
        "voxels": (np.stack(voxels) if V else np.zeros((0, P, width), dtype=np.uint32)).view(np.float32),
        "coordinates": np.asarray(coords, dtype=np.int32).reshape(V, 3),
        "num_points_per_voxel": np.asarray(num, dtype=np.int32).reshape(V),
        "voxel_point_mask": np.stack(mask) if V else np.zeros((0, P), dtype=np.int32),
        "voxel_num": V,
    }


def collate(outs, n_points):
    """pcdet/datasets/dataset.py collate_batch for the four keys: outs = per-cloud dicts, n_points = rows per cloud.
    -> (voxels, voxel_coords (sum V, 4) [b, z, y, x], voxel_num_points, voxel_point_mask with stacked indices, counts)"""
    P, width = outs[0]["voxels"].shape[1:]
    masks, coords, count = [], [], 0
    for b, (o, n) in enumerate(zip(outs, n_points)):
        v = o["voxel_point_mask"].copy()
        v[v >= 0] += count
        masks.append(v)
        count += n
        coords.append(np.pad(o["coordinates"], ((0, 0), (1, 0)), mode="constant", constant_values=b))
    return (np.concatenate([o["voxels"] for o in outs]).reshape(-1, P, width),
            np.concatenate(coords).astype(np.int32).reshape(-1, 4),
            np.concatenate([o["num_points_per_voxel"] for o in outs]).astype(np.int32),
            np.concatenate(masks).astype(np.int32).reshape(-1, P),
            np.asarray([o["voxel_num"] for o in outs], dtype=np.int32))


def stack_points(clouds):
    """the collated `points`: (sum N, 1 + C) with the batch index in column 0"""
    width = clouds[0].shape[1]
    return np.concatenate([np.concatenate([np.full((len(c), 1), b, dtype=np.float32), c.astype(np.float32)], axis=1)
                           for b, c in enumerate(clouds)]).reshape(-1, 1 + width)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float32:
        return np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return np.array_equal(a, b)
