"""Dataset infos + ground-truth database for detector training: a drop-in for the reference's
``python -m pcdet.datasets.kitti.kitti_dataset create_kitti_infos <cfg.yaml> [<data_path>]`` (step 2 of every MODEST round).

Writes what OpenPCDet's ``KittiDataset`` and its ``gt_sampling`` augmentor open: ``kitti_infos_train.pkl``,
``kitti_infos_val.pkl`` (when asked), ``kitti_dbinfos_train.pkl`` and ``gt_database/<idx>_<name>_<i>.bin``.

Reference (downstream/OpenPCDet/pcdet/): datasets/kitti/kitti_dataset.py:176-259 get_infos, :261-314
create_groundtruth_database, :487-540 create_kitti_infos + __main__; utils/object3d_kitti.py; utils/calibration_kitti.py;
utils/box_utils.py:10-53 in_hull / boxes_to_corners_3d; ops/roiaware_pool3d/src/roiaware_pool3d.cpp:121-168.

What stays on the host, bit for bit as the reference computes it: label parsing, the calib dicts, ``gt_boxes_lidar``
(numpy's float32 ``inv`` / ``dot``), the float32 corner table (torch's CPU ops in the reference's order), the host libm's
``cosf`` / ``sinf`` of every heading (ctypes).  What runs on the GPU (``ops.infos_count`` / ``ops.infos_gather``,
csrc/kitti_infos.hip), batched over scans: the FOV flag, ``num_points_in_gt`` and the database rows.  The hull count is a
float64 box test with an undecided band of half width tau; only the points inside the band go to the reference's own
predicate, ``scipy.spatial.Delaunay(corners_f32).find_simplex``.  The train split's ``.bin`` files are read once for
both the infos and the database.

``create_kitti_infos_host`` (``--host``) is the plain numpy / scipy restatement, line for line: the CPU reference of the
GPU path and the baseline of tools/infos_bench.py.

    python -m modest_amd.kitti_infos create_kitti_infos tools/cfgs/dataset_configs/lyft_dataset_dynamic_obj.yaml ../data/lyft_r0
"""
from __future__ import annotations

import argparse
import json
import os
import os.path as osp
import pickle
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

MARGIN = np.float32(1e-2)   # roiaware_pool3d.cpp:131
TAU0 = 2.0 ** -15           # metres; the undecided band of the hull test, see hull_tau


class AttrDict(dict):
    """the YAML mapping with attribute access (the reference wraps it in EasyDict)"""

    def __getattr__(self, k):
        try:
            v = self[k]
        except KeyError:
            raise AttributeError(k) from None
        return AttrDict(v) if isinstance(v, dict) and not isinstance(v, AttrDict) else v


def _say(verbose, *a):
    if verbose:
        print(*a, file=sys.stderr)


# ---- the reference's host pieces --------------------------------------------------------------------------------------
class Calibration:
    """utils/calibration_kitti.py:4-84: P2, R0, V2C in float32 from lines 2, 4 and 5 of the file"""

    def __init__(self, calib_file):
        with open(calib_file) as f:
            lines = f.readlines()
        row = lambda k: np.array(lines[k].strip().split(" ")[1:], dtype=np.float32)   # noqa: E731
        self.P2 = row(2).reshape(3, 4)
        self.R0 = row(4).reshape(3, 3)
        self.V2C = row(5).reshape(3, 4)

    @staticmethod
    def cart_to_hom(pts):
        return np.hstack((pts, np.ones((pts.shape[0], 1), dtype=np.float32)))

    def rect_to_lidar(self, pts_rect):
        """:51-62"""
        pts_rect_hom = self.cart_to_hom(pts_rect)
        R0_ext = np.hstack((self.R0, np.zeros((3, 1), dtype=np.float32)))
        R0_ext = np.vstack((R0_ext, np.zeros((1, 4), dtype=np.float32)))
        R0_ext[3, 3] = 1
        V2C_ext = np.vstack((self.V2C, np.zeros((1, 4), dtype=np.float32)))
        V2C_ext[3, 3] = 1
        pts_lidar = np.dot(pts_rect_hom, np.linalg.inv(np.dot(R0_ext, V2C_ext).T))
        return pts_lidar[:, 0:3]

    def lidar_to_rect_matrix(self):
        """the (4,3) float32 matrix of :64-73"""
        return np.dot(self.V2C.T, self.R0.T)

    def lidar_to_rect(self, pts_lidar):
        return np.dot(self.cart_to_hom(pts_lidar), self.lidar_to_rect_matrix())

    def rect_to_img(self, pts_rect):
        """:75-84"""
        pts_rect_hom = self.cart_to_hom(pts_rect)
        pts_2d_hom = np.dot(pts_rect_hom, self.P2.T)
        with np.errstate(divide="ignore", invalid="ignore"):
            pts_img = (pts_2d_hom[:, 0:2].T / pts_rect_hom[:, 2]).T
        pts_rect_depth = pts_2d_hom[:, 2] - self.P2.T[3, 2]
        return pts_img, pts_rect_depth


class LabelObject:
    """one line of a label_2 file (utils/object3d_kitti.py:18-52)"""

    def __init__(self, line):
        v = line.strip().split(" ")
        self.cls_type = v[0]
        self.truncation, self.occlusion, self.alpha = float(v[1]), float(v[2]), float(v[3])
        self.box2d = np.array((float(v[4]), float(v[5]), float(v[6]), float(v[7])), dtype=np.float32)
        self.h, self.w, self.l = float(v[8]), float(v[9]), float(v[10])
        self.loc = np.array((float(v[11]), float(v[12]), float(v[13])), dtype=np.float32)
        self.ry = float(v[14])
        self.score = float(v[15]) if len(v) == 16 else -1.0
        self.level = self.kitti_level()

    def kitti_level(self):
        height = float(self.box2d[3]) - float(self.box2d[1]) + 1
        if height >= 40 and self.truncation <= 0.15 and self.occlusion <= 0:
            return 0
        if height >= 25 and self.truncation <= 0.3 and self.occlusion <= 1:
            return 1
        if height >= 25 and self.truncation <= 0.5 and self.occlusion <= 2:
            return 2
        return -1


def get_objects_from_label(label_file):
    with open(label_file) as f:
        return [LabelObject(line) for line in f.readlines()]


def get_image_shape(img_file):
    """(H, W) int32 from the file's header; the reference decodes the whole image for the same two numbers"""
    from PIL import Image
    with Image.open(img_file) as im:
        w, h = im.size
    return np.array((h, w), dtype=np.int32)


def boxes_to_corners_3d(boxes3d):
    """utils/box_utils.py:28-53 on a numpy array: torch's float32 CPU ops in the reference's order -> (N, 8, 3) float32"""
    import torch
    b = torch.from_numpy(np.ascontiguousarray(boxes3d)).float()
    template = b.new_tensor(([1, 1, -1], [1, -1, -1], [-1, -1, -1], [-1, 1, -1],
                             [1, 1, 1], [1, -1, 1], [-1, -1, 1], [-1, 1, 1])) / 2
    corners = b[:, None, 3:6].repeat(1, 8, 1) * template[None, :, :]
    angle = b[:, 6]
    cosa, sina = torch.cos(angle), torch.sin(angle)
    zeros, ones = angle.new_zeros(corners.shape[0]), angle.new_ones(corners.shape[0])
    rot = torch.stack((cosa, sina, zeros, -sina, cosa, zeros, zeros, zeros, ones), dim=1).view(-1, 3, 3).float()
    corners = torch.matmul(corners.view(-1, 8, 3)[:, :, 0:3], rot).view(-1, 8, 3)
    corners += b[:, None, 0:3]
    return corners.numpy()


def in_hull(p, corners):
    """utils/box_utils.py:10-25: Delaunay of the eight corners; a degenerate box counts nothing (with the warning)"""
    from scipy.spatial import Delaunay, QhullError
    if len(p) == 0:
        return np.zeros(0, dtype=bool)
    try:
        return Delaunay(corners).find_simplex(p) >= 0
    except QhullError:
        print("Warning: not a hull %s" % str(corners), file=sys.stderr)
        return np.zeros(p.shape[0], dtype=bool)


def in_hull_near(p, corners, pad=1e-3):
    """in_hull, asking Delaunay only about the points inside the corners' bounding box grown by `pad` (a point
    farther out lies outside the hull by a thousand times Qhull's tolerance): same flags, a fraction of the time"""
    lo, hi = corners.min(axis=0) - pad, corners.max(axis=0) + pad
    near = np.nonzero(((p >= lo) & (p <= hi)).all(axis=1))[0]
    flag = np.zeros(p.shape[0], dtype=bool)
    flag[near] = in_hull(p[near], corners)
    return flag


def get_fov_flag(points, calib, img_shape):
    """kitti_dataset.py:158-173 on lidar rows"""
    pts_rect = calib.lidar_to_rect(points[:, 0:3])
    pts_img, depth = calib.rect_to_img(pts_rect)
    f1 = np.logical_and(pts_img[:, 0] >= 0, pts_img[:, 0] < img_shape[1])
    f2 = np.logical_and(pts_img[:, 1] >= 0, pts_img[:, 1] < img_shape[0])
    return np.logical_and(np.logical_and(f1, f2), depth >= 0)


_LIBM = None


def _libm():
    global _LIBM
    if _LIBM is None:
        import ctypes
        import ctypes.util
        lib = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        for fn in (lib.cosf, lib.sinf):
            fn.restype, fn.argtypes = ctypes.c_float, [ctypes.c_float]
        _LIBM = lib
    return _LIBM


def host_cos_sin_f32(rz_f32):
    """roiaware_pool3d.cpp:122: ``float cosa = cos(-rot_angle), sina = sin(-rot_angle)`` on a float argument binds to the
    float overloads, i.e. the host C library's ``cosf`` / ``sinf`` (the compiled reference imports exactly these two
    symbols).  They are not correctly rounded -- glibc's differ from the rounded double cos / sin on about 1.3 % of the
    angles -- so they are called here, through ctypes, and nothing else stands in for them."""
    m = _libm()
    a = np.asarray(rz_f32, dtype=np.float32).ravel()
    cosa = np.array([m.cosf(-float(v)) for v in a], dtype=np.float32)
    sina = np.array([m.sinf(-float(v)) for v in a], dtype=np.float32)
    return cosa, sina


def points_in_boxes_host(points, boxes):
    """roiaware_pool3d.cpp:128-168 as numpy: (B, N) int32.  float32 differences and products (numpy does not fuse),
    the three comparisons in float64."""
    pts = np.ascontiguousarray(points, dtype=np.float32)
    bx = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 7)
    out = np.zeros((len(bx), len(pts)), dtype=np.int32)
    if len(bx) == 0 or len(pts) == 0:
        return out
    cosa, sina = host_cos_sin_f32(bx[:, 6])
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    for i, b in enumerate(bx):
        zok = ~(np.abs(z - b[2]).astype(np.float64) > np.float64(b[5]) / 2.0)
        sx, sy = x - b[0], y - b[1]
        lx = sx * cosa[i] + sy * (-sina[i])
        ly = sx * sina[i] + sy * cosa[i]
        assert lx.dtype == np.float32
        inx = np.abs(lx).astype(np.float64) < np.float64(b[3]) / 2.0 + np.float64(MARGIN)
        iny = np.abs(ly).astype(np.float64) < np.float64(b[4]) / 2.0 + np.float64(MARGIN)
        out[i] = zok & inx & iny
    return out


def box_margin64(points, box7):
    """distance-like margin of float32 points against the ideal float64 box: min over the axes of half extent - |local|
    (the extents without their sign, as _box_table hands them to the device)"""
    b = np.array(box7, dtype=np.float64)
    b[3:6] = np.abs(b[3:6])
    p = np.asarray(points, dtype=np.float64)
    sx, sy, sz = p[:, 0] - b[0], p[:, 1] - b[1], p[:, 2] - b[2]
    c, s = np.cos(b[6]), np.sin(b[6])
    lx, ly = sx * c + sy * s, -sx * s + sy * c
    return np.minimum(np.minimum(b[3] * 0.5 - np.abs(lx), b[4] * 0.5 - np.abs(ly)), b[5] * 0.5 - np.abs(sz))


def hull_tau(corners_f32):
    """half width of the band in which the ideal float64 box and the hull of the float32 corners may disagree:
    2^-15 m, growing with the corner coordinates beyond 128 m (half a float32 ulp at 128 m is 3.8e-6 m)"""
    m = float(np.max(np.abs(corners_f32))) if np.size(corners_f32) else 0.0
    return TAU0 * max(1.0, m / 128.0)


# ---- infos without the counts (host only) -----------------------------------------------------------------------------
def scene_info(split_dir, sample_idx, has_label=True):
    """kitti_dataset.py:179-231: everything of one scan's info except num_points_in_gt.  Returns (info, calib)."""
    split_dir = Path(split_dir)
    info = {"point_cloud": {"num_features": 4, "lidar_idx": sample_idx}}
    info["image"] = {"image_idx": sample_idx, "image_shape": get_image_shape(split_dir / "image_2" / ("%s.png" % sample_idx))}
    calib = Calibration(split_dir / "calib" / ("%s.txt" % sample_idx))
    P2 = np.concatenate([calib.P2, np.array([[0., 0., 0., 1.]])], axis=0)
    R0_4x4 = np.zeros([4, 4], dtype=calib.R0.dtype)
    R0_4x4[3, 3] = 1.
    R0_4x4[:3, :3] = calib.R0
    V2C_4x4 = np.concatenate([calib.V2C, np.array([[0., 0., 0., 1.]])], axis=0)
    info["calib"] = {"P2": P2, "R0_rect": R0_4x4, "Tr_velo_to_cam": V2C_4x4}
    if not has_label:
        return info, calib
    objs = get_objects_from_label(split_dir / "label_2" / ("%s.txt" % sample_idx))
    a = {}
    a["name"] = np.array([o.cls_type for o in objs])
    a["truncated"] = np.array([o.truncation for o in objs])
    a["occluded"] = np.array([o.occlusion for o in objs])
    a["alpha"] = np.array([o.alpha for o in objs])
    a["bbox"] = np.concatenate([o.box2d.reshape(1, 4) for o in objs], axis=0) if len(objs) > 0 else np.array([]).reshape(0, 4)
    a["dimensions"] = np.array([[o.l, o.h, o.w] for o in objs]).reshape(-1, 3)
    a["location"] = np.concatenate([o.loc.reshape(1, 3) for o in objs], axis=0) if len(objs) > 0 else np.array([]).reshape(0, 3)
    a["rotation_y"] = np.array([o.ry for o in objs])
    a["score"] = np.array([o.score for o in objs])
    a["difficulty"] = np.array([o.level for o in objs], np.int32)
    num_objects = len([o.cls_type for o in objs if o.cls_type != "DontCare"])
    num_gt = len(a["name"])
    a["index"] = np.array(list(range(num_objects)) + [-1] * (num_gt - num_objects), dtype=np.int32)
    if len(objs) > 0:
        loc, dims, rots = a["location"][:num_objects], a["dimensions"][:num_objects], a["rotation_y"][:num_objects]
        loc_lidar = calib.rect_to_lidar(loc)
        l, h, w = dims[:, 0:1], dims[:, 1:2], dims[:, 2:3]
        loc_lidar[:, 2] += h[:, 0] / 2
        a["gt_boxes_lidar"] = np.concatenate([loc_lidar, l, w, h, -(np.pi / 2 + rots[..., np.newaxis])], axis=1)
    else:
        a["gt_boxes_lidar"] = np.array([])
    info["annos"] = a
    return info, calib


def _read_split(root, split):
    f = Path(root) / "ImageSets" / (split + ".txt")
    if not f.exists():
        raise FileNotFoundError("%s: no such split file (data path %s)" % (f, Path(root).resolve()))
    return [x.strip() for x in open(f).readlines()]


def _split_dir(root, split):
    return Path(root) / ("training" if split != "test" else "testing")


def _read_bin(split_dir, idx):
    return np.fromfile(str(Path(split_dir) / "velodyne" / ("%s.bin" % idx)), dtype=np.float32).reshape(-1, 4)


def _atomic_write(path, data: bytes):
    """the PP CLI's temporary file + os.replace (pre_compute_pp_score.write_atomic): no truncated file survives a kill"""
    from .pre_compute_pp_score import write_atomic

    def put(tmp):
        with open(tmp, "wb") as f:
            f.write(data)
    write_atomic(path, put)


def _db_dir(root, split):
    return Path(root) / ("gt_database" if split == "train" else ("gt_database_%s" % split))


def _db_info(root, db_dir, sample_idx, annos, i, n_pts, used_classes, all_db_infos):
    """kitti_dataset.py:296-306"""
    names = annos["name"]
    filepath = Path(db_dir) / ("%s_%s_%d.bin" % (sample_idx, names[i], i))
    if (used_classes is None) or names[i] in used_classes:
        db_info = {"name": names[i], "path": str(filepath.relative_to(root)), "image_idx": sample_idx, "gt_idx": i,
                   "box3d_lidar": annos["gt_boxes_lidar"][i], "num_points_in_gt": n_pts,
                   "difficulty": annos["difficulty"][i], "bbox": annos["bbox"][i], "score": annos["score"][i]}
        all_db_infos.setdefault(names[i], []).append(db_info)
    return filepath


# ---- host mirror ------------------------------------------------------------------------------------------------------
def count_points_host(points, info, calib, fov_points_only=True, exact_hull=False):
    """kitti_dataset.py:233-255: num_points_in_gt of one scan (and the FOV flag it used, or None)"""
    a = info["annos"]
    num_gt = len(a["name"])
    if num_gt == 0:
        return np.ones(0, dtype=np.int32), None
    num_objects = len(a["gt_boxes_lidar"])
    fov = get_fov_flag(points, calib, info["image"]["image_shape"]) if fov_points_only else None
    pts_fov = points[fov] if fov_points_only else points
    corners = boxes_to_corners_3d(a["gt_boxes_lidar"])
    num = -np.ones(num_gt, dtype=np.int32)
    hull = in_hull if exact_hull else in_hull_near
    for k in range(num_objects):
        num[k] = hull(pts_fov[:, 0:3], corners[k]).sum()
    return num, fov


def get_infos_host(root, split, fov_points_only=True, has_label=True, count_inside_pts=True, sample_id_list=None,
                   num_workers=4, verbose=False, exact_hull=False):
    """KittiDataset.get_infos (kitti_dataset.py:176-259) in numpy / scipy, `num_workers` threads as the reference"""
    sd = _split_dir(root, split)
    ids = sample_id_list if sample_id_list is not None else _read_split(root, split)

    def one(idx):
        _say(verbose, "%s sample_idx: %s" % (split, idx))
        info, calib = scene_info(sd, idx, has_label)
        if has_label and count_inside_pts:
            pts = _read_bin(sd, idx) if len(info["annos"]["name"]) > 0 else None
            info["annos"]["num_points_in_gt"], _ = count_points_host(pts, info, calib, fov_points_only, exact_hull)
        return info

    with ThreadPoolExecutor(num_workers) as ex:
        return list(ex.map(one, ids))


def create_groundtruth_database_host(root, info_path, used_classes=None, split="train", verbose=False):
    """KittiDataset.create_groundtruth_database (kitti_dataset.py:261-314) in numpy"""
    root = Path(root)
    db_dir = _db_dir(root, split)
    db_dir.mkdir(parents=True, exist_ok=True)
    sd = _split_dir(root, split)
    all_db_infos = {}
    with open(info_path, "rb") as f:
        infos = pickle.load(f)
    n_rows = 0
    for k, info in enumerate(infos):
        _say(verbose, "gt_database sample: %d/%d" % (k + 1, len(infos)))
        sample_idx = info["point_cloud"]["lidar_idx"]
        annos = info["annos"]
        gt_boxes = annos["gt_boxes_lidar"]
        if gt_boxes.shape[0] == 0:
            continue
        points = _read_bin(sd, sample_idx)
        mask = points_in_boxes_host(points[:, 0:3], gt_boxes)
        for i in range(gt_boxes.shape[0]):
            gt_points = points[mask[i] > 0]
            gt_points[:, :3] -= gt_boxes[i, :3]
            filepath = _db_info(root, db_dir, sample_idx, annos, i, gt_points.shape[0], used_classes, all_db_infos)
            _atomic_write(filepath, gt_points.tobytes())
            n_rows += len(gt_points)
    for k, v in all_db_infos.items():
        _say(verbose, "Database %s: %d" % (k, len(v)))
    _atomic_write(root / ("kitti_dbinfos_%s.pkl" % split), pickle.dumps(all_db_infos))
    return all_db_infos, n_rows


def create_kitti_infos_host(dataset_cfg, class_names, data_path, save_path, if_val=True, workers=4, verbose=False, stats=None):
    """create_kitti_infos (kitti_dataset.py:487-524) from the host mirror alone (no GPU)"""
    data_path, save_path = Path(data_path), Path(save_path)
    fov = bool(dataset_cfg.get("FOV_POINTS_ONLY", False))
    t0 = time.perf_counter()
    train = get_infos_host(data_path, "train", fov, num_workers=workers, verbose=verbose)
    _atomic_write(save_path / "kitti_infos_train.pkl", pickle.dumps(train))
    val = []
    if if_val:
        val = get_infos_host(data_path, "val", fov, num_workers=workers, verbose=verbose)
        _atomic_write(save_path / "kitti_infos_val.pkl", pickle.dumps(val))
    t1 = time.perf_counter()
    db, n_rows = create_groundtruth_database_host(data_path, save_path / "kitti_infos_train.pkl", split="train", verbose=verbose)
    t2 = time.perf_counter()
    if stats is not None:
        stats.update(scans=len(train) + len(val), boxes=sum(len(i["annos"]["gt_boxes_lidar"]) for i in train + val),
                     db_points=n_rows, host_boxes=None, infos_s=t1 - t0, db_s=t2 - t1, wall_s=t2 - t0)
    return train, val, db


# ---- the batched GPU path ---------------------------------------------------------------------------------------------
def _box_table(gt_boxes, corners):
    """ops.INFOS_BOX rows of one scan's boxes"""
    from . import ops
    nb = len(gt_boxes)
    t = np.zeros(nb, dtype=ops.INFOS_BOX)
    if nb == 0:
        return t
    b64 = np.ascontiguousarray(gt_boxes, dtype=np.float64)
    b32 = b64.astype(np.float32)
    t["b"], t["bf"] = b64, b32
    # the hull test sees the extents without their sign: the eight corners of a box with a negative size are those of
    # the box with its absolute value, and the reference counts the points inside their hull (bf, which the database
    # predicate reads, keeps the sign: |local| < negative / 2 + MARGIN holds for no point, as in the reference)
    t["b"][:, 3:6] = np.abs(b64[:, 3:6])
    t["cs"][:, 0], t["cs"][:, 1] = np.cos(b64[:, 6]), np.sin(b64[:, 6])
    t["cosa"], t["sina"] = host_cos_sin_f32(b32[:, 6])
    tau = np.array([hull_tau(corners[k]) for k in range(nb)])
    t["tau"] = tau
    # no member and no undecided point beyond this in max(|x-cx|, |y-cy|): half diagonal of the footprint, the
    # database margin on both axes (0.01 * sqrt 2), tau, and 1e-5 of the coordinates for the float32 differences
    half_diag = 0.5 * np.hypot(np.abs(b64[:, 3]), np.abs(b64[:, 4]))
    reach = np.maximum(np.abs(b64[:, 0]), np.abs(b64[:, 1])) + half_diag
    t["reject"] = (half_diag + 0.015 + tau + 1e-3 + 1e-5 * reach).astype(np.float32) * np.float32(1.001)
    return t


class _Batcher:
    """one split through the GPU in batches of scans: infos (counts) and / or database rows"""

    def __init__(self, root, split, fov_points_only, batch, readers, und_cap, pass_boxes, device, verbose):
        import torch
        from . import ops
        from ._lib import default_context
        from .ground_planes import _Reader
        self.root, self.split, self.sd = Path(root), split, _split_dir(root, split)
        self.fov_only, self.batch, self.und_cap, self.pass_boxes = bool(fov_points_only), int(batch), int(und_cap), int(pass_boxes)
        self.verbose = verbose
        self.dev = torch.device("cuda", device)
        torch.cuda.set_device(self.dev)
        default_context(device)
        self.reader = _Reader(readers)
        self.rows_dev = torch.empty((0, 4), dtype=torch.float32, device=self.dev)
        self.t = dict(read_s=0.0, host_s=0.0, h2d_s=0.0, gpu_s=0.0, hull_host_s=0.0, write_s=0.0, scans=0, boxes=0, db_points=0,
                      host_boxes=0, undecided_points=0, overflow_boxes=0, bytes=0)

    def _load(self, ids, infos):
        """reader thread: the batch's .bin files into pinned memory; host tables.  infos: None (parse here) or given"""
        from . import ops
        t0 = time.perf_counter()
        host, offs, nbytes = self.reader.read([str(self.sd / "velodyne" / (i + ".bin")) for i in ids])
        t1 = time.perf_counter()
        if infos is None:
            infos = []
            for i in ids:
                _say(self.verbose, "%s sample_idx: %s" % (self.split, i))
                info, calib = scene_info(self.sd, i)
                infos.append((info, calib))
        fr = np.zeros(len(ids), dtype=ops.INFOS_FRAME)
        fr["row_offset"], fr["n"] = offs[:-1], np.diff(offs)
        tabs, corners_all = [], []
        nb_run = cnt_run = 0
        chunk = ops.infos_chunk_rows()
        for k, (info, calib) in enumerate(infos):
            gt = info["annos"]["gt_boxes_lidar"]
            gt = gt if gt.ndim == 2 else np.zeros((0, 7))
            corners = boxes_to_corners_3d(gt) if len(gt) else np.zeros((0, 8, 3), dtype=np.float32)
            tabs.append(_box_table(gt, corners))
            corners_all.append(corners)
            fr["box_begin"][k], fr["box_count"][k], fr["cnt_offset"][k] = nb_run, len(gt), cnt_run
            nb_run += len(gt)
            cnt_run += -(-int(fr["n"][k]) // chunk) * len(gt)
            if calib is not None:
                fr["m1"][k] = calib.lidar_to_rect_matrix().reshape(-1)
                fr["p2t"][k] = np.ascontiguousarray(calib.P2.T).reshape(-1)
            fr["height"][k], fr["width"][k] = info["image"]["image_shape"]
            fr["fov_only"][k] = int(self.fov_only)
        boxes = np.concatenate(tabs) if tabs else np.zeros(0, dtype=ops.INFOS_BOX)
        self.t["read_s"] += t1 - t0
        self.t["host_s"] += time.perf_counter() - t1
        self.t["bytes"] += nbytes
        return host, offs, infos, fr, boxes, corners_all, cnt_run

    def run(self, ids, infos_in=None, want_counts=True, emit=None):
        """yields nothing; fills num_points_in_gt of every info (want_counts) and calls emit(idx, info, rows, counts,
        bases) per scan with the database rows of the batch (emit given).  Returns the infos in order."""
        import torch
        from . import ops
        out = []
        batches = [(ids[b:b + self.batch], None if infos_in is None else infos_in[b:b + self.batch])
                   for b in range(0, len(ids), self.batch)]
        with ThreadPoolExecutor(1) as rd:
            nxt = rd.submit(self._load, *batches[0]) if batches else None
            for bi in range(len(batches)):
                host, offs, infos, fr, boxes, corners_all, cnt_words = nxt.result()
                # the reader has two pinned slots used in turn: the next batch is read while this one is worked on
                nxt = rd.submit(self._load, *batches[bi + 1]) if bi + 1 < len(batches) else None
                R = int(offs[-1])
                if self.rows_dev.shape[0] < R:
                    self.rows_dev = torch.empty((R + R // 8, 4), dtype=torch.float32, device=self.dev)
                ec, e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                ec.record()
                self.rows_dev[:R].copy_(host, non_blocking=True)
                e0.record()
                st = ops.infos_count(self.rows_dev, R, fr, boxes, cnt_words, pass_boxes=self.pass_boxes, und_cap=self.und_cap)
                res = st.read()                                   # synchronisation 1: the sizes
                rows = None
                if emit is not None:
                    rows = ops.infos_gather(st)                   # synchronisation 2: the rows
                e1.record()
                torch.cuda.synchronize()
                self.t["h2d_s"] += ec.elapsed_time(e0) / 1e3    # the upload of the batch's rows
                self.t["gpu_s"] += e0.elapsed_time(e1) / 1e3    # count, read-back, gather, read-back
                hostv = host.numpy()
                t0 = time.perf_counter()
                hull, und_n, und_idx, db_count = res
                for k, (info, calib) in enumerate(infos):
                    b0, nb = int(fr["box_begin"][k]), int(fr["box_count"][k])
                    a = info["annos"]
                    if want_counts:
                        num_gt = len(a["name"])
                        if num_gt == 0:
                            a["num_points_in_gt"] = np.ones(0, dtype=np.int32)
                        else:
                            num = -np.ones(num_gt, dtype=np.int32)
                            pts = hostv[int(offs[k]):int(offs[k + 1])]
                            fov = None
                            for j in range(nb):
                                g = b0 + j
                                c = int(hull[g])
                                if und_n[g] > self.und_cap:       # the list overflowed: the whole box on the host
                                    if fov is None and self.fov_only:
                                        fov = get_fov_flag(pts, calib, info["image"]["image_shape"])
                                    pf = pts[fov] if self.fov_only else pts
                                    c = int(in_hull_near(pf[:, 0:3], corners_all[k][j]).sum())
                                    self.t["overflow_boxes"] += 1
                                    self.t["host_boxes"] += 1
                                elif und_n[g] > 0:
                                    sel = np.sort(und_idx[g, :und_n[g]])
                                    c += int(in_hull(pts[sel, 0:3], corners_all[k][j]).sum())
                                    self.t["undecided_points"] += int(und_n[g])
                                    self.t["host_boxes"] += 1
                                num[j] = c
                            a["num_points_in_gt"] = num
                    self.t["boxes"] += nb
                self.t["hull_host_s"] += time.perf_counter() - t0
                if emit is not None:
                    base = np.concatenate([[0], np.cumsum(db_count)]).astype(np.int64)
                    for k, (info, calib) in enumerate(infos):
                        b0, nb = int(fr["box_begin"][k]), int(fr["box_count"][k])
                        emit(info, rows, base[b0:b0 + nb + 1])
                    self.t["db_points"] += int(base[-1])
                self.t["scans"] += len(infos)
                out.extend(info for info, _ in infos)
        return out


class _DbWriter:
    """writer thread of the database files (atomic rename) + the db_info dicts in the reference's order"""

    def __init__(self, root, split, used_classes, t):
        self.root, self.db_dir, self.used = Path(root), _db_dir(root, split), used_classes
        self.db_dir.mkdir(parents=True, exist_ok=True)
        self.all_db_infos = {}
        self.pool = ThreadPoolExecutor(1)
        self.pending = []
        self.t = t

    def emit(self, info, rows, base):
        annos = info["annos"]
        idx = info["point_cloud"]["lidar_idx"]
        jobs = []
        for i in range(len(base) - 1):
            n = int(base[i + 1] - base[i])
            path = _db_info(self.root, self.db_dir, idx, annos, i, n, self.used, self.all_db_infos)
            jobs.append((path, rows[int(base[i]):int(base[i + 1])]))
        if jobs:
            self.pending.append(self.pool.submit(self._write, jobs))

    def _write(self, jobs):
        t0 = time.perf_counter()
        for path, r in jobs:
            _atomic_write(path, r.tobytes())
        self.t["write_s"] += time.perf_counter() - t0

    def close(self):
        for p in self.pending:
            p.result()
        self.pool.shutdown()


def get_infos(root, split, fov_points_only=True, has_label=True, count_inside_pts=True, sample_id_list=None, *,
              batch=64, readers=8, und_cap=32, pass_boxes=256, device=0, verbose=False, stats=None, _db=None):
    """KittiDataset.get_infos with num_points_in_gt counted on the GPU"""
    ids = sample_id_list if sample_id_list is not None else _read_split(root, split)
    if not (has_label and (count_inside_pts or _db is not None)):
        sd = _split_dir(root, split)
        return [scene_info(sd, i, has_label)[0] for i in ids]
    bt = _Batcher(root, split, fov_points_only, batch, readers, und_cap, pass_boxes, device, verbose)
    infos = bt.run(ids, None, want_counts=count_inside_pts, emit=_db.emit if _db is not None else None)
    if stats is not None:
        for k, v in bt.t.items():
            stats[k] = stats.get(k, 0) + v
    return infos


def create_groundtruth_database(root, info_path, used_classes=None, split="train", *, batch=64, readers=8,
                                pass_boxes=256, device=0, verbose=False, stats=None):
    """KittiDataset.create_groundtruth_database from an infos pickle, the members gathered on the GPU"""
    root = Path(root)
    with open(info_path, "rb") as f:
        infos = pickle.load(f)
    t = dict(write_s=0.0)
    db = _DbWriter(root, split, used_classes, t)
    bt = _Batcher(root, split, False, batch, readers, 0, pass_boxes, device, verbose)
    ids = [i["point_cloud"]["lidar_idx"] for i in infos]
    for k in range(len(infos)):
        _say(verbose, "gt_database sample: %d/%d" % (k + 1, len(infos)))
    bt.run(ids, [(i, None) for i in infos], want_counts=False, emit=db.emit)
    db.close()
    for k, v in db.all_db_infos.items():
        _say(verbose, "Database %s: %d" % (k, len(v)))
    _atomic_write(root / ("kitti_dbinfos_%s.pkl" % split), pickle.dumps(db.all_db_infos))
    if stats is not None:
        stats.update(bt.t)
        stats["write_s"] = t["write_s"]
    return db.all_db_infos


def create_kitti_infos(dataset_cfg, class_names, data_path, save_path, if_val=True, workers=4, *, batch=64, readers=8,
                       und_cap=32, pass_boxes=256, device=0, verbose=False, stats=None):
    """create_kitti_infos (kitti_dataset.py:487-524).  One pass over the train split serves both its infos and its
    database; the three pickles are written last.  `workers` is accepted for the reference's signature (the scans go
    through the GPU in batches instead)."""
    data_path, save_path = Path(data_path), Path(save_path)
    fov = bool(dataset_cfg.get("FOV_POINTS_ONLY", False))
    st = {} if stats is None else stats
    wall0 = time.perf_counter()
    wt = dict(write_s=0.0)
    db = _DbWriter(data_path, "train", None, wt)
    kw = dict(batch=batch, readers=readers, und_cap=und_cap, pass_boxes=pass_boxes, device=device, verbose=verbose, stats=st)
    train = get_infos(data_path, "train", fov, _db=db, **kw)
    val = get_infos(data_path, "val", fov, **kw) if if_val else None
    db.close()
    for k, v in db.all_db_infos.items():
        _say(verbose, "Database %s: %d" % (k, len(v)))
    t0 = time.perf_counter()
    _atomic_write(save_path / "kitti_infos_train.pkl", pickle.dumps(train))
    if if_val:
        _atomic_write(save_path / "kitti_infos_val.pkl", pickle.dumps(val))
    _atomic_write(data_path / "kitti_dbinfos_train.pkl", pickle.dumps(db.all_db_infos))
    st["write_s"] = st.get("write_s", 0.0) + wt["write_s"]
    st["pickle_s"] = time.perf_counter() - t0
    st["wall_s"] = time.perf_counter() - wall0
    return train, val, db.all_db_infos


# ---- CLI --------------------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("func", choices=["create_kitti_infos"])
    p.add_argument("cfg", help="dataset YAML (FOV_POINTS_ONLY and DATA_PATH are read)")
    p.add_argument("data_path", nargs="?", default=None,
                   help="dataset root; a relative path is taken from the YAML's tools/ directory (<cfg dir>/../..) as the "
                        "reference does, or from the working directory when it exists there")
    p.add_argument("if_val", nargs="?", default=None, help='"True": also write kitti_infos_val.pkl (the reference\'s argv[4])')
    p.add_argument("--batch", type=int, default=64, help="scans per GPU call")
    p.add_argument("--readers", type=int, default=8, help="host threads reading .bin files")
    p.add_argument("--und_cap", type=int, default=32, help="undecided points kept per box before the whole box goes to the host")
    p.add_argument("--pass_boxes", type=int, default=256, help="boxes of a scan held in LDS per pass (at most 256)")
    p.add_argument("--host", action="store_true", help="the numpy / scipy mirror, no GPU")
    p.add_argument("--workers", type=int, default=4, help="threads of the mirror (the reference's num_workers)")
    p.add_argument("--overwrite", action="store_true", help="run even when kitti_infos_train.pkl exists")
    p.add_argument("--verbose", action="store_true", help="the reference's progress lines, on stderr")
    return p.parse_args(argv)


def resolve_data_path(cfg_file, data_path):
    """an absolute path as it is; a relative one from <cfg dir>/../.. (the reference's ROOT_DIR / 'tools' when the YAML
    lies in its tree, kitti_dataset.py:531-536), and only when nothing is there from the working directory"""
    if osp.isabs(data_path):
        return Path(data_path)
    ref = (Path(cfg_file).resolve().parent / ".." / ".." / data_path).resolve()
    if ref.is_dir() or not osp.isdir(data_path):
        return ref
    return Path(data_path).resolve()


def main(argv=None):
    import yaml
    a = parse_args(argv)
    with open(a.cfg) as f:
        cfg = AttrDict(yaml.safe_load(f))
    root = resolve_data_path(a.cfg, cfg.DATA_PATH if a.data_path is None else a.data_path)
    if_val = a.if_val == "True"
    if not (root / "ImageSets" / "train.txt").exists():
        print("modest_amd.kitti_infos: %s not found; the data path %r was resolved to %s"
              % (root / "ImageSets" / "train.txt", cfg.DATA_PATH if a.data_path is None else a.data_path, root), file=sys.stderr)
        return 2
    if (root / "kitti_infos_train.pkl").exists() and not a.overwrite:
        print("modest_amd.kitti_infos: %s exists, NOTHING WAS WRITTEN (the reference regenerates on every call): pass "
              "--overwrite to regenerate the infos and the database" % (root / "kitti_infos_train.pkl"), file=sys.stderr)
        print(json.dumps({"tool": "kitti_infos", "skipped": True, "data_path": str(root)}), flush=True)
        return 0
    st = {}
    fn = create_kitti_infos_host if a.host else create_kitti_infos
    kw = dict(workers=a.workers, verbose=a.verbose, stats=st)
    if not a.host:
        kw.update(batch=a.batch, readers=a.readers, und_cap=a.und_cap, pass_boxes=a.pass_boxes)
    fn(cfg, ["Car", "Pedestrian", "Cyclist"], root, root, if_val=if_val, **kw)
    out = {"tool": "kitti_infos", "host": bool(a.host), "scans": st.get("scans"), "boxes": st.get("boxes"),
           "db_points": st.get("db_points"), "host_boxes": st.get("host_boxes")}
    for k in ("undecided_points", "overflow_boxes"):
        if k in st:
            out[k] = st[k]
    for k in ("wall_s", "read_s", "host_s", "h2d_s", "gpu_s", "hull_host_s", "write_s", "pickle_s", "infos_s", "db_s"):
        if k in st:
            out[k] = round(st[k], 4)
    if st.get("wall_s"):
        out["scans_per_s"] = round(st["scans"] / st["wall_s"], 1)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
