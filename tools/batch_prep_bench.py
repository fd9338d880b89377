"""Training-batch preparation: the device path (modest_amd.utils.batch_prep.BatchPrepOnDevice) next to the host path a user of
this stack has today, in one run on the GPU machine.

Per batch of B Lyft-shaped scans (120 000 FOV points, 30 gts, up to 40 candidates, PointRCNN's processors at 16 384 points):
  device   wall time of BatchPrepOnDevice per batch (host plan, the raw scans' host-to-device copy, stage 1 with the batch's one
           synchronise, the stage-2 draws, the gather, a final synchronise), the copy and the draws also on their own;
           synchronising calls: what PyTorch's sync debug mode reports around one warm batch, next to the library's one blocking
           call; launches and copies are read from the code, not counted
  host     the reference-shaped numpy steps of ONE sample, single process: the sampler's two IoU matrices through this repository's
           boxes_bev_iou_cpu, np.fromfile per kept object from a tmpfs tree, points_in_boxes_cpu's dense (boxes, points) mask,
           flip / rotation (torch.matmul) / scaling, the range masks, sample_points, shuffle_points
The bar: a device batch costs less than one sample of the host path (a DataLoader with >= B workers hides the other samples).
Prints one JSON line.  Nothing here reads the reference tree."""
import argparse
import json
import os
import pickle
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from modest_amd.utils import batch_prep as bp  # noqa: E402
from modest_amd.utils.iou3d_nms import iou3d_nms_utils  # noqa: E402
from modest_amd.utils import roiaware_pool3d_utils  # noqa: E402

CLASS_NAMES = ["car", "pedestrian", "cyclist"]
RANGE = [-80.0, -80.0, -5.0, 80.0, 80.0, 3.0]
F32 = np.float32


def write_database(root, rng, per_class=400):
    os.makedirs(os.path.join(root, "gt_database"), exist_ok=True)
    infos = {}
    for name in CLASS_NAMES:
        infos[name] = []
        for i in range(per_class):
            k = int(rng.integers(20, 400))
            pts = np.c_[rng.uniform(-1, 1, (k, 3)) * np.array([2.0, 0.9, 0.8]), rng.uniform(0, 1, (k, 1))].astype(F32)
            path = f"gt_database/{name}_{i}.bin"
            pts.tofile(os.path.join(root, path))
            box = np.array([rng.uniform(-70, 70), rng.uniform(-70, 70), rng.uniform(-1.5, -0.5), rng.uniform(3.5, 5), rng.uniform(1.6, 2.1),
                            rng.uniform(1.4, 1.9), rng.uniform(-3.14, 3.14)], F32)
            infos[name].append({"name": name, "path": path, "box3d_lidar": box, "num_points_in_gt": k, "difficulty": 0})
    with open(os.path.join(root, "dbinfos.pkl"), "wb") as f:
        pickle.dump(infos, f)


def config(num_points):
    sampler = {"NAME": "gt_sampling", "USE_ROAD_PLANE": True, "DB_INFO_PATH": ["dbinfos.pkl"],
               "PREPARE": {"filter_by_min_points": [f"{c}:5" for c in CLASS_NAMES]}, "SAMPLE_GROUPS": ["car:20", "pedestrian:10", "cyclist:10"],
               "NUM_POINT_FEATURES": 4, "REMOVE_EXTRA_WIDTH": [0.0, 0.0, 0.0], "LIMIT_WHOLE_SCENE": True}
    aug = [sampler, {"NAME": "random_world_flip", "ALONG_AXIS_LIST": ["x"]},
           {"NAME": "random_world_rotation", "WORLD_ROT_ANGLE": [-0.78539816, 0.78539816]},
           {"NAME": "random_world_scaling", "WORLD_SCALE_RANGE": [0.95, 1.05]}]
    proc = [{"NAME": "mask_points_and_boxes_outside_range", "REMOVE_OUTSIDE_BOXES": True},
            {"NAME": "sample_points", "NUM_POINTS": {"train": num_points, "test": num_points}},
            {"NAME": "shuffle_points", "SHUFFLE_ENABLED": {"train": True, "test": False}}]
    return {"POINT_CLOUD_RANGE": RANGE, "DATA_AUGMENTOR": {"DISABLE_AUG_LIST": [], "AUG_CONFIG_LIST": aug},
            "POINT_FEATURE_ENCODING": {"encoding_type": "absolute_coordinates_encoding", "used_feature_list": ["x", "y", "z", "intensity"]},
            "DATA_PROCESSOR": proc}


def raw_batch(rng, B, n, n_gt):
    V2C = np.array([[7.5e-3, -0.99997, -6.2e-4, -4.1e-3], [1.48e-2, 7.3e-4, -0.99989, -7.6e-2], [0.99986, 7.5e-3, 1.48e-2, -0.272]], F32)
    R0 = np.eye(3, dtype=F32)
    out = {"points": [], "gt_boxes": [], "gt_classes": [], "gt_names": [], "road_plane": [], "V2C": [V2C] * B, "R0": [R0] * B, "batch_size": B,
           "frame_id": np.arange(B), "raw_batch": True}
    for _ in range(B):
        out["points"].append(np.c_[rng.uniform(-85, 85, (n, 2)), rng.uniform(-3, 1, n), rng.uniform(0, 1, n)].astype(F32))
        out["gt_boxes"].append(np.c_[rng.uniform(-70, 70, (n_gt, 2)), rng.uniform(-1.5, -0.5, n_gt), rng.uniform(3.5, 5, n_gt),
                                     rng.uniform(1.6, 2.1, n_gt), rng.uniform(1.4, 1.9, n_gt), rng.uniform(-3.14, 3.14, n_gt)].astype(F32))
        cls = rng.integers(1, 4, n_gt)
        out["gt_classes"].append(cls.astype(np.int64))
        out["gt_names"].append(np.array(CLASS_NAMES)[cls - 1])
        out["road_plane"].append(np.array([0.0, -1.0, 0.0, 1.65]))
    return out


def host_sample(prep, raw, b, root, num_points):
    """one sample the way the reference's host code prepares it, with this repository's drop-ins for its two compiled calls"""
    r = {k: raw[k][b] for k in ("points", "gt_boxes", "gt_classes", "gt_names", "road_plane", "V2C", "R0")}
    s = prep.plan_sample(r, np.random)                       # the sampler's draws and the road plane: host work on either path
    points, gt = r["points"].copy(), r["gt_boxes"].copy()
    existed, kept = gt, []
    for g in np.unique(s["cand_groups"]):
        idx = np.nonzero(s["cand_groups"] == g)[0]
        sampled = s["cand_boxes"][idx]
        iou1 = iou3d_nms_utils.boxes_bev_iou_cpu(sampled, existed)
        iou2 = iou3d_nms_utils.boxes_bev_iou_cpu(sampled, sampled)
        iou2[range(len(idx)), range(len(idx))] = 0
        ok = ((iou1.max(axis=1) + iou2.max(axis=1)) == 0).nonzero()[0]
        existed = np.concatenate((existed, sampled[ok]), axis=0)
        kept.extend(idx[ok].tolist())
    db = prep.database
    infos = [i for c in db.class_names for i in db.db_infos[c]]
    objs = []
    for j in kept:
        op = np.fromfile(os.path.join(root, infos[int(s["cand_objects"][j])]["path"]), dtype=F32).reshape(-1, 4)
        op[:, :3] += s["cand_boxes"][j, :3]
        op[:, 2] -= s["mv_height"][j]
        objs.append(op)
    boxes = s["cand_boxes"][kept].copy()
    boxes[:, 2] = s["cand_z"][kept]
    if len(kept):
        mask = roiaware_pool3d_utils.points_in_boxes_cpu(points[:, :3], boxes)
        points = np.concatenate(objs + [points[mask.sum(axis=0) == 0]], axis=0)
    gt = np.concatenate([gt, boxes], axis=0)
    if s.get("flip_x"):
        gt[:, 1], gt[:, 6], points[:, 1] = -gt[:, 1], -gt[:, 6], -points[:, 1]
    rot = torch.tensor([[s["cos"], s["sin"], 0], [-s["sin"], s["cos"], 0], [0, 0, 1]], dtype=torch.float32)
    points[:, :3] = torch.matmul(torch.from_numpy(points[:, :3]), rot).numpy()
    gt[:, :3] = torch.matmul(torch.from_numpy(gt[:, :3]), rot).numpy()
    gt[:, 6] += s["angle"]
    points[:, :3] *= s["scale"]
    gt[:, :6] *= s["scale"]
    m = (points[:, 0] >= RANGE[0]) & (points[:, 0] <= RANGE[3]) & (points[:, 1] >= RANGE[1]) & (points[:, 1] <= RANGE[4])
    points = points[m]
    near = np.linalg.norm(points[:, :3], axis=1) < 40.0
    far_idx, near_idx = np.where(~near)[0], np.where(near)[0]
    if num_points < len(points):
        if num_points > len(far_idx):
            choice = np.concatenate((np.random.choice(near_idx, num_points - len(far_idx), replace=False), far_idx))
        else:
            choice = np.random.choice(len(points), num_points, replace=False)
        np.random.shuffle(choice)
        points = points[choice]
    points = points[np.random.permutation(len(points))]
    return points, gt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--points", type=int, default=120_000)
    ap.add_argument("--gts", type=int, default=30)
    ap.add_argument("--num-points", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the measurement needs the GPU: there is no CPU fallback"
    rng = np.random.default_rng(0)
    tmp = "/dev/shm" if os.path.isdir("/dev/shm") else None
    with tempfile.TemporaryDirectory(dir=tmp) as root:
        write_database(root, rng)
        prep = bp.BatchPrepOnDevice(config(a.num_points), CLASS_NAMES, root)
        raw = raw_batch(rng, a.batch, a.points, a.gts)
        np.random.seed(0)

        def device_batch():
            out = prep(dict(raw))
            torch.cuda.synchronize()
            return out

        for _ in range(a.warmup):
            out = device_batch()
            host_sample(prep, raw, 0, root, a.num_points)
        t = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            out = device_batch()
            t.append(time.perf_counter() - t0)
        host = np.concatenate(raw["points"], axis=0)
        h2d, plan, draws = [], [], []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            torch.from_numpy(host).pin_memory().to(prep.device, non_blocking=True)
            torch.cuda.synchronize()
            h2d.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            for b in range(a.batch):
                prep.plan_sample({k: raw[k][b] for k in ("points", "gt_boxes", "gt_classes", "gt_names", "road_plane", "V2C", "R0")}, np.random)
            plan.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            from modest_amd import ops
            ops.batch_prep_order_draws(out["batch_prep_table"], a.num_points, True)
            draws.append(time.perf_counter() - t0)
        import warnings
        torch.cuda.synchronize()
        with warnings.catch_warnings(record=True) as seen:          # what PyTorch itself waits for in one warm batch
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            try:
                prep(dict(raw))
            finally:
                torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        torch_syncs = sum("called a synchronizing" in str(w.message) for w in seen)
        hs = []
        for k in range(a.steps):
            t0 = time.perf_counter()
            host_sample(prep, raw, k % a.batch, root, a.num_points)
            hs.append(time.perf_counter() - t0)
    ms = lambda v: round(1e3 * float(np.median(v)), 3)    # noqa: E731
    res = {"tool": "batch_prep_bench", "batch": a.batch, "points": a.points, "gts": a.gts, "num_points": a.num_points, "steps": a.steps,
           "device_batch_ms": ms(t), "device_batch_ms_min_max": [round(1e3 * min(t), 3), round(1e3 * max(t), 3)],
           "h2d_raw_scans_ms": ms(h2d), "host_plan_ms": ms(plan), "host_stage2_draws_ms": ms(draws),
           "synchronising_calls_reported_by_torch": torch_syncs, "blocking_library_calls_by_contract": 1,
           "launches_read_from_the_code": 5, "copies_read_from_the_code": 3,
           "host_path_one_sample_ms": ms(hs), "host_path_one_sample_ms_min_max": [round(1e3 * min(hs), 3), round(1e3 * max(hs), 3)],
           "table": np.asarray(out["batch_prep_table"]).tolist(),
           "device_batch_below_one_host_sample": bool(np.median(t) < np.median(hs))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
