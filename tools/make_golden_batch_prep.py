"""Golden training samples for modest_amd.utils.batch_prep (BUILD CONTAINER ONLY -- needs /root/reference).

A child process imports the reference's own DataBaseSampler, DataAugmentor and DataProcessor from where they lie (empty package
modules that keep their __path__, pcdet_bind.install(stand_ins=False), an empty stand-in for skimage) and runs them on the CPU on
seeded scenes, one sample at a time, with two substitutions -- the CPU statements the device code is pinned to:
  boxes_bev_iou_cpu's compiled half      the C twin of oracle/ (glibc cosf / sinf, atan2 as the double function)
  points_in_boxes_cpu's compiled half    kitti_infos.points_in_boxes_host
It writes tests/golden/batch_prep.npz: per scene the config (JSON), the seed, the raw sample, the database (boxes, names, point
counts, difficulties, points), and what the three classes returned (points, gt_boxes with the class index).

The tool asserts what makes the reference alone unambiguous on these inputs (it rotates with torch.matmul, whose roundings depend
on the shape): every returned point lies farther than ten times the float32 rotation bound from the four x / y faces and, with
sample_points, from the 40 m sphere; every corner of a returned box lies farther than that from the six faces; every pair of boxes the
sampler compares (a candidate with a gt, with a candidate of its own or of an earlier group) either overlaps by more than ten times the
BEV overlap bound of tests/iou3d_cases.py or is disjoint with no corner within 0.02 m of the other box (a gap wider than that bound and
than the 0.01 m margin of the reference's containment test).  A scene that misses is drawn again from another seed; at most a quarter of
all draws may be dropped that way, which is asserted at the end and recorded in the fixture.

Usage:  python tools/make_golden_batch_prep.py
"""
import json
import os
import pickle
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = "/root/reference/downstream/OpenPCDet"
GOLD = os.path.join(ROOT, "tests", "golden", "batch_prep.npz")

_CHILD = r"""
import os, pickle, sys, types
import numpy as np
import torch
ref, root, job = sys.argv[1], sys.argv[2], pickle.load(open(sys.argv[3], "rb"))
sys.path.insert(0, root)
for name in ("pcdet", "pcdet.datasets", "pcdet.datasets.augmentor", "pcdet.datasets.processor", "pcdet.utils", "pcdet.ops",
             "pcdet.ops.iou3d_nms", "pcdet.ops.roiaware_pool3d"):
    m = types.ModuleType(name)
    m.__path__ = [os.path.join(ref, *name.split("."))]
    sys.modules[name] = m
sk = types.ModuleType("skimage")
sk.transform = types.ModuleType("skimage.transform")
sys.modules["skimage"], sys.modules["skimage.transform"] = sk, sk.transform
from modest_amd.utils import pcdet_bind
pcdet_bind.install(stand_ins=False)
from modest_amd import kitti_infos
from modest_amd.kitti_infos import AttrDict
from oracle import labels as ol
from pcdet.ops.iou3d_nms import iou3d_nms_utils
from pcdet.ops.roiaware_pool3d import roiaware_pool3d_utils
from pcdet.datasets.augmentor.data_augmentor import DataAugmentor
from pcdet.datasets.processor.data_processor import DataProcessor
from pcdet.utils import calibration_kitti, common_utils
for mod in (iou3d_nms_utils, roiaware_pool3d_utils, sys.modules[DataAugmentor.__module__], sys.modules[DataProcessor.__module__]):
    assert mod.__file__.startswith(ref), mod.__file__

def boxes_iou_bev_cpu(a, b, out):
    out.copy_(torch.from_numpy(ol.boxes_iou_bev(a.numpy(), b.numpy(), arith="atan2_f64")))
def points_in_boxes_cpu(boxes, pts, out):
    out.copy_(torch.from_numpy(kitti_infos.points_in_boxes_host(pts.numpy(), boxes.numpy())))
iou3d_nms_utils.iou3d_nms_cuda = types.SimpleNamespace(boxes_iou_bev_cpu=boxes_iou_bev_cpu)
roiaware_pool3d_utils.roiaware_pool3d_cuda = types.SimpleNamespace(points_in_boxes_cpu=points_in_boxes_cpu)

def attr(v):
    if isinstance(v, dict):
        return AttrDict({k: attr(x) for k, x in v.items()})
    if isinstance(v, list):
        return [attr(x) for x in v]
    return v

from pcdet.datasets.augmentor import database_sampler as dsm
LOG = []
_sample = dsm.DataBaseSampler.sample_with_fixed_number
def logged(self, class_name, sample_group):
    got = _sample(self, class_name, sample_group)
    LOG.append(np.stack([x["box3d_lidar"] for x in got], axis=0).astype(np.float32).reshape(-1, 7))
    return got
dsm.DataBaseSampler.sample_with_fixed_number = logged

from pathlib import Path
out = []
for scene in job:
    cfg, names = attr(scene["cfg"]), scene["class_names"]
    rng = np.array(cfg.POINT_CLOUD_RANGE, dtype=np.float32)
    aug = DataAugmentor(Path(scene["root"]), cfg.DATA_AUGMENTOR, names, logger=None)
    proc = DataProcessor(cfg.DATA_PROCESSOR, point_cloud_range=rng, training=True)
    res = []
    np.random.seed(scene["seed"])
    for s in scene["samples"]:
        calib = calibration_kitti.Calibration({"P2": np.eye(3, 4, dtype=np.float32), "R0": s["R0"], "Tr_velo2cam": s["V2C"]})
        d = {"points": s["points"].copy(), "gt_boxes": s["gt_boxes"].copy(), "gt_names": s["gt_names"].copy(),
             "road_plane": s["road_plane"].copy(), "calib": calib,
             "gt_boxes_mask": np.array([n in names for n in s["gt_names"]], dtype=np.bool_)}
        del LOG[:]
        d = aug.forward(data_dict=d)
        cand = np.concatenate(LOG, axis=0) if LOG else np.zeros((0, 7), np.float32)
        groups = np.concatenate([np.full(len(x), k) for k, x in enumerate(LOG)]) if LOG else np.zeros(0, np.int64)
        sel = common_utils.keep_arrays_by_name(d["gt_names"], names)
        d["gt_boxes"], d["gt_names"] = d["gt_boxes"][sel], d["gt_names"][sel]
        cls = np.array([names.index(n) + 1 for n in d["gt_names"]], dtype=np.int32)
        d["gt_boxes"] = np.concatenate((d["gt_boxes"], cls.reshape(-1, 1).astype(np.float32)), axis=1)
        d["use_lead_xyz"] = True
        d = proc.forward(data_dict=d)
        assert d["points"].dtype == np.float32 and d["gt_boxes"].dtype == np.float32
        res.append({"points": d["points"], "gt_boxes": d["gt_boxes"], "cand_boxes": cand, "cand_groups": groups.astype(np.int64)})
    out.append(res)
pickle.dump(out, open(sys.argv[4], "wb"))
"""


def margins_ok(cfg, rec):
    """the tool's assertions on one recorded sample (the module docstring)"""
    r = np.asarray(cfg["POINT_CLOUD_RANGE"], np.float64)
    p = rec["points"].astype(np.float64)
    rad = np.hypot(p[:, 0], p[:, 1])
    bound = 2.0 ** -24 * (3 * np.sqrt(2) * rad + np.abs(p[:, :2]).max(axis=1))
    face = np.minimum.reduce([p[:, 0] - r[0], r[3] - p[:, 0], p[:, 1] - r[1], r[4] - p[:, 1]])
    ok = bool((face > 10 * bound).all())
    if any(c["NAME"] == "sample_points" for c in cfg["DATA_PROCESSOR"]):
        ok = ok and bool((np.abs(np.sqrt((p[:, :3] ** 2).sum(1)) - 40.0) > 10 * 2 * bound).all())
    b = rec["gt_boxes"][:, :7].astype(np.float64)
    for q in range(8):
        lx, ly, lz = b[:, 3] * (-.5 if q & 1 else .5), b[:, 4] * (-.5 if q & 2 else .5), b[:, 5] * (-.5 if q & 4 else .5)
        cx = lx * np.cos(b[:, 6]) - ly * np.sin(b[:, 6]) + b[:, 0]
        cy = lx * np.sin(b[:, 6]) + ly * np.cos(b[:, 6]) + b[:, 1]
        cz = lz + b[:, 2]
        d = np.minimum.reduce([np.abs(cx - r[0]), np.abs(cx - r[3]), np.abs(cy - r[1]), np.abs(cy - r[4]), np.abs(cz - r[2]), np.abs(cz - r[5])])
        ok = ok and bool((d > 10 * 2.0 ** -24 * 8 * (np.abs(cx) + np.abs(cy) + np.abs(cz) + 1)).all())
    return ok


def pairs_ok(gt, cand, groups):
    """the tool's assertion on the box pairs the sampler compares in one sample (the module docstring)"""
    import iou3d_cases as ic
    gt, cand = np.asarray(gt, np.float32).reshape(-1, 7), np.asarray(cand, np.float32).reshape(-1, 7)
    if len(cand) == 0:
        return True
    others = np.concatenate([gt, cand], axis=0)
    e = ic.Exact.all_pairs(cand, others, margin=0.02)
    groups = np.asarray(groups)
    seen = np.ones((len(cand), len(others)), bool)
    seen[:, len(gt):] = groups[None, :] <= groups[:, None]
    seen[np.arange(len(cand)), len(gt) + np.arange(len(cand))] = False
    fine = (e.overlap > 10 * e.overlap_bound) | ((e.overlap == 0) & e.well)
    return bool(fine[seen].all())


def scenes():
    """(name, config, B, seed, database, edit of the raw batch, NUM_POINTS as a multiple of sample 0's point count plus a rest)"""
    import batch_prep_cases as cases
    shuffle_only = cases.dataset_cfg("pillars")
    shuffle_only["DATA_PROCESSOR"] = shuffle_only["DATA_PROCESSOR"][:2]       # the voxels are VoxelizeOnDevice's business (section 7f)

    def on_the_gt(raw):
        raw["gt_boxes"][0] = np.array([[33, 0, -1, 4, 2, 1.5, 0], [-30, 40, -1, 4, 2, 1.5, 1.2]], np.float32)
        raw["gt_names"][0] = np.array(["Car", "Van"])

    def full_scene(raw):
        raw["gt_boxes"][0] = np.array([[33, 0, -1, 4, 2, 1.5, 0], [-30, 40, -1, 4, 2, 1.5, 1.2], [0, -50, -1, 0.8, 0.8, 1.7, 0.4],
                                       [50, 20, -1, 1.8, 0.8, 1.7, 2.0]], np.float32)
        raw["gt_names"][0] = np.array(["Car", "Car", "Pedestrian", "Cyclist"])

    few = ("Car:2", "Pedestrian:1", "Cyclist:1")
    return [("lyft order B=1", cases.dataset_cfg("pointrcnn"), 1, 31, "db", None, None),
            ("lyft order B=3", cases.dataset_cfg("pointrcnn"), 3, 32, "db", None, None),
            ("shuffle only", shuffle_only, 2, 33, "db", None, None),
            ("limit whole scene, narrow scale, flips y x", cases.dataset_cfg("pointrcnn", True, (1.0, 1.0005), ("y", "x")), 2, 34, "db", None, None),
            ("no road plane", cases.dataset_cfg("pointrcnn", road_plane=False), 2, 35, "db", None, None),
            ("NUM_POINTS between the far points and the count", cases.dataset_cfg("pointrcnn", num_points=400), 2, 36, "db", None, None),
            ("more far points than NUM_POINTS", cases.dataset_cfg("pointrcnn", num_points=256), 2, 37, "db", None, None),
            ("two class groups: a candidate on a kept and one on a dropped candidate of the first; a sample without gts",
             cases.dataset_cfg("pointrcnn", sample_groups=("Car:2", "Pedestrian:2", "Cyclist:1")), 2, 38, "dbc", on_the_gt, None),
            ("LIMIT_WHOLE_SCENE leaves nothing to sample", cases.dataset_cfg("pointrcnn", True, sample_groups=few), 2, 39, "db", full_scene, None),
            ("NUM_POINTS equal to the point count", cases.dataset_cfg("pointrcnn"), 1, 40, "db", None, (1, 0)),
            ("NUM_POINTS above twice the point count", cases.dataset_cfg("pointrcnn"), 1, 41, "db", None, (2, 37)),
            ("shuffle_points ahead of sample_points", cases.dataset_cfg("shuffle first", num_points=400), 2, 42, "db", None, None)]


def set_num_points(cfg, n):
    for c in cfg["DATA_PROCESSOR"]:
        if c["NAME"] == "sample_points":
            c["NUM_POINTS"] = {"train": int(n), "test": int(n)}


def run_reference(tmp, root, cfg, seed, samples):
    import batch_prep_cases as cases
    one = [{"cfg": cfg, "class_names": cases.CLASS_NAMES, "root": root, "seed": seed, "samples": samples}]
    pickle.dump(one, open(os.path.join(tmp, "job.pkl"), "wb"))
    open(os.path.join(tmp, "child.py"), "w").write(_CHILD)
    subprocess.run([sys.executable, os.path.join(tmp, "child.py"), REF, ROOT, os.path.join(tmp, "job.pkl"), os.path.join(tmp, "out.pkl")],
                   check=True)
    return pickle.load(open(os.path.join(tmp, "out.pkl"), "rb"))[0]


def save_database(out, prefix, root, infos):
    names, rows = [], []
    for c, lst in infos.items():
        for i in lst:
            names.append(c)
            rows.append(np.fromfile(os.path.join(root, i["path"]), np.float32).reshape(-1, 4))
    out[prefix + "_names"] = np.array(names)
    out[prefix + "_boxes"] = np.stack([i["box3d_lidar"] for lst in infos.values() for i in lst]).astype(np.float32)
    out[prefix + "_difficulty"] = np.array([i["difficulty"] for lst in infos.values() for i in lst], np.int64)
    out[prefix + "_counts"] = np.array([len(r) for r in rows], np.int64)
    out[prefix + "_points"] = np.concatenate(rows, axis=0)


def main():
    import batch_prep_cases as cases
    assert os.path.isdir(REF), "the recording needs the reference tree"
    out, meta, total, rejected = {}, [], 0, 0
    with tempfile.TemporaryDirectory() as tmp:
        roots = {"db": os.path.join(tmp, "db"), "dbc": os.path.join(tmp, "dbc")}
        save_database(out, "db", roots["db"], cases.write_database(roots["db"]))
        save_database(out, "dbc", roots["dbc"], cases.write_database(roots["dbc"], given=cases.COLLIDING))
        for name, cfg, B, seed, db, edit, num in scenes():
            for attempt in range(4):
                total += 1
                raw = cases.raw_batch(B=B, n=420, seed=seed + 100 * attempt)
                if edit is not None:
                    edit(raw)
                samples = [{k: raw[k][b] for k in ("points", "gt_boxes", "gt_names", "road_plane", "V2C", "R0")} for b in range(B)]
                if num is not None:          # the point count does not depend on the stage-2 draws: a run that keeps all points tells it
                    set_num_points(cfg, -1)
                    count = len(run_reference(tmp, roots[db], cfg, seed, samples)[0]["points"])
                    set_num_points(cfg, num[0] * count + num[1])
                res = run_reference(tmp, roots[db], cfg, seed, samples)
                if all(margins_ok(cfg, r) and pairs_ok(s["gt_boxes"], r["cand_boxes"], r["cand_groups"]) for r, s in zip(res, samples)):
                    break
                rejected += 1
            else:
                raise AssertionError(f"{name}: no seed in four leaves the reference unambiguous")
            k = len(meta)
            meta.append({"name": name, "cfg": cfg, "seed": seed, "B": B, "db": db})
            for b in range(B):
                for key in ("points", "gt_boxes", "road_plane", "V2C", "R0"):
                    out[f"s{k}_{b}_{key}"] = samples[b][key]
                out[f"s{k}_{b}_gt_names"] = np.array([str(x) for x in samples[b]["gt_names"]])
                out[f"s{k}_{b}_out_points"] = res[b]["points"]
                out[f"s{k}_{b}_out_gt_boxes"] = res[b]["gt_boxes"]
                out[f"s{k}_{b}_cand_boxes"] = res[b]["cand_boxes"]
                out[f"s{k}_{b}_cand_groups"] = res[b]["cand_groups"]
    assert rejected * 4 <= total, (rejected, total)          # at most a quarter of the draws dropped
    out["meta"] = np.array(json.dumps({"scenes": meta, "class_names": cases.CLASS_NAMES, "draws": {"total": total, "rejected": rejected}}))
    np.savez_compressed(GOLD, **out)
    print(GOLD, os.path.getsize(GOLD), "bytes,", len(meta), "scenes,", rejected, "of", total, "draws dropped")


if __name__ == "__main__":
    main()
