"""Golden dataset infos + gt database for modest_amd.kitti_infos (BUILD CONTAINER ONLY -- needs /root/reference).

Runs the reference's own ``KittiDataset.get_infos`` / ``create_groundtruth_database`` / ``Calibration`` (imported from
where they lie, nothing copied) in a child process.  The child stubs what is not installed: ``skimage.io.imread`` (PIL),
the package ``__init__`` files (empty modules that keep their ``__path__``), ``pcdet.datasets.dataset.DatasetTemplate``
(the detector-side imports) and ``roiaware_pool3d_cuda``, which it builds from the reference's ``roiaware_pool3d.cpp`` plus
a file of three empty launcher bodies into a temporary directory (nothing compiled is kept).

Trees (modest_amd.synth.infos_*): ``dyn`` -- nine scans of class Dynamic, 0..12 boxes, one empty label file, overlapping
boxes, boxes across the image border and behind the camera, and in three boxes planted rows 1e-7..1e-4 m on both sides of
every face and at |local| = half extent + 0.01 +- a few float32 ulps, and in every box whose heading is one where the host
libm's cosf / sinf differ from the rounded double functions up to 40 rows on the margin whose membership depends on which
of the two is used; ``car`` -- three scans with Car / Pedestrian /
DontCare rows and scores.  Recorded: label / calib text, image sizes, generator seeds + planted rows + digests of the
scans, both infos lists, the counts with FOV_POINTS_ONLY off, the dbinfos, every database file's name, row count, member
row numbers and digest, the FOV flags, and the reference's in_hull flag of every (box, row).

Usage:  python tools/make_golden_infos.py        (writes tests/golden/kitti_infos.npz)
"""
import os
import pickle
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = "/root/reference/downstream/OpenPCDet"
GOLD = os.path.join(ROOT, "tests", "golden")

_LAUNCHERS = """
void roiaware_pool3d_launcher(int, int, int, int, int, int, int, const float *, const float *, const float *, int *, int *, float *, int) {}
void roiaware_pool3d_backward_launcher(int, int, int, int, int, int, const int *, const int *, const float *, float *, int) {}
void points_in_boxes_launcher(int, int, int, const float *, const float *, int *) {}
"""

_CHILD = r"""
import importlib.util, os, pickle, subprocess, sys, sysconfig, types
from pathlib import Path
import numpy as np
ref, work, job = sys.argv[1], sys.argv[2], pickle.load(open(sys.argv[3], "rb"))
import torch
from torch.utils import cpp_extension
so = os.path.join(work, "roiaware_pool3d_cuda.so")
open(os.path.join(work, "launchers.cpp"), "w").write(job["launchers"])
tlib = Path(torch.__file__).parent / "lib"
cmd = ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-w", "-DTORCH_EXTENSION_NAME=roiaware_pool3d_cuda",
       "-DTORCH_API_INCLUDE_EXTENSION_H", "-D_GLIBCXX_USE_CXX11_ABI=%d" % int(torch._C._GLIBCXX_USE_CXX11_ABI)]
cmd += ["-I" + p for p in cpp_extension.include_paths() + [sysconfig.get_paths()["include"]]]
cmd += [os.path.join(ref, "pcdet/ops/roiaware_pool3d/src/roiaware_pool3d.cpp"), os.path.join(work, "launchers.cpp"), "-o", so,
        "-L%s" % tlib, "-ltorch", "-ltorch_cpu", "-lc10", "-ltorch_python", "-Wl,-rpath,%s" % tlib]
subprocess.run(cmd, check=True)
spec = importlib.util.spec_from_file_location("roiaware_pool3d_cuda", so)
ext = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ext)
for name in ("pcdet", "pcdet.datasets", "pcdet.datasets.kitti", "pcdet.ops", "pcdet.ops.roiaware_pool3d", "pcdet.utils"):
    m = types.ModuleType(name)
    m.__path__ = [os.path.join(ref, *name.split("."))]
    sys.modules[name] = m
sys.modules["pcdet.ops.roiaware_pool3d.roiaware_pool3d_cuda"] = ext
sys.modules["pcdet.ops.roiaware_pool3d"].roiaware_pool3d_cuda = ext
sk, skio = types.ModuleType("skimage"), types.ModuleType("skimage.io")
def imread(f):
    from PIL import Image
    return np.array(Image.open(str(f)))
skio.imread = imread
sk.io = skio
sys.modules["skimage"], sys.modules["skimage.io"] = sk, skio
ds = types.ModuleType("pcdet.datasets.dataset")
class DatasetTemplate:
    def __init__(self, dataset_cfg=None, class_names=None, training=True, root_path=None, logger=None):
        self.dataset_cfg, self.class_names, self.training, self.root_path, self.logger = dataset_cfg, class_names, training, root_path, logger
    @property
    def mode(self):
        return "train" if self.training else "test"
ds.DatasetTemplate = DatasetTemplate
sys.modules["pcdet.datasets.dataset"] = ds
import pcdet.datasets.kitti.kitti_dataset as kd
from pcdet.utils import box_utils
kd.Path = Path   # the reference binds it in its __main__ block only (kitti_dataset.py:529)
class Cfg(dict):
    __getattr__ = dict.__getitem__
res = {}
for name, root in job["trees"].items():
    root = Path(root)
    r = res[name] = {}
    for fov in (True, False):
        cfg = Cfg(DATA_SPLIT={"train": "train", "test": "val"}, INFO_PATH={"train": [], "test": []}, FOV_POINTS_ONLY=fov)
        dset = kd.KittiDataset(dataset_cfg=cfg, class_names=["Car", "Pedestrian", "Cyclist"], root_path=root, training=False)
        if fov:
            kd.create_kitti_infos(cfg, ["Car", "Pedestrian", "Cyclist"], root, root, if_val=True)
            for f in ("kitti_infos_train.pkl", "kitti_infos_val.pkl", "kitti_dbinfos_train.pkl"):
                r[f] = pickle.load(open(root / f, "rb"))
            r["db"] = {f: np.fromfile(str(root / "gt_database" / f), dtype=np.float32).reshape(-1, 4)
                       for f in sorted(os.listdir(root / "gt_database"))}
            r["fov"], r["hull"], r["mask"] = {}, {}, {}
            for split in ("train", "val"):
                dset.set_split(split)
                for idx in dset.sample_id_list:
                    pts, calib = dset.get_lidar(idx), dset.get_calib(idx)
                    r["fov"][idx] = dset.get_fov_flag(calib.lidar_to_rect(pts[:, 0:3]), dset.get_image_shape(idx), calib)
                    info = [i for i in r["kitti_infos_%s.pkl" % split] if i["point_cloud"]["lidar_idx"] == idx][0]
                    gt = info["annos"]["gt_boxes_lidar"]
                    if gt.ndim == 2 and len(gt):
                        corners = box_utils.boxes_to_corners_3d(gt)
                        r["hull"][idx] = np.stack([box_utils.in_hull(pts[:, 0:3], corners[k]) for k in range(len(gt))])
                        r["mask"][idx] = kd.roiaware_pool3d_utils.points_in_boxes_cpu(torch.from_numpy(pts[:, 0:3]), torch.from_numpy(gt)).numpy()
        else:
            for split in ("train", "val"):
                dset.set_split(split)
                infos = dset.get_infos(num_workers=4, has_label=True, count_inside_pts=True)
                r["counts_nofov_" + split] = [i["annos"]["num_points_in_gt"] for i in infos]
pickle.dump(res, open(sys.argv[4], "wb"))
"""


def planted_rows(rs, box, n_face=10, ulps=3):
    """rows (float32) 1e-7..1e-4 m on both sides of every face of `box` (float64 x y z dx dy dz heading), and rows at
    |local x / y| = half extent + 0.01 nudged by -ulps..ulps float32 steps"""
    c, s = np.cos(box[6]), np.sin(box[6])
    half = box[3:6] / 2
    out = []

    def world(loc):
        return np.array([box[0] + loc[0] * c - loc[1] * s, box[1] + loc[0] * s + loc[1] * c, box[2] + loc[2]])

    for axis in range(3):
        for sign in (-1.0, 1.0):
            for d in np.logspace(-7, -4, n_face):
                for side in (-1.0, 1.0):
                    loc = (2 * rs.random_sample(3) - 1) * half * 0.8
                    loc[axis] = sign * (half[axis] + side * d)
                    out.append(world(loc))
    for axis in range(2):
        for sign in (-1.0, 1.0):
            for rep in range(3):
                loc = (2 * rs.random_sample(3) - 1) * half * 0.8
                loc[axis] = sign * (half[axis] + 0.01)
                w = world(loc).astype(np.float32)
                for k in range(-ulps, ulps + 1):
                    v = w.copy()
                    for _ in range(abs(k)):
                        v[0] = np.nextafter(v[0], np.float32(np.inf if k > 0 else -np.inf))
                    out.append(v.astype(np.float64))
    rows = np.concatenate([np.array(out), rs.random_sample((len(out), 1))], axis=1)
    return rows.astype(np.float32)


def libm_sensitive_rows(rs, box, want=40, tries=400_000):
    """rows on the database margin of `box` on which the predicate's answer depends on whether cosa / sina are the
    host libm's cosf / sinf or the rounded double cos / sin (they differ for about 1.3 % of the headings); empty when
    the two agree for this heading"""
    import math
    from modest_amd import kitti_infos as ki
    b = box.astype(np.float32)
    c1, s1 = (float(v[0]) for v in ki.host_cos_sin_f32(b[6:7]))
    c2, s2 = float(np.float32(math.cos(-float(b[6])))), float(np.float32(math.sin(-float(b[6]))))
    if (c1, s1) == (c2, s2):
        return np.zeros((0, 4), dtype=np.float32)
    c, s = np.cos(box[6]), np.sin(box[6])
    half = box[3:6] / 2
    loc = (2 * rs.random_sample((tries, 3)) - 1) * half * 0.9
    axis = np.arange(tries) % 2
    edge = np.where(rs.random_sample(tries) < 0.5, -1.0, 1.0) * (half[axis] + 0.01 + 4e-6 * (rs.random_sample(tries) - 0.5))
    loc[np.arange(tries), axis] = edge
    w = np.stack([box[0] + loc[:, 0] * c - loc[:, 1] * s, box[1] + loc[:, 0] * s + loc[:, 1] * c, box[2] + loc[:, 2]], axis=1).astype(np.float32)
    sx, sy = w[:, 0] - b[0], w[:, 1] - b[1]

    def member(ca, sa):
        ca, sa = np.float32(ca), np.float32(sa)
        lx, ly = sx * ca + sy * (-sa), sx * sa + sy * ca
        return (np.abs(lx).astype(np.float64) < np.float64(b[3]) / 2.0 + np.float64(ki.MARGIN)) & \
               (np.abs(ly).astype(np.float64) < np.float64(b[4]) / 2.0 + np.float64(ki.MARGIN))
    pick = np.nonzero(member(c1, s1) != member(c2, s2))[0][:want]
    rows = np.concatenate([w[pick], rs.random_sample((len(pick), 1)).astype(np.float32)], axis=1)
    return rows.astype(np.float32)


def build_trees(work):
    """writes the trees under work/<name>; returns {name: dict of recorded inputs}"""
    from modest_amd import kitti_infos as ki, synth
    rec = {}
    plan = {"dyn": dict(n=9, seed=11, names=("Dynamic",), val=("000002", "000007"), empty=4, plant=((0, 0), (3, 1), (5, 2))),
            "car": dict(n=3, seed=23, names=("Car", "Pedestrian", "Car", "Cyclist"), val=("000001",), empty=None, plant=())}
    for name, p in plan.items():
        root = os.path.join(work, name)
        rs = np.random.RandomState(p["seed"])
        r = rec[name] = dict(ids=[], labels=[], calibs=[], sizes=[], seeds=[], n_bg=[], extras=[], bin_sha=[])
        for k in range(p["n"]):
            idx = "%06d" % k
            nb = 0 if k == p["empty"] else (12 if k == 1 else 1 + int(rs.random_sample() * 12))
            label = synth.infos_label_text(rs, nb, p["names"], n_dontcare=2 if name == "car" else 0, with_score=(name == "car" and k == 2))
            calib = synth.infos_calib_text(k)
            seed, n_bg = p["seed"] * 1000 + k, 9000 + int(rs.random_sample() * 6000)
            base = synth.infos_points(seed, label, n_bg, (50, 2000))
            size = synth.INFOS_IMAGE_SIZES[k % 3]
            synth.write_infos_scan(root, idx, base, label, calib, size)
            extra = np.zeros((0, 4), dtype=np.float32)
            for (scan, box) in p["plant"]:
                if scan == k:
                    info, _ = ki.scene_info(os.path.join(root, "training"), idx)
                    extra = np.concatenate([extra, planted_rows(rs, info["annos"]["gt_boxes_lidar"][box])])
            if name == "dyn" and nb:   # every box whose heading tells cosf / sinf from the rounded double functions
                info, _ = ki.scene_info(os.path.join(root, "training"), idx)
                for box in info["annos"]["gt_boxes_lidar"]:
                    sens = libm_sensitive_rows(rs, box)
                    r["libm_rows"] = r.get("libm_rows", 0) + len(sens)
                    extra = np.concatenate([extra, sens])
            rows = np.ascontiguousarray(np.concatenate([base, extra]), dtype=np.float32)
            synth.write_infos_scan(root, idx, rows, label, calib, size)
            from tests.infos_tree import sha
            for key, v in (("ids", idx), ("labels", label), ("calibs", calib), ("sizes", size), ("seeds", seed), ("n_bg", n_bg),
                           ("extras", extra), ("bin_sha", sha(rows.tobytes()))):
                r[key].append(v)
        assert name != "dyn" or r.pop("libm_rows") >= 20, "no heading of the tree tells the libm's cosf from the rounded cos"
        r["val"] = list(p["val"])
        r["train"] = [i for i in r["ids"] if i not in p["val"]]
        synth.write_infos_splits(root, r["train"], r["val"])
    return rec


def main():
    from tests.infos_tree import sha, store
    out = {}
    with tempfile.TemporaryDirectory() as work:
        rec = build_trees(work)
        job = {"launchers": _LAUNCHERS, "trees": {n: os.path.join(work, n) for n in rec}}
        pickle.dump(job, open(os.path.join(work, "job.pkl"), "wb"))
        open(os.path.join(work, "child.py"), "w").write(_CHILD)
        subprocess.run([sys.executable, os.path.join(work, "child.py"), REF, work, os.path.join(work, "job.pkl"),
                        os.path.join(work, "res.pkl")], check=True, stdout=subprocess.DEVNULL)
        res = pickle.load(open(os.path.join(work, "res.pkl"), "rb"))
    for name, r in rec.items():
        g = res[name]
        for key in ("ids", "labels", "calibs", "train", "val", "bin_sha"):
            out["%s/%s" % (name, key)] = np.array(r[key])
        out[name + "/sizes"] = np.array(r["sizes"], dtype=np.int32)
        out[name + "/seeds"] = np.array(r["seeds"], dtype=np.int64)
        out[name + "/n_bg"] = np.array(r["n_bg"], dtype=np.int64)
        out[name + "/extras"] = np.concatenate(r["extras"])
        out[name + "/extra_offsets"] = np.concatenate([[0], np.cumsum([len(e) for e in r["extras"]])]).astype(np.int64)
        store(out, name + "/infos_train", g["kitti_infos_train.pkl"])
        store(out, name + "/infos_val", g["kitti_infos_val.pkl"])
        store(out, name + "/dbinfos", g["kitti_dbinfos_train.pkl"])
        for split in ("train", "val"):
            store(out, "%s/counts_nofov_%s" % (name, split), g["counts_nofov_" + split])
        names = sorted(g["db"])
        out[name + "/db_names"] = np.array(names)
        out[name + "/db_counts"] = np.array([len(g["db"][f]) for f in names], dtype=np.int64)
        out[name + "/db_sha"] = np.array([sha(np.ascontiguousarray(g["db"][f]).tobytes()) for f in names])
        for idx in r["ids"]:
            out["%s/fov/%s" % (name, idx)] = np.packbits(g["fov"][idx])
            if idx in g["hull"]:
                out["%s/hull/%s" % (name, idx)] = np.packbits(g["hull"][idx], axis=1)
                out["%s/mask/%s" % (name, idx)] = np.packbits(g["mask"][idx] > 0, axis=1)
        print(name, "scans", len(r["ids"]), "db files", len(names), "db rows", int(out[name + "/db_counts"].sum()),
              "planted rows", len(out[name + "/extras"]))
    path = os.path.join(GOLD, "kitti_infos.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
