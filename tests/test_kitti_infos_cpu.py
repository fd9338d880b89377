"""CPU: the host mirror of modest_amd.kitti_infos against tests/golden/kitti_infos.npz, which tools/make_golden_infos.py
made with the reference's own KittiDataset.get_infos / create_groundtruth_database / Calibration and its compiled
points_in_boxes_cpu.  Infos and dbinfos must be equal after load (keys in order, dtypes, shapes, values bit for bit),
database files byte for byte with the same names."""
import json
import os
import pickle
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from modest_amd import kitti_infos as ki
from tests.infos_tree import TREES, assert_same, check_outputs, expected, golden, tree_scans, write_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g():
    return golden()


@pytest.mark.parametrize("name", TREES)
def test_host_mirror_reproduces_reference_files(g, tmp_path, name):
    write_tree(g, name, tmp_path)
    st = {}
    ki.create_kitti_infos_host(ki.AttrDict(FOV_POINTS_ONLY=True), ["Car", "Pedestrian", "Cyclist"], tmp_path, tmp_path,
                               if_val=True, stats=st)
    check_outputs(g, name, tmp_path)
    assert st["db_points"] == int(g[name + "/db_counts"].sum())


@pytest.mark.parametrize("name", TREES)
def test_host_mirror_counts_without_fov(g, tmp_path, name):
    write_tree(g, name, tmp_path)
    tr, va, _ = expected(g, name, fov=False)
    assert_same(ki.get_infos_host(tmp_path, "train", fov_points_only=False), tr)
    assert_same(ki.get_infos_host(tmp_path, "val", fov_points_only=False, exact_hull=True), va)


def test_cli_host_writes_the_reference_files(g, tmp_path):
    write_tree(g, "car", tmp_path)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("DATASET: 'KittiDataset'\nDATA_PATH: '%s'\nFOV_POINTS_ONLY: True\n" % tmp_path)
    cmd = [sys.executable, "-m", "modest_amd.kitti_infos", "create_kitti_infos", str(cfg), str(tmp_path), "True", "--host"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["tool"] == "kitti_infos" and out["host"] and out["scans"] == 3 and out["db_points"] == int(g["car/db_counts"].sum())
    assert "sample_idx" not in r.stderr
    check_outputs(g, "car", tmp_path)
    # a second run leaves an existing tree alone unless told otherwise; without argv[4] no val infos (the reference's default)
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert json.loads(r.stdout.strip().splitlines()[-1]).get("skipped") is True
    assert "NOTHING WAS WRITTEN" in r.stderr and "--overwrite" in r.stderr
    os.remove(tmp_path / "kitti_infos_val.pkl")
    r = subprocess.run(cmd[:5] + ["--host", "--overwrite", "--verbose"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not (tmp_path / "kitti_infos_val.pkl").exists()
    assert "train sample_idx: 000000" in r.stderr and "gt_database sample: 1/2" in r.stderr and "Database Car:" in r.stderr
    check_outputs(g, "car", tmp_path, val=False)


def test_fov_flags_and_database_mask_equal_the_reference(g):
    for name in TREES:
        for k, (idx, rows, label, calib_text, size) in enumerate(tree_scans(g, name)):
            with tempfile.TemporaryDirectory() as d:
                open(os.path.join(d, "c.txt"), "w").write(calib_text)
                calib = ki.Calibration(os.path.join(d, "c.txt"))
            fov = ki.get_fov_flag(rows, calib, np.array((size[1], size[0]), dtype=np.int32))
            assert np.array_equal(np.packbits(fov), g["%s/fov/%s" % (name, idx)]), (name, idx)
            assert 0 < fov.sum() < len(fov)
            if "%s/mask/%s" % (name, idx) not in g.files:
                continue
            infos = expected(g, name)[0] + expected(g, name)[1]
            info = [i for i in infos if i["point_cloud"]["lidar_idx"] == idx][0]
            mask = ki.points_in_boxes_host(rows[:, :3], info["annos"]["gt_boxes_lidar"])
            assert mask.dtype == np.int32
            assert np.array_equal(np.packbits(mask > 0, axis=1), g["%s/mask/%s" % (name, idx)]), (name, idx)


def test_label_parsing_levels_index_and_dontcare(tmp_path):
    sd = tmp_path / "training"
    for d in ("label_2", "calib", "image_2", "velodyne"):
        (sd / d).mkdir(parents=True)
    from PIL import Image
    from modest_amd import synth
    text = ("Car 0.00 0 -1.50 100.00 100.00 150.00 140.00 1.50 1.60 3.90 1.00 1.50 20.00 0.10\n"      # height 41: easy
            "Pedestrian 0.20 1 0.30 10.00 10.00 20.00 35.00 1.70 0.60 0.80 -2.00 1.40 12.00 -1.00 0.8750\n"   # 26: moderate
            "Cyclist 0.40 2 0.30 10.00 10.00 20.00 35.00 1.70 0.60 1.80 3.00 1.40 30.00 2.00\n"       # hard
            "Car 0.60 0 0.30 10.00 10.00 20.00 60.00 1.50 1.60 3.90 4.00 1.50 40.00 0.00\n"           # truncated: unknown
            "DontCare -1 -1 -10 5.00 6.00 7.00 8.00 -1 -1 -1 -1000 -1000 -1000 -10\n")
    for idx, label in (("000000", text), ("000001", "")):
        (sd / "label_2" / (idx + ".txt")).write_text(label)
        (sd / "calib" / (idx + ".txt")).write_text(synth.CALIB_TXT)
        Image.new("RGB", (97, 53)).save(sd / "image_2" / (idx + ".png"))
        synth.infos_points(3, label, 500).tofile(str(sd / "velodyne" / (idx + ".bin")))
    full, empty = ki.get_infos_host(tmp_path, "train", sample_id_list=["000000", "000001"])
    a = full["annos"]
    assert list(full.keys()) == ["point_cloud", "image", "calib", "annos"]
    assert full["image"]["image_shape"].dtype == np.int32 and full["image"]["image_shape"].tolist() == [53, 97]
    assert a["name"].tolist() == ["Car", "Pedestrian", "Cyclist", "Car", "DontCare"]
    assert a["difficulty"].tolist() == [0, 1, 2, -1, -1] and a["difficulty"].dtype == np.int32
    assert a["index"].tolist() == [0, 1, 2, 3, -1] and a["index"].dtype == np.int32
    assert a["score"].tolist() == [-1.0, 0.875, -1.0, -1.0, -1.0]
    assert a["bbox"].dtype == np.float32 and a["location"].dtype == np.float32 and a["dimensions"].dtype == np.float64
    assert a["dimensions"][0].tolist() == [3.9, 1.5, 1.6]   # l h w
    assert a["gt_boxes_lidar"].shape == (4, 7) and a["gt_boxes_lidar"].dtype == np.float64
    assert a["gt_boxes_lidar"][0, 6] == -(np.pi / 2 + 0.10)
    assert a["num_points_in_gt"].dtype == np.int32 and a["num_points_in_gt"][-1] == -1 and (a["num_points_in_gt"][:4] >= 0).all()
    e = empty["annos"]
    assert e["name"].shape == (0,) and e["bbox"].shape == (0, 4) and e["gt_boxes_lidar"].shape == (0,)
    assert e["num_points_in_gt"].shape == (0,) and e["num_points_in_gt"].dtype == np.int32 and e["index"].dtype == np.int32
    # the database step skips the empty scan and names files <idx>_<name>_<i>.bin
    pickle.dump([full, empty], open(tmp_path / "infos.pkl", "wb"))
    db, _ = ki.create_groundtruth_database_host(tmp_path, tmp_path / "infos.pkl", used_classes=["Car"], split="val")
    assert list(db.keys()) == ["Car"] and [d["gt_idx"] for d in db["Car"]] == [0, 3]
    assert sorted(os.listdir(tmp_path / "gt_database_val")) == ["000000_Car_0.bin", "000000_Car_3.bin", "000000_Cyclist_2.bin",
                                                                "000000_Pedestrian_1.bin"]
    assert db["Car"][0]["path"] == "gt_database_val/000000_Car_0.bin"


def test_image_shape_comes_from_the_header(tmp_path):
    from PIL import Image
    f = tmp_path / "a.png"
    Image.new("L", (640, 480)).save(f)
    data = f.read_bytes()
    f.write_bytes(data[:data.index(b"IDAT") + 4])   # everything up to the pixel data: a decode fails
    with pytest.raises(Exception):
        with Image.open(f) as im:
            im.load()
    assert ki.get_image_shape(f).tolist() == [480, 640]


def test_margin_band_holds_every_disagreement_with_the_reference_hull(g):
    """Pins tau to the reference: wherever the ideal float64 box and the reference's recorded in_hull flag disagree,
    the point lies inside the undecided band |margin| < tau, so the GPU's decided points are the reference's."""
    worst, near_face, disagreements = 0.0, 0, 0
    for name in TREES:
        infos = {i["point_cloud"]["lidar_idx"]: i for i in expected(g, name)[0] + expected(g, name)[1]}
        for idx, rows, *_ in tree_scans(g, name):
            key = "%s/hull/%s" % (name, idx)
            if key not in g.files:
                continue
            gt = infos[idx]["annos"]["gt_boxes_lidar"]
            hull = np.unpackbits(g[key], axis=1)[:, :len(rows)].astype(bool)
            corners = ki.boxes_to_corners_3d(gt)
            for k in range(len(gt)):
                m = ki.box_margin64(rows[:, :3], gt[k])
                tau = ki.hull_tau(corners[k])
                bad = (m > 0) != hull[k]
                disagreements += int(bad.sum())
                near_face += int((np.abs(m) < tau).sum())
                if bad.any():
                    worst = max(worst, float(np.abs(m[bad]).max()))
                assert (np.abs(m[bad]) < tau).all(), (name, idx, k, float(np.abs(m[bad]).max()), tau)
    print("disagreements %d, farthest %.3g m from the face, points inside the band %d" % (disagreements, worst, near_face))
    assert near_face > 100, "the planted points must exercise the band"
    assert disagreements > 0, "no planted row straddles the float32 hull: the band assertion above would be vacuous"


def test_cos_sin_are_the_host_libms_float_functions(g):
    """roiaware_pool3d.cpp:122 binds to cosf / sinf, which are not the rounded double functions; the fixture holds rows
    whose membership (recorded from the reference's compiled predicate) depends on the difference"""
    import ctypes
    import ctypes.util
    import math
    m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    m.cosf.restype = m.sinf.restype = ctypes.c_float
    m.cosf.argtypes = m.sinf.argtypes = [ctypes.c_float]
    a = (np.random.RandomState(0).random_sample(100_000) * 6.6 - 3.3).astype(np.float32)
    cosa, sina = ki.host_cos_sin_f32(a)
    assert cosa.dtype == np.float32 and sina.dtype == np.float32
    assert np.array_equal(cosa, np.array([m.cosf(-float(v)) for v in a], dtype=np.float32))
    assert np.array_equal(sina, np.array([m.sinf(-float(v)) for v in a], dtype=np.float32))
    # the fixture tells the two apart: with the rounded double functions the recorded mask is not reproduced
    infos = {i["point_cloud"]["lidar_idx"]: i for i in expected(g, "dyn")[0] + expected(g, "dyn")[1]}
    flipped = 0
    real = ki.host_cos_sin_f32
    try:
        ki.host_cos_sin_f32 = lambda rz: (np.array([math.cos(-float(v)) for v in np.ravel(rz)]).astype(np.float32),
                                          np.array([math.sin(-float(v)) for v in np.ravel(rz)]).astype(np.float32))
        for idx, rows, *_ in tree_scans(g, "dyn"):
            key = "dyn/mask/%s" % idx
            if key in g.files:
                mask = ki.points_in_boxes_host(rows[:, :3], infos[idx]["annos"]["gt_boxes_lidar"])
                flipped += int((np.unpackbits(g[key], axis=1)[:, :len(rows)] != (mask > 0)).sum())
    finally:
        ki.host_cos_sin_f32 = real
    assert flipped >= 20, flipped


def test_prefiltered_hull_equals_delaunay_on_all_points(g):
    """in_hull_near (what the mirror and the overflow path ask) == in_hull on the planted scans, FOV points only"""
    infos = {i["point_cloud"]["lidar_idx"]: i for i in expected(g, "dyn")[0] + expected(g, "dyn")[1]}
    checked = 0
    for idx, rows, label, calib_text, size in tree_scans(g, "dyn"):
        gt = infos[idx]["annos"]["gt_boxes_lidar"]
        if gt.ndim != 2 or not len(gt):
            continue
        with tempfile.TemporaryDirectory() as d:
            open(os.path.join(d, "c.txt"), "w").write(calib_text)
            calib = ki.Calibration(os.path.join(d, "c.txt"))
        pts = rows[ki.get_fov_flag(rows, calib, np.array((size[1], size[0]), dtype=np.int32))][:, :3]
        corners = ki.boxes_to_corners_3d(gt)
        for k in range(len(gt)):
            assert np.array_equal(ki.in_hull_near(pts, corners[k]), ki.in_hull(pts, corners[k])), (idx, k)
            checked += 1
    assert checked >= 30


def test_data_path_resolution_and_missing_tree(tmp_path, monkeypatch):
    """a relative data path is the reference's ROOT_DIR / 'tools' / path first (the YAML two levels below tools/), the
    working directory only when nothing lies there; a path that leads nowhere is named on stderr"""
    cfgs = tmp_path / "OpenPCDet" / "tools" / "cfgs" / "dataset_configs"
    cfgs.mkdir(parents=True)
    cfg = cfgs / "d.yaml"
    cfg.write_text("DATA_PATH: '../data/x'\nFOV_POINTS_ONLY: True\n")
    (tmp_path / "OpenPCDet" / "data" / "x").mkdir(parents=True)
    (tmp_path / "OpenPCDet" / "tools" / "run").mkdir()
    (tmp_path / "OpenPCDet" / "tools" / "data" / "x").mkdir(parents=True)     # ../data/x as seen from tools/run
    monkeypatch.chdir(tmp_path / "OpenPCDet" / "tools" / "run")
    assert ki.resolve_data_path(cfg, "../data/x") == (tmp_path / "OpenPCDet" / "data" / "x").resolve()
    (tmp_path / "OpenPCDet" / "tools" / "data" / "y").mkdir()
    assert ki.resolve_data_path(cfg, "../data/y") == (tmp_path / "OpenPCDet" / "tools" / "data" / "y").resolve()
    assert ki.resolve_data_path(cfg, str(tmp_path)) == tmp_path
    r = subprocess.run([sys.executable, "-m", "modest_amd.kitti_infos", "create_kitti_infos", str(cfg), "../data/nowhere", "--host"],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "ImageSets" in r.stderr and str(tmp_path / "OpenPCDet" / "data" / "nowhere") in r.stderr
