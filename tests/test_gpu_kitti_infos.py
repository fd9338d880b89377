"""GPU: modest_amd.kitti_infos (csrc/kitti_infos.hip) against the reference's recorded outputs
(tests/golden/kitti_infos.npz) and, on full-size synthetic trees, against the numpy / scipy host mirror: infos and
dbinfos equal after load, database files byte for byte.  Every test here fails on a tree without the module."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from tests.infos_tree import TREES, assert_same, check_outputs, expected, golden, tree_scans, write_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cli(cfg, root, *extra, timeout=900):
    r = subprocess.run([sys.executable, "-m", "modest_amd.kitti_infos", "create_kitti_infos", str(cfg), str(root), *extra],
                       cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def _cfg(tmp_path, fov=True):
    f = tmp_path / ("cfg_%s.yaml" % fov)
    f.write_text("DATASET: 'KittiDataset'\nDATA_PATH: '../data/lyft'\nFOV_POINTS_ONLY: %s\n" % fov)
    return f


@pytest.mark.gpu
@pytest.mark.parametrize("name", TREES)
@pytest.mark.parametrize("caps", [(), ("--und_cap", "1", "--pass_boxes", "2", "--batch", "2")], ids=["default", "overflow"])
def test_cli_reproduces_reference_files(gpu, tmp_path, name, caps):
    g = golden()
    for fov in (True, False):
        root = tmp_path / ("fov_%s" % fov)
        write_tree(g, name, root)
        out = _cli(_cfg(tmp_path, fov), root, "True", *caps)
        print(out)
        check_outputs(g, name, root, fov=fov)
        assert out["scans"] == len(g[name + "/ids"]) and out["db_points"] == int(g[name + "/db_counts"].sum())
        if name == "dyn":   # the planted rows lie inside the band: the host predicate must have been asked
            assert out["host_boxes"] > 0
            if caps:
                assert out["overflow_boxes"] > 0


@pytest.mark.gpu
def test_fov_flags_equal_the_reference(gpu):
    import torch
    from modest_amd import kitti_infos as ki, ops
    import tempfile
    g = golden()
    for name in TREES:
        for idx, rows, label, calib_text, size in tree_scans(g, name):
            with tempfile.TemporaryDirectory() as d:
                open(os.path.join(d, "c.txt"), "w").write(calib_text)
                calib = ki.Calibration(os.path.join(d, "c.txt"))
            fr = np.zeros(1, dtype=ops.INFOS_FRAME)
            fr["n"], fr["height"], fr["width"], fr["fov_only"] = len(rows), size[1], size[0], 1
            fr["m1"][0], fr["p2t"][0] = calib.lidar_to_rect_matrix().reshape(-1), np.ascontiguousarray(calib.P2.T).reshape(-1)
            st = ops.infos_count(torch.from_numpy(rows).to(gpu), len(rows), fr, np.zeros(0, dtype=ops.INFOS_BOX), want_fov=True)
            fov = st.fov.cpu().numpy().astype(bool)
            assert np.array_equal(np.packbits(fov), g["%s/fov/%s" % (name, idx)]), (name, idx)


@pytest.mark.gpu
def test_points_in_boxes_cpu_equals_the_mirror(gpu):
    import torch
    from modest_amd import kitti_infos as ki
    from modest_amd.utils.roiaware_pool3d_utils import points_in_boxes_cpu
    g = golden()
    for name in TREES:
        infos = {i["point_cloud"]["lidar_idx"]: i for i in expected(g, name)[0] + expected(g, name)[1]}
        for idx, rows, *_ in tree_scans(g, name):
            key = "%s/mask/%s" % (name, idx)
            if key not in g.files:
                continue
            gt = infos[idx]["annos"]["gt_boxes_lidar"]
            m = points_in_boxes_cpu(rows[:, :3], gt)
            assert isinstance(m, np.ndarray) and m.dtype == np.int32 and m.shape == (len(gt), len(rows))
            assert np.array_equal(np.packbits(m > 0, axis=1), g[key]), (name, idx)
    # 64 boxes x 120 k points, tensors in -> tensor out
    from modest_amd import synth
    rs = np.random.RandomState(5)
    text = synth.infos_label_text(rs, 64)
    rows = synth.infos_points(77, text, 120_000 - 64 * 600, (400, 800))
    boxes = np.stack([[float(v) for v in ln.split(" ")[8:15]] for ln in text.splitlines()])
    b7 = np.stack([boxes[:, 5] + 0.5, -boxes[:, 3], -boxes[:, 4] - 0.3 + boxes[:, 0] / 2, boxes[:, 2], boxes[:, 1], boxes[:, 0],
                   -(np.pi / 2 + boxes[:, 6])], axis=1)
    ref = ki.points_in_boxes_host(rows[:, :3], b7)
    got = points_in_boxes_cpu(torch.from_numpy(rows[:, :3]), torch.from_numpy(b7))
    assert isinstance(got, torch.Tensor) and got.dtype == torch.int32 and not got.is_cuda
    assert np.array_equal(got.numpy(), ref) and ref.sum() > 10_000
    got = points_in_boxes_cpu(torch.from_numpy(rows[:, :3]).to(gpu), torch.from_numpy(b7).to(gpu))
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), ref)


@pytest.mark.gpu
def test_python_entry_points_on_the_fixture_tree(gpu, tmp_path):
    """get_infos (a sample list, labels off) and create_groundtruth_database from an infos pickle (another split's
    directory name, used_classes) against the fixture and the mirror"""
    from modest_amd import kitti_infos as ki
    g = golden()
    write_tree(g, "car", tmp_path)
    tr, va, db = expected(g, "car")
    ids = [str(x) for x in g["car/train"]]
    assert_same(ki.get_infos(tmp_path, "train", batch=1), tr)
    assert_same(ki.get_infos(tmp_path, "train", sample_id_list=ids[1:]), tr[1:])
    bare = ki.get_infos(tmp_path, "val", has_label=False)
    assert list(bare[0].keys()) == ["point_cloud", "image", "calib"]
    pickle.dump(tr, open(tmp_path / "kitti_infos_train.pkl", "wb"))
    st = {}
    assert_same(ki.create_groundtruth_database(tmp_path, tmp_path / "kitti_infos_train.pkl", stats=st), db)
    assert st["db_points"] == int(g["car/db_counts"].sum())
    check_outputs(g, "car", tmp_path, val=False)
    got = ki.create_groundtruth_database(tmp_path, tmp_path / "kitti_infos_train.pkl", used_classes=["Pedestrian"], split="val")
    assert list(got.keys()) == ["Pedestrian"] and all(d["path"].startswith("gt_database_val/") for d in got["Pedestrian"])
    assert sorted(os.listdir(tmp_path / "gt_database_val")) == sorted(os.listdir(tmp_path / "gt_database"))
    assert_same(pickle.load(open(tmp_path / "kitti_dbinfos_val.pkl", "rb")), got)


def _load(root, f):
    return pickle.load(open(os.path.join(str(root), f), "rb"))


def _same_trees(a, b):
    for f in ("kitti_infos_train.pkl", "kitti_infos_val.pkl", "kitti_dbinfos_train.pkl"):
        assert_same(_load(a, f), _load(b, f), f)
    fa = sorted(os.listdir(os.path.join(str(a), "gt_database")))
    assert fa == sorted(os.listdir(os.path.join(str(b), "gt_database")))
    for f in fa:
        assert open(os.path.join(str(a), "gt_database", f), "rb").read() == open(os.path.join(str(b), "gt_database", f), "rb").read(), f


@pytest.mark.gpu
def test_full_size_tree_equals_the_host_mirror(gpu, tmp_path):
    """256 Lyft-shape scans (60-120 k points, 300 boxes in some), batches of 64 and of 7, a rerun over an existing tree,
    and the bound that keeps the host predicate from hiding a dead kernel: without planted rows at most 15 % of the boxes
    may touch it (uniformly scattered float32 points put a point into the band of ~5 % of boxes holding ~250 points)."""
    import shutil
    from modest_amd import synth
    root = tmp_path / "gpu"
    c = synth.write_infos_tree(str(root), 9, 256, big_every=64)
    host = tmp_path / "host"
    shutil.copytree(root, host)
    cfg = _cfg(tmp_path)
    ref = _cli(cfg, host, "True", "--host", "--workers", "4", timeout=1500)
    out = _cli(cfg, root, "True")
    print(c, ref, out)
    assert out["scans"] == 256 and out["boxes"] == c["boxes"] and out["db_points"] == ref["db_points"] > 100_000
    assert out["overflow_boxes"] == 0
    assert out["host_boxes"] <= 0.15 * out["boxes"], out
    _same_trees(root, host)
    out7 = _cli(cfg, root, "True", "--batch", "7", "--overwrite")   # a batch boundary inside both splits, over the existing tree
    assert out7["db_points"] == out["db_points"] and out7["host_boxes"] == out["host_boxes"]
    _same_trees(root, host)
    assert _cli(cfg, root, "True").get("skipped") is True


@pytest.mark.gpu
def test_round_tree_from_labels_planes_and_infos(gpu, golden_dir, tmp_path):
    """the label -> dataset -> planes chain of a round on the e2e fixture: pre_compute_pp_score, generate_mask and
    gen_label_files write the origin scan's label file, modest_amd.ground_planes the planes, modest_amd.kitti_infos the
    infos and the database; the tree then holds everything KittiDataset and its gt_sampling augmentor open"""
    import shutil
    from PIL import Image
    from modest_amd import config, gen_label_files, generate_mask, pre_compute_pp_score, synth
    from tests.golden_tree import unpack_tree
    g, train, paths = unpack_tree(golden_dir, str(tmp_path))
    out = str(tmp_path / "out")
    origin = "%06d" % int(g["origin"])
    ov = [f"data_root={train}"] + [f"data_paths.{k}={v}" for k, v in paths.items()] + [
        f"data_paths.pp_score_path={out}/pp", f"data_paths.seg_save_dst={out}/seg",
        f"data_paths.bbox_info_save_dst={out}/bbox", f"data_paths.label_file_save_dst={out}/labels"]
    pre_compute_pp_score.main(config.compose("pp_score", ov))
    generate_mask.main(config.compose("generate_mask", ov))
    gen_label_files.main(config.compose("generate_label_files", ov))
    root = tmp_path / "data"
    other = "%06d" % ((int(g["origin"]) + 1) % (len(g["bin_offsets"]) - 1))
    os.makedirs(root / "training" / "label_2")
    os.makedirs(root / "training" / "image_2")
    shutil.copy(f"{out}/labels/{origin}.txt", root / "training" / "label_2" / (origin + ".txt"))
    (root / "training" / "label_2" / (other + ".txt")).write_text("")
    for idx in (origin, other):
        Image.new("L", (1224, 1024)).save(root / "training" / "image_2" / (idx + ".png"))
    synth.write_infos_splits(str(root), [origin], [other])
    t = root / "training"
    r = subprocess.run([sys.executable, "-m", "modest_amd.ground_planes", "--calib_dir", str(t / "calib"), "--lidar_dir",
                        str(t / "velodyne"), "--planes_dir", str(t / "planes"), "--min_h", "1.5", "--max_h", "2.5"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = _cli(_cfg(tmp_path), root, "True")
    assert res["scans"] == 2
    tr, va, db = (_load(root, f) for f in ("kitti_infos_train.pkl", "kitti_infos_val.pkl", "kitti_dbinfos_train.pkl"))
    n_lab = len(open(f"{out}/labels/{origin}.txt").read().splitlines())
    assert n_lab > 0 and [i["point_cloud"]["lidar_idx"] for i in tr] == [origin] and len(va) == 1
    a = tr[0]["annos"]
    assert a["gt_boxes_lidar"].shape == (n_lab, 7) and a["num_points_in_gt"].shape == (n_lab,) and set(a["name"]) == {"Dynamic"}
    assert va[0]["annos"]["num_points_in_gt"].shape == (0,)
    assert (t / "planes" / (origin + ".txt")).exists()
    assert list(db.keys()) == ["Dynamic"] and len(db["Dynamic"]) == n_lab
    mirror = tmp_path / "mirror"
    shutil.copytree(root, mirror, ignore=shutil.ignore_patterns("*.pkl", "gt_database"))
    _cli(_cfg(tmp_path), mirror, "True", "--host")
    _same_trees(root, mirror)
    for d in db["Dynamic"]:
        rows = np.fromfile(str(root / d["path"]), dtype=np.float32).reshape(-1, 4)
        assert len(rows) == d["num_points_in_gt"]
    assert sum(d["num_points_in_gt"] for d in db["Dynamic"]) > 0
