"""AP evaluation without a GPU: the sequential restatement (tests/kitti_eval_seq.py) against the reference's recorded
outputs, the label reader, get_thresholds and the range-bucket flags."""
import os
import pickle

import numpy as np
import pytest

from modest_amd import kitti_eval as ke
from modest_amd import synth

import kitti_eval_seq as seq
import kitti_golden


@pytest.fixture(scope="module")
def gold():
    return kitti_golden.load()


def test_restatement_reproduces_the_reference_range_eval(gold):
    s, d = seq.range_eval(gold["gt"], gold["dt"], gold["bev"], gold["d3"])
    want_s, want_d = gold["range"]
    assert s == want_s
    assert list(d) == list(want_d)
    assert all(float(d[k]) == want_d[k] for k in d)


def test_restatement_reproduces_the_reference_statistics_table(gold):
    frames = list(zip(gold["gt"], gold["dt"], gold["bev"]))
    fl = seq.range_flags(frames, 6, (0, 80))
    pr, thr = seq.eval_config(frames, 1, 6, 3, 0.7, flags=fl)
    assert np.array_equal(thr, gold["z"]["thr_range_bev07"])
    assert np.array_equal(pr[:, :3].astype(np.int64), gold["z"]["pr_range_bev07"])


def test_restatement_reproduces_the_reference_official_eval_tp_tables(gold):
    # metric 0 (image boxes, float64 overlaps on the host) for Car: the AP the reference printed
    gt, dt = gold["gt"], gold["dt"]
    blocks = [ke.image_box_overlap(d["bbox"], g["bbox"]) for g, d in zip(gt, dt)]
    frames = list(zip(gt, dt, blocks))
    prec = np.zeros((1, 3, 1, 41))
    aos = np.zeros((1, 3, 1, 41))
    for diff in range(3):
        pr, _ = seq.eval_config(frames, 0, 0, diff, 0.7, compute_aos=True)
        _, prec[0, diff, 0], aos[0, diff, 0] = seq.curves(pr, True)
    want = gold["car"][1]
    r40 = ke.get_mAP_R40(prec)
    a40 = ke.get_mAP_R40(aos)
    assert float(r40[0, 0, 0]) == want["Car_image/easy_R40"]
    assert float(r40[0, 1, 0]) == want["Car_image/moderate_R40"]
    assert float(r40[0, 2, 0]) == want["Car_image/hard_R40"]
    assert float(a40[0, 1, 0]) == want["Car_aos/moderate_R40"]


def _write_tree(root, annos, with_score):
    os.makedirs(root, exist_ok=True)
    for i, a in enumerate(annos):
        b = dict(a)
        if not with_score:
            b.pop("score", None)
        open(os.path.join(root, "%06d.txt" % i), "w").write(synth.label_text(b))


def _f4(v):
    """what a label file written with %.4f reads back as (float() of the text)"""
    v = np.asarray(v)
    if v.dtype.kind == "i":
        return v
    return np.array([float("%.4f" % x) for x in v.reshape(-1)]).reshape(v.shape)


def test_label_reader_matches_label_text_and_pickle(gold, tmp_path):
    gt, dt = gold["gt"], gold["dt"]
    _write_tree(str(tmp_path / "gt"), gt, False)
    _write_tree(str(tmp_path / "dt"), dt, True)
    rg = ke.get_label_annos(str(tmp_path / "gt"), list(range(len(gt))))
    rd = ke.get_label_annos(str(tmp_path / "dt"))
    for a, r in zip(gt, rg):
        if len(a["name"]) == 0:
            assert r["name"].shape == (0,) and r["bbox"].shape == (0, 4) and r["score"].shape == (0,)
            continue
        assert r["name"].tolist() == a["name"].tolist()
        assert r["occluded"].dtype == np.int64 and r["truncated"].dtype == np.float64
        for k in ("truncated", "occluded", "alpha", "bbox", "dimensions", "location", "rotation_y"):
            assert np.array_equal(r[k], _f4(a[k])), k
        assert np.array_equal(r["score"], np.zeros(len(a["name"])))     # no score column: zeros
    for a, r in zip(dt, rd):
        if len(a["name"]):
            assert np.array_equal(r["score"], _f4(a["score"]))
            assert np.array_equal(r["dimensions"], _f4(a["dimensions"]))
    # a result.pkl holds the same dicts
    p = tmp_path / "result.pkl"
    pickle.dump([dict(a, frame_id="%06d" % i) for i, a in enumerate(dt)], open(p, "wb"))
    from modest_amd import evaluate
    rp = evaluate.read_detections(str(p), list(range(len(dt))))
    for a, r in zip(dt, rp):
        assert np.array_equal(r["score"], a["score"]) and r["name"].tolist() == a["name"].tolist()
    # filter_annos_low_score keeps score >= thresh
    f = ke.filter_annos_low_score(rd, 0.5)
    assert all((x["score"] >= 0.5).all() for x in f)
    assert sum(len(x["name"]) for x in f) == sum(int((x["score"] >= 0.5).sum()) for x in rd)


@pytest.mark.parametrize("seed", range(6))
def test_get_thresholds_equals_the_sequential_loop(seed):
    rng = np.random.default_rng(seed)
    for n, num_gt in ((1, 1), (7, 7), (40, 41), (200, 1000), (999, 1003), (3000, 3001), (500, 40), (81, 82)):
        n = min(n, num_gt)
        s = rng.random(n) if seed % 2 else np.round(rng.random(n) * 5) / 5      # ties
        want = seq.get_thresholds_loop(s.copy(), num_gt)
        got = ke.get_thresholds(s.copy(), num_gt)
        assert len(got) == len(want) and all(a == b for a, b in zip(got, want))


def test_range_flags_equal_filtered_annos(gold):
    frames = list(zip(gold["gt"], gold["dt"], gold["bev"]))
    for rng in ((0, 30), (30, 50), (50, 80)):
        pr_flags, thr_flags = seq.eval_config(frames, 1, 6, 3, 0.25, flags=seq.range_flags(frames, 6, rng))
        filt = []
        for g, d, ov in frames:
            ig, idd = seq.in_range(g, *rng), seq.in_range(d, *rng)
            gi, di = np.nonzero(ig)[0], np.nonzero(idd)[0]
            filt.append(({k: v[gi] for k, v in g.items()}, {k: v[di] for k, v in d.items()}, ov[np.ix_(di, gi)]))
        pr_f, thr_f = seq.eval_config(filt, 1, 6, 3, 0.25)
        assert np.array_equal(thr_flags, thr_f) and np.array_equal(pr_flags, pr_f)


def test_coco_eval_raises():
    with pytest.raises(NotImplementedError, match="4 of do_eval"):
        ke.get_coco_eval_result([], [], 0)


def test_official_eval_rejects_dynamic():
    with pytest.raises(KeyError):
        ke.get_official_eval_result([], [], "Dynamic")


def test_sys_modules_binding_resolves_openpcdet_import(tmp_path):
    """INTEGRATION.md's binding: OpenPCDet's `from .kitti_object_eval_python import eval as kitti_eval` gets this module"""
    import subprocess
    import sys
    pkg = tmp_path / "pcdet" / "datasets" / "kitti" / "kitti_object_eval_python"
    pkg.mkdir(parents=True)
    for d in (tmp_path / "pcdet", tmp_path / "pcdet" / "datasets", pkg):
        (d / "__init__.py").write_text("")
    (pkg / "eval.py").write_text("import numba\n")              # the reference's module cannot import here
    (tmp_path / "pcdet" / "datasets" / "kitti" / "__init__.py").write_text("")
    (tmp_path / "pcdet" / "datasets" / "kitti" / "kitti_dataset.py").write_text(
        "from .kitti_object_eval_python import eval as kitti_eval\n")
    code = ("import sys, modest_amd.kitti_eval as kitti_eval\n"
            "sys.modules['pcdet.datasets.kitti.kitti_object_eval_python.eval'] = kitti_eval\n"
            "from pcdet.datasets.kitti import kitti_dataset\n"
            "assert kitti_dataset.kitti_eval is kitti_eval\n"
            "assert callable(kitti_dataset.kitti_eval.get_official_eval_result)\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(tmp_path), root]))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
