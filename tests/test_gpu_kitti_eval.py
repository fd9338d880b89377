"""AP evaluation on the GPU (csrc/kitti_eval.hip) against the reference's recorded outputs (tests/golden/kitti_eval.npz)
and the sequential restatement (tests/kitti_eval_seq.py)."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import kitti_eval_seq as seq
import kitti_golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return kitti_golden.load()


def _same(got, want):
    s, d = got
    ws, wd = want
    assert s == ws
    assert list(d) == list(wd)
    for k in d:
        assert float(d[k]) == wd[k], k


def test_overlaps_match_the_reference_blocks(gold):
    """2e-5 absolute, the float32 noise the reference itself carries, for all but a few pairs: where a corner lies on
    the other box's edge, its inside test turns on the last bit of a float32 cosine and a sliver joins or leaves the
    polygon (the fixture's AP does not depend on those pairs: see test_range_and_official_eval_equal_the_reference)"""
    from modest_amd import kitti_eval as ke
    blocks = ke.frame_overlaps(gold["gt"], gold["dt"])
    err = []
    for (b, d), wb, wd in zip(blocks, gold["bev"], gold["d3"]):
        assert b.shape == wb.shape
        if b.size:
            err += [np.abs(b - wb).reshape(-1), np.abs(d - wd).reshape(-1)]
    err = np.concatenate(err)
    print("overlaps vs the reference: largest difference %.3g, %d of %d values beyond 2e-5"
          % (err.max(), int((err > 2e-5).sum()), err.size))
    assert (err > 2e-5).sum() <= err.size // 500
    assert err.max() <= 1e-3


def test_identical_and_disjoint_boxes():
    from modest_amd import kitti_eval as ke
    rng = np.random.default_rng(0)
    b = np.concatenate([rng.uniform(-40, 40, (64, 2)), rng.uniform(0.5, 5, (64, 2)), rng.uniform(-3, 3, (64, 1))], 1)
    iou = ke.rotate_iou_gpu_eval(b, b)
    assert np.all(np.diag(iou) >= 1 - 2e-5)
    far = b.copy()
    far[:, 0] += 1000
    assert np.all(ke.rotate_iou_gpu_eval(b, far) == 0)
    b7 = np.concatenate([b[:, :1], np.ones((64, 1)), b[:, 1:2], b[:, 2:3], np.full((64, 1), 1.5), b[:, 3:4], b[:, 4:]], 1)
    assert np.all(np.diag(ke.d3_box_overlap(b7, b7)) >= 1 - 2e-5)


def test_range_and_official_eval_equal_the_reference(gold):
    from modest_amd import kitti_eval as ke
    _same(ke.get_range_eval_result(gold["gt"], gold["dt"], "Dynamic"), gold["range"])
    _same(ke.get_official_eval_result(gold["gt"], gold["dt"], "Car"), gold["car"])
    _same(ke.get_official_eval_result(gold["gt"], gold["dt"], "Pedestrian"), gold["ped"])


def _stress_frames(seed, n=200):
    from modest_amd import synth
    gt, dt = synth.eval_frames(seed, n_frames=n, max_gt=10, max_dt=14)
    rng = np.random.default_rng(seed)
    for d in dt:                                  # some small boxes: ignored_det == 1 at difficulties 0-2
        if len(d["name"]):
            m = rng.random(len(d["name"])) < 0.2
            d["bbox"][m, 3] = d["bbox"][m, 1] + 10
    return gt, dt


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_statistics_equal_the_restatement(metric):
    from modest_amd import kitti_eval as ke
    gt, dt = _stress_frames(3 + metric)
    es = ke.EvalSet(gt, dt)
    if metric == 0:
        blocks = [ke.image_box_overlap(d["bbox"], g["bbox"]) for g, d in zip(gt, dt)]
    else:
        blocks = [x[metric - 1] for x in ke.frame_overlaps(gt, dt)]
    frames = list(zip(gt, dt, blocks))
    rows = [(1, 0, None), (0, 2, None), (6, 3, (0, 40)), (6, 3, None)]
    configs = [(r, mo) for r in range(len(rows)) for mo in (0.25, 0.5, 0.7)]
    pr, nt = es.statistics(metric, rows, configs, compute_aos=(metric == 0))
    for c, (r, mo) in enumerate(configs):
        cls, diff, rng = rows[r]
        fl = seq.range_flags(frames, cls, rng) if rng else None
        want, thr = seq.eval_config(frames, metric, cls, diff, mo, compute_aos=(metric == 0), flags=fl)
        assert nt[c] == len(thr)
        assert np.array_equal(pr[c, :nt[c], :3], want[:, :3]), (c, rows[r], mo)
        if metric == 0:
            assert np.array_equal(pr[c, :nt[c], 3], want[:, 3])


def test_frame_order_and_pair_budget_do_not_change_ap(gold, monkeypatch):
    from modest_amd import kitti_eval as ke
    gt, dt = _stress_frames(11, 400)
    base = ke.get_range_eval_result(gt, dt, "Dynamic")
    perm = np.random.default_rng(1).permutation(len(gt))
    shuf = ke.get_range_eval_result([gt[i] for i in perm], [dt[i] for i in perm], "Dynamic")
    assert base[0] == shuf[0] and all(base[1][k] == shuf[1][k] for k in base[1])
    biggest = max(len(g["name"]) * len(d["name"]) for g, d in zip(gt, dt))
    monkeypatch.setenv("MODEST_EVAL_PAIR_BUDGET", str(max(1, biggest - 1)))     # one frame exceeds the budget
    small = ke.get_range_eval_result(gt, dt, "Dynamic")
    assert base[0] == small[0] and all(base[1][k] == small[1][k] for k in base[1])
    _same(ke.get_official_eval_result(gold["gt"], gold["dt"], "Car"), gold["car"])


def test_frame_order_at_dataset_scale():
    from modest_amd import kitti_eval as ke
    from modest_amd import synth
    gt, dt = synth.eval_frames(5, n_frames=11872, max_gt=10, max_dt=14, names=("Dynamic", "Car", "DontCare"))
    base = ke.get_range_eval_result(gt, dt, "Dynamic")
    perm = np.random.default_rng(2).permutation(len(gt))
    shuf = ke.get_range_eval_result([gt[i] for i in perm], [dt[i] for i in perm], "Dynamic")
    assert base[0] == shuf[0] and all(base[1][k] == shuf[1][k] for k in base[1])


def test_self_evaluation_is_100():
    from modest_amd import kitti_eval as ke
    from modest_amd import synth
    gt, _ = synth.eval_frames(9, n_frames=150, names=("Dynamic", "Car"))
    dt = [dict(g, score=np.ones(len(g["name"]))) for g in gt]
    _, d = ke.get_range_eval_result(gt, dt, "Dynamic")
    z = np.abs(np.concatenate([g["location"][:, 2] for g in gt if len(g["name"])]))
    dyn = np.concatenate([g["name"] for g in gt if len(g["name"])]) == "Dynamic"
    for (s, e) in ((0, 30), (30, 50), (50, 80), (0, 80)):
        has = bool(((z > s) & (z <= e) & dyn).any())
        for k in ("3d_iou0.7", "3d_iou0.5", "bev_iou0.7", "bev_iou0.5"):
            v = d[f"Dynamic_{k}/{s:02d}-{e:02d}_R40"]
            assert (v == 100.0) if has else (v == 0.0), (k, s, e, v)


def test_large_frame_evaluates():
    from modest_amd import kitti_eval as ke
    from modest_amd import synth
    rng = np.random.default_rng(4)
    g = synth._eval_anno(rng, 300, ("Dynamic",), False)
    d = synth._eval_anno(rng, 5000, ("Dynamic",), True)
    d["location"][:300] = g["location"]
    d["dimensions"][:300] = g["dimensions"]
    d["rotation_y"][:300] = g["rotation_y"]
    pr, nt = ke.EvalSet([g], [d]).statistics(1, [(6, 3, None)], [(0, 0.5)])
    frames = [(g, d, ke.frame_overlaps([g], [d])[0][0])]
    want, thr = seq.eval_config(frames, 1, 6, 3, 0.5)
    assert nt[0] == len(thr) and np.array_equal(pr[0, :nt[0], :3], want[:, :3])


def _write_tree(root, annos, with_score):
    from modest_amd import synth
    os.makedirs(root, exist_ok=True)
    for i, a in enumerate(annos):
        b = {k: v for k, v in a.items() if with_score or k != "score"}
        open(os.path.join(root, "%06d.txt" % i), "w").write(synth.label_text(b))


def test_cli_on_label_tree_and_result_pkl(tmp_path):
    from modest_amd import kitti_eval as ke
    from modest_amd import synth
    gt, dt = synth.eval_frames(21, n_frames=60)
    _write_tree(str(tmp_path / "gt"), gt, False)
    _write_tree(str(tmp_path / "dt"), dt, True)
    split = tmp_path / "val.txt"
    split.write_text("".join("%06d\n" % i for i in range(len(gt))))
    g2 = ke.get_label_annos(str(tmp_path / "gt"), list(range(len(gt))))
    d2 = ke.get_label_annos(str(tmp_path / "dt"), list(range(len(gt))))
    want = ke.get_range_eval_result(g2, d2, "Dynamic")[0]
    pickle.dump([dict(a, frame_id="%06d" % i) for i, a in enumerate(d2)], open(tmp_path / "result.pkl", "wb"))
    for res in (str(tmp_path / "dt"), str(tmp_path / "result.pkl")):
        out = subprocess.run([sys.executable, "-m", "modest_amd.evaluate", "evaluate", f"--label_path={tmp_path / 'gt'}",
                              "--result_path", res, "--label_split_file", str(split), "--current_class", "Dynamic"],
                             cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        assert out.stdout.startswith(want + "\n")
        assert '"frames": 60' in out.stdout.splitlines()[-1]


# ------------------------------------------------------------------------------------------------ past every capacity
def _limit_frame(nd, seed=12):
    """one frame of nd Car detections and 8 gt (6 Car, 2 DontCare).  Only detections at indices >= nd - 32 (the last
    bitmap word) and three early duplicates overlap anything: the rest lie 1000 m and 3000 px away."""
    from modest_amd import synth
    rng = np.random.default_rng(seed)
    g = synth._eval_anno(rng, 8, ("Car",), False)
    g["name"] = np.array(["Car"] * 6 + ["DontCare"] * 2)
    g["occluded"][:] = 0
    g["truncated"][:] = 0.0
    g["bbox"][:, 3] = g["bbox"][:, 1] + np.round(rng.uniform(45, 120, 8), 2)     # every Car easy
    g["bbox"][6:] = [[1500, 150, 1600, 250], [1700, 150, 1800, 250]]              # apart from every Car
    d = synth._eval_anno(rng, nd, ("Car",), True)
    d["location"][:, 0] += 1000
    d["bbox"][:, [0, 2]] += 3000
    last = nd - 32
    for k in range(6):                              # gt k: matched by detection last + k (and k < 3 by detection k)
        for j in ([last + k, k] if k < 3 else [last + k]):
            for key in ("location", "dimensions", "rotation_y", "bbox", "alpha"):
                d[key][j] = g[key][k]
        d["score"][last + k] = (0.95, 0.6, 0.3, 0.85, 0.45, 0.2)[k]
    for k in range(6):                              # inside the DontCare boxes: taken by DontCare at metric 0
        j = last + 10 + k
        bb = g["bbox"][6 + k % 2]
        d["bbox"][j] = [bb[0] + 1, bb[1] + 1, bb[2] - 1, bb[3] - 1]
        d["score"][j] = 0.9
    return g, d


def _equal_to_restatement(es, frames, metric, rows, configs, compute_aos=False):
    pr, nt = es.statistics(metric, rows, configs, compute_aos=compute_aos)
    out = []
    for c, (r, mo) in enumerate(configs):
        cls, diff, rng = rows[r]
        fl = seq.range_flags(frames, cls, rng) if rng else None
        want, thr = seq.eval_config(frames, metric, cls, diff, mo, compute_aos=compute_aos, flags=fl)
        assert nt[c] == len(thr), (c, rows[r], mo)
        assert np.array_equal(pr[c, :nt[c], :3], want[:, :3]), (c, rows[r], mo)
        if compute_aos:
            assert np.array_equal(pr[c, :nt[c], 3], want[:, 3]), (c, rows[r], mo)
        out.append(want)
    return out


def test_a_frame_at_the_detection_limit():
    """8 192 detections: the last of the 256 bitmap words per lane, 64 KiB of dynamic LDS per workgroup"""
    import ctypes
    from modest_amd import _lib
    from modest_amd import kitti_eval as ke
    lim_t, lim_d = ctypes.c_int32(), ctypes.c_int32()
    _lib.check(_lib.load().modest_eval_limits(ctypes.byref(lim_t), ctypes.byref(lim_d)), "modest_eval_limits")
    nd = lim_d.value
    assert nd == 8192
    g, d = _limit_frame(nd)
    es = ke.EvalSet([g], [d])
    assert es.max_nd == nd
    rows = [(0, 3, None), (0, 0, None)]
    configs = [(0, 0.7), (0, 0.5), (1, 0.7)]
    frames = [(g, d, ke.frame_overlaps([g], [d])[0][0])]
    want = _equal_to_restatement(es, frames, 1, rows, configs)
    assert max(w[:, 0].max() for w in want) >= 4      # gt 3-5 are matched only by detections in the last word
    frames = [(g, d, ke.image_box_overlap(d["bbox"], g["bbox"]))]
    want = _equal_to_restatement(es, frames, 0, rows, configs, compute_aos=True)
    assert max(w[:, 0].max() for w in want) >= 4
    # the DontCare boxes take the last word's detections: without them those would be false positives
    _, ig, idt, dc = ke.clean_data(g, d, 0, 3)
    ov = frames[0][2]
    with_dc = seq.compute_statistics(ov, g["alpha"], d["alpha"], d["bbox"], d["score"], ig, idt, dc, 0, 0.5, 0.9, True)
    without = seq.compute_statistics(ov, g["alpha"], d["alpha"], d["bbox"], d["score"], ig, idt, [], 0, 0.5, 0.9, True)
    assert without[1] - with_dc[1] == 6
    # one detection more is refused by name
    g2, d2 = _limit_frame(nd + 1)
    with pytest.raises(ValueError, match="8193 detections: at most 8192"):
        ke.EvalSet([g2], [d2])


def test_more_than_128_configurations_in_one_call():
    """pass A runs 64 configurations per lane group (blockIdx.y) and ke_thresholds 64 per block: a third of each"""
    from modest_amd import kitti_eval as ke
    gt, dt = _stress_frames(13, 40)
    es = ke.EvalSet(gt, dt)
    rows = [(6, 3, None), (6, 0, None), (6, 1, None), (6, 2, None), (0, 0, None), (0, 3, None), (6, 3, (0, 30)),
            (6, 3, (30, 50)), (6, 3, (50, 80))]
    overlaps = np.round(np.linspace(0.05, 0.75, 15), 2)
    configs = [(r, mo) for r in range(len(rows)) for mo in overlaps]
    assert len(configs) > 128
    frames = list(zip(gt, dt, [x[0] for x in ke.frame_overlaps(gt, dt)]))
    want = _equal_to_restatement(es, frames, 1, rows, configs)
    assert sum(int(w[:, 0].max(initial=0) > 0) for w in want[128:]) >= 3     # the third group finds TPs


def test_more_than_64_configurations_through_the_public_api():
    """seven classes and four range buckets plus the whole range: 7 x 5 x 2 = 70 configurations per metric"""
    from modest_amd import kitti_eval as ke
    from modest_amd import synth
    names = ("Car", "Pedestrian", "Cyclist", "Van", "Person_sitting", "Truck", "Dynamic", "DontCare")
    gt, dt = synth.eval_frames(14, n_frames=80, max_gt=10, max_dt=14, names=names)
    ranges = (0, 20, 40, 60, 80)
    classes = list(names[:7])
    s_all, d_all = ke.get_range_eval_result(gt, dt, classes, ranges=ranges)
    s_one = ""
    for c in classes:
        s, d = ke.get_range_eval_result(gt, dt, c, ranges=ranges)
        assert len(d) == 4 * 5
        for k in d:
            assert float(d_all[k]) == float(d[k]), k
        s_one += s
    assert s_all == s_one
    assert any(float(v) > 0 for k, v in d_all.items() if k.startswith("Dynamic"))


def test_every_frame_its_own_batch(gold, monkeypatch):
    """MODEST_EVAL_PAIR_BUDGET=1: the overlaps, pass A and pass B (with the aos similarity rebuilt per batch) run frame
    by frame, and every number is the single-batch number"""
    from modest_amd import kitti_eval as ke
    gt, dt = _stress_frames(15, 120)
    rows = [(0, 0, None), (0, 2, None), (1, 1, None), (6, 3, None)]
    configs = [(r, mo) for r in range(len(rows)) for mo in (0.5, 0.7)]
    one = ke.EvalSet(gt, dt)
    assert len(one.batches) == 1
    want = one.statistics(0, rows, configs, compute_aos=True)
    want_off = ke.get_official_eval_result(gold["gt"], gold["dt"], "Car")
    monkeypatch.setenv("MODEST_EVAL_PAIR_BUDGET", "1")
    each = ke.EvalSet(gt, dt)
    assert len(each.batches) >= sum(1 for g, d in zip(gt, dt) if len(g["name"]) * len(d["name"])) > 90
    got = each.statistics(0, rows, configs, compute_aos=True)
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[0], want[0], equal_nan=True)
    assert (got[0][:, :, 3] > 0).any()
    _same(ke.get_official_eval_result(gold["gt"], gold["dt"], "Car"), want_off)
    _same(ke.get_official_eval_result(gold["gt"], gold["dt"], "Car"), gold["car"])
