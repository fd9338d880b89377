"""CPU: tests/point_targets_seq.py (the numpy restatement the GPU tests compare with) reproduces every output that
tools/make_golden_point_targets.py recorded from the reference's own PointHeadTemplate.assign_stack_targets and
PointResidualCoder -- labels and box labels bit for bit, part labels within the bound DESIGN.md section 7l derives from
the inputs -- and the fixture holds every case it promises.  Also: every case of tests/point_targets_cases.py holds its
edge (the cases of PAST, past 65 boxes, 3 samples and one workgroup's rounds, too), a second restatement that walks
as the kernel does (workgroups, rounds, tiles) equals the first everywhere and every fault it can be asked for shows on a
named PAST case, the branch that is not provided, the reference's assertions, the opt-in binding, the header / ctypes
mirror of the new entry point, no scratch and no spill in the kernel, and the benchmark's yardstick against the recorded outputs."""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import pytest

import point_targets_cases as cases
import point_targets_seq as seq
import roipool_seq

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "point_targets.npz")
GOLD_CROWD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "point_targets_crowd.npz")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def crowd():
    return dict(np.load(GOLD_CROWD))


def ours_of(gold, name):
    cfg, pts, gt, ext, mean = seq.scene_inputs(gold, name)
    return seq.assign(pts, gt, ext, cfg["num_class"], mean, cfg["want_box"], cfg["want_part"])


def test_fixture_is_small(gold):
    assert os.path.getsize(GOLD) <= 64 * 1024
    assert seq.scenes(gold) == ["box_part", "box", "box_no_mean", "part", "labels"]
    assert all(150 <= len(gold[n + "_points"]) <= 400 for n in seq.scenes(gold))


def test_crowd_fixture_is_small(crowd):
    assert os.path.getsize(GOLD_CROWD) <= 96 * 1024
    assert seq.scenes(crowd) == ["crowd"]
    cfg, pts, gt, _, mean = seq.scene_inputs(crowd, "crowd")
    assert gt.shape == (3, 140, 8) and [int(gt[b].any(axis=1).sum()) for b in range(3)] == [140, 100, 66]
    assert 380 <= len(pts) <= 420 and cfg["want_box"] and cfg["want_part"] and cfg["num_class"] == 3 and mean.shape == (3, 3)
    k = seq.sample_of(pts, 3)
    assert min(len(set(k[i:i + 64])) for i in range(0, len(k) - 63, 64)) >= 3      # shuffled


def every_scene(*recs):
    return [(rec, name) for rec in recs for name in seq.scenes(rec)]


def test_restatement_reproduces_the_reference(gold, crowd):
    for rec, name in every_scene(gold, crowd):
        cfg, pts, gt, ext, _ = seq.scene_inputs(rec, name)
        ref = seq.recorded(rec, name)
        bound = seq.part_bound(pts, gt, ext, cfg["want_box"]) if cfg["want_part"] else None
        why = seq.mismatches(ours_of(rec, name), ref, bound=bound)
        assert not why, name + "\n" + "\n".join(why)
        assert ref["point_cls_labels"].dtype == np.int64 and (ref["point_cls_labels"] > 0).any()
        assert seq.same_bits(ext, seq.enlarge(gt, cfg["extra_width"]))


def test_the_comparison_is_not_vacuous(gold):
    name = "box_part"
    cfg, pts, gt, ext, _ = seq.scene_inputs(gold, name)
    ref = seq.recorded(gold, name)
    bound = seq.part_bound(pts, gt, ext, True)
    k, idx, _ = seq.membership(pts, gt, ext)
    live = np.flatnonzero((idx >= 0) & (np.abs(gt[k, np.maximum(idx, 0), 3]) > 1))[0]    # a foreground point of an ordinary box
    assert 0 < bound[live, 0] < 1e-5 and 0 < bound[live, 1] < 1e-5 and bound[live, 2] == 0
    assert (bound[idx < 0] == 0).all()
    for key, col in (("point_box_labels", 0), ("point_box_labels", 4), ("point_box_labels", 7), ("point_part_labels", 2)):
        bad = {k_: None if v is None else v.copy() for k_, v in ref.items()}
        bad[key][live, col] = np.nextafter(bad[key][live, col], F(9))        # one float: these are compared bit for bit
        assert seq.mismatches(bad, ref, bound=bound), (key, col)
    for col in (0, 1):
        bad = {k_: None if v is None else v.copy() for k_, v in ref.items()}
        bad["point_part_labels"][live, col] += F(4 * bound[live, col]) + F(2.0 ** -22)
        assert seq.mismatches(bad, ref, bound=bound), col
        ok = {k_: None if v is None else v.copy() for k_, v in ref.items()}
        ok["point_part_labels"][live, col] = np.nextafter(ok["point_part_labels"][live, col], F(9))
        assert not seq.mismatches(ok, ref, bound=bound) and seq.mismatches(ok, ref), col
    bad = {k_: None if v is None else v.copy() for k_, v in ref.items()}
    bad["point_cls_labels"][live] = -1
    assert seq.mismatches(bad, ref, bound=bound)


def test_the_coder_clamp_reaches_the_part_labels(gold):
    """encode_torch clamps the sizes of the foreground rows in place, and the part labels divide by those rows afterwards:
    with box labels asked for, a box with dx = 0 gives l / 1e-5 + 0.5, without them l / 0"""
    cfg, pts, gt, ext, _ = seq.scene_inputs(gold, "box_part")
    k, idx, _ = seq.membership(pts, gt, ext)
    at = np.flatnonzero((idx >= 0) & (gt[k, np.maximum(idx, 0), 3] == 0) & gt[k, np.maximum(idx, 0)].any(axis=1))
    assert len(at) == 2
    ref = seq.recorded(gold, "box_part")["point_part_labels"][at]
    assert np.isfinite(ref).all() and sorted(ref[:, 0]) == [F(0.5), F(F(2.0 ** -18) / seq.TINY + F(0.5))]
    cfg, pts, gt, ext, _ = seq.scene_inputs(gold, "part")
    k, idx, _ = seq.membership(pts, gt, ext)
    at = np.flatnonzero((idx >= 0) & (gt[k, np.maximum(idx, 0), 3] == 0) & gt[k, np.maximum(idx, 0)].any(axis=1))
    ref = seq.recorded(gold, "part")["point_part_labels"][at]
    assert len(at) == 2 and not np.isfinite(ref[:, 0]).any()


def test_fixture_cases(gold, crowd):
    got = seq.fixture_cases(gold)
    assert len(got) >= 15 and all(got.values()), [k for k, v in got.items() if not v]
    got = seq.crowd_cases(crowd, cases.TILE)
    assert len(got) >= 4 and all(got.values()), [k for k, v in got.items() if not v]


@pytest.mark.parametrize("name", list(cases.CASES))
def test_every_case_holds_its_edge(name):
    c = cases.CASES[name]()
    assert c["present"](c)
    assert c["gt"].shape[0] <= 3 and len(c["points"]) <= 1600 and c["gt"].shape[1] <= cases.TILE + 1
    assert c["ext"].shape == c["gt"].shape and c["points"].dtype == F


def test_kernel_constants_are_the_ones_the_cases_cross():
    assert (cases.WG, cases.TILE) == (256, 64)
    assert {"N = 255", "N = 256", "N = 257", "N = 1", "N = 63", "N = 65"} <= set(cases.CASES)
    assert cases.CASES["last row past the tile"]()["gt"].shape[1] == cases.TILE + 1
    # PAST crosses 2 * TILE and 3 * TILE rows, 16 and 40 rounds in one workgroup, and a workgroup of one point
    rows = {n: cases.past(n)["gt"].shape[1] for n in cases.PAST}
    assert any(m == 2 * cases.TILE for m in rows.values()) and any(m == 2 * cases.TILE + 1 for m in rows.values())
    assert any(2 * cases.TILE < m < 3 * cases.TILE for m in rows.values()) and any(m > 3 * cases.TILE for m in rows.values())
    assert max(rounds_per_workgroup(cases.past("16 samples in one workgroup"))) == 16
    assert max(rounds_per_workgroup(cases.past("40 samples shuffled, two tiles"))) == 40
    assert 4 * cases.WG + 1 in {len(cases.past(n)["points"]) for n in cases.PAST}


def rounds_per_workgroup(c):
    k = seq.sample_of(c["points"], c["gt"].shape[0])
    return [len(set(k[i:i + cases.WG]) - {-1}) for i in range(0, len(k), cases.WG)]


@pytest.mark.parametrize("name", list(cases.PAST))
def test_every_case_past_the_tile_holds_its_edge(name):
    c = cases.past(name)
    assert c["present"](c)
    assert c["gt"].shape[0] <= 40 and c["gt"].shape[1] <= 4 * cases.TILE and len(c["points"]) <= 20100
    assert c["ext"].shape == c["gt"].shape and c["points"].dtype == F
    assert c["num_class"] == 3 and c["mean"] is cases.KITTI and c["want_box"] and c["want_part"]


# ------------------------------------------------------------------------------------------------ the kernel's walk
def tiled(c, fault=None):
    return seq.membership_tiled(c["points"], c["gt"], c["ext"], cases.WG, cases.TILE, fault)


def same_membership(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", list(cases.CASES) + list(cases.PAST))
def test_the_tiled_walk_is_the_restatement(name):
    c = cases.past(name) if name in cases.PAST else cases.CASES[name]()
    assert same_membership(tiled(c), seq.membership(c["points"], c["gt"], c["ext"]))


def test_the_tiled_walk_is_the_restatement_on_the_fixtures(gold, crowd):
    for rec, name in every_scene(gold, crowd):
        _, pts, gt, ext, _ = seq.scene_inputs(rec, name)
        for wg, tile in ((cases.WG, cases.TILE), (64, 8)):
            assert same_membership(seq.membership_tiled(pts, gt, ext, wg, tile), seq.membership(pts, gt, ext)), name


# fault -> the PAST cases on which it changes idx, the enlarged hit or a label (each is asserted)
SEEN_BY = {
    "tile index restarts": ["M = 2 tiles + 1", "M = 3 tiles + 37", "first hit wins across tiles", "enlarged rows elsewhere",
                            "detector-sized"],
    "last tile wins": ["M = 2 tiles", "M = 3 tiles + 37", "first hit wins across tiles", "enlarged rows elsewhere"],
    "enlarged latch per tile": ["M = 2 tiles", "enlarged rows elsewhere", "40 samples shuffled, two tiles",
                                "one point in the tail workgroup"],
    "three rounds only": ["16 samples in one workgroup", "40 samples shuffled, two tiles"],
    "rounds in order of appearance": ["40 samples shuffled, two tiles", "samples descending"],
    "sample by rank among those present": ["samples that no point names"],
    "minimum of the first wavefront only": ["16 samples in one workgroup", "samples descending", "detector-sized"],
    "strays join sample 0": ["a wavefront and a workgroup of strays"],
}


def test_every_fault_is_named_with_its_cases():
    assert set(SEEN_BY) == set(seq.FAULTS) and all(set(v) <= set(cases.PAST) for v in SEEN_BY.values())
    assert set().union(*SEEN_BY.values()) == set(cases.PAST)               # and every PAST case sees a fault


@pytest.mark.parametrize("fault", list(seq.FAULTS))
def test_every_fault_shows_on_its_cases(fault):
    for name in SEEN_BY[fault]:
        c = cases.past(name)
        m = tiled(c, fault)
        out = seq.assign(c["points"], c["gt"], c["ext"], c["num_class"], c["mean"], c["want_box"], c["want_part"], member=m)
        true = seq.membership(c["points"], c["gt"], c["ext"])
        assert not np.array_equal(m[1], true[1]) or not np.array_equal(out["point_cls_labels"], c["want"]["point_cls_labels"]), \
            (fault, name)
        assert seq.mismatches(out, c["want"]), (fault, name)               # what the device tests compare


def test_the_crowd_scene_sees_the_faults_of_the_tile_loop(crowd):
    """against what the reference itself recorded, not against the restatement"""
    cfg, pts, gt, ext, mean = seq.scene_inputs(crowd, "crowd")
    ref = seq.recorded(crowd, "crowd")
    bound = seq.part_bound(pts, gt, ext, cfg["want_box"])
    for fault in (None, "tile index restarts", "last tile wins", "enlarged latch per tile"):
        m = seq.membership_tiled(pts, gt, ext, cases.WG, cases.TILE, fault)
        out = seq.assign(pts, gt, ext, cfg["num_class"], mean, cfg["want_box"], cfg["want_part"], member=m)
        assert bool(seq.mismatches(out, ref, bound=bound)) == (fault is not None), fault


def test_the_old_cases_miss_all_faults_of_the_walk_but_three():
    """why PAST exists: of the eight faults, the 29 cases of CASES see the order of the rounds ("shuffled bs_idx"), the
    missing reduction across wavefronts and the strays; the tile loop's three and the other two of the round loop pass"""
    seen = {f: [n for n, mk in cases.CASES.items() for c in [mk()] if not same_membership(tiled(c, f), tiled(c))]
            for f in seq.FAULTS}
    assert seen["rounds in order of appearance"] == ["shuffled bs_idx"] and seen["strays join sample 0"] == ["bs_idx -1, B, 0.5"]
    assert seen["minimum of the first wavefront only"]
    assert not any(seen[f] for f in ("tile index restarts", "last tile wins", "enlarged latch per tile", "three rounds only",
                                     "sample by rank among those present"))


# ------------------------------------------------------------------------------------------------ the Python side
def stub_head(mean=None, num_class=3):
    from modest_amd.utils import point_head_targets as pht
    head = pht.bind(type("Head", (), {}))()
    head.num_class = num_class
    head.box_coder = types.SimpleNamespace(use_mean_size=mean is not None, mean_size=mean)
    return head


def test_the_ball_constraint_is_not_provided():
    import torch
    head = stub_head()
    pts, gt = torch.zeros((5, 4)), torch.zeros((2, 3, 8))
    with pytest.raises(NotImplementedError, match="use_ball_constraint"):
        head.assign_stack_targets(pts, gt, set_ignore_flag=False, use_ball_constraint=True, central_radius=2.0)
    with pytest.raises(NotImplementedError, match="use_ball_constraint"):
        head.assign_stack_targets(pts, gt, extend_gt_boxes=gt, set_ignore_flag=False, use_ball_constraint=True)


def test_the_assertions_of_the_reference():
    import torch
    head = stub_head()
    pts, gt = torch.zeros((5, 4)), torch.zeros((2, 3, 8))
    with pytest.raises(AssertionError, match="points.shape"):
        head.assign_stack_targets(torch.zeros((5, 3)), gt, extend_gt_boxes=gt)
    with pytest.raises(AssertionError, match="points.shape"):
        head.assign_stack_targets(torch.zeros((1, 5, 4)), gt, extend_gt_boxes=gt)
    with pytest.raises(AssertionError, match="gt_boxes.shape"):
        head.assign_stack_targets(pts, torch.zeros((2, 3, 7)), extend_gt_boxes=gt)
    with pytest.raises(AssertionError, match="extend_gt_boxes.shape"):
        head.assign_stack_targets(pts, gt, extend_gt_boxes=torch.zeros((2, 3, 9)))
    for both in (True, False):
        with pytest.raises(AssertionError, match="Choose one only"):
            head.assign_stack_targets(pts, gt, extend_gt_boxes=gt, set_ignore_flag=both, use_ball_constraint=both)
    with pytest.raises(ValueError, match="extend_gt_boxes"):
        head.assign_stack_targets(pts, gt)


def test_cpu_tensors_are_refused_without_loading_the_library(monkeypatch):
    import torch
    from modest_amd import _lib, ops

    def no_load(*a, **k):
        raise AssertionError("the library was opened")
    monkeypatch.setattr(_lib, "load", no_load)
    monkeypatch.setattr(ops, "load", no_load)
    head = stub_head()
    with pytest.raises(ValueError, match="device"):
        head.assign_stack_targets(torch.zeros((5, 4)), torch.zeros((2, 3, 8)), extend_gt_boxes=torch.zeros((2, 3, 8)))
    with pytest.raises(ValueError, match="device"):
        ops.point_targets(torch.zeros((5, 4)), torch.zeros((2, 3, 8)), torch.zeros((2, 3, 8)), 3)


# ------------------------------------------------------------------------------------------------ the binding
def test_binding_is_opt_in():
    from modest_amd.utils import pcdet_bind
    from modest_amd.utils import point_head_targets as pht
    name = "pcdet.models.dense_heads.point_head_template"
    names = list(pcdet_bind.SHIMS) + list(pcdet_bind.STAND_INS) + ["spconv.utils", name]
    saved = {k: sys.modules.get(k) for k in names}
    try:
        for k in names:
            sys.modules.pop(k, None)
        assert name == pcdet_bind.POINT_TARGETS_NAME and name not in pcdet_bind.SHIMS and name not in pcdet_bind.STAND_INS
        keys = sorted(list(pcdet_bind.SHIMS) + list(pcdet_bind.STAND_INS))
        if importlib.util.find_spec("pcdet") is None:
            # nothing to bind onto: the name is left out, nothing is registered under it
            assert sorted(pcdet_bind.install(point_targets=True)) == keys and name not in sys.modules

        def reference_method(self):
            return "reference"
        fake = types.ModuleType(name)
        fake.PointHeadTemplate = type("PointHeadTemplate", (), {"assign_stack_targets": reference_method})
        sub = type("PointHeadBox", (fake.PointHeadTemplate,), {})
        sys.modules[name] = fake
        for kw in ({}, {"sparse_conv": True}, {"point_stack": True}, {"point_targets": False}):   # the default call does what it did
            bound = pcdet_bind.install(**kw)
            assert sorted(bound) == keys, kw
            assert fake.PointHeadTemplate.assign_stack_targets is reference_method and sys.modules[name] is fake
        bound = pcdet_bind.install(point_targets=True)
        assert sorted(bound) == sorted(keys + [name]) and bound[name] is fake and sys.modules[name] is fake
        assert fake.PointHeadTemplate.assign_stack_targets is pht.assign_stack_targets
        assert sub.assign_stack_targets is pht.assign_stack_targets           # the heads inherit it
        again = pcdet_bind.install(point_targets=True)                        # idempotent
        assert sorted(again) == sorted(bound) and all(again[k] is bound[k] for k in bound)
        assert sorted(pcdet_bind.install()) == keys and fake.PointHeadTemplate.assign_stack_targets is pht.assign_stack_targets
        assert sorted(pcdet_bind.install(stand_ins=False, point_targets=True)) == sorted(list(pcdet_bind.SHIMS) + [name])
        # a module of that name without the class: nothing to bind onto
        sys.modules[name] = types.ModuleType(name)
        assert name not in pcdet_bind.install(point_targets=True)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    assert all(sys.modules.get(k) is v for k, v in saved.items())


# ------------------------------------------------------------------------------------------------ the build
def test_header_ctypes_mirror_and_no_scratch():
    import ctypes as C
    import re
    from modest_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "modest_hip.h")).read(), flags=re.S)
    ctype = {"int": C.c_int, "int64_t": C.c_int64}
    fn = "modest_point_targets"
    m = re.search(r"\b(int64_t|int)\s+%s\s*\(([^)]*)\)" % fn, src)
    assert m, fn
    args = [a.strip() for a in m.group(2).split(",")]
    want = [_lib.VP if "*" in a else ctype[a.split()[0]] for a in args]
    res, have = _lib.SIGNATURES[fn]
    assert res is ctype[m.group(1)] and have == want and len(want) == 20
    assert hasattr(lib, fn)
    # refused arguments launch nothing and need no device
    assert lib.modest_point_targets(-1, None, 4, 1, 1, None, 0, 0, 0, None, 0, 0, 0, None, 0, 3, None, None, None, None) != 0
    assert b"negative" in lib.modest_last_error()
    assert lib.modest_point_targets(0, None, 4, 1, 1, None, 0, 0, 0, None, 0, 0, 0, None, 0, 3, None, None, None, None) == 0
    assert lib.modest_point_targets(5, None, 4, 1, 1, None, 0, 0, 0, None, 0, 0, 0, None, 0, 3, None, None, None, None) != 0
    res = json.load(open(os.path.join(os.path.dirname(build.LIB), "kernel_resources.json")))
    mine = {k: v for k, v in res.items() if v.get("file") == "point_targets.hip"}
    assert len(mine) == 1 and "pt_assign" in next(iter(mine))
    assert all(v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 for v in mine.values()), mine
    text = open(os.path.join(ROOT, "modest_amd", "csrc", "point_targets.hip")).read()
    assert "atomic" not in text.split("namespace {", 1)[1] and "hipMalloc" not in text and "hipMemset" not in text


# ------------------------------------------------------------------------------------------------ the benchmark's yardstick
def test_the_benchmark_yardstick_computes_the_reference_results(gold, crowd):
    """tools/point_targets_bench.py's PyTorch restatement of the path before this op, on the CPU with the numpy
    membership in place of the device's points_in_boxes_gpu, against the recorded outputs"""
    import torch
    spec = importlib.util.spec_from_file_location("point_targets_bench", os.path.join(ROOT, "tools", "point_targets_bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)

    def pib(points, boxes):
        return torch.from_numpy(roipool_seq.points_in_boxes(boxes.numpy(), points.numpy()))
    for rec, name in every_scene(gold, crowd):
        cfg, pts, gt, ext, mean = seq.scene_inputs(rec, name)
        out = bench.yard_assign(torch.from_numpy(pts.copy()), torch.from_numpy(gt.copy()), torch.from_numpy(ext.copy()),
                                cfg["num_class"], None if mean is None else torch.from_numpy(mean.copy()), cfg["want_box"],
                                cfg["want_part"], pib)
        out = {k: None if v is None else v.numpy() for k, v in out.items()}
        assert not seq.mismatches(out, seq.recorded(rec, name)), name
