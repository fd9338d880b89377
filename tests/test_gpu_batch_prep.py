"""GPU: training-batch preparation (modest_amd/csrc/batch_prep.hip through ops.batch_prep_*) against the numpy restatement
(tests/batch_prep_seq.py), bit for bit, on the hand-built cases (tests/batch_prep_cases.py) and at the workload's size."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_prep_cases as cases  # noqa: E402
import batch_prep_seq as seq  # noqa: E402
from modest_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def dev_of(a):
    return torch.from_numpy(np.array(a, copy=True)).to(DEV)


def inputs(c):
    pl = ops.batch_prep_plan(c["samples"], c["db_offsets"], c["F"], c["steps"], c["road_plane"])
    scene = dev_of(np.concatenate([s["points"] for s in c["samples"]], axis=0).astype(np.float32).reshape(-1, c["F"]))
    return pl, scene, dev_of(c["db_points"])


def run(c, pl=None, scene=None, db=None, **kw):
    if pl is None:
        pl, scene, db = inputs(c)
    return ops.batch_prep_stage1(pl, scene, db, c["range"], remove_extra_width=c["extra"], want_near=c["want_near"],
                                 remove_outside_boxes=c["remove_outside"], min_num_corners=c["min_corners"], **kw)[0]


def check_stage1(c, st, want):
    tab = np.array([[len(w["points"]), int((~w["near"]).sum()), len(w["gt"]), int(w["valid"].sum()), int((~w["valid"]).sum())] for w in want],
                   np.int32).reshape(-1, 5)
    assert np.array_equal(st.table, tab), (st.table, tab)
    assert np.array_equal(st.valid.cpu().numpy().astype(bool), np.concatenate([w["valid"] for w in want] + [np.zeros(0, bool)]))
    pts, gt = seq.batch(c, want)
    n = int(tab[:, 0].sum())
    assert seq.same_bits(st.points[:n].cpu().numpy(), pts)
    got_gt = st.gt_boxes.cpu().numpy()
    assert seq.same_bits(got_gt[:, :gt.shape[1]], gt) and not got_gt[:, gt.shape[1]:].any()
    lists = st.lists[:n].cpu().numpy()
    at = 0
    for w in want:
        k = len(w["points"])
        assert np.array_equal(lists[at:at + k], np.concatenate([np.where(w["near"])[0], np.where(~w["near"])[0]]))
        at += k


@pytest.mark.parametrize("name", list(cases.CASES))
def test_stage1_bit_for_bit(name):
    c = cases.case(name)
    st = run(c)
    check_stage1(c, st, cases.want(name))


@pytest.mark.parametrize("order", list(cases.ORDERS))
def test_stage2_bit_for_bit(order):
    procs, num, shuffle, *first = cases.ORDERS[order]
    c, want = cases.case("far"), cases.want("far")
    st = run(c)
    picks, rows, *perm = ops.batch_prep_order_draws(st.table, num, shuffle, np.random.RandomState(3), *first)
    got, _ = ops.batch_prep_order(st, picks, perm=perm[0] if perm else None)
    ref = seq.order_rows(want, procs, np.random.RandomState(3))
    assert rows.tolist() == [len(r) for r in ref]
    assert seq.same_bits(got.cpu().numpy(), seq.batch(c, want, ref)[0])


def test_picks_outside_their_lists_are_refused_before_the_launch():
    c = cases.case("far")
    st = run(c)
    k, far = int(st.table[0, 0]), int(st.table[0, 1])
    for bad in ([[0, k]], [[1, k - far]], [[2, far]], [[4 * 3, 0]], [[3, 0]], [[0, -1]]):
        with pytest.raises(ValueError, match="picks name"):
            ops.batch_prep_order(st, np.array(bad, np.int32))
    with pytest.raises(ValueError, match=r"\(n_out, 2\) int32"):
        ops.batch_prep_order(st, np.zeros((3, 2), np.int64))
    c2 = dict(c, want_near=False)
    with pytest.raises(ValueError, match="without want_near"):
        ops.batch_prep_order(run(c2), np.array([[1, 0]], np.int32))
    out, _ = ops.batch_prep_order(st, np.zeros((0, 2), np.int32))
    assert tuple(out.shape) == (0, 5)
    total = int(st.table[:, 0].sum())
    ok = np.concatenate([np.arange(n, dtype=np.int32) for n in st.table[:, 0]])
    with pytest.raises(ValueError, match="a place per point kept"):
        ops.batch_prep_order(st, np.array([[0, 0]], np.int32), perm=ok[:-1])
    bad = ok.copy()
    bad[0] = k                                              # one past the first sample's survivors
    with pytest.raises(ValueError, match="perm names a survivor"):
        ops.batch_prep_order(st, np.array([[0, 0]], np.int32), perm=bad)
    assert total == len(ok)


def test_bad_arguments_are_named():
    c = cases.case("collisions")
    pl, scene, db = inputs(c)
    with pytest.raises(ValueError, match="scene_points must be a device tensor"):
        ops.batch_prep_stage1(pl, scene.cpu(), db, c["range"])
    with pytest.raises(ValueError, match=r"scene_points \(599, 4\) must be a contiguous \(600, 4\)"):
        ops.batch_prep_stage1(pl, scene[:-1], db, c["range"])
    with pytest.raises(ValueError, match="db_points"):
        ops.batch_prep_stage1(pl, scene, db[:, :3].contiguous(), c["range"])
    with pytest.raises(ValueError, match="6 numbers"):
        ops.batch_prep_stage1(pl, scene, db, c["range"][:5])
    with pytest.raises(ValueError, match="min_num_corners"):
        ops.batch_prep_stage1(pl, scene, db, c["range"], min_num_corners=9)
    with pytest.raises(Exception, match="outside the database points"):
        ops.batch_prep_stage1(pl, scene, db[:10].contiguous(), c["range"])
    with pytest.raises(ValueError, match="pinned int32"):
        ops.batch_prep_stage1(pl, scene, db, c["range"], table=torch.zeros(64, dtype=torch.int32))


def test_no_samples_and_no_rows():
    c = cases.case("collisions")
    db = dev_of(c["db_points"])
    pl = ops.batch_prep_plan([], c["db_offsets"], 4, c["steps"], True)
    st, _ = ops.batch_prep_stage1(pl, torch.zeros((0, 4), device=DEV), db, c["range"])
    assert st.table.shape == (0, 5) and tuple(st.points.shape) == (0, 5) and tuple(st.gt_boxes.shape) == (0, 0, 8)
    empty = {"n_points": 0, "gt_boxes": np.zeros((0, 7), np.float32), "gt_classes": np.zeros(0, int), "flip_x": 1, "flip_y": 0, "cos": 1.0,
             "sin": 0.0, "angle": 0.0, "scale": 1.0}
    pl = ops.batch_prep_plan([empty, empty], c["db_offsets"], 4, c["steps"], True)
    st, _ = ops.batch_prep_stage1(pl, torch.zeros((0, 4), device=DEV), db, c["range"])
    assert not st.table.any() and st.table.shape == (2, 5)


@pytest.fixture(scope="module")
def workload():
    c = cases.workload()
    return c, seq.stage1(c), inputs(c)


def test_workload_size_twice_with_equal_bits(workload):
    """B = 4 x 120 000 points with 30 gts and 40 candidates, PointRCNN's order at 16 384 points"""
    c, want, (pl, scene, db) = workload
    st = run(c, pl, scene, db)
    check_stage1(c, st, want)
    picks, rows = ops.batch_prep_order_draws(st.table, 16384, True, np.random.RandomState(1))
    got, _ = ops.batch_prep_order(st, picks)
    ref = seq.order_rows(want, [("sample_points", 16384), ("shuffle_points",)], np.random.RandomState(1))
    assert rows.tolist() == [16384] * 4 and seq.same_bits(got.cpu().numpy(), seq.batch(c, want, ref)[0])
    first = (st.points.clone(), st.lists.clone(), st.gt_boxes.clone(), st.valid.clone(), st.table.copy(), got.clone())
    st2 = run(c, pl, scene, db)
    got2, _ = ops.batch_prep_order(st2, picks)
    n = int(st.table[:, 0].sum())
    assert torch.equal(first[0][:n].view(torch.int32), st2.points[:n].view(torch.int32)) and torch.equal(first[1][:n], st2.lists[:n])
    assert torch.equal(first[2].view(torch.int32), st2.gt_boxes.view(torch.int32)) and torch.equal(first[3], st2.valid)
    assert np.array_equal(first[4], st2.table) and torch.equal(first[5].view(torch.int32), got2.view(torch.int32))


def torch_reported_syncs(fn):
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    return sum("called a synchronizing" in str(w.message) for w in seen)


def test_one_synchronising_call_per_batch(monkeypatch):
    """PyTorch waits nowhere (sync debug mode reports none, with reused workspace, table and staging buffers): the batch's one
    host wait is the library's stream synchronise at the end of stage 1, counted around the library call"""
    c = cases.case("far")
    pl, scene, db = inputs(c)
    kw = dict(remove_extra_width=c["extra"], want_near=True)
    st, stg = ops.batch_prep_stage1(pl, scene, db, c["range"], **kw)
    table = torch.zeros((64,), dtype=torch.int32).pin_memory()
    picks, _ = ops.batch_prep_order_draws(st.table, 400, True, np.random.RandomState(0))
    _, stg2 = ops.batch_prep_order(st, picks)
    out = (st.points, st.lists, st.gt_boxes, st.valid)
    calls = []
    lib = ops.load()
    inner1, inner2 = lib.modest_batch_prep_stage1, lib.modest_batch_prep_order

    class Lib:
        def __getattr__(self, name):
            return getattr(lib, name)

        def modest_batch_prep_stage1(self, *a):
            calls.append("stage1")
            return inner1(*a)

        def modest_batch_prep_order(self, *a):
            calls.append("order")
            return inner2(*a)

    monkeypatch.setattr(ops, "load", lambda: Lib())

    def batch():
        s, _ = ops.batch_prep_stage1(pl, scene, db, c["range"], workspace=st.workspace, table=table, staging=stg, out=out, **kw)
        p, _ = ops.batch_prep_order_draws(s.table, 400, True, np.random.RandomState(0))
        ops.batch_prep_order(s, p, staging=stg2)

    assert torch_reported_syncs(batch) == 0
    assert calls == ["stage1", "order"]          # stage 1 blocks once, the gather only enqueues


def test_on_a_side_stream():
    c, want = cases.case("collisions"), cases.want("collisions")
    pl, scene, db = inputs(c)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        st = run(c, pl, scene, db)
    side.synchronize()
    check_stage1(c, st, want)


# ------------------------------------------------------------------------------------------------------------ the module
from modest_amd.utils import batch_prep as bp  # noqa: E402


def module_want(cfg, root, raw, seed):
    """the restatement fed by the module's own host plan (tests/test_batch_prep_cpu.py holds that plan to the reference's sampler
    and draws) on a twin database with the same generator -> (case, stage, rows)"""
    twin = bp.BatchPrepOnDevice(cfg, cases.CLASS_NAMES, root,
                                database=bp.GtDatabaseOnDevice(root, cfg["DATA_AUGMENTOR"]["AUG_CONFIG_LIST"][0], cases.CLASS_NAMES, device="cpu"))
    rs = np.random.RandomState(seed)
    samples = []
    for b in range(raw["batch_size"]):
        r = {k: raw[k][b] for k in ("points", "gt_boxes", "gt_classes", "gt_names", "road_plane", "V2C", "R0")}
        samples.append(dict(twin.plan_sample(r, rs), points=raw["points"][b]))
    c = {"F": 4, "range": twin.range, "extra": np.asarray(twin.extra, np.float32), "road_plane": twin.road_plane, "steps": twin.steps,
         "want_near": twin.num_points is not None, "remove_outside": twin.remove_outside, "min_corners": twin.min_corners,
         "db_points": twin.database.points.numpy(), "db_offsets": twin.database.offsets, "samples": samples}
    stage = seq.stage1(c)
    procs = ([("sample_points", twin.num_points)] if twin.num_points is not None else []) + ([("shuffle_points",)] if twin.shuffle else [])
    return c, stage, seq.order_rows(stage, procs[::-1] if twin.shuffle_first else procs, rs)


@pytest.mark.parametrize("kind", ["pointrcnn", "shuffle first", "pillars", "limit whole scene, narrow scale, both flips"])
def test_the_module_end_to_end(tmp_path, kind):
    cases.write_database(str(tmp_path))
    cfg = cases.dataset_cfg("pointrcnn", True, (1.0, 1.0005), ("y", "x")) if kind.startswith("limit") else cases.dataset_cfg(kind)
    raw = cases.raw_batch()
    prep = bp.BatchPrepOnDevice(cfg, cases.CLASS_NAMES, tmp_path)
    assert ("scaling" in prep.steps) == (not kind.startswith("limit"))
    c, stage, rows = module_want(cfg, tmp_path, raw, 6)
    for _ in range(2):                                       # the second batch reuses the workspace, the table and the staging
        prep.database.sample_groups = bp.GtDatabaseOnDevice(tmp_path, prep.sampler_cfg, cases.CLASS_NAMES, device="cpu").sample_groups
        out = prep(dict(raw), np.random.RandomState(6))
        pts, gt = seq.batch(c, stage, rows)
        assert seq.same_bits(out["points"].cpu().numpy(), pts) and seq.same_bits(out["gt_boxes"].cpu().numpy(), gt)
        assert out["batch_size"] == 3 and out["frame_id"].tolist() == raw["frame_id"].tolist() and "raw_batch" not in out
        assert out["empty_samples"] == [b for b, st in enumerate(stage) if len(st["gt"]) == 0]
        assert out["batch_prep_table"][:, 3].tolist() == [int(st["valid"].sum()) for st in stage]
        assert out["batch_prep_table"][:, 4].tolist() == [int((~st["valid"]).sum()) for st in stage]
        assert prep.shuffle_first == (kind == "shuffle first")
    if kind == "pillars":
        from modest_amd.utils.spconv_utils import VoxelGenerator
        p = cfg["DATA_PROCESSOR"][-1]
        gen = VoxelGenerator(p["VOXEL_SIZE"], cfg["POINT_CLOUD_RANGE"], p["MAX_POINTS_PER_VOXEL"], p["MAX_NUMBER_OF_VOXELS"]["train"])
        vox, coords, num = [], [], []
        for b in range(3):
            v = gen.generate(pts[pts[:, 0] == b][:, 1:])
            vox.append(v["voxels"])
            num.append(v["num_points_per_voxel"])
            coords.append(np.pad(v["coordinates"], ((0, 0), (1, 0)), mode="constant", constant_values=b))
        assert seq.same_bits(out["voxels"].cpu().numpy(), np.concatenate(vox))
        assert np.array_equal(out["voxel_coords"].cpu().numpy(), np.concatenate(coords).astype(np.float32))
        assert np.array_equal(out["voxel_num_points"].cpu().numpy(), np.concatenate(num).astype(np.float32))
    else:
        assert (out["batch_prep_table"][:, 0] > 0).all() and out["points"].shape[0] == 3 * 512


@pytest.mark.parametrize("k", range(len(cases.golden()[1]["scenes"])))
def test_the_module_against_the_recording_of_the_reference_s_classes(tmp_path, k):
    """every recorded scene, sample by sample on one generator as the reference draws: no row left out.  Number and order of the
    points, z, the features, box z / dx / dy / dz, heading and class bit for bit; x and y within twice the rotation bound"""
    m, raws, recs = cases.golden_samples(k)
    want = cases.restate_scene(k, tmp_path)                 # (writes the scene's database under tmp_path)
    prep = bp.BatchPrepOnDevice(m["cfg"], cases.CLASS_NAMES, tmp_path)
    rs = np.random.RandomState(m["seed"])
    for raw, (rp, rg), (wp, wg, st, rows) in zip(raws, recs, want):
        out = prep(dict(raw), rs)
        pts, gt = out["points"].cpu().numpy(), out["gt_boxes"].cpu().numpy()
        assert (pts[:, 0] == 0).all() and gt.shape[0] == 1
        assert seq.same_bits(pts[:, 1:], wp) and seq.same_bits(gt[0], wg)
        assert cases.within_contract(pts[:, 1:], gt[0], rp, rg, st, rows), m["name"]


@pytest.mark.parametrize("kind", ["pointrcnn", "shuffle first"])
def test_the_module_waits_once_per_batch(tmp_path, monkeypatch, kind):
    """BatchPrepOnDevice.__call__ itself under the sync debug mode, warm (its pinned scan rows, pinned table, staging buffers and
    workspace exist): PyTorch reports no synchronising call, and the library is entered twice, of which stage 1 alone blocks"""
    cases.write_database(str(tmp_path))
    prep = bp.BatchPrepOnDevice(cases.dataset_cfg(kind), cases.CLASS_NAMES, tmp_path)
    raw = cases.raw_batch()
    prep(dict(raw), np.random.RandomState(1))
    table, scan, ws = prep._table, prep._scan, prep._workspace
    assert table is not None and table.is_pinned() and scan.is_pinned()
    calls, lib = [], ops.load()

    class Lib:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name in ("modest_batch_prep_stage1", "modest_batch_prep_order"):
                return lambda *a: (calls.append(name), fn(*a))[1]
            return fn

    monkeypatch.setattr(ops, "load", lambda: Lib())
    assert torch_reported_syncs(lambda: prep(dict(raw), np.random.RandomState(2))) == 0
    assert calls == ["modest_batch_prep_stage1", "modest_batch_prep_order"]
    assert prep._table is table and prep._scan is scan and prep._workspace is ws       # kept from batch to batch

