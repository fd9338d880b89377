"""CPU: the host half of training-batch preparation (ops.batch_prep_plan, ops.batch_prep_order_draws), the restatement
(tests/batch_prep_seq.py) on the hand-built cases, the refusals and the C ABI.  No GPU."""
import json
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import batch_prep_cases as cases  # noqa: E402
import batch_prep_seq as seq  # noqa: E402
from modest_amd import _lib, build, kitti_infos, ops  # noqa: E402

F32 = np.float32


def plan_of(c):
    return ops.batch_prep_plan(c["samples"], c["db_offsets"], c["F"], c["steps"], c["road_plane"])


# ------------------------------------------------------------------------------------------------------- the restatement
def test_fmaf_is_the_exact_fused_product():
    rng = np.random.default_rng(0)
    a, b, c = (rng.standard_normal(4000).astype(F32) * F32(10.0 ** rng.integers(-3, 4)) for _ in range(3))
    got = seq.fmaf(a, b, c)
    for x, y, z, g in zip(a, b, c, got):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo, hi = np.nextafter(g, F32(-np.inf)), np.nextafter(g, F32(np.inf))
        assert abs(Fraction(float(g)) - exact) <= abs(Fraction(float(lo)) - exact)
        assert abs(Fraction(float(g)) - exact) <= abs(Fraction(float(hi)) - exact)
    # a tie that is one: x x = 2^-24, so 1 + 2^-24 exactly, and it goes to even
    x = np.array([2.0 ** -12], F32)
    assert seq.fmaf(x, x, np.array([1.0], F32))[0] == F32(1.0)
    # a tie that is none: (1 + 2^-23)(1 - 2^-23) 2^-24 = 2^-24 - 2^-70, and c = 1 + 2^-23 has an odd last bit.  The float64 sum
    # is the midpoint c + 2^-24, which would go to even, 1 + 2^-22; the exact sum lies below it and goes to c
    a1, b1, c1 = F32(1 + 2.0 ** -23), F32((1 - 2.0 ** -23) * 2.0 ** -24), F32(1 + 2.0 ** -23)
    assert (np.float64(a1) * np.float64(b1) + np.float64(c1)).astype(F32) == F32(1 + 2.0 ** -22)       # rounding twice is wrong
    assert seq.fmaf([a1, -a1], [b1, b1], [c1, -c1]).tolist() == [c1, -c1]


def test_the_box_predicate_is_the_one_points_in_boxes_cpu_decides():
    rng = np.random.default_rng(1)
    bx = cases.boxes(rng, 12, spread=10.0)
    pts = cases.scene(rng, 3000, spread=12.0)[:, :3]
    want = kitti_infos.points_in_boxes_host(pts, bx).any(axis=0)
    assert want.sum() > 20
    assert np.array_equal(seq.in_boxes(pts, bx, seq.host_trig(bx[:, 6])[:, 2:4]), want)


def test_faces_of_the_range_and_of_a_box():
    c, (w, gone) = cases.case("faces"), cases.want("faces")
    assert w["valid"].tolist() == [True] and len(gone["points"]) == 0
    kept = set(w["points"][:, 3].astype(int).tolist())
    r = c["range"]
    # rows 0-7: on a face, one step outside, per face; 8: the x1 / y1 corner; 9-14: NaN and infinities (z alone may be anything)
    assert kept & set(range(15)) == {0, 2, 4, 6, 8, 11, 14}
    assert w["points"][[i for i, v in enumerate(w["points"][:, 3]) if v == 0][0], 0] == r[0]
    # the box: on +-tx / +-ty the point is outside the box (kept), one step inside it is removed; on +-tz inside, one step above outside
    box_rows = np.arange(15, 27).reshape(2, 6)
    for row in box_rows:
        assert [int(i) in kept for i in row] == [True, False, True, False, False, True]
    n_obj = int(np.diff(c["db_offsets"])[3])
    assert len(w["points"]) == n_obj + 7 + 6 and not w["near"][[i for i, v in enumerate(w["points"][:, 3]) if v == 8][0]]


def test_collisions_are_the_sampler_s():
    w = cases.want("collisions")
    # 0, 1 overlap each other; 2 touches a gt (the clipped polygon has no area); 3 free; 4 on the kept 3; 5 on the dropped 0;
    # 6 on a gt of another name; 7 zero size; 8 free
    assert w[0]["valid"].tolist() == [False, False, True, True, False, True, False, True, True]
    cls = w[0]["gt"][:, 7].astype(int).tolist()
    assert cls == [1, 2, 1, 3, 1, 1, 1, 2, 2]       # the gts of a known name in order, then the kept candidates of a known class
    assert len(w[1]["gt"]) == int(w[1]["valid"].sum()) and 0 < w[1]["valid"].sum() < 6       # no gts: candidates against candidates
    assert w[2]["valid"].tolist() == [True]
    h = w[0]["gt"][:, 6]
    assert (h >= -np.pi - 1e-6).all() and (h <= np.pi + 1e-6).all()


def test_corner_counts():
    c = cases.case("corners min 1")
    n = seq.corners_inside(np.concatenate([c["samples"][0]["gt_boxes"][:, :6], seq.limit_period(c["samples"][0]["gt_boxes"][:, 6:7])], axis=1),
                           c["range"])
    assert n.tolist() == [8, 4, 3, 0]
    assert len(cases.want("corners min 1")[0]["gt"]) == 3 and len(cases.want("corners min 4")[0]["gt"]) == 2


# ------------------------------------------------------------------------------------------------------------ stage 2
def resolve(picks, rows, stage, perm=None):
    """the survivor each pick names, per sample, through the near / far lists the device would hold; with `perm` the places
    and the lists are those of the shuffled sample, as bp_shuffled_lists rebuilds them"""
    out, at, pa = [], 0, 0
    for b, st in enumerate(stage):
        p = picks[at:at + rows[b]]
        at += rows[b]
        assert (p[:, 0] >> 2 == b).all()
        k = len(st["points"])
        order = np.arange(k) if perm is None else perm[pa:pa + k]
        pa += k
        flags = st["near"][order]
        near, far = np.where(flags)[0], np.where(~flags)[0]
        lid, pos = p[:, 0] & 3, p[:, 1]
        place = np.where(lid == 0, pos, np.where(lid == 1, near[np.minimum(pos, max(len(near) - 1, 0))] if len(near) else 0,
                                                 far[np.minimum(pos, max(len(far) - 1, 0))] if len(far) else 0))
        out.append(order[place])
    assert at == len(picks)
    return out


def table_of(stage):
    return np.array([[len(st["points"]), int((~st["near"]).sum()), len(st["gt"]), int(st["valid"].sum()), int((~st["valid"]).sum())]
                     for st in stage], np.int32)


@pytest.mark.parametrize("name", list(cases.ORDERS))
def test_order_draws_are_the_reference_s_on_row_numbers(name):
    procs, num, shuffle, *first = cases.ORDERS[name]
    stage = cases.want("far")
    tab = table_of(stage)
    k, far = tab[:, 0], tab[:, 1]
    if num == 400:     # the three branches: the near points are drawn, all points are drawn, the loop pads in three rounds
        assert far[0] < 400 < k[0] and 400 <= far[1] and 3 * k[2] < 400 <= 4 * k[2]
    picks, rows, *perm = ops.batch_prep_order_draws(tab, num, shuffle, np.random.RandomState(5), *first)
    assert len(perm) == len(first) and all(len(p) == k.sum() and p.dtype == np.int32 for p in perm)
    want = seq.order_rows(stage, procs, np.random.RandomState(5))
    got = resolve(picks, rows, stage, *perm)
    assert [len(g) for g in got] == [len(w) for w in want]
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_order_draws_with_as_many_points_as_asked_for_and_on_the_global_generator():
    stage = cases.want("far")
    tab = table_of(stage)
    n = int(tab[2, 0])
    np.random.seed(9)
    picks, rows = ops.batch_prep_order_draws(tab[2:], n, True)
    np.random.seed(9)
    want = seq.order_rows(stage[2:], [("sample_points", n), ("shuffle_points",)], np.random)
    assert rows.tolist() == [n] and np.array_equal(resolve(picks, rows, stage[2:])[0], want[0])
    with pytest.raises(ValueError, match="without points"):
        ops.batch_prep_order_draws(np.zeros((1, 5), np.int32), 16, False)


# ------------------------------------------------------------------------------------------------- the plan and refusals
def test_plan_tables():
    c = cases.case("sizes")
    pl = plan_of(c)
    tile = ops.batch_prep_tile()
    assert pl.B == 10 and pl.n_scene == sum(len(s["points"]) for s in c["samples"]) and pl.gt_capacity == 11
    rows = pl.samp[:, 1] + pl.samp[:, 3]
    assert np.array_equal(pl.samp[:, 0], np.concatenate([[0], np.cumsum(rows)[:-1]])) and pl.n_rows == rows.sum()
    assert np.array_equal(pl.samp[:, 8], np.concatenate([[0], np.cumsum(-(-rows // tile))[:-1]]))
    assert pl.samp[0, 1] == 0 and pl.samp[1, 1] > 0 and (pl.samp[1, 1] + 1) % tile != 0          # the seam lies inside a tile
    assert pl.boxes.shape == (pl.n_boxes, 12) and pl.cand.shape == (pl.n_cand, 3) and pl.steps.tolist() == [1, 2, 3, 4]
    assert seq.same_bits(pl.boxes[:, 7:11], seq.host_trig(pl.boxes[:, 6]))
    assert ops.batch_prep_max_boxes() == 512 and tile == cases.TILE


def test_limits_and_what_is_not_provided():
    ok = cases.case("limit")
    assert plan_of(ok).gt_capacity == 512
    with pytest.raises(ValueError, match="313 gts plus 200 candidates are above the limit of 512"):
        plan_of(cases._limit(513))
    c = cases.case("collisions")
    s0 = dict(c["samples"][0])
    with pytest.raises(NotImplementedError, match="velocity"):
        ops.batch_prep_plan([dict(s0, gt_boxes=np.zeros((2, 9), F32), gt_classes=[1, 1])], c["db_offsets"], 4, c["steps"], True)
    for f in (3, 9):
        with pytest.raises(ValueError, match="4 to 8 point features"):
            ops.batch_prep_plan([s0], c["db_offsets"], f, c["steps"], True)
    with pytest.raises(NotImplementedError, match="random_image_flip"):
        ops.batch_prep_plan([s0], c["db_offsets"], 4, ["random_image_flip"], True)
    with pytest.raises(NotImplementedError, match="twice"):
        ops.batch_prep_plan([s0], c["db_offsets"], 4, ["rotation", "rotation"], True)
    with pytest.raises(ValueError, match="cand_objects outside"):
        ops.batch_prep_plan([dict(s0, cand_objects=np.full(9, 20))], c["db_offsets"], 4, c["steps"], True)
    with pytest.raises(ValueError, match="above the limit of 65535"):
        ops.batch_prep_plan([None] * 65536, c["db_offsets"], 4, (), False)
    with pytest.raises(_lib.ModestHipError, match="batch_size <= 65535"):
        ops.batch_prep_workspace_bytes(10, 65536)
    with pytest.raises(_lib.ModestHipError, match="n_rows <= 2147483647"):
        ops.batch_prep_workspace_bytes(2 ** 31, 1)
    assert ops.batch_prep_workspace_bytes(0, 0) > 0


def test_the_library_refuses_tables_that_point_outside_before_any_launch():
    """modest_batch_prep_stage1 checks the host tables first and fails on a NULL device pointer only after them: with no GPU
    a table that passes reaches the NULL check, one that does not is named"""
    c = cases.case("collisions")
    pl = plan_of(c)
    lib = _lib.load()
    rng, extra = np.asarray(c["range"], F32).copy(), np.asarray(c["extra"], F32).copy()

    def call(samp, cand, n_db=10 ** 6, n_scene=None, features=4, steps=pl.steps):
        fake = 4096         # never dereferenced: every call below is refused
        return lib.modest_batch_prep_stage1(pl.B, features, pl.n_scene if n_scene is None else n_scene, fake, n_db, fake, samp.ctypes.data,
                                            fake, pl.n_boxes, fake, pl.n_cand, cand.ctypes.data, fake, fake, fake, fake, len(steps),
                                            steps.ctypes.data, rng.ctypes.data, extra.ctypes.data, 1, 1, 1, 1, pl.n_rows, fake, fake, fake,
                                            fake, pl.gt_capacity, None, fake, 0, None)

    def refused(**kw):
        rc = call(kw.pop("samp", pl.samp), kw.pop("cand", pl.cand), **kw)
        assert rc != 0
        return lib.modest_last_error().decode()

    assert "NULL table" in refused()                      # the tables themselves pass
    bad = pl.samp.copy(); bad[2, 3] += 1
    assert "scene rows outside" in refused(samp=bad)
    bad = pl.samp.copy(); bad[1, 0] += 1
    assert "must follow one another" in refused(samp=bad)
    bad = pl.cand.copy(); bad[2, 1] += 1
    assert "object rows" in refused(cand=bad)
    assert "outside the database points" in refused(n_db=10)
    assert "4 to 8 point features" in refused(features=9)
    assert "augmentor steps are" in refused(steps=np.array([5], np.int32))
    bad = pl.samp.copy(); bad[0, 5] = 600
    assert "at most modest_batch_prep_max_boxes() = 512" in refused(samp=bad)


def test_abi_and_kernel_resources():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "modest_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for fn in ("modest_batch_prep_max_boxes", "modest_batch_prep_tile", "modest_batch_prep_table_words", "modest_batch_prep_workspace_bytes",
               "modest_batch_prep_stage1", "modest_batch_prep_order"):
        m = re.search(r"\b" + fn + r"\s*\(([^;]*)\)\s*;", src)
        assert m and hasattr(lib, fn), fn
        args = [a for a in m.group(1).split(",") if a.strip() != "void"]
        assert len(args) == len(_lib.SIGNATURES[fn][1]), fn
    assert lib.modest_batch_prep_table_words() == 6 == len(ops.BATCH_PREP_TABLE) + 1
    res = json.load(open(os.path.join(os.path.dirname(build.LIB), "kernel_resources.json")))
    mine = {k: v for k, v in res.items() if v["file"] == "batch_prep.hip"}
    assert len(mine) == 6 and all(v["ScratchSize [bytes/lane]"] == 0 for v in mine.values()), mine
    assert max(v["LDS Size [bytes/block]"] for v in mine.values()) <= 160 * 1024


# ------------------------------------------------------------------------------------------------------------ the module
from modest_amd.utils import batch_prep as bp  # noqa: E402


def reference_sampler(infos, cfg, class_names, gt_names_per_sample, rs):
    """database_sampler.py:10-96, 183-190 on lists, as the reference keeps them -> per sample [(class, info), ...]"""
    db = {c: list(infos[c]) for c in class_names}
    for name_num in cfg["PREPARE"]["filter_by_min_points"]:
        name, m = name_num.split(":")
        if int(m) > 0 and name in db:
            db[name] = [i for i in db[name] if i["num_points_in_gt"] >= int(m)]
    db = {k: [i for i in v if i["difficulty"] not in cfg["PREPARE"]["filter_by_difficulty"]] for k, v in db.items()}
    groups, num = {}, {}
    for x in cfg["SAMPLE_GROUPS"]:
        name, n = x.split(":")
        if name not in class_names:
            continue
        num[name] = n
        groups[name] = {"sample_num": n, "pointer": len(db[name]), "indices": np.arange(len(db[name]))}
    out = []
    for gt_names in gt_names_per_sample:
        got = []
        for name, g in groups.items():
            if cfg["LIMIT_WHOLE_SCENE"]:
                g["sample_num"] = str(int(num[name]) - np.sum(name == gt_names))
            if int(g["sample_num"]) > 0:
                sample_num, pointer, indices = int(g["sample_num"]), g["pointer"], g["indices"]
                if pointer >= len(db[name]):
                    indices = rs.permutation(len(db[name]))
                    pointer = 0
                got += [(name, db[name][idx]) for idx in indices[pointer: pointer + sample_num]]
                g["pointer"], g["indices"] = pointer + sample_num, indices
        out.append(got)
    return out


@pytest.mark.parametrize("limit", [False, True])
def test_the_sampler_state_machine(tmp_path, limit):
    """the pointer runs out in mid-sample (a slice that comes up short), and Pedestrian has fewer objects than its sample_num"""
    infos = cases.write_database(str(tmp_path))
    cfg = cases.dataset_cfg(limit_whole_scene=limit)["DATA_AUGMENTOR"]["AUG_CONFIG_LIST"][0]
    db = bp.GtDatabaseOnDevice(tmp_path, cfg, cases.CLASS_NAMES, device="cpu")
    assert list(db.sample_groups) == ["Car", "Pedestrian", "Cyclist"] and db.features == 4
    assert len(db.db_infos["Pedestrian"]) < 4
    names = [np.array(["Car", "Van", "Car"]), np.array([], str), np.array(["Cyclist"] * 4 + ["Car"]), np.array(["Pedestrian"])] * 3
    want = reference_sampler(infos, cfg, cases.CLASS_NAMES, names, np.random.RandomState(4))
    rs = np.random.RandomState(4)
    short = 0
    for gt_names, w in zip(names, want):
        c = db.candidates(gt_names, rs)
        assert len(c["cand_boxes"]) == len(w)
        for j, (name, info) in enumerate(w):
            o = int(c["cand_objects"][j])
            pts = np.fromfile(str(tmp_path / info["path"]), np.float32).reshape(-1, 4)
            assert np.array_equal(db.points[db.offsets[o]:db.offsets[o + 1]].numpy(), pts)
            assert np.array_equal(c["cand_boxes"][j], info["box3d_lidar"].astype(np.float32))
            assert c["cand_classes"][j] == cases.CLASS_NAMES.index(name) + 1
        assert (np.diff(c["cand_groups"]) >= 0).all()
        for name, asked in (("Car", 5), ("Pedestrian", 4), ("Cyclist", 4)):
            asked -= int(np.sum(gt_names == name)) if limit else 0
            short += 0 < sum(n == name for n, _ in w) < asked
    assert short > 0                         # a slice came up short at the end of the class's list


def test_road_plane_rows_do_not_depend_on_the_other_rows():
    rng = np.random.default_rng(5)
    bx = cases.boxes(rng, 40)
    plane = np.array([0.01, -0.999, 0.02, 1.65])
    z, mv = bp.put_boxes_on_road_planes(bx, plane, cases.V2C, cases.R0)
    assert z.dtype == np.float32 and mv.dtype == np.float64
    for rows in ([0], [3, 4], list(range(7)), list(range(5, 40))):
        z1, mv1 = bp.put_boxes_on_road_planes(bx[rows], plane, cases.V2C, cases.R0)
        assert np.array_equal(z1, z[rows]) and np.array_equal(mv1, mv[rows])
    assert np.array_equal(z, (bx[:, 2].astype(np.float64) - mv).astype(np.float32))


def test_what_the_module_does_not_provide():
    ok = cases.dataset_cfg()
    with pytest.raises(NotImplementedError, match="test mode"):
        bp.BatchPrepOnDevice(ok, cases.CLASS_NAMES, ".", training=False)

    def aug(extra=None, **sampler):
        c = cases.dataset_cfg()
        c["DATA_AUGMENTOR"]["AUG_CONFIG_LIST"][0].update(sampler)
        if extra:
            c["DATA_AUGMENTOR"]["AUG_CONFIG_LIST"].append(extra)
        return c

    for name in ("random_image_flip", "point_quantize", "random_local_rotation"):
        with pytest.raises(NotImplementedError, match=name):
            bp.BatchPrepOnDevice(aug({"NAME": name}), cases.CLASS_NAMES, ".")
    c = cases.dataset_cfg()
    c["DATA_AUGMENTOR"]["AUG_CONFIG_LIST"].reverse()
    with pytest.raises(NotImplementedError, match="gt_sampling anywhere but first"):
        bp.BatchPrepOnDevice(c, cases.CLASS_NAMES, ".")
    c = cases.dataset_cfg()
    c["DATA_PROCESSOR"].append({"NAME": "downsample_depth_map"})
    with pytest.raises(NotImplementedError, match="downsample_depth_map"):
        bp.BatchPrepOnDevice(c, cases.CLASS_NAMES, ".")
    c = cases.dataset_cfg()
    c["POINT_FEATURE_ENCODING"]["used_feature_list"] = ["intensity", "x", "y", "z"]
    with pytest.raises(NotImplementedError, match="use_lead_xyz"):
        bp.BatchPrepOnDevice(c, cases.CLASS_NAMES, ".")
    for flag in ("DATABASE_WITH_FAKELIDAR", "DEBUG"):
        with pytest.raises(NotImplementedError, match=flag):
            bp.GtDatabaseOnDevice(".", aug(**{flag: True})["DATA_AUGMENTOR"]["AUG_CONFIG_LIST"][0], cases.CLASS_NAMES, device="cpu")


def test_the_binder_sets_and_restores_exactly_three_attributes():
    import types

    class DatasetTemplate:
        training = True

        def prepare_data(self, data_dict):
            return "theirs"

        @staticmethod
        def collate_batch(batch_list, _unused=False):
            return "their batch"

    models = types.ModuleType("models")
    models.load_data_to_gpu = lambda batch_dict: batch_dict.update(loaded=True)
    models.other = object()
    before_cls, before_mod = dict(vars(DatasetTemplate)), dict(vars(models))
    bp.bind(DatasetTemplate, models)
    bp.bind(DatasetTemplate, models)                         # idempotent
    changed = {k for k, v in vars(DatasetTemplate).items() if before_cls.get(k) is not v}
    assert changed == {"prepare_data", "collate_batch", "_modest_prepare_data", "_modest_collate_batch"}
    assert {k for k, v in vars(models).items() if before_mod.get(k) is not v} == {"load_data_to_gpu"}
    ds = DatasetTemplate()
    ds.training = False
    assert ds.prepare_data({}) == "theirs" and DatasetTemplate.collate_batch([{"points": 1}]) == "their batch"
    d = {"points": np.zeros((2, 5))}
    models.load_data_to_gpu(d)
    assert d["loaded"]                                       # a batch that is not raw goes to the original
    with pytest.raises(RuntimeError, match="load_data_to_gpu.dataset"):
        models.load_data_to_gpu({"raw_batch": True})
    raw = DatasetTemplate.collate_batch([{"points": np.zeros((3, 4)), "gt_classes": np.zeros(0), "frame_id": "7"}] * 2)
    assert raw["raw_batch"] and raw["batch_size"] == 2 and len(raw["points"]) == 2 and raw["frame_id"].tolist() == ["7", "7"]
    bp.unbind(DatasetTemplate, models)
    assert dict(vars(DatasetTemplate)) == before_cls and dict(vars(models)) == before_mod
    from modest_amd.utils import pcdet_bind
    assert callable(pcdet_bind.bind_batch_prep)


# ------------------------------------------------------------------------ against the recording of the reference's classes
@pytest.mark.parametrize("k", range(len(cases.golden()[1]["scenes"])))
def test_the_restatement_reproduces_the_recording_from_the_seeds(tmp_path, k):
    """the draw order of B = 1 (and of B = 3 run sample by sample) is the reference's: one wrong draw anywhere changes the
    sampler's slots, the flip, the angle or the order of the points"""
    m, _, recs = cases.golden_samples(k)
    got = cases.restate_scene(k, tmp_path)
    assert len(got) == m["B"]
    kept = [(int(st["valid"].sum()), int((~st["valid"]).sum())) for _, _, st, _ in got]
    if m["name"].startswith("two class groups"):
        # with the gt: the Car on it goes, the Pedestrian on the kept Car goes, the one on the dropped Car stays; without gts
        # (iou1 = iou2) both Cars stay and both Pedestrians go
        assert [st["valid"].sum() for _, _, st, _ in got] == [3, 3] and kept == [(3, 2), (3, 2)]
        assert sorted(got[0][2]["gt"][:, 7].astype(int).tolist()) == [1, 1, 2, 3] and sorted(got[1][2]["gt"][:, 7].astype(int).tolist()) == [1, 1, 3]
    if m["name"].startswith("LIMIT_WHOLE_SCENE leaves nothing"):
        assert kept[0] == (0, 0) and kept[1][0] > 0
    if m["name"].startswith("NUM_POINTS equal"):
        assert len(got[0][2]["points"]) == len(recs[0][0])
    if m["name"].startswith("NUM_POINTS above twice"):
        assert 2 * len(got[0][2]["points"]) < len(recs[0][0]) < 3 * len(got[0][2]["points"])
    for (p, g, st, rows), (rp, rg) in zip(got, recs):
        assert len(rp) > 100 and len(rg) > 0
        print(m["name"], "error over bound: restatement", cases.error_over_bound(p, g, st, rows), "recording",
              cases.error_over_bound(rp, rg, st, rows) if rp.shape == p.shape and rg.shape == g.shape else None)
        assert cases.within_contract(p, g, rp, rg, st, rows), m["name"]


def test_the_recording_holds_the_tool_s_margins():
    """the tool's own assertions (tools/make_golden_batch_prep.py: margins_ok -- the x / y faces, the 40 m sphere, the box
    corners -- and pairs_ok, the candidates' pairwise overlaps) re-checked on the committed fixture"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_golden_batch_prep as tool
    g, meta = cases.golden()
    assert [s["name"] for s in meta["scenes"]] == [name for name, *_ in tool.scenes()]
    assert os.path.getsize(cases.GOLD) < 512 * 1024
    assert meta["draws"]["rejected"] * 4 <= meta["draws"]["total"]
    for k, s in enumerate(meta["scenes"]):
        for b in range(s["B"]):
            rec = {"points": g[f"s{k}_{b}_out_points"], "gt_boxes": g[f"s{k}_{b}_out_gt_boxes"]}
            assert tool.margins_ok(s["cfg"], rec), (s["name"], b)
            assert tool.pairs_ok(g[f"s{k}_{b}_gt_boxes"], g[f"s{k}_{b}_cand_boxes"], g[f"s{k}_{b}_cand_groups"]), (s["name"], b)
            n = [c for c in s["cfg"]["DATA_PROCESSOR"] if c["NAME"] == "sample_points"]
            if n and n[0]["NUM_POINTS"]["train"] != -1:
                assert len(rec["points"]) == n[0]["NUM_POINTS"]["train"]
