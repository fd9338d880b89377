"""CPU: the registry of tests/post_process_cases.py has the edges it claims, on the numpy restatement
tests/post_process_seq.py of modest_amd.ops.post_process (csrc/post_process.hip): every case asserts its
edge, every named fault changes its case, the oracle's greedy walk and the kernel's chunked walk agree.  Also what can be
checked without a device so that the GPU test has to take nothing out: every sigmoid lies far from a float32 rounding
midpoint, every recall decision lies more than ten derived bounds from its threshold or is tied on purpose, torch compares
a float32 tensor with a Python scalar in float32, and the recorded fixture equals the restatement."""
import os
import types

import numpy as np
import pytest
import torch

import iou3d_cases as ic
import post_process_cases as cases
import post_process_seq as seq
import proposals_seq as ps
from modest_amd import ops

F = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "post_process.npz")
SMALL = [n for n in cases.CASES if n != "B 65535"]


def test_the_op_exists():
    assert callable(ops.post_process) and callable(ops.post_process_workspace_bytes)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_every_case_has_its_edge(name):
    c = cases.case(name)
    inf = cases.info(c) if name != "B 65535" else None
    assert c["present"](c, inf), name
    preds, recall = cases.want(c)
    assert len(preds) == c["B"] and all(g[0].shape == (len(g[1]), c["box"].shape[-1]) and g[2].dtype == np.int64 for g in preds)
    assert (recall is None) == (c["gt_boxes"] is None)
    if inf is not None:
        assert [len(g[0]) for g in preds] == [o["kept"] for o in inf]


def test_the_registry_covers_the_issue():
    inf = {n: cases.info(cases.case(n)) for n in ("pass 0", "pass 1", "pass 63", "pass 64", "pass 65", "pass 129")}
    assert [inf[n][0]["passing"] for n in inf] == [0, 1, 63, 64, 65, 129]
    empty = cases.want(cases.case("pass 0"))
    assert empty[0][0][0].shape == (0, 7) and empty[1]["gt"] == 6 and not any(empty[1]["rcnn"])      # no final box, but gts
    assert cases.TILE == ps.CHUNK == 64
    assert {cases.case(n)["score_thresh"] for n in cases.CASES} >= {None, 0.0, 0.01, 0.1, 0.7}
    assert {cases.case(n)["rotated"] for n in SMALL} == {True, False}
    assert {cases.case(n)["gt_boxes"].shape[1] for n in SMALL if cases.case(n)["gt_boxes"] is not None} >= {0, 1, 63, 64, 65, 255, 257}
    assert any(cases.case(n)["gt_boxes"] is None for n in SMALL)


@pytest.mark.parametrize("fault", list(seq.FAULTS))
def test_every_fault_changes_its_case(fault):
    c = cases.case(seq.FAULTS[fault])
    assert not seq.same(cases.want(c, fault=fault), cases.want(c)), fault


@pytest.mark.parametrize("name", SMALL)
def test_the_two_walks_agree(name):
    c = cases.case(name)
    why = seq.describe(cases.want(c, walk=ps.chunked_walk), cases.want(c))
    assert not why, "\n".join(why)


def test_torch_compares_with_a_python_scalar_in_float32():
    """0.3 as a double lies below float32(0.3): a comparison in double would say float32(0.3) > 0.3"""
    t = F(0.3)
    x = torch.tensor([np.nextafter(t, F(0)), t, np.nextafter(t, F(1))])
    assert float(t) > 0.3 and (x > 0.3).tolist() == [False, False, True] and (x >= 0.3).tolist() == [False, True, True]
    assert (x.numpy() > F(0.3)).tolist() == (x > 0.3).tolist()


def test_no_sigmoid_lies_near_a_rounding_midpoint():
    """On every non-normalised row of the registry the double sigmoid lies at least 2^-40 (relative) from the two float32
    rounding midpoints next to it, so a device exp a few double ulps off rounds to the same float32."""
    rows = worst = 0
    for name in SMALL:
        c = cases.case(name)
        if c["normalized"]:
            continue
        x = np.unique(ps.score_label(ps._flat(c["box"], c["cls"], c["batch_index"])[1])[0])
        x = x[np.isfinite(x)].astype(np.float64)
        with np.errstate(over="ignore"):
            s = 1.0 / (1.0 + np.exp(-x))
        f = s.astype(F)
        for side in (-1, 1):
            nxt = np.nextafter(f, F(side) * F(np.inf)).astype(np.float64)
            mid = (f.astype(np.float64) + nxt) / 2
            rel = np.abs(s - mid) / np.maximum(np.abs(mid), np.finfo(np.float64).tiny)
            rel = rel[(s > 0) & (mid != f)]
            worst = max(worst, float((2.0 ** -40 / rel).max())) if len(rel) else worst
            assert (rel >= 2.0 ** -40).all(), name
        rows += len(x)
    print(f"non-normalised scores of the registry: {rows}; nearest midpoint at 2^-40 / {worst:.3g} of the allowed distance")
    assert rows > 1000


def test_no_recall_decision_is_open():
    """every gt's maximum IoU is either more than ten derived bounds (tests/iou3d_cases.py: the float32 polygon walk against
    exact geometry; the boxes of the registry share z and dz, so the 3-D IoU is the BEV IoU up to the 1e-6 of the bound)
    from every threshold, or equals it exactly on purpose"""
    tied = checked = 0
    for name in SMALL:
        c = cases.case(name)
        if c["gt_boxes"] is None or not len(c["recall_thresh"]):
            continue
        preds, _ = cases.want(c)
        box = ps._flat(c["box"], c["cls"], c["batch_index"])[0]
        for b in range(c["B"]):
            gt = c["gt_boxes"][b]
            gt = gt[:seq.trim(gt)]
            lists = [preds[b][0]] if c["rois"] is None else [box.reshape(c["B"], -1, box.shape[-1])[b], c["rois"][b]]
            for boxes in lists:
                ok = np.isfinite(gt[:, :7]).all(1)
                if not len(boxes) or not ok.any():
                    continue
                g = np.ascontiguousarray(gt[ok][:, :7])
                best = seq.max_iou(boxes, g)
                ex = ic.Exact.all_pairs(np.ascontiguousarray(boxes[:, :7]), g)
                bound = ex.iou_bound.max(0)
                for t in c["recall_thresh"]:
                    d = np.abs(best.astype(np.float64) - float(F(t)))
                    exact_tie = best == F(t)
                    assert (exact_tie | (d > 10 * bound)).all(), (name, t, float(d[~exact_tie].min()), float(bound.max()))
                    tied += int(exact_tie.sum())
                    checked += len(best)
    print(f"recall decisions checked: {checked}, tied on purpose: {tied}")
    assert tied >= 1 and checked > 1000
    assert cases.case("recall tie")["tie"] in cases.case("recall tie")["recall_thresh"]


def test_the_recorded_scenes_equal_the_restatement():
    """the reference's own post_processing (tools/make_golden_post_process.py): boxes, labels, counts and the recall dict bit
    for bit, pred_scores of the non-normalised scenes within the recorded ulp distance of torch's CPU sigmoid"""
    rec = dict(np.load(GOLD))
    names = seq.scenes(rec)
    assert len(names) >= 3
    ulp = int(rec["sigmoid_ulp"])
    for name in names:
        cfg, a = seq.scene_inputs(rec, name)
        got = seq.post_process(a["box"], a["cls"], cfg["batch_size"], cfg["NMS_PRE_MAXSIZE"], cfg["NMS_POST_MAXSIZE"], cfg["NMS_THRESH"],
                               rotated=cfg["NMS_TYPE"] == "nms_gpu", score_thresh=cfg["SCORE_THRESH"], normalized=cfg["cls_preds_normalized"],
                               output_raw_score=cfg["OUTPUT_RAW_SCORE"], labels=a["labels"], batch_index=a["batch_index"],
                               gt_boxes=a["gt_boxes"], rois=a["rois"] if cfg["rois_in_batch"] else None,
                               recall_thresh=cfg["RECALL_THRESH_LIST"])
        compare_with_recorded(got, rec, name, cfg, ulp)


def compare_with_recorded(got, rec, name, cfg, ulp):
    want_preds, want_recall = seq.recorded(rec, name)
    preds, recall = got
    assert seq.recall_dict(recall, cfg["RECALL_THRESH_LIST"]) == want_recall, name
    assert list(seq.recall_dict(recall, cfg["RECALL_THRESH_LIST"])) == list(want_recall), name
    loose = not cfg["cls_preds_normalized"] and not cfg["OUTPUT_RAW_SCORE"]
    for b, (g, w) in enumerate(zip(preds, want_preds)):
        assert g[0].shape == w[0].shape and np.array_equal(seq.bits(g[0]), seq.bits(w[0])), (name, b)
        assert np.array_equal(g[2], w[2].reshape(-1)), (name, b)
        if loose:
            assert (np.abs(g[1].view(np.int32).astype(np.int64) - w[1].view(np.int32)) <= ulp).all(), (name, b)
        else:
            assert np.array_equal(seq.bits(g[1]), seq.bits(w[1])), (name, b)


# ------------------------------------------------------------------------------------------------ limits, without a device
def test_library_constants_and_limits():
    from modest_amd.utils import post_processing as pp
    lib = ops.load()
    assert ops.post_process_tile() == cases.TILE
    assert lib.modest_post_process_max_thresholds() == seq.THRESH_MAX == ops.POST_PROCESS_THRESH_MAX == pp.THRESH_MAX
    assert (pp.POST_MAX, pp.BATCH_MAX) == (seq.POST_MAX, seq.BATCH_MAX)
    assert ops.post_process_workspace_bytes(1000, 4) >= ops.proposals_workspace_bytes(1000) + 16
    assert ops.post_process_table_words(4, 3) == 4 * 8
    assert lib.modest_post_process_workspace_bytes(2 ** 31, 1) < 0 and lib.modest_post_process_workspace_bytes(8, 65536) < 0

    def call(n=8, B=1, per=8, cols=7, K=1, post=10, T=0, with_gt=0, G=0, R=-1, rcols=7, thr=None):
        return lib.modest_post_process(n, B, per, None, cols, None, K, None, 0, 1, 1, 0.1, 0, None, 100, post, 0.7, 1, with_gt, G,
                                       None, 0, 0, 0, R, None, rcols, T, thr, None, None, None, None, None, 0, None)
    thr = np.zeros(32, F)
    for kw, word in ((dict(post=1025), b"1024"), (dict(B=65536, per=0, n=0), b"65535"), (dict(n=2 ** 31, per=2 ** 31), b"2^31 - 1"),
                     (dict(cols=4097), b"4096"), (dict(K=4097), b"4096"), (dict(T=17, with_gt=1, thr=thr.ctypes.data), b"16 thresholds"),
                     (dict(with_gt=1, R=4, rcols=4097), b"4096"), (dict(R=4), b"rois without gts"),
                     (dict(with_gt=1, B=65535, per=0, n=0, G=32769), b"2^31 - 1")):
        assert call(**kw) != 0, kw
        err = lib.modest_last_error()
        assert b"requirement failed" in err and word in err, (kw, err)
    # at each limit the requirement that fails is a later one (no table: nothing is launched without a device either)
    for kw in (dict(post=1024), dict(B=65535, per=0, n=0), dict(cols=4096), dict(K=4096), dict(T=16, with_gt=1, thr=thr.ctypes.data)):
        assert call(**kw) != 0 and b"NULL table" in lib.modest_last_error(), (kw, lib.modest_last_error())


def stand_in(cfg, num_class=3):
    from modest_amd.utils import post_processing as pp
    det = pp.bind(type("Detector", (), {}))()
    det.model_cfg, det.num_class = cfg, num_class
    return det


def config(as_dict=False, **kw):
    nms = dict(MULTI_CLASSES_NMS=False, NMS_TYPE="nms_gpu", NMS_THRESH=0.1, NMS_PRE_MAXSIZE=4096, NMS_POST_MAXSIZE=500)
    nms.update({k: v for k, v in kw.items() if k in nms})
    post = dict(RECALL_THRESH_LIST=[0.3, 0.5, 0.7], SCORE_THRESH=0.1, OUTPUT_RAW_SCORE=False)
    post.update({k: v for k, v in kw.items() if k in post})
    if as_dict:
        return {"POST_PROCESSING": dict(post, NMS_CONFIG=nms)}
    return types.SimpleNamespace(POST_PROCESSING=types.SimpleNamespace(NMS_CONFIG=types.SimpleNamespace(**nms), **post))


def test_what_the_drop_in_refuses_names_itself():
    box, cls = torch.zeros((2, 8, 7)), torch.zeros((2, 8, 3))
    d = dict(batch_size=2, batch_box_preds=box, batch_cls_preds=cls, cls_preds_normalized=True)
    with pytest.raises(ValueError, match="device"):
        stand_in(config()).post_processing(dict(d))
    with pytest.raises(ValueError, match="device"):
        ops.post_process(box, cls, 2, 100, 10, 0.1)
    with pytest.raises(NotImplementedError, match="MULTI_CLASSES_NMS"):
        stand_in(config(as_dict=True, MULTI_CLASSES_NMS=True)).post_processing(dict(d))
    with pytest.raises(NotImplementedError, match="list"):
        stand_in(config()).post_processing(dict(d, batch_cls_preds=[cls]))
    with pytest.raises(ValueError, match="NMS_TYPE"):
        stand_in(config(NMS_TYPE="nms_cpu")).post_processing(dict(d))
    with pytest.raises(ValueError, match="1024"):
        stand_in(config(NMS_POST_MAXSIZE=1025)).post_processing(dict(d))
    with pytest.raises(ValueError, match="65535"):
        stand_in(config()).post_processing(dict(d, batch_size=65536))
    with pytest.raises(ValueError, match="16"):
        stand_in(config(RECALL_THRESH_LIST=[0.1] * 17)).post_processing(dict(d))
    s = dict(batch_size=2, batch_box_preds=box.reshape(-1, 7), batch_cls_preds=cls.reshape(-1, 3), cls_preds_normalized=True,
             batch_index=torch.zeros(16))
    with pytest.raises(NotImplementedError, match="batch_index"):
        stand_in(config()).post_processing(dict(s, has_class_labels=True, roi_labels=torch.ones((2, 8), dtype=torch.long)))
    with pytest.raises(NotImplementedError, match="batch_index"):
        stand_in(config()).post_processing(dict(s, rois=torch.zeros((2, 4, 7))))
    with pytest.raises(AssertionError):
        stand_in(config(), num_class=5).post_processing(dict(d))      # K is neither 1 nor num_class: the reference's assertion
    with pytest.raises(AssertionError):
        stand_in(config()).post_processing(dict(d, batch_index=torch.zeros(16)))


def test_header_ctypes_mirror_and_no_scratch():
    import ctypes as C
    import json
    import re
    from modest_amd import _lib, build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    build.build(verbose=False)
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "modest_hip.h")).read(), flags=re.S)
    ctype = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float}
    for fn, count in (("modest_post_process", 36), ("modest_post_process_workspace_bytes", 2), ("modest_post_process_tile", 0),
                      ("modest_post_process_max_thresholds", 0)):
        m = re.search(r"\b(int64_t|int)\s+%s\s*\(([^)]*)\)" % fn, src)
        assert m, fn
        args = [a.strip() for a in m.group(2).split(",") if a.strip() != "void"]
        want = [_lib.VP if "*" in a else ctype[a.split()[0]] for a in args]
        res, have = _lib.SIGNATURES[fn]
        assert res is ctype[m.group(1)] and have == want and len(want) == count, fn
        assert hasattr(lib, fn)
    res = json.load(open(os.path.join(os.path.dirname(build.LIB), "kernel_resources.json")))
    mine = {k: v for k, v in res.items() if v.get("file") == "post_process.hip"}
    assert len(mine) == 4 and sum("post_walk" in k for k in mine) == 2 and sum("rank_keysILb1E" in k for k in mine) == 1 \
        and sum("post_recall" in k for k in mine) == 1
    # no scratch memory: no vector register is spilled (a scalar one may move to a vector lane, which costs no memory)
    assert all(v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 for v in mine.values()), mine
    assert max(v["LDS Size [bytes/block]"] for v in mine.values()) <= 160 * 1024
    text = open(os.path.join(root, "modest_amd", "csrc", "post_process.hip")).read()
    assert "hipMalloc" not in text and "hipMemcpy" not in text and text.count("hipStreamSynchronize") == 1
    # one walk: both kernels call the body in the shared header, which neither file restates
    walk = open(os.path.join(root, "modest_amd", "csrc", "prop_walk.h")).read()
    prop = open(os.path.join(root, "modest_amd", "csrc", "proposals.hip")).read()
    assert walk.count("Walked walk_segment(") == 1 and "walk_segment<ROTATED>(" in text and "walk_segment<ROTATED>(" in prop
    assert "s_mat" not in text and "s_mat" not in prop
    steps = open(os.path.join(root, "modest_amd", "csrc", "iou3d_steps.h")).read()
    match = open(os.path.join(root, "modest_amd", "csrc", "roi_targets.hip")).read()
    assert "iou3d_from_bev(" in text and "iou3d_from_bev(" in match and steps.count("float iou3d_from_bev(") == 1
