"""GPU: modest_amd.ops.post_process and the drop-in post_processing (csrc/post_process.hip) against
the numpy restatement tests/post_process_seq.py, bit for bit on boxes, scores, labels, counts and the recall counters, on
every case of tests/post_process_cases.py (each asserts its edge in tests/test_post_process_cpu.py) and on the scenes
recorded from the reference's own post_processing (tests/golden/post_process.npz).  Rows whose heading the device's double
cos / sin, or whose logit the device's double sigmoid, rounds differently from the host's are taken out of the inputs first
and counted (at most 0.1 % of the rows, the MAX_DROPPED of tests/test_gpu_iou3d.py; the CPU test's conditions make 0 the
expected count).  On the cases without open order the outputs also equal, with nothing taken out, the path before this op:
the reference's loop over the existing shims.  Every case runs into outputs filled with a sentinel.  Also: one workspace
and table for a large call and then a small one, a side stream, the drop-in through bind() on a stand-in detector in both
forms under torch's sync debug mode, repeated calls, and the limits."""
import os
import types
import warnings

import numpy as np
import pytest
import torch

import post_process_cases as cases
import post_process_seq as seq
from modest_amd import ops
from modest_amd.utils import post_processing as pp
from test_gpu_proposals import trig_differs
from test_post_process_cpu import compare_with_recorded, config

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "post_process.npz")
MAX_DROPPED = 0.001
DEV = torch.device("cuda")
SENTINEL = 0x5A5A5A5A
ALL = list(cases.CASES)


def sigmoid_differs(x):
    """rows whose logit the device's double sigmoid, rounded to float32, evaluates differently from the host's"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    xd = torch.from_numpy(x.copy()).to(DEV)
    dev = (1 / (1 + torch.exp(-xd.double()))).float().cpu().numpy()
    host = seq.sigmoid(x)
    return (dev.view(np.uint32) != host.view(np.uint32)) & ~(np.isnan(dev) & np.isnan(host))


def without_dropped(c):
    """-> (case with the rows of differing trig or sigmoid taken out, rows, rows taken out): a dense case loses the
    position in every sample; gts and rois of differing trig are taken out too"""
    cols = c["box"].shape[-1]
    n = c["box"].size // cols
    if n == 0:
        return c, n, 0
    drop = np.zeros(n, bool)
    if c["rotated"] or c["gt_boxes"] is not None:
        drop |= trig_differs(c["box"][..., 6])
    if not c["normalized"]:
        drop |= sigmoid_differs(c["cls"]).reshape(n, -1).any(1)
    d = dict(c)
    taken = 0
    for k in ("gt_boxes", "rois"):
        if c[k] is not None and c[k].size:
            bad = trig_differs(c[k][..., 6]).reshape(c[k].shape[:2]).any(0)
            if bad.any():
                d[k] = np.ascontiguousarray(c[k][:, ~bad])
                taken += int(bad.sum()) * c[k].shape[0]
    if not drop.any() and not taken:
        return c, n, 0
    d.pop("name", None)
    if c["batch_index"] is None:
        pos = drop.reshape(c["box"].shape[:2]).any(0)
        d["box"], d["cls"] = np.ascontiguousarray(c["box"][:, ~pos]), np.ascontiguousarray(c["cls"][:, ~pos])
        if c["labels"] is not None:
            d["labels"] = np.ascontiguousarray(c["labels"][:, ~pos])
        return d, n, int(pos.sum()) * c["box"].shape[0] + taken
    d["box"], d["cls"], d["batch_index"] = c["box"][~drop], c["cls"][~drop], c["batch_index"][~drop]
    return d, n, int(drop.sum()) + taken


def dev_of(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def sentinel_outputs(B, post, cols):
    return (torch.full((B, post, cols), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32),
            torch.full((B, post), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32),
            torch.full((B, post), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV))


def run(c, out=None, workspace=None, table=None, padded=False):
    """-> (preds, recall) in the restatement's form"""
    res = ops.post_process(dev_of(c["box"]), dev_of(c["cls"]), c["B"], c["pre"], c["post"], c["nms_thresh"], rotated=c["rotated"],
                           score_thresh=c["score_thresh"], normalized=c["normalized"], output_raw_score=c["output_raw_score"],
                           labels=dev_of(c["labels"]), batch_index=dev_of(c["batch_index"]), gt_boxes=dev_of(c["gt_boxes"]),
                           rois=dev_of(c["rois"]), recall_thresh=c["recall_thresh"], workspace=workspace, table=table, out=out)
    boxes, scores, labels, counts, recall = res
    assert boxes.dtype == torch.float32 and scores.dtype == torch.float32 and labels.dtype == torch.int64
    assert boxes.shape == (c["B"], c["post"], c["box"].shape[-1]) and scores.shape == labels.shape == (c["B"], c["post"])
    assert counts.shape == (c["B"],) and (counts >= 0).all() and (counts <= c["post"]).all()
    b, s, l = boxes.cpu().numpy(), scores.cpu().numpy(), labels.cpu().numpy()
    preds = [(b[k, :counts[k]], s[k, :counts[k]], l[k, :counts[k]]) for k in range(c["B"])]
    return ((preds, recall), (b, s, l, counts)) if padded else (preds, recall)


def want_of(c):
    return cases.want(c) if "name" in c else seq.post_process(c["box"], c["cls"], **cases.args(c))


@pytest.mark.parametrize("name", ALL)
def test_cases_against_the_restatement(name):
    """into outputs the test filled with a sentinel: the same objects come back, every visible element written, nothing
    behind a sample's count touched, the restatement's bits"""
    c, n, dropped = without_dropped(cases.case(name))
    assert dropped <= max(1, MAX_DROPPED * n), (dropped, n)
    out = sentinel_outputs(c["B"], c["post"], c["box"].shape[-1])
    got, (b, s, l, counts) = run(c, out=out, padded=True)
    for k in range(c["B"]):
        vis = slice(0, counts[k])
        assert not (b[k, vis, :7].view(np.uint32) == SENTINEL).any() and not (s[k, vis].view(np.uint32) == SENTINEL).any()
        assert not (l[k, vis] == 0x5A5A5A5A5A5A5A5A).any()
        assert (b[k, counts[k]:].view(np.uint32) == SENTINEL).all() and (l[k, counts[k]:] == 0x5A5A5A5A5A5A5A5A).all()
    why = seq.describe(got, want_of(c))
    assert not why, "\n".join(why)


def test_dropped_rows_are_few():
    """the rows taken out over all cases: counted, printed, at most 0.1 %"""
    rows = dropped = 0
    for name in ALL:
        _, n, d = without_dropped(cases.case(name))
        rows, dropped = rows + n, dropped + d
    print(f"rows whose device trig or sigmoid differs from the host's: {dropped} of {rows}")
    assert dropped <= MAX_DROPPED * rows, (dropped, rows)


def test_the_tile_is_the_library_s():
    assert ops.post_process_tile() == cases.TILE


# ------------------------------------------------------------------------------------------------ the path before this op
def double_sigmoid(x):
    return (1 / (1 + torch.exp(-x.double()))).float()


def parent_path(c):
    """Detector3DTemplate.post_processing over class_agnostic_nms and generate_recall_record, restated over the existing
    shims (nms_gpu / nms_normal_gpu, boxes_iou3d_gpu), torch.sigmoid replaced by the double rule"""
    from modest_amd.utils.iou3d_nms import iou3d_nms_utils
    box_all, cls_all, bidx = dev_of(c["box"]), dev_of(c["cls"]), dev_of(c["batch_index"])
    gt_all, rois_all, labels = dev_of(c["gt_boxes"]), dev_of(c["rois"]), dev_of(c["labels"])
    nms = getattr(iou3d_nms_utils, "nms_gpu" if c["rotated"] else "nms_normal_gpu")
    T = len(c["recall_thresh"])
    recall = None if gt_all is None else {"gt": 0, "rcnn": [0] * T, "roi": [0] * T}
    preds = []
    for index in range(c["B"]):
        mask = (bidx == index) if bidx is not None else index
        box_preds, src_cls = box_all[mask], cls_all[mask]
        cls_preds = src_cls if c["normalized"] else double_sigmoid(src_cls)
        cls_preds, label_preds = torch.max(cls_preds, dim=-1)
        label_preds = labels[index].reshape(-1) if labels is not None else label_preds + 1
        scores, boxes = cls_preds, box_preds
        if c["score_thresh"] is not None:
            sm = scores >= c["score_thresh"]
            scores, boxes = scores[sm], boxes[sm]
        selected = torch.zeros((0,), dtype=torch.long, device=DEV)
        if scores.shape[0] > 0:
            top, indices = torch.topk(scores, k=min(c["pre"], scores.shape[0]))
            keep, _ = nms(boxes[indices][:, 0:7], top, c["nms_thresh"])
            selected = indices[keep[:c["post"]]]
        if c["score_thresh"] is not None:
            selected = sm.nonzero().view(-1)[selected]
        final_scores = cls_preds[selected]
        if c["output_raw_score"]:
            final_scores = torch.max(src_cls, dim=-1)[0][selected]
        final_boxes = box_preds[selected]
        preds.append((final_boxes.cpu().numpy(), final_scores.cpu().numpy(), label_preds[selected].cpu().numpy()))
        if gt_all is not None:
            cur_gt = gt_all[index]
            k = len(cur_gt) - 1
            while k > 0 and cur_gt[k].sum() == 0:
                k -= 1
            cur_gt = cur_gt[:k + 1]
            if cur_gt.shape[0] > 0:
                lists = {"rcnn": final_boxes if rois_all is None else box_preds}
                if rois_all is not None:
                    lists["roi"] = rois_all[index]
                for kind, lst in lists.items():
                    if lst.shape[0] == 0:
                        continue
                    iou = iou3d_nms_utils.boxes_iou3d_gpu(lst[:, 0:7].contiguous(), cur_gt[:, 0:7].contiguous())
                    for q, t in enumerate(c["recall_thresh"]):
                        recall[kind][q] += (iou.max(dim=0)[0] > t).sum().item()
                recall["gt"] += cur_gt.shape[0]
    return preds, recall


DISTINCT = [n for n in ALL if n != "B 65535" and cases.is_distinct(cases.case(n))]


def test_enough_cases_leave_no_order_open():
    assert len(DISTINCT) >= 30, DISTINCT
    assert {"pass 0", "pass 1", "pass 63", "pass 64", "pass 65", "pass 129", "pass 129 logits", "POST inside a chunk",
            "threshold 0.7 axis-aligned", "given labels", "3 samples and strays", "gt 65", "gt 257", "rois present", "recall tie",
            "all-zero gts", "trailing zero rows", "OUTPUT_RAW_SCORE normalised"} <= set(DISTINCT)


@pytest.mark.parametrize("name", DISTINCT)
def test_distinct_cases_equal_the_parent_path(name):
    """nothing taken out: both paths evaluate their trig and their sigmoid on the device"""
    c = cases.case(name)
    why = seq.describe(run(c), parent_path(c))
    assert not why, "\n".join(why)


# ------------------------------------------------------------------------------------------------ the recorded fixture
def scene_case(cfg, a):
    return dict(box=a["box"], cls=a["cls"], batch_index=a["batch_index"], B=cfg["batch_size"], pre=cfg["NMS_PRE_MAXSIZE"],
                post=cfg["NMS_POST_MAXSIZE"], nms_thresh=cfg["NMS_THRESH"], rotated=cfg["NMS_TYPE"] == "nms_gpu",
                score_thresh=cfg["SCORE_THRESH"], normalized=cfg["cls_preds_normalized"], output_raw_score=cfg["OUTPUT_RAW_SCORE"],
                labels=a["labels"] if cfg["has_class_labels"] else None, gt_boxes=a["gt_boxes"],
                rois=a["rois"] if cfg["rois_in_batch"] else None, recall_thresh=cfg["RECALL_THRESH_LIST"])


def test_recorded_scenes():
    rec = dict(np.load(GOLD))
    for name in seq.scenes(rec):
        cfg, a = seq.scene_inputs(rec, name)
        for k in ("box", "gt_boxes", "rois"):
            assert a[k] is None or not trig_differs(a[k][..., 6]).any(), (name, k)      # the scenes' headings were drawn for this
        compare_with_recorded(run(scene_case(cfg, a)), rec, name, cfg, int(rec["sigmoid_ulp"]))


# ------------------------------------------------------------------------------------------------ the call
def test_a_large_call_then_a_small_one_on_the_same_workspace_and_table():
    big, small = cases.case("POST inside a chunk"), cases.case("pass 63")
    ws = torch.empty((ops.post_process_workspace_bytes(len(big["box"]), 1),), dtype=torch.uint8, device=DEV)
    ws.fill_(0xFF)
    table = torch.full((64,), -1, dtype=torch.int32).pin_memory()
    assert ops.post_process_workspace_bytes(len(small["box"]), 1) < ws.numel()
    want_big, want_small = run(big), run(small)
    assert seq.same(run(big, workspace=ws, table=table), want_big)
    assert seq.same(run(small, workspace=ws, table=table), want_small)      # no survivor of the large call is left
    empty = cases.case("pass 0")
    assert seq.same(run(empty, workspace=ws, table=table), cases.want(empty))
    assert seq.same(run(big, workspace=ws, table=table), want_big)


def test_repeated_calls_give_the_same_bits():
    for name in ("dense", "rois present", "gt 257"):
        c = cases.case(name)
        first, (b0, s0, l0, n0) = run(c, out=sentinel_outputs(c["B"], c["post"], c["box"].shape[-1]), padded=True)
        again, (b1, s1, l1, n1) = run(c, out=sentinel_outputs(c["B"], c["post"], c["box"].shape[-1]), padded=True)
        assert seq.same(first, again) and b0.tobytes() == b1.tobytes() and s0.tobytes() == s1.tobytes() and l0.tobytes() == l1.tobytes()
        assert np.array_equal(n0, n1)


def test_a_side_stream():
    c = cases.case("dense")
    want = run(c)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = run(c)
    side.synchronize()
    assert seq.same(got, want)


def test_no_rows_and_no_samples():
    box, cls = torch.zeros((0, 7), device=DEV), torch.zeros((0, 1), device=DEV)
    gt = torch.zeros((2, 3, 8), device=DEV)
    gt[0, 1, 0] = 1
    b, s, l, counts, recall = ops.post_process(box, cls, 2, 4096, 5, 0.1, score_thresh=0.1, batch_index=torch.zeros((0,), device=DEV),
                                               gt_boxes=gt, recall_thresh=(0.3, 0.5))
    assert b.shape == (2, 5, 7) and counts.tolist() == [0, 0] and recall == {"gt": 3, "rcnn": [0, 0], "roi": [0, 0]}
    b, s, l, counts, recall = ops.post_process(torch.zeros((2, 0, 9), device=DEV), torch.zeros((2, 0, 3), device=DEV), 2, 4096, 5, 0.1)
    assert b.shape == (2, 5, 9) and counts.tolist() == [0, 0] and recall is None
    b, s, l, counts, recall = ops.post_process(box, cls, 0, 4096, 5, 0.1, batch_index=torch.zeros((0,), device=DEV))
    assert b.shape == (0, 5, 7) and counts.shape == (0,)
    c = cases.case("pass 65")
    got = run(dict(c, post=0))
    assert [len(g[0]) for g in got[0]] == [0] and got[1]["gt"] == 6 and not any(got[1]["rcnn"])


def test_integer_batch_index_kinds_and_gt_strides():
    c = cases.case("3 samples and strays")
    want = cases.want(c)
    bidx = dev_of(c["batch_index"])
    k = torch.where(torch.isfinite(bidx) & (bidx == bidx.floor()) & (bidx.abs() < 100), bidx, torch.full_like(bidx, 7))
    gt = dev_of(c["gt_boxes"])
    wide = torch.zeros((3, gt.shape[1] * 2, gt.shape[2] + 3), device=DEV)
    wide[:, ::2, 3:] = gt
    for dtype in (torch.int64, torch.int32, torch.int16, torch.float64):
        res = ops.post_process(dev_of(c["box"]), dev_of(c["cls"]), 3, c["pre"], c["post"], c["nms_thresh"], score_thresh=c["score_thresh"],
                               batch_index=k.to(dtype), gt_boxes=wide[:, ::2, 3:], recall_thresh=c["recall_thresh"])
        n = res[3]
        got = ([(res[0][b, :n[b]].cpu().numpy(), res[1][b, :n[b]].cpu().numpy(), res[2][b, :n[b]].cpu().numpy()) for b in range(3)], res[4])
        assert seq.same(got, want), dtype


# ------------------------------------------------------------------------------------------------ the drop-in
def detector_for(c, as_dict=False):
    cfg = config(as_dict, NMS_TYPE="nms_gpu" if c["rotated"] else "nms_normal_gpu", NMS_THRESH=c["nms_thresh"], NMS_PRE_MAXSIZE=c["pre"],
                 NMS_POST_MAXSIZE=c["post"], RECALL_THRESH_LIST=list(c["recall_thresh"]), SCORE_THRESH=c["score_thresh"],
                 OUTPUT_RAW_SCORE=c["output_raw_score"])
    det = pp.bind(type("Detector", (), {}))()
    det.model_cfg, det.num_class = cfg, c["cls"].shape[-1]
    return det


def batch_of(c):
    d = dict(batch_size=c["B"], batch_box_preds=dev_of(c["box"]), batch_cls_preds=dev_of(c["cls"]), cls_preds_normalized=c["normalized"])
    if c["batch_index"] is not None:
        d["batch_index"] = dev_of(c["batch_index"])
    if c["labels"] is not None:
        d["has_class_labels"] = True
        d["roi_labels" if c["rois"] is not None else "batch_pred_labels"] = dev_of(c["labels"])
    if c["gt_boxes"] is not None:
        d["gt_boxes"] = dev_of(c["gt_boxes"])
    if c["rois"] is not None:
        d["rois"] = dev_of(c["rois"])
    return d


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


@pytest.mark.parametrize("name", ["3 samples and strays", "dense", "dense axis-aligned logits", "given labels (B, N, 1)", "rois present",
                                  "pass 0", "OUTPUT_RAW_SCORE", "no threshold"])
def test_the_drop_in_through_bind(name, monkeypatch):
    """the reference's return: (pred_dicts, recall_dict); contiguous views, int64 labels, Python ints in the reference's key
    order.  Under torch's sync debug mode "error" PyTorch may wait nowhere: the call's one host wait is the library's stream
    synchronise, counted around the library call."""
    c = cases.case(name)
    want_preds, want_recall = cases.want(c)
    det = detector_for(c, as_dict=name == "dense")
    d = batch_of(c)
    waits = []
    inner = ops.post_process
    monkeypatch.setattr(ops, "post_process", lambda *a, **k: (waits.append(1), inner(*a, **k))[1])
    for _ in range(2):                                       # the second call reuses the detector's workspace and table
        torch.cuda.synchronize()
        mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            pred_dicts, recall_dict = det.post_processing(dict(d))
        finally:
            torch.cuda.set_sync_debug_mode(mode)
        assert isinstance(pred_dicts, list) and len(pred_dicts) == c["B"]
        for p, w in zip(pred_dicts, want_preds):
            assert list(p) == ["pred_boxes", "pred_scores", "pred_labels"]
            assert p["pred_boxes"].shape == (len(w[0]), c["box"].shape[-1]) and p["pred_scores"].shape == p["pred_labels"].shape == (len(w[0]),)
            assert p["pred_boxes"].dtype == p["pred_scores"].dtype == torch.float32 and p["pred_labels"].dtype == torch.int64
            assert all(p[k].is_contiguous() and p[k].is_cuda for k in p)
        got = [(p["pred_boxes"].cpu().numpy(), p["pred_scores"].cpu().numpy(), p["pred_labels"].cpu().numpy()) for p in pred_dicts]
        why = seq.describe((got, None), (want_preds, None))
        assert not why, "\n".join(why)
        want_dict = seq.recall_dict(want_recall, c["recall_thresh"])
        assert recall_dict == want_dict and list(recall_dict) == list(want_dict) and all(type(v) is int for v in recall_dict.values())
    assert len(waits) == 2                                   # one library call, hence one wait, per post_processing
    assert det._modest_post_process_workspace.numel() >= ops.post_process_workspace_bytes(c["box"].size // c["box"].shape[-1], c["B"])
    assert det._modest_post_process_table.is_pinned()


def test_one_host_wait_reported_by_none_of_torch_s_own():
    c = cases.case("rois present")
    det, d = detector_for(c), batch_of(c)
    det.post_processing(dict(d))                             # warm: the workspace and the table exist
    assert torch_reported_syncs(lambda: det.post_processing(dict(d))) == 0
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    det.post_processing(dict(d))
    assert torch.cuda.memory_stats()["allocation.all.allocated"] - before == 3      # the three output buffers


def test_other_dtypes_go_through_float32_and_come_back():
    c = cases.case("dense")
    det, d = detector_for(c), batch_of(c)
    d["batch_box_preds"], d["batch_cls_preds"] = d["batch_box_preds"].double(), d["batch_cls_preds"].double()
    pred_dicts, recall_dict = det.post_processing(d)
    want_preds, want_recall = cases.want(c)
    for p, w in zip(pred_dicts, want_preds):
        assert p["pred_boxes"].dtype == p["pred_scores"].dtype == torch.float64 and p["pred_labels"].dtype == torch.int64
        assert np.array_equal(p["pred_boxes"][:, :7].float().cpu().numpy(), w[0][:, :7]) and np.array_equal(p["pred_labels"].cpu().numpy(), w[2])
    assert recall_dict == seq.recall_dict(want_recall, c["recall_thresh"])


def test_limits_name_themselves():
    from modest_amd._lib import ModestHipError
    c = cases.case("pass 63")
    box, cls, bidx = dev_of(c["box"]), dev_of(c["cls"]), dev_of(c["batch_index"])
    with pytest.raises(ModestHipError, match="1024"):
        ops.post_process(box, cls, 1, 4096, seq.POST_MAX + 1, 0.7, batch_index=bidx)
    with pytest.raises(ModestHipError, match="65535"):
        ops.post_process(box, cls, seq.BATCH_MAX + 1, 4096, 1, 0.7, batch_index=bidx)
    with pytest.raises(ValueError, match="16"):
        ops.post_process(box, cls, 1, 4096, 10, 0.7, batch_index=bidx, gt_boxes=dev_of(c["gt_boxes"]), recall_thresh=[0.5] * 17)
    wide = torch.zeros((len(c["box"]), 4097), device=DEV)
    wide[:, :7] = box
    with pytest.raises(ModestHipError, match="4096"):
        ops.post_process(wide, cls, 1, 4096, 10, 0.7, batch_index=bidx)
    with pytest.raises(ModestHipError, match="4096"):
        ops.post_process(box, wide, 1, 4096, 10, 0.7, batch_index=bidx)
    with pytest.raises(NotImplementedError, match="batch_index"):
        ops.post_process(box, cls, 1, 4096, 10, 0.7, batch_index=bidx, labels=torch.ones(len(box), dtype=torch.long, device=DEV))
    det = detector_for(dict(c, post=seq.POST_MAX + 1))
    with pytest.raises(ValueError, match="1024"):
        det.post_processing(batch_of(c))
    # the limits themselves work: test_cases_against_the_restatement runs "POST 1024 full", "B 65535", both 4096-column cases
    # and "16 thresholds"; a refused call leaves the next one right
    assert seq.same(run(c), cases.want(c))
