"""GPU: modest_amd.ops.proposals and the drop-in proposal_layer (csrc/proposals.hip) against the numpy
restatement tests/proposals_seq.py, bit for bit on all three outputs, on the cases of tests/proposals_cases.py (CASES and EDGE_CASES: logit scores, zeros and
denormals, non-finite boxes, POST 1024 reached, PRE 0 - 65, thresholds -1 - +inf and NaN, B = 65535, 4096 columns; each asserts
its edge in tests/test_proposals_cpu.py) and on the scenes recorded from the reference's own proposal_layer
(tests/golden/proposals.npz).  Rows whose heading the device's double cos / sin rounds differently from the host's are taken
out of the inputs first and counted (at most 0.1 % of the rows, the MAX_DROPPED of tests/test_gpu_iou3d.py).  On the cases
whose scores and class values are pairwise distinct the outputs also equal, with nothing taken out, the path before this op:
the reference's loop over torch.max, torch.topk and the existing iou3d_nms_utils.nms_gpu / nms_normal_gpu.  Every case runs
into outputs filled with a sentinel.  Also: one workspace for a large call and then a small one, a side stream, the drop-in
through bind() on a stand-in head in both forms, and the limits."""
import math
import os
import types

import numpy as np
import pytest
import torch

import proposals_cases as cases
import proposals_seq as seq
from modest_amd import ops
from modest_amd.utils import proposal_layer as pl

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "proposals.npz")
MAX_DROPPED = 0.001
DEV = torch.device("cuda")


def trig_differs(h):
    """rows whose heading the device's double cos / sin, rounded to float32, evaluates differently from the host's double
    libm (tests/test_gpu_iou3d.py:_trig_differs); a NaN on both sides (a non-finite heading) is no difference"""
    h = np.ascontiguousarray(h, np.float32).reshape(-1)
    hd = torch.from_numpy(h.copy()).to(DEV).double()
    dev = torch.stack([torch.cos(hd).float(), torch.sin(hd).float(), torch.cos(-hd).float(), torch.sin(-hd).float()], 1).cpu().numpy()
    trig = lambda f, v: f(v) if math.isfinite(v) else math.nan      # noqa: E731  (math.cos(inf) raises, C's gives NaN)
    host = np.array([[trig(math.cos, v), trig(math.sin, v), trig(math.cos, -v), trig(math.sin, -v)]
                     for v in h.astype(np.float64)]).astype(np.float32)
    return ((dev != host) & ~(np.isnan(dev) & np.isnan(host))).any(1)


def without_dropped(c):
    """-> (case with the rows of differing trig taken out, rows, rows taken out): a dense case loses the position in
    every sample"""
    n = c["box"].size // c["box"].shape[-1]
    if not c["rotated"] or n == 0:
        return c, n, 0
    drop = trig_differs(c["box"][..., 6])
    if not drop.any():
        return c, n, 0
    d = dict(c)
    d.pop("name", None)
    if c["batch_index"] is None:
        pos = drop.reshape(c["box"].shape[:2]).any(0)
        d["box"], d["cls"] = np.ascontiguousarray(c["box"][:, ~pos]), np.ascontiguousarray(c["cls"][:, ~pos])
        return d, n, int(pos.sum()) * c["box"].shape[0]
    d["box"], d["cls"], d["batch_index"] = c["box"][~drop], c["cls"][~drop], c["batch_index"][~drop]
    return d, n, int(drop.sum())


def device_inputs(c):
    box, cls = torch.from_numpy(np.array(c["box"])).to(DEV), torch.from_numpy(np.array(c["cls"])).to(DEV)
    bidx = None if c["batch_index"] is None else torch.from_numpy(np.array(c["batch_index"])).to(DEV)
    return box, cls, bidx


def sentinel_outputs(B, post, cols):
    return (torch.full((B, post, cols), 0x5A5A5A5A, dtype=torch.int32, device=DEV).view(torch.float32),
            torch.full((B, post), 0x5A5A5A5A, dtype=torch.int32, device=DEV).view(torch.float32),
            torch.full((B, post), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV))


def run(c, out=None, workspace=None):
    box, cls, bidx = device_inputs(c)
    res = ops.proposals(box, cls, c["B"], c["pre"], c["post"], c["thresh"], rotated=c["rotated"], batch_index=bidx, out=out,
                        workspace=workspace)
    assert res[0].dtype == torch.float32 and res[1].dtype == torch.float32 and res[2].dtype == torch.int64
    assert res[0].shape == (c["B"], c["post"], c["box"].shape[-1]) and res[1].shape == res[2].shape == (c["B"], c["post"])
    return tuple(t.cpu().numpy() for t in res)


def want_of(c):
    return cases.want(c) if "name" in c else seq.proposals(c["box"], c["cls"], c["B"], c["pre"], c["post"], c["thresh"],
                                                           c["rotated"], c["batch_index"])


ALL = list(cases.CASES) + list(cases.EDGE_CASES)


@pytest.mark.parametrize("name", ALL)
def test_cases_against_the_restatement(name):
    """into outputs the test filled with a sentinel: the same objects come back, every element written, the
    restatement's bits"""
    c, n, dropped = without_dropped(cases.case(name))
    assert dropped <= max(1, MAX_DROPPED * n), (dropped, n)
    out = sentinel_outputs(c["B"], c["post"], c["box"].shape[-1])
    box, cls, bidx = device_inputs(c)
    res = ops.proposals(box, cls, c["B"], c["pre"], c["post"], c["thresh"], rotated=c["rotated"], batch_index=bidx, out=out)
    assert all(r is o for r, o in zip(res, out))
    got = tuple(t.cpu().numpy() for t in res)
    assert not (got[0].view(np.uint32) == 0x5A5A5A5A).any() and not (got[1].view(np.uint32) == 0x5A5A5A5A).any()
    assert not (got[2] == 0x5A5A5A5A5A5A5A5A).any()
    why = seq.describe(got, want_of(c))
    assert seq.same(got, want_of(c)) and not why, "\n".join(why)


def test_dropped_rows_are_few():
    """the rows taken out over all cases of both registries: counted, printed, at most 0.1 %"""
    rows = dropped = 0
    for name in ALL:
        _, n, d = without_dropped(cases.case(name))
        rows, dropped = rows + n, dropped + d
    print(f"rows whose device trig differs from the host's: {dropped} of {rows}")
    assert dropped <= MAX_DROPPED * rows, (dropped, rows)


# ------------------------------------------------------------------------------------------------ the path before this op
def parent_path(box_preds, cls_preds, batch_size, pre, post, thresh, nms_type, batch_index=None):
    """RoIHeadTemplate.proposal_layer over class_agnostic_nms, restated over the existing shims"""
    from modest_amd.utils.iou3d_nms import iou3d_nms_utils
    rois = box_preds.new_zeros((batch_size, post, box_preds.shape[-1]))
    roi_scores = box_preds.new_zeros((batch_size, post))
    roi_labels = box_preds.new_zeros((batch_size, post), dtype=torch.long)
    for index in range(batch_size):
        mask = (batch_index == index) if batch_index is not None else index
        box, cls = box_preds[mask], cls_preds[mask]
        cur_scores, cur_labels = torch.max(cls, dim=1)
        selected = []
        if cur_scores.shape[0] > 0:
            top, indices = torch.topk(cur_scores, k=min(pre, cur_scores.shape[0]))
            keep, _ = getattr(iou3d_nms_utils, nms_type)(box[indices][:, 0:7], top, thresh)
            selected = indices[keep[:post]]
        rois[index, :len(selected), :] = box[selected]
        roi_scores[index, :len(selected)] = cur_scores[selected]
        roi_labels[index, :len(selected)] = cur_labels[selected]
    return rois, roi_scores, roi_labels + 1


DISTINCT = [n for n in cases.CASES if cases.is_distinct(cases.case(n))] + cases.EDGE_DISTINCT


def test_enough_cases_leave_no_order_open():
    assert len(DISTINCT) >= 25 + 12 and {"past every capacity", "dense", "3 samples", "POST inside a chunk", "fewer than POST",
                                         "thresh 0.7 axis-aligned", "64 rows", "65 rows"} <= set(DISTINCT)
    # the edges: negative scores, the full kept list, PRE down to no candidate, the finite thresholds
    assert {"logits", "logits axis-aligned", "logits K 3", "POST 1024 full", "PRE 0", "PRE 1", "PRE 64", "PRE 65", "thresh -1", "thresh 0",
            "thresh 1", "thresh -1 axis-aligned"} <= set(DISTINCT)
    assert all(cases.is_distinct(cases.case(n)) for n in cases.EDGE_DISTINCT)
    assert not any(cases.case(n)["B"] > 3 for n in DISTINCT)      # the path before loops over the samples in Python


@pytest.mark.parametrize("name", DISTINCT)
def test_distinct_cases_equal_the_parent_path(name):
    """nothing taken out: both paths evaluate their trig on the device"""
    c = cases.case(name)
    box, cls, bidx = device_inputs(c)
    want = parent_path(box, cls, c["B"], c["pre"], c["post"], c["thresh"], "nms_gpu" if c["rotated"] else "nms_normal_gpu", bidx)
    want = tuple(t.cpu().numpy() for t in want)
    got = run(c)
    why = seq.describe(got, want)
    assert seq.same(got, want) and not why, "\n".join(why)


# ------------------------------------------------------------------------------------------------ the recorded fixture
def test_recorded_scenes():
    rec = dict(np.load(GOLD))
    for name in seq.scenes(rec):
        cfg, box, cls, bidx = seq.scene_inputs(rec, name)
        c = dict(box=box, cls=cls, batch_index=bidx, B=cfg["batch_size"], pre=cfg["NMS_PRE_MAXSIZE"], post=cfg["NMS_POST_MAXSIZE"],
                 thresh=cfg["NMS_THRESH"], rotated=cfg["NMS_TYPE"] == "nms_gpu")
        assert not trig_differs(box[..., 6]).any(), name      # the scenes' headings were drawn for this
        got = run(c)
        why = seq.describe(got, seq.recorded(rec, name))
        assert seq.same(got, seq.recorded(rec, name)) and not why, name + "\n" + "\n".join(why)


# ------------------------------------------------------------------------------------------------ the call
def test_empty_outputs_come_back_fully_written():
    """outputs allocated with torch.empty and filled with garbage; then freshly allocated ones"""
    c = cases.case("3 samples")
    want = cases.want(c)
    out = (torch.empty((3, 100, 7), device=DEV), torch.empty((3, 100), device=DEV), torch.empty((3, 100), dtype=torch.int64, device=DEV))
    out[0].fill_(float("nan")), out[1].fill_(-3.0), out[2].fill_(99)
    assert seq.same(run(c, out=out), want)
    assert seq.same(run(c), want)


def test_a_large_call_then_a_small_one_on_the_same_workspace():
    big, small = cases.case("past every capacity"), cases.case("63 rows")
    ws = torch.empty((ops.proposals_workspace_bytes(len(big["box"])),), dtype=torch.uint8, device=DEV)
    assert ops.proposals_workspace_bytes(len(small["box"])) < ws.numel()
    want_big, want_small = run(big), run(small)
    assert seq.same(run(big, workspace=ws), want_big)
    assert seq.same(run(small, workspace=ws), want_small)          # no survivor of the large call is left
    few = cases.case("fewer than POST")
    assert seq.same(run(few, workspace=ws), run(few))
    assert seq.same(run(small, workspace=ws), want_small)


def test_all_samples_then_a_small_call_on_the_same_workspace():
    """B = 65535: 65 535 workgroups, 48 key bits; then one sample of 63 rows, whose segment search meets only its own keys"""
    big, small = cases.case("B 65535 stacked"), cases.case("63 rows")
    ws = torch.empty((ops.proposals_workspace_bytes(len(big["box"])),), dtype=torch.uint8, device=DEV)
    ws.fill_(0xFF)
    assert ops.proposals_workspace_bytes(len(small["box"])) < ws.numel()
    want_big, want_small = run(big), run(small)
    assert seq.same(run(big, workspace=ws), want_big)
    assert seq.same(run(small, workspace=ws), want_small)
    assert seq.same(run(big, workspace=ws), want_big)


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
    rois, scores, labels = ops.proposals(box, cls, 2, 9000, 5, 0.7, batch_index=torch.zeros((0,), device=DEV))
    assert not rois.any() and not scores.any() and (labels == 1).all() and rois.shape == (2, 5, 7)
    rois, scores, labels = ops.proposals(torch.zeros((2, 0, 9), device=DEV), torch.zeros((2, 0, 3), device=DEV), 2, 9000, 5, 0.7)
    assert not rois.any() and not scores.any() and (labels == 1).all() and rois.shape == (2, 5, 9)
    assert ops.proposals(box, cls, 0, 9000, 5, 0.7, batch_index=torch.zeros((0,), device=DEV))[0].shape == (0, 5, 7)


def test_integer_batch_index_kinds():
    c = cases.case("3 samples and strays")
    want = cases.want(c)
    box, cls, bidx = device_inputs(c)
    k = torch.where(torch.isfinite(bidx) & (bidx == bidx.floor()) & (bidx.abs() < 100), bidx, torch.full_like(bidx, 7))
    for dtype in (torch.int64, torch.int32, torch.int16, torch.float64):
        got = ops.proposals(box, cls, 3, c["pre"], c["post"], c["thresh"], batch_index=k.to(dtype))
        assert seq.same(tuple(t.cpu().numpy() for t in got), want), dtype


# ------------------------------------------------------------------------------------------------ the drop-in
def stand_in_head():
    return pl.bind(type("RoIHead", (), {}))()


@pytest.mark.parametrize("name", ["3 samples and strays", "dense", "dense axis-aligned"])
def test_the_drop_in_through_bind(name):
    c = cases.case(name)
    box, cls, bidx = device_inputs(c)
    cfg = types.SimpleNamespace(MULTI_CLASSES_NMS=False, NMS_TYPE="nms_gpu" if c["rotated"] else "nms_normal_gpu",
                                NMS_PRE_MAXSIZE=c["pre"], NMS_POST_MAXSIZE=c["post"], NMS_THRESH=c["thresh"])
    head = stand_in_head()
    d = dict(batch_size=c["B"], batch_box_preds=box, batch_cls_preds=cls)
    if bidx is not None:
        d["batch_index"] = bidx
    for _ in range(2):                                       # the second call reuses the head's workspace
        out = head.proposal_layer(dict(d), cfg)
        assert out is not d and "batch_index" not in out
        assert out["has_class_labels"] is (c["cls"].shape[-1] > 1)
        got = tuple(out[k].cpu().numpy() for k in ("rois", "roi_scores", "roi_labels"))
        assert seq.same(got, cases.want(c)), "\n".join(seq.describe(got, cases.want(c)))
    assert head._modest_proposals_workspace.numel() >= ops.proposals_workspace_bytes(c["box"].size // c["box"].shape[-1])


def test_limits_name_themselves():
    from modest_amd._lib import ModestHipError
    c = cases.case("63 rows")
    box, cls, bidx = device_inputs(c)
    with pytest.raises(ModestHipError, match="1024"):
        ops.proposals(box, cls, 1, 9000, seq.POST_MAX + 1, 0.7, batch_index=bidx)
    with pytest.raises(ModestHipError, match="65535"):
        ops.proposals(box, cls, seq.BATCH_MAX + 1, 9000, 1, 0.7, batch_index=bidx)
    ok = ops.proposals(box, cls, 1, 9000, seq.POST_MAX, 0.7, batch_index=bidx)        # the limit itself works
    want = seq.proposals(c["box"], c["cls"], 1, 9000, seq.POST_MAX, 0.7, True, c["batch_index"])
    assert seq.same(tuple(t.cpu().numpy() for t in ok), want)
    head = stand_in_head()
    cfg = dict(MULTI_CLASSES_NMS=False, NMS_TYPE="nms_gpu", NMS_PRE_MAXSIZE=9000, NMS_POST_MAXSIZE=seq.POST_MAX + 1, NMS_THRESH=0.7)
    with pytest.raises(ValueError, match="1024"):
        head.proposal_layer(dict(batch_size=1, batch_box_preds=box, batch_cls_preds=cls, batch_index=bidx), cfg)
    # 4096 box columns and 4096 class columns work (test_cases_against_the_restatement runs both cases), 4097 are refused
    for name in ("4096 box columns", "4096 class columns"):
        w = cases.case(name)
        wbox, wcls, wbidx = device_inputs(w)
        assert 4096 in (wbox.shape[1], wcls.shape[1])
        ok = ops.proposals(wbox, wcls, 1, w["pre"], w["post"], w["thresh"], batch_index=wbidx)
        assert seq.same(tuple(t.cpu().numpy() for t in ok), cases.want(w)), name
    wide = torch.zeros((len(c["box"]), 4097), device=DEV)
    wide[:, :7] = box
    with pytest.raises(ModestHipError, match="4096"):
        ops.proposals(wide, cls, 1, 9000, 10, 0.7, batch_index=bidx)
    with pytest.raises(ModestHipError, match="4096"):
        ops.proposals(box, wide, 1, 9000, 10, 0.7, batch_index=bidx)
    # B = 65535 itself works
    many = cases.case("B 65535 dense")
    assert many["B"] == seq.BATCH_MAX and seq.same(run(many), cases.want(many))
    # a refused call leaves the next one right
    assert seq.same(run(c), cases.want(c))
