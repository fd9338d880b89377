"""GPU: modest_amd.ops.roi_targets and the drop-in assign_targets (csrc/roi_targets.hip) against the
numpy restatement tests/roi_targets_seq.py, bit for bit on all eight outputs under the same seeds, on every case of
tests/roi_targets_cases.py and on the scenes recorded from the reference's own assign_targets
(tests/golden/roi_targets.npz).  Rows whose heading (or ry, or gt heading) the device's double cos / sin rounds differently
from the host's are taken out first and counted: at most 1 % of the rows.  Every ops call runs on a workspace filled with
0xFF bytes.  Also: the counts and lists a match call leaves, against the restatement's; the path before (the reference's own
method over this project's shims, where pcdet can be imported); one host wait and no device allocation per call; the limits
on both sides."""
import importlib.util
import math
import os
import types
import warnings

import numpy as np
import pytest
import torch

import roi_targets_cases as cases
import roi_targets_seq as seq
from modest_amd import ops
from modest_amd.utils import roi_targets as rt

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "roi_targets.npz")
MAX_DROPPED = 0.01
DEV = torch.device("cuda")
INPUTS = ("rois", "roi_scores", "roi_labels", "gt_boxes")


def trig_differs(h):
    """values whose double cos / sin (of v and -v), rounded to float32, the device evaluates differently from the host's libm
    (tests/test_gpu_proposals.py:trig_differs); a NaN on both sides is no difference"""
    h = np.ascontiguousarray(h, np.float32).reshape(-1)
    hd = torch.from_numpy(h.copy()).to(DEV).double()
    dev = torch.stack([torch.cos(hd).float(), torch.sin(hd).float(), torch.cos(-hd).float(), torch.sin(-hd).float()], 1).cpu().numpy()
    trig = lambda f, v: f(v) if math.isfinite(v) else math.nan      # noqa: E731
    host = np.array([[trig(math.cos, v), trig(math.sin, v), trig(math.cos, -v), trig(math.sin, -v)]
                     for v in h.astype(np.float64)]).astype(np.float32).reshape(-1, 4)
    return ((dev != host) & ~(np.isnan(dev) & np.isnan(host))).any(1)


def without_dropped(c):
    """-> (case without the roi and gt positions whose trig differs, rows, rows taken out)"""
    rois, gt = c["rois"], c["gt_boxes"]
    rows = rois.shape[0] * (rois.shape[1] + gt.shape[1])
    bad_r = (trig_differs(rois[..., 6]) | trig_differs(seq.rem(rois[..., 6], seq.TWO_PI))).reshape(rois.shape[:2]).any(0)
    bad_g = trig_differs(gt[..., 6]).reshape(gt.shape[:2]).any(0)
    if not bad_r.any() and not bad_g.any():
        return c, rows, 0
    d = dict(c)
    for k in ("rois", "roi_scores", "roi_labels"):
        d[k] = np.ascontiguousarray(c[k][:, ~bad_r])
    d["gt_boxes"] = np.ascontiguousarray(gt[:, ~bad_g])
    d["reduced"] = True
    return d, rows, int(bad_r.sum() + bad_g.sum()) * rois.shape[0]


def expected(c):
    if not c.get("reduced"):
        return cases.expected(c["name"])
    details = {}
    return seq.assign_targets(c["rois"], c["roi_scores"], c["roi_labels"], c["gt_boxes"], c["cfg"], cases.seeded_draws(c), details=details), details


def device_inputs(c):
    t = {k: torch.from_numpy(np.array(c[k])).to(DEV) for k in INPUTS}
    if c.get("gt_view") == "strided":      # every second column of every second row of a larger tensor
        g = t["gt_boxes"]
        big = torch.full((g.shape[0], 2 * g.shape[1], 2 * g.shape[2]), 7.0, device=DEV)
        big[:, ::2, ::2] = g
        t["gt_boxes"] = big[:, ::2, ::2]
        assert not t["gt_boxes"].is_contiguous()
    return t


def seed(c):
    np.random.seed(c["seeds"][0])
    torch.manual_seed(c["seeds"][1])


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def filled_workspace(B, N):
    return torch.full((max(ops.roi_targets_workspace_bytes(B, N), 256),), 0xFF, dtype=torch.uint8, device=DEV)


def head_for(cfg, attribute=True):
    head = rt.bind(type("RoIHead", (), {}))()
    head.model_cfg = types.SimpleNamespace(TARGET_CONFIG=types.SimpleNamespace(**cfg)) if attribute else {"TARGET_CONFIG": dict(cfg)}
    return head


@pytest.mark.parametrize("name", cases.NAMES)
def test_against_restatement(name):
    c, rows, dropped = without_dropped(cases.case(name))
    assert dropped <= max(1, MAX_DROPPED * rows), (dropped, rows)
    t = device_inputs(c)
    B, N = c["rois"].shape[:2]
    if c["raises"]:
        seed(c)
        with pytest.raises(c["raises"], match="sample 1: FG=0, BG=0"):
            ops.roi_targets(t["rois"], t["roi_scores"], t["roi_labels"], t["gt_boxes"], c["cfg"], workspace=filled_workspace(B, N))
        with pytest.raises(c["raises"]):
            head_for(c["cfg"]).assign_targets(dict(batch_size=B, **t))
        return
    want, _ = expected(c)
    seed(c)
    got = host(ops.roi_targets(t["rois"], t["roi_scores"], t["roi_labels"], t["gt_boxes"], c["cfg"], workspace=filled_workspace(B, N)))
    assert list(got) == list(seq.KEYS)
    assert seq.same(got, want), "\n".join(seq.describe(got, want))
    head = head_for(c["cfg"], attribute=B % 2 == 0)
    seed(c)
    got = host(head.assign_targets(dict(batch_size=B, **t)))
    assert list(got) == list(seq.KEYS)
    assert seq.same(got, want), "\n".join(seq.describe(got, want))


def test_dropped_rows_are_few():
    rows = dropped = 0
    for name in cases.NAMES:
        _, n, d = without_dropped(cases.case(name))
        rows, dropped = rows + n, dropped + d
    print(f"rows whose device trig differs from the host's: {dropped} of {rows}")
    assert dropped <= MAX_DROPPED * rows, (dropped, rows)


@pytest.mark.parametrize("name", [n for n in cases.NAMES if n != "all_nan"])
def test_lists_after_match(name):
    c, _, _ = without_dropped(cases.case(name))
    _, d = expected(c)
    t = device_inputs(c)
    B, N = c["rois"].shape[:2]
    cfg = c["cfg"]
    ws = filled_workspace(B, N)
    pinned = torch.zeros((3 * B,), dtype=torch.int32).pin_memory()
    counts = ops.roi_targets_match(t["rois"], t["roi_labels"], t["gt_boxes"], min(cfg["REG_FG_THRESH"], cfg["CLS_FG_THRESH"]),
                                   cfg["CLS_BG_THRESH_LO"], cfg["REG_FG_THRESH"], cfg.get("SAMPLE_ROI_BY_EACH_CLASS", False), ws, pinned)
    assert np.array_equal(counts.numpy(), d["counts"])
    wc, iou, at, lists = ops.roi_targets_lists(ws, B, N)
    assert np.array_equal(wc, d["counts"])
    for b in range(B):
        assert np.array_equal(seq.bits(iou[b]), seq.bits(d["found"][b][0])), (name, b)
        assert np.array_equal(at[b], d["found"][b][1]), (name, b)
        for l in range(3):
            assert np.array_equal(lists[b][l], d["found"][b][2][l]), (name, b, seq.LISTS[l])


def test_out_of_range_picks_write_zero_slots():
    c = cases.case("rois_65")
    t = device_inputs(c)
    B, N = c["rois"].shape[:2]
    cfg = c["cfg"]
    ws = filled_workspace(B, N)
    pinned = torch.zeros((3 * B,), dtype=torch.int32).pin_memory()
    counts = ops.roi_targets_match(t["rois"], t["roi_labels"], t["gt_boxes"], 0.55, 0.1, 0.55, True, ws, pinned).numpy()
    picks = np.zeros((B, 6, 2), np.int32)
    picks[:, 1] = (0, -1)
    picks[:, 2, 0], picks[:, 2, 1] = 0, counts[:, 0]             # one past the list
    picks[:, 3] = (3, 0)                                         # no such list
    picks[:, 4] = (-1, 0)
    picks[:, 5] = (2, 2 ** 31 - 1)
    _, d = cases.expected("rois_65")
    want = seq.sample(picks.astype(np.int64), d["found"], c["rois"], c["roi_scores"], c["roi_labels"], c["gt_boxes"], cfg)
    for p in (torch.from_numpy(picks).to(DEV), torch.from_numpy(picks).pin_memory()):      # device and pinned tables
        got = host(ops.roi_targets_sample(p, t["rois"], t["roi_scores"], t["roi_labels"], t["gt_boxes"], cfg["REG_FG_THRESH"],
                                          cfg["CLS_FG_THRESH"], cfg["CLS_BG_THRESH"], "cls", ws))
        assert seq.same(got, want), "\n".join(seq.describe(got, want))
        assert not got["rois"][:, 1:].any() and got["rois"][:, 0].any()


@pytest.mark.parametrize("name", ["cls", "roi_iou", "any_class"])
def test_against_the_fixture(name):
    rec = dict(np.load(GOLD))
    cfg, seeds, rois, scores, labels, gt = seq.scene_inputs(rec, name)
    assert not trig_differs(rois[..., 6]).any() and not trig_differs(seq.rem(rois[..., 6], seq.TWO_PI)).any() \
        and not trig_differs(gt[..., 6]).any()
    c = dict(rois=rois, roi_scores=scores, roi_labels=labels, gt_boxes=gt, seeds=seeds)
    t = device_inputs(c)
    want = seq.recorded(rec, name)
    seed(c)
    got = host(head_for(cfg).assign_targets(dict(batch_size=len(rois), **t)))
    assert seq.same(got, want), "\n".join(seq.describe(got, want))
    layer = types.SimpleNamespace(roi_sampler_cfg=types.SimpleNamespace(**cfg))
    seed(c)
    fwd = host(rt.forward(layer, dict(batch_size=len(rois), **t)))
    assert list(fwd) == list(seq.KEYS[:7]) and np.array_equal(seq.bits(fwd["gt_of_rois"]), seq.bits(want["gt_of_rois_src"]))
    assert all(np.array_equal(seq.bits(fwd[k]), seq.bits(want[k])) for k in seq.KEYS[:7] if k != "gt_of_rois")


def test_other_dtypes_go_through_float32():
    c = cases.case("rois_63")
    t = device_inputs(c)
    want, _ = cases.expected("rois_63")
    seed(c)
    got = ops.roi_targets(t["rois"].double(), t["roi_scores"].double(), t["roi_labels"].int(), t["gt_boxes"].double(), c["cfg"])
    assert got["rois"].dtype == torch.float64 and got["roi_labels"].dtype == torch.int32 and got["rcnn_cls_labels"].dtype == torch.int64
    assert np.array_equal(got["gt_of_rois"].float().cpu().numpy().view(np.uint32), want["gt_of_rois"].view(np.uint32))


def test_pick_tables_outlive_the_sample_kernel(monkeypatch):
    """The sample kernel is only enqueued and reads its picks later.  Without a caller's table it must not read a pinned
    block of the call's own, which PyTorch's host allocator would hand out again at once: it gets a device copy.  With a
    caller's table it reads that table.  A head that replaces its table for a larger call waits for the stream first, and
    both calls' results are the restatement's."""
    seen = []
    inner = ops.roi_targets_sample
    monkeypatch.setattr(ops, "roi_targets_sample", lambda picks, *a, **k: (seen.append(picks), inner(picks, *a, **k))[1])
    small, large = cases.case("m_1"), cases.case("m_128")
    ts, tl = device_inputs(small), device_inputs(large)
    seed(small)
    first = ops.roi_targets(ts["rois"], ts["roi_scores"], ts["roi_labels"], ts["gt_boxes"], small["cfg"])
    seed(large)
    second = ops.roi_targets(tl["rois"], tl["roi_scores"], tl["roi_labels"], tl["gt_boxes"], large["cfg"])     # no wait in between
    assert seen[0].is_cuda and seen[1].is_cuda
    assert seq.same(host(first), cases.expected("m_1")[0]) and seq.same(host(second), cases.expected("m_128")[0])
    mine = torch.zeros((2 * 2 * 128,), dtype=torch.int32).pin_memory()
    seed(large)
    third = ops.roi_targets(tl["rois"], tl["roi_scores"], tl["roi_labels"], tl["gt_boxes"], large["cfg"], picks_pinned=mine)
    assert seen[2].is_pinned() and seen[2].data_ptr() == mine.data_ptr()
    assert seq.same(host(third), cases.expected("m_128")[0])
    # a head whose table grows between two calls
    head = head_for(small["cfg"])
    waits = []
    stream_type = type(torch.cuda.current_stream())
    wait = stream_type.synchronize
    monkeypatch.setattr(stream_type, "synchronize", lambda self: (waits.append(1), wait(self))[1])
    seed(small)
    first = head.assign_targets(dict(batch_size=2, **ts))
    old = head._modest_roi_targets_picks
    assert not waits
    head.model_cfg = types.SimpleNamespace(TARGET_CONFIG=types.SimpleNamespace(**large["cfg"]))
    seed(large)
    second = head.assign_targets(dict(batch_size=2, **tl))
    assert head._modest_roi_targets_picks is not old and len(waits) == 1
    assert seq.same(host(first), cases.expected("m_1")[0]) and seq.same(host(second), cases.expected("m_128")[0])


def reference_head():
    """the reference's RoIHeadTemplate over this project's shims, or None where there is no pcdet; where there is one, a
    failure to import it over the shims is the shims' fault and is raised"""
    if importlib.util.find_spec("pcdet") is None:
        return None
    from modest_amd.utils import pcdet_bind
    pcdet_bind.install()
    from pcdet.models.roi_heads.roi_head_template import RoIHeadTemplate
    from pcdet.models.roi_heads.target_assigner.proposal_target_layer import ProposalTargetLayer
    return RoIHeadTemplate, ProposalTargetLayer


@pytest.mark.parametrize("name", [n for n in cases.NAMES if n not in ("all_nan", "nonfinite", "fg_only", "fg_only_many",
                                                                      "c_2", "c_2_roi_iou")])
def test_against_the_path_before(name):
    """the reference's own method in this process under the same seeds.  Left out: the fg-only branch, which the reference
    ends in torch.cat of a tensor and a list, and C > 0, where its boxes_iou3d_gpu asserts 7 columns.  On rows whose maximum
    is 0 gt_of_rois / gt_of_rois_src are not compared: torch.max on the device may pick any zero."""
    ref = reference_head()
    if ref is None:
        pytest.skip("no pcdet here")
    RoIHeadTemplate, ProposalTargetLayer = ref
    c = cases.case(name)
    t = device_inputs(c)

    class Cfg(dict):
        __getattr__ = dict.__getitem__
    yard = types.SimpleNamespace(proposal_target_layer=ProposalTargetLayer(roi_sampler_cfg=Cfg(c["cfg"])))
    seed(c)
    want = host(RoIHeadTemplate.assign_targets(yard, dict(batch_size=len(c["rois"]), **{k: v.clone() for k, v in t.items()})))
    seed(c)
    got = host(head_for(c["cfg"]).assign_targets(dict(batch_size=len(c["rois"]), **t)))
    positive = got["gt_iou_of_rois"] > 0
    for k in seq.KEYS:
        g, w = seq.bits(got[k]), seq.bits(want[k])
        if k in ("gt_of_rois", "gt_of_rois_src"):
            g, w = g[positive], w[positive]
        assert np.array_equal(g, w), (name, k)
    zero_rows_equal = all(np.array_equal(seq.bits(got[k])[~positive], seq.bits(want[k])[~positive]) for k in ("gt_of_rois", "gt_of_rois_src"))
    print(f"{name}: rows with maximum 0 equal too: {zero_rows_equal}")


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


def test_one_host_wait_and_no_device_allocation():
    """the match call's stream synchronise, inside the library, is the call's one host wait: PyTorch reports none of its own
    (counted as tools/proposals_bench.py counts); after a warm-up a call takes no memory from the device"""
    c = cases.case("m_128")
    t = device_inputs(c)
    head = head_for(c["cfg"])
    call = lambda: head.assign_targets(dict(batch_size=len(c["rois"]), **t))      # noqa: E731
    seed(c)
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    assert torch_reported_syncs(call) == 0
    before = torch.cuda.memory_stats()
    kept = (head._modest_roi_targets_workspace.data_ptr(), head._modest_roi_targets_counts.data_ptr(), head._modest_roi_targets_picks.data_ptr())
    out = call()
    after = torch.cuda.memory_stats()
    assert all(after[k] == before[k] for k in ("reserved_bytes.all.allocated", "segment.all.allocated", "num_device_alloc") if k in before)
    assert kept == (head._modest_roi_targets_workspace.data_ptr(), head._modest_roi_targets_counts.data_ptr(), head._modest_roi_targets_picks.data_ptr())
    # enqueue only after the match call: the outputs are not complete until the stream is
    torch.cuda.synchronize()
    assert out["rois"].shape == (len(c["rois"]), 128, 7)


def test_limits_on_both_sides():
    rng = np.random.default_rng(5)
    cfg = dict(cases.POINTRCNN, ROI_PER_IMAGE=1)

    def inputs(B, N, cols):
        rois = torch.from_numpy(rng.uniform(1, 2, (B, N, cols)).astype(np.float32)).to(DEV)
        gt = torch.cat([rois[:, :1], torch.ones((B, 1, 1), device=DEV)], 2).contiguous()
        return rois, torch.zeros((B, N), device=DEV), torch.ones((B, N), dtype=torch.int64, device=DEV), gt
    r, s, l, g = inputs(1, 2, rt.COLS_MAX)                       # 4096 columns run: the gt is roi 0 itself
    out = ops.roi_targets(r, s, l, g, cfg)
    assert torch.equal(out["gt_of_rois_src"][0, 0], g[0, 0]) and out["rois"].shape == (1, 1, rt.COLS_MAX)
    with pytest.raises(ValueError, match=str(rt.COLS_MAX)):
        ops.roi_targets(*inputs(1, 2, rt.COLS_MAX + 1), cfg)
    r, s, l, g = inputs(rt.BATCH_MAX, 1, 7)                      # 65535 samples run
    out = ops.roi_targets(r, s, l, g, cfg)
    assert torch.equal(out["rois"], r) and torch.equal(out["gt_of_rois_src"], g) and bool((out["rcnn_cls_labels"] == 1).all())
    head = head_for(cfg)
    with pytest.raises(ValueError, match=str(rt.BATCH_MAX)):
        head.assign_targets(dict(batch_size=rt.BATCH_MAX + 1, rois=r[:1].expand(rt.BATCH_MAX + 1, 1, 7), roi_scores=s[:1].expand(rt.BATCH_MAX + 1, 1),
                                 roi_labels=l[:1].expand(rt.BATCH_MAX + 1, 1), gt_boxes=g[:1].expand(rt.BATCH_MAX + 1, 1, 8)))
    with pytest.raises(ValueError, match="ROI_PER_IMAGE"):
        ops.roi_targets(*inputs(1, 2, 7), dict(cfg, ROI_PER_IMAGE=0))
    with pytest.raises(NotImplementedError):
        ops.roi_targets(*inputs(1, 2, 7), dict(cfg, CLS_SCORE_TYPE="raw_roi_iou"))
    # no gt rows at all: one box of zeros, nothing read
    r, s, l, g = inputs(2, 5, 7)
    out = ops.roi_targets(r, s, l, g[:, :0], dict(cfg, ROI_PER_IMAGE=4))
    assert not out["gt_of_rois_src"].any() and not out["gt_iou_of_rois"].any() and bool((out["rois"] != 0).all())
