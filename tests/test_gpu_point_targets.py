"""GPU: modest_amd.ops.point_targets and the drop-in assign_stack_targets (csrc/point_targets.hip)
against the numpy restatement tests/point_targets_seq.py, bit for bit (a NaN equal to a NaN), on the cases of
tests/point_targets_cases.py -- each asserts from its inputs that the edge it is named after is present -- and against the
outputs recorded from the reference's own assign_stack_targets (tests/golden/point_targets.npz): labels and box labels
bit for bit, part labels within the bound section 7l derives from the inputs.  Every case also runs into outputs filled
with a sentinel (none survives), twice (identical bits) and through a non-contiguous gt tensor.  The cases of PAST (past
two and three tiles of boxes, up to 40 rounds in a workgroup, samples nobody names, 79 workgroups) run the same checks
and four layouts in which the gt and the enlarged boxes differ in every stride; the scene of
tests/golden/point_targets_crowd.npz (140 rows) runs with the five of the first fixture."""
import os
import types

import numpy as np
import pytest
import torch

import point_targets_cases as cases
import point_targets_seq as seq
from modest_amd import ops
from modest_amd.utils import point_head_targets as pht

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "point_targets.npz")
GOLD_CROWD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "point_targets_crowd.npz")
F = np.float32
KEYS = ("point_cls_labels", "point_box_labels", "point_part_labels")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def crowd():
    return dict(np.load(GOLD_CROWD))


def strided_copy(t):
    """t (B, M, 8) as every second row and column of a larger tensor, the batch dimension last in memory"""
    wide = torch.full((t.shape[1] * 2 + 1, t.shape[2] * 2 + 1, max(t.shape[0], 1)), 7.0, device=t.device)
    view = wide[::2, 1::2, :][:t.shape[1], :t.shape[2], :t.shape[0]].permute(2, 0, 1)
    view.copy_(t)
    assert view.shape == t.shape and (t.numel() <= 8 or not view.is_contiguous())
    return view


def device_inputs(c, strided=False):
    dev = torch.device("cuda")
    pts, gt, ext = (torch.from_numpy(c[k]).to(dev) for k in ("points", "gt", "ext"))
    if strided:
        gt, ext = strided_copy(gt), strided_copy(ext)
    mean = None if c["mean"] is None else torch.from_numpy(np.ascontiguousarray(c["mean"])).to(dev)
    return pts, gt, ext, mean


def to_host(out):
    return {k: None if v is None else v.cpu().numpy() for k, v in zip(KEYS, out)}


def run(c, strided=False, out=None):
    pts, gt, ext, mean = device_inputs(c, strided)
    res = ops.point_targets(pts, gt, ext, c["num_class"], mean_size=mean, want_box=c["want_box"], want_part=c["want_part"],
                            out=out)
    assert res[0].dtype == torch.int64 and res[0].shape == (len(c["points"]),)
    assert (res[1] is None) == (not c["want_box"]) and (res[2] is None) == (not c["want_part"])
    return to_host(res)


def sentinel_outputs(c):
    dev = torch.device("cuda")
    n = len(c["points"])
    labels = torch.full((n,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    box = torch.full((n, 8), 0x5A5A5A5A, dtype=torch.int32, device=dev).view(torch.float32) if c["want_box"] else None
    part = torch.full((n, 3), 0x5A5A5A5A, dtype=torch.int32, device=dev).view(torch.float32) if c["want_part"] else None
    return labels, box, part


@pytest.mark.parametrize("name", list(cases.CASES))
def test_cases_against_the_restatement(name):
    c = cases.CASES[name]()
    assert c["present"](c), "the case does not hold its edge"
    assert c["gt"].shape[0] <= 3 and len(c["points"]) <= 1600 and c["gt"].shape[1] <= cases.TILE + 1
    want = cases.run(c)
    got = run(c)
    why = seq.mismatches(got, want)
    assert not why, "against the restatement\n" + "\n".join(why)
    # into outputs the test filled: the same objects come back, the same bits, no sentinel is left
    out = sentinel_outputs(c)
    res = ops.point_targets(*device_inputs(c)[:3], c["num_class"], mean_size=device_inputs(c)[3], want_box=c["want_box"],
                            want_part=c["want_part"], out=out)
    assert all(a is b for a, b in zip(res, out))
    again = to_host(res)
    assert not seq.mismatches(again, want), "into given outputs"
    assert not (again["point_cls_labels"] == 0x5A5A5A5A5A5A5A5A).any()
    for k in KEYS[1:]:
        if again[k] is not None:
            assert not (seq.bits(again[k]) == 0x5A5A5A5A).any(), k
    for k in KEYS:   # two runs: identical bytes, NaN payloads included
        assert (got[k] is None and again[k] is None) or got[k].tobytes() == again[k].tobytes(), k
    why = seq.mismatches(run(c, strided=True), want)
    assert not why, "a non-contiguous gt tensor\n" + "\n".join(why)


def call(c, pts, gt, ext, mean, out=None):
    return ops.point_targets(pts, gt, ext, c["num_class"], mean_size=mean, want_box=c["want_box"], want_part=c["want_part"],
                             out=out)


@pytest.mark.parametrize("name", list(cases.PAST))
def test_past_the_tile_against_the_restatement(name):
    c = cases.past(name)
    want = c["want"]
    pts, gt, ext, mean = device_inputs(c)
    got = to_host(call(c, pts, gt, ext, mean))
    why = seq.mismatches(got, want)
    assert not why, "against the restatement\n" + "\n".join(why)


@pytest.mark.parametrize("name", list(cases.PAST))
def test_past_the_tile_into_given_outputs_and_twice(name):
    c = cases.past(name)
    want = c["want"]
    pts, gt, ext, mean = device_inputs(c)
    out = sentinel_outputs(c)
    res = call(c, pts, gt, ext, mean, out=out)
    assert all(a is b for a, b in zip(res, out))
    first = to_host(res)
    assert not seq.mismatches(first, want), "into given outputs"
    assert not (first["point_cls_labels"] == 0x5A5A5A5A5A5A5A5A).any()
    for k in KEYS[1:]:
        assert not (seq.bits(first[k]) == 0x5A5A5A5A).any(), k
    again = to_host(call(c, pts, gt, ext, mean))
    for k in KEYS:   # two runs: identical bytes, NaN payloads included
        assert first[k].tobytes() == again[k].tobytes(), k


def permuted_copy(t, order):
    """t (B, M, 8) stored with its dimensions in `order` (a permutation of 0, 1, 2), as a view of shape (B, M, 8)"""
    stored = t.permute(*order).contiguous()
    view = stored.permute(*[order.index(d) for d in range(3)])
    assert view.shape == t.shape and torch.equal(view, t)
    return view


LAYOUTS = {
    "gt contiguous, ext strided": (lambda t: t.contiguous(), strided_copy),
    "gt strided, ext contiguous": (strided_copy, lambda t: t.contiguous()),
    "gt as (8, B, M), ext as (M, 8, B)": (lambda t: permuted_copy(t, (2, 0, 1)), lambda t: permuted_copy(t, (1, 2, 0))),
    "gt as (M, 8, B), ext as (8, B, M)": (lambda t: permuted_copy(t, (1, 2, 0)), lambda t: permuted_copy(t, (2, 0, 1))),
}


@pytest.mark.parametrize("name", list(cases.PAST))
def test_past_the_tile_with_unequal_box_strides(name):
    c = cases.past(name)
    pts, gt, ext, mean = device_inputs(c)
    for layout, (lay_gt, lay_ext) in LAYOUTS.items():
        g, e = lay_gt(gt), lay_ext(ext)
        assert all(a != b for a, b in zip(g.stride(), e.stride())), (layout, g.stride(), e.stride())
        why = seq.mismatches(to_host(call(c, pts, g, e, mean)), c["want"])
        assert not why, layout + "\n" + "\n".join(why)


def test_the_same_boxes_for_every_sample():
    """a batch stride of 0: gt one (1, M, 8) tensor expanded over B samples beside a materialised enlargement, then the
    enlarged boxes expanded beside a materialised gt"""
    B, M = 4, 2 * cases.TILE + 5
    pts, one = cases.random_scene(50, 1, M, 1200, live=[M])
    pts[:, 0] = np.arange(len(pts)) * B // len(pts)                 # the same boxes, four samples' points
    gt = np.ascontiguousarray(np.broadcast_to(one, (B, M, 8)))
    c = cases.case(pts, gt, None)
    want = cases.run(c)
    k, idx, hit = seq.membership(c["points"], c["gt"], c["ext"])
    assert set(k[idx >= 0]) == set(range(B)) and set(idx[idx >= 0] // cases.TILE) == {0, 1, 2} and bool((hit & (idx < 0)).any())
    dev = torch.device("cuda")
    p, mean = torch.from_numpy(c["points"]).to(dev), torch.from_numpy(c["mean"]).to(dev)
    g1, e1 = torch.from_numpy(c["gt"][:1]).to(dev), torch.from_numpy(c["ext"][:1]).to(dev)
    g, e = torch.from_numpy(c["gt"]).to(dev), torch.from_numpy(c["ext"]).to(dev)
    for gt_t, ext_t in ((g1.expand(B, M, 8), e), (g, e1.expand(B, M, 8))):
        assert 0 in (gt_t.stride(0), ext_t.stride(0)) and gt_t.stride(0) != ext_t.stride(0)
        why = seq.mismatches(to_host(call(c, p, gt_t, ext_t, mean)), want)
        assert not why, "\n".join(why)


def test_fixture_scenes(gold, crowd):
    for rec, name in [(rec, name) for rec in (gold, crowd) for name in seq.scenes(rec)]:
        cfg, pts, gt, ext, mean = seq.scene_inputs(rec, name)
        c = dict(points=pts, gt=gt, ext=ext, num_class=cfg["num_class"], mean=mean, want_box=cfg["want_box"],
                 want_part=cfg["want_part"])
        got = run(c)
        bound = seq.part_bound(pts, gt, ext, cfg["want_box"]) if cfg["want_part"] else None
        why = seq.mismatches(got, seq.recorded(rec, name), bound=bound)
        assert not why, f"{name} against the reference\n" + "\n".join(why)
        why = seq.mismatches(got, cases.run(c))
        assert not why, f"{name} against the restatement\n" + "\n".join(why)


def test_the_drop_in_method_is_the_op_and_does_not_synchronise():
    c = cases.CASES["grouped, three samples"]()
    pts, gt, ext, mean = device_inputs(c)
    coder = types.SimpleNamespace(use_mean_size=True, mean_size=mean.clone(), code_size=8)
    head = pht.bind(type("Head", (), {}))()
    head.num_class, head.box_coder = 3, coder
    want = to_host(ops.point_targets(pts, gt, ext, 3, mean_size=mean, want_box=True, want_part=True))
    head.assign_stack_targets(pts, gt, extend_gt_boxes=ext, ret_box_labels=True)   # uploads and caches the table
    cached = coder._modest_mean_size[2]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(side):
            out = head.assign_stack_targets(pts, gt, extend_gt_boxes=ext, ret_box_labels=True, ret_part_labels=True,
                                            set_ignore_flag=True, use_ball_constraint=False)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    side.synchronize()
    assert coder._modest_mean_size[2] is cached and list(out) == list(KEYS)
    assert not seq.mismatches({k: v.cpu().numpy() for k, v in out.items()}, want)
    only = head.assign_stack_targets(pts, gt, extend_gt_boxes=ext)
    assert only["point_box_labels"] is None and only["point_part_labels"] is None
    assert np.array_equal(only["point_cls_labels"].cpu().numpy(), want["point_cls_labels"])
    # a coder without mean sizes, its table given as a list on another head
    plain = pht.bind(type("Head", (), {}))()
    plain.num_class, plain.box_coder = 3, types.SimpleNamespace(use_mean_size=False)
    got = plain.assign_stack_targets(pts, gt, extend_gt_boxes=ext, ret_box_labels=True)
    ref = to_host(ops.point_targets(pts, gt, ext, 3, mean_size=None, want_box=True))
    assert seq.same_bits(got["point_box_labels"].cpu().numpy(), ref["point_box_labels"])
    listed = pht.bind(type("Head", (), {}))()
    listed.num_class, listed.box_coder = 3, types.SimpleNamespace(use_mean_size=True, mean_size=c["mean"].tolist())
    got = listed.assign_stack_targets(pts, gt, extend_gt_boxes=ext, ret_box_labels=True)
    assert seq.same_bits(got["point_box_labels"].cpu().numpy(), want["point_box_labels"])


def test_points_rows_may_be_strided():
    c = cases.CASES["N = 257"]()
    dev = torch.device("cuda")
    wide = torch.full((len(c["points"]), 7), 3.0, device=dev)
    wide[:, :4] = torch.from_numpy(c["points"]).to(dev)
    _, gt, ext, mean = device_inputs(c)
    view = wide[:, :4]
    assert not view.is_contiguous()
    got = to_host(ops.point_targets(view, gt, ext, 3, mean_size=mean, want_box=True, want_part=True))
    assert not seq.mismatches(got, cases.run(c))
    # columns two elements apart: the wrapper hands the kernel a contiguous copy
    wide = torch.full((len(c["points"]), 9), 3.0, device=dev)
    wide[:, 0:8:2] = torch.from_numpy(c["points"]).to(dev)
    view = wide[:, ::2][:, :4]
    assert view.stride(1) == 2 and view.shape == (len(c["points"]), 4)
    got = to_host(ops.point_targets(view, gt, ext, 3, mean_size=mean, want_box=True, want_part=True))
    assert not seq.mismatches(got, cases.run(c))


def test_arguments_are_validated():
    c = cases.CASES["N = 65"]()
    pts, gt, ext, mean = device_inputs(c)
    good = dict(mean_size=mean, want_box=True, want_part=True)
    with pytest.raises(ValueError, match="device"):
        ops.point_targets(pts.cpu(), gt, ext, 3, **good)
    with pytest.raises(ValueError, match="float32"):
        ops.point_targets(pts.double(), gt, ext, 3, **good)
    with pytest.raises(ValueError, match=r"\(N, 4\)"):
        ops.point_targets(pts[:, :3], gt, ext, 3, **good)
    with pytest.raises(ValueError, match=r"\(B, M, 8\)"):
        ops.point_targets(pts, gt[:, :, :7], ext[:, :, :7], 3, **good)
    with pytest.raises(ValueError, match=r"\(B, M, 8\)"):
        ops.point_targets(pts, gt, ext[:, :-1], 3, **good)
    with pytest.raises(ValueError, match="mean_size"):
        ops.point_targets(pts, gt, ext, 3, mean_size=mean[:, :2], want_box=True)
    with pytest.raises(ValueError, match="out point_box_labels"):
        ops.point_targets(pts, gt, ext, 3, **good, out=(torch.empty(65, dtype=torch.int64, device="cuda"), None,
                                                        torch.empty((65, 3), device="cuda")))
    with pytest.raises(ValueError, match="shape"):
        ops.point_targets(pts, gt, ext, 3, **good, out=(torch.empty(65, dtype=torch.int64, device="cuda"),
                                                        torch.empty((65, 7), device="cuda"), torch.empty((65, 3), device="cuda")))
    with pytest.raises(ValueError, match="not asked for"):
        ops.point_targets(pts, gt, ext, 3, out=(torch.empty(65, dtype=torch.int64, device="cuda"),
                                                torch.empty((65, 8), device="cuda"), None))
