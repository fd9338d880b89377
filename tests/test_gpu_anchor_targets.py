"""GPU: modest_amd.utils.target_assigner.AxisAlignedTargetAssigner (csrc/anchor_targets.hip)
against the outputs recorded from the reference's own assigner (tests/golden/anchor_targets.npz) and against the numpy
restatement tests/anchor_targets_seq.py: labels, weights and every target column bit for bit; against the reference the two
sincos columns to the bound derived in section 7i.  A mismatch reports (sample, anchor, class) and the IoUs involved.
The cases of tests/anchor_targets_cases.py cross the kernels' constants (64 gt rows per ballot, 256 gts per LDS tile, 256
anchors per workgroup, classes of unequal length); they also run into sentinel-filled outputs with a pre-filled workspace."""
import os

import numpy as np
import pytest
import torch

import anchor_targets_cases as cases
import anchor_targets_seq as seq
from modest_amd import ops
from modest_amd.utils import target_assigner as ta

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "anchor_targets.npz")
F = np.float32
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def assigner_of(cfg):
    return ta.AxisAlignedTargetAssigner(seq.model_cfg(cfg), cfg["class_names"], seq.Coder(cfg))


def run(cfg, anchors, gt, assigner=None, strided=False):
    dev = torch.device("cuda")
    a = assigner or assigner_of(cfg)
    g = torch.from_numpy(np.ascontiguousarray(gt)).to(dev)
    if strided:   # every second row and column of a larger tensor, the batch dimension last in memory
        wide = torch.full((g.shape[1] * 2, g.shape[2] * 2 + 1, g.shape[0]), 7.0, device=dev)
        view = wide[::2, 1::2, :][:, :g.shape[2], :].permute(2, 0, 1)
        view.copy_(g)
        assert not view.is_contiguous() and view.shape == g.shape
        g = view
    out = a.assign_targets([torch.from_numpy(x).to(dev) for x in anchors], g)
    assert out["box_cls_labels"].dtype == torch.int32 and out["box_reg_targets"].dtype == torch.float32
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("name", ["small", "big", "multi", "lyft", "crowd", "crowd_multi"])
def test_fixture_scenes(gold, name):
    cfg, gt = next((c, g) for n, c, g in seq.scenes(gold) if n == name)
    anchors = seq.make_anchors(cfg)
    got = run(cfg, anchors, gt)
    why = seq.report(got, seq.recorded(gold, name), cfg, anchors, gt, sincos_cols_bounded=bool(cfg["sincos"]))
    assert not why, f"against the reference\n{why}"
    why = seq.report(got, seq.assign(cfg, anchors, gt), cfg, anchors, gt)
    assert not why, f"against the restatement\n{why}"
    why = seq.report(run(cfg, anchors, gt, strided=True), got, cfg, anchors, gt)
    assert not why, f"a non-contiguous gt tensor\n{why}"


# ---- small random shapes ----------------------------------------------------------------------------------------------
def head_cfg(grid, multi):
    nx, ny = grid
    c = lambda n, s, z, m, u: dict(class_name=n, anchor_sizes=[s], anchor_rotations=[0, 1.57], anchor_bottom_heights=[z],   # noqa: E731
                                   align_center=False, matched_threshold=m, unmatched_threshold=u, grid_size=[nx, ny])
    return dict(anchor_range=[0, -1.5 * (ny - 1), -3, 3.0 * (nx - 1), 1.5 * (ny - 1), 1], use_multihead=multi,
                code_size=9 if multi else 7, sincos=multi, class_names=["Car", "Pedestrian", "Cyclist", "Van"],
                classes=[c("Car", [3.9, 1.6, 1.56], -1.78, 0.6, 0.45), c("Pedestrian", [0.8, 0.6, 1.73], -0.6, 0.5, 0.35),
                         c("Cyclist", [1.76, 0.6, 1.73], -0.6, 0.5, 0.35)])


def random_gt(rs, cfg, anchors, counts, pad=3):
    """(B, max(counts) + pad, cols) gts near anchors of their class, one in five of a class without anchors or far away"""
    cols = 8 + (2 if cfg["code_size"] == 9 else 0)
    gt = np.zeros((len(counts), max(counts) + pad, cols), dtype=F)
    for b, n in enumerate(counts):
        for j in range(n):
            ci = rs.randint(len(anchors))
            flat = seq.flatten(anchors[ci], False)
            a = flat[rs.randint(len(flat))]
            size = a[3:6] * rs.uniform(0.8, 1.25, 3)
            row = [a[0] + rs.normal(0, 0.3) * a[3], a[1] + rs.normal(0, 0.3) * a[4], a[2] + rs.normal(0, 0.2), *size,
                   a[6] + rs.normal(0, 0.25) + np.pi * rs.randint(-3, 4)]
            row += list(rs.normal(0, 2, cols - 8)) + [ci + 1]
            kind = rs.randint(10)
            if kind == 0:
                row[-1] = 4          # Van: no anchors
            elif kind == 1:
                row[0] += 1000.0     # far from every anchor
            gt[b, j] = row
    return gt


SHAPES = {70: ((7, 5), False), 512: ((16, 16), True), 2640: ((40, 33), False)}


@pytest.mark.parametrize("counts", [(0,), (1,), (2,), (12,), (12, 0, 2), (1, 12, 12)], ids=str)
@pytest.mark.parametrize("per_class", [70, 512, 2640])
def test_random_shapes_against_the_restatement(per_class, counts):
    grid, multi = SHAPES[per_class]
    cfg = head_cfg(grid, multi)
    anchors = seq.make_anchors(cfg)
    assert all(int(np.prod(a.shape[:5])) == per_class for a in anchors)
    rs = np.random.RandomState(per_class + 7 * sum(counts) + len(counts))
    gt = random_gt(rs, cfg, anchors, counts)
    ref = seq.assign(cfg, anchors, gt)
    got = run(cfg, anchors, gt, strided=len(counts) > 1)
    why = seq.report(got, ref, cfg, anchors, gt)
    assert not why, why
    if max(counts) >= 12:
        assert (ref["box_cls_labels"] > 0).any()
    if counts == (0,):
        assert not got["box_cls_labels"].any() and not got["box_reg_targets"].any() and not got["reg_weights"].any()


# ---- the full shape ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full():
    """B = 4, 1 x 248 x 280 x 2 anchors of one class (138 880 per sample), 5..25 gts"""
    cfg = dict(anchor_range=[-80, -80, -5, 80, 80, 3], use_multihead=False, code_size=7, sincos=False, class_names=["car"],
               classes=[dict(class_name="car", anchor_sizes=[[4.75, 1.92, 1.71]], anchor_rotations=[0, 1.57],
                             anchor_bottom_heights=[-1.07], align_center=False, matched_threshold=0.5, unmatched_threshold=0.35,
                             grid_size=[280, 248])])
    anchors = seq.make_anchors(cfg)
    assert anchors[0].shape[:5] == (1, 248, 280, 1, 2)
    rs = np.random.RandomState(4)
    counts = (5, 25, 13, 19)
    gt = random_gt(rs, cfg, anchors, counts, pad=5)
    gt[1, 3, 3:5] = (0.9, 0.5)   # a gt so small that every anchor stays below `matched`: only its best anchors are foreground
    dev = torch.device("cuda")
    a = assigner_of(cfg)
    at = [torch.from_numpy(x).to(dev) for x in anchors]
    gd = torch.from_numpy(gt).to(dev)
    out = a.assign_targets(at, gd)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    return dict(cfg=cfg, anchors=anchors, gt=gt, assigner=a, at=at, gd=gd, got=got)


def test_full_shape(full):
    cfg, anchors, gt = full["cfg"], full["anchors"], full["gt"]
    details = []
    ref = seq.assign(cfg, anchors, gt, details)
    d = details[1][0]
    j = int(np.flatnonzero(d["rows"] == 3)[0])
    assert 0 < d["colmax"][j] < d["matched"] and (d["rowmax"][d["iou"][:, j] > 0] < d["matched"]).all()
    assert ref["box_cls_labels"].shape == (4, 138880) and (ref["box_cls_labels"] > 0).sum() > 20 and (ref["box_cls_labels"] < 0).any()
    why = seq.report(full["got"], ref, cfg, anchors, gt)
    assert not why, why


def test_side_stream_without_a_synchronisation(full):
    a, at, gd = full["assigner"], full["at"], full["gd"]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(side):
            out = a.assign_targets(at, gd)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    side.synchronize()
    for k, v in out.items():
        assert np.array_equal(v.cpu().numpy().view(np.uint32), full["got"][k].view(np.uint32)), k


def test_two_calls_are_bit_identical(full):
    a, at, gd = full["assigner"], full["at"], full["gd"]
    one = a.assign_targets(at, gd)
    two = a.assign_targets(at, gd)
    for k in one:
        assert torch.equal(one[k].view(torch.int32), two[k].view(torch.int32)), k
        assert np.array_equal(one[k].cpu().numpy().view(np.uint32), full["got"][k].view(np.uint32)), k
    assert a._device_tables(at) is a._tables   # the tables are built once per list of anchor tensors


# ---- past the kernels' constants (tests/anchor_targets_cases.py) -----------------------------------------------------------
def sentinel_outputs(B, n_out, code, dev):
    fill = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.int32, device=dev)   # noqa: E731
    return fill(B, n_out), fill(B, n_out, code).view(torch.float32), fill(B, n_out).view(torch.float32)


def raw_bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("name", cases.names())
def test_cases_against_the_restatement(name):
    case = cases.by_name(name)
    cfg, gt = case["cfg"], case["gt"].copy()     # the case's own array is read-only
    ref = cases.reference(case)
    anchors, want = ref["anchors"], ref["out"]
    dev = torch.device("cuda")
    a = assigner_of(cfg)
    at = [torch.from_numpy(x).to(dev) for x in anchors]
    gd = torch.from_numpy(gt).to(dev)
    first = a.assign_targets(at, gd)
    got = {k: v.cpu().numpy() for k, v in first.items()}
    why = seq.report(got, want, cfg, anchors, gt)
    assert not why, why
    again = a.assign_targets(at, gd)
    for k in first:
        assert first[k] is not again[k] and np.array_equal(raw_bits(first[k]), raw_bits(again[k])), k
    if gt.size:
        why = seq.report(run(cfg, anchors, gt, strided=True), want, cfg, anchors, gt)
        assert not why, f"a non-contiguous gt tensor\n{why}"
    # the library call itself into sentinel outputs, the workspace pre-filled: every element written, nothing read that
    # was not written first
    t = a._device_tables(at)
    B, M = gt.shape[:2]
    nbytes = ops.anchor_targets_workspace_bytes(B, len(anchors), M)
    for fill in (0xFF, 0x00):
        out = sentinel_outputs(B, t["n_out"], want["box_reg_targets"].shape[-1], dev)
        ws = torch.full((max(nbytes, 256),), fill, dtype=torch.uint8, device=dev)
        res = ops.anchor_targets(gd, t["anchors"], t["cls"], t["thr"], t["match"], t["max_rows"], t["n_out"], a.sincos,
                                 workspace=ws, out=out)
        assert all(r is o for r, o in zip(res, out))
        for r, k in zip(res, ("box_cls_labels", "box_reg_targets", "reg_weights")):
            b = raw_bits(r)
            assert not (b == SENTINEL).any(), f"{k}: {int((b == SENTINEL).sum())} elements never written (workspace fill {fill:#x})"
            assert np.array_equal(b, raw_bits(first[k])), f"{k} differs with the workspace filled with {fill:#x}"
        if B and fill:
            assert not bool((ws[:nbytes] == fill).all()), "the workspace handed in was not the one used"


def test_out_is_validated():
    case = cases.by_name("columns: anchors 7, gt 8")
    dev = torch.device("cuda")
    a = assigner_of(case["cfg"])
    at = [torch.from_numpy(x).to(dev) for x in cases.reference(case)["anchors"]]
    gd = torch.from_numpy(case["gt"].copy()).to(dev)
    t = a._device_tables(at)
    args = (gd, t["anchors"], t["cls"], t["thr"], t["match"], t["max_rows"], t["n_out"], False)
    B, n = gd.shape[0], t["n_out"]
    good = sentinel_outputs(B, n, 7, dev)
    with pytest.raises(TypeError, match="labels"):
        ops.anchor_targets(*args, out=(good[0].float(), good[1], good[2]))
    with pytest.raises(ValueError, match="targets has shape"):
        ops.anchor_targets(*args, out=(good[0], good[1][:, :, :6].contiguous(), good[2]))
    with pytest.raises(ValueError, match="contiguous"):
        ops.anchor_targets(*args, out=(good[0], good[1], torch.zeros((n, B), device=dev).t()))
    with pytest.raises(ValueError, match="device"):
        ops.anchor_targets(*args, out=(good[0].cpu(), good[1], good[2]))
    with pytest.raises(ValueError, match="labels, targets, weights"):
        ops.anchor_targets(*args, out=good[:2])
    assert all((raw_bits(g) == SENTINEL).all() for g in good)      # a refused call writes nothing
