"""CPU: the numpy restatement of the box decoding (tests/box_decode_seq.py) against the boxes recorded
from the reference's own generate_predicted_boxes methods (tests/golden/box_decode.npz): bit for bit on the columns made of
+ - * / floor only (z, the extra columns, the heading rt + ra with the direction rule, the RoI heading), within the derived
bound of the exact value everywhere else -- for the restatement and the recording alike -- and with equal NaN / inf / zero
patterns.  x, y and the sizes are NOT compared bit for bit: float32 torch.sqrt and torch.exp on the CPU are not correctly
rounded, so the reference is not its own bit-exact oracle.  Then the named cases, and every NotImplementedError / ValueError of
the three drop-in methods, each one step past its limit, raised before anything reaches the device."""
import os

import numpy as np
import pytest
import torch

import box_decode_seq as seq
from box_decode_cases import CASES, MID, TILE_ROWS
from modest_amd import ops
from modest_amd.utils import box_decode as bd

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "box_decode.npz")
F = np.float32
SCENES = ["anchor_code7_dir", "anchor_code9_dir", "anchor_code7", "anchor_sincos", "point_k3", "point_k1", "point_no_mean",
          "roi_2x3", "roi_4x100"]


@pytest.fixture(scope="module")
def gold():
    return {name: (case, out) for name, case, out in seq.scenes(dict(np.load(GOLD)))}


def test_the_recorded_scenes_are_the_ones_asked_for(gold):
    assert list(gold) == SCENES
    shape = {n: seq.restate_shape(c) for n, (c, _) in gold.items()}
    assert shape["anchor_code7_dir"] == (2, 24, 7) and shape["anchor_code9_dir"] == (2, 24, 9) and shape["anchor_sincos"] == (2, 24, 7)
    assert gold["anchor_code7"][0]["dir"] is None and gold["anchor_code7_dir"][0]["dir"].shape == (2, 24, 2)
    assert gold["anchor_sincos"][0]["sincos"] and gold["anchor_sincos"][0]["box"].shape[-1] == 8
    assert gold["point_k3"][0]["cls"].shape[1] == 3 and gold["point_k1"][0]["cls"].shape[1] == 1
    assert gold["point_no_mean"][0]["mean"] is None and gold["point_k3"][0]["mean"].shape == (3, 3)
    assert gold["roi_2x3"][0]["rois"].shape == (2, 3, 7) and gold["roi_4x100"][0]["rois"].shape == (4, 100, 7)
    assert os.path.getsize(GOLD) <= 128 * 1024


@pytest.mark.parametrize("name", SCENES)
def test_restatement_against_the_recording(gold, name):
    case, rec = gold[name]
    ours = seq.restate(case)
    rec = rec.reshape(ours.shape)
    cols = seq.exact_columns(case)
    why = seq.report(ours[..., cols], rec[..., cols], f"columns {cols}:")
    assert not why, why
    ex = seq.exact(case)
    free = [k for k in range(ours.shape[-1]) if k not in cols]          # the columns that are only bounded
    ratios = {}
    for who, got in (("the restatement", ours), ("the reference", rec)):
        why, _ = seq.bound_report(got, ex, who)
        assert not why, why
        _, ratios[who] = seq.bound_report(got[..., free], (ex[0][..., free], ex[1][..., free], None), who)
    print(f"{name}: largest error / bound on columns {free}: {ratios}")
    why = seq.pattern_report(ours, rec)
    assert not why, why


def test_the_recorded_rois_carry_their_edges(gold):
    case, rec = gold["roi_4x100"]
    rec = rec.reshape(400, 7)
    assert np.isposinf(rec[5, 2]) and np.isnan(rec[5, 0]) and np.isnan(rec[5, 1])          # zg infinite: x and y NaN through zg * 0
    assert np.isnan(rec[6, 2]) and np.isinf(rec[7, 3])                                       # xg infinite: z NaN; exp(89) overflows


@pytest.mark.parametrize("name", sorted(CASES) + ["mid_" + k for k in MID])
def test_named_cases_lie_within_their_bound(name):
    case = MID[name[4:]] if name.startswith("mid_") else CASES[name]
    out = seq.restate(case)
    assert out.shape == seq.restate_shape(case) and out.dtype == F
    why, _ = seq.bound_report(out, seq.exact(case), name)
    assert not why, why


def test_the_cases_hold_what_their_names_say():
    assert {f"{k}_rows{n}" for n in TILE_ROWS for k in ("anchor", "anchor_code8", "point", "roi", "roi_code9")} <= set(CASES)
    assert TILE_ROWS == (1, 63, 64, 65, 255, 256, 257, 513) and (63 * 7) % 4 and (257 * 7) % 4      # tiles off the 16-byte path
    # the argmax rule on its own
    x = np.array([[1, 3, 3], [np.nan, 5, np.nan], [2, np.nan, np.nan], [0, 0, 0], [-np.inf, -np.inf, -np.inf], [-0.0, 0.0, 0.0]], dtype=F)
    assert seq.argmax_rule(x).tolist() == [1, 0, 1, 0, 0, 0]
    assert seq.argmax_rule(x).tolist() == torch.from_numpy(x).max(dim=-1)[1].tolist()              # torch's own rule on the CPU
    for name in ("anchor_argmax_bins8", "point_argmax_k32"):
        logits = CASES[name]["dir"][0] if "dir" in CASES[name] else CASES[name]["cls"]
        assert seq.argmax_rule(logits).tolist() == torch.from_numpy(logits).max(dim=-1)[1].tolist()
    # bin edges: exact integers of v / period + dir_limit_offset, and both neighbours
    c = CASES["anchor_bin_edges_bins2"]
    v = c["box"][0, :15, 6] - F(c["dir_offset"])
    q = v / seq.period_of(2) + F(c["dir_limit_offset"])
    assert (q == np.round(q)).sum() >= 3 and (np.floor(q[0::3]) < np.floor(q[2::3])).any()
    # non-finite encodings reach the output as inf / NaN, and 0 * inf as NaN
    out = seq.restate(CASES["anchor_nonfinite"])[1]
    assert np.isposinf(out[0, 3]) and out[1, 3] == 0 and np.isnan(out[2, 3]) and np.isposinf(out[3, 3]) and np.isnan(out[4, 0])
    out = seq.restate(CASES["anchor_sincos_zeros"])[0]
    assert out[8, 6] == 0 and out[9, 6] == 0 and out[4, 6] == F(-np.pi) and out[5, 6] == F(np.pi)      # atan2(0, 0), atan2(-+0, -1)
    out = seq.restate(CASES["point_atan2_zeros"])
    assert [float(v) for v in out[:4, 6]] == [0.0, -0.0, float(F(np.pi)), float(F(-np.pi))] and np.signbit(out[1, 6])
    out = seq.restate(CASES["roi_nonfinite"])
    assert np.isposinf(out[6, 2]) and np.isnan(out[6, 0]) and np.isnan(out[6, 1]) and np.isnan(out[4, 2])


def test_flat_anchors_moved_and_unchanged():
    from modest_amd.utils import _anchors, anchor_head_loss
    assert anchor_head_loss._flat_anchors is _anchors.flat_anchors is bd.flat_anchors
    per_class = seq.anchor_grid(extra=2, seed=3)
    head, _ = seq.bare_head(seq.make_anchor(1, B=1, N=24, extra=2, anchors=seq.flat_anchors(per_class)), per_class=per_class)
    flat = bd.flat_anchors(head)
    assert np.array_equal(flat.numpy(), seq.flat_anchors(per_class)) and bd.flat_anchors(head) is flat


# ---------------------------------------------------------------------------------------------- what is not provided, and the limits
def call(case, per_class=None, **change):
    head, args = seq.bare_head(case, per_class=per_class)
    for k, v in change.items():
        setattr(head, k, v)
    return head, args


def test_every_option_that_is_not_provided_is_named():
    anchor, point, roi = seq.make_anchor(1, B=2, N=24, bins=2), seq.make_point(2, N=30), seq.make_roi(3, B=2, M=5)
    # list-valued predictions (USE_MULTIHEAD)
    head, (B, cls, box, dirp) = call(anchor)
    for args in ((B, [cls], box, dirp), (B, cls, [box], dirp), (B, cls, box, [dirp])):
        with pytest.raises(NotImplementedError, match="USE_MULTIHEAD"):
            head.generate_predicted_boxes(*args)
    head, args = call(anchor, use_multihead=True)
    with pytest.raises(NotImplementedError, match="USE_MULTIHEAD"):
        head.generate_predicted_boxes(*args)
    head, (pts, cls, box) = call(point)
    with pytest.raises(NotImplementedError, match="list-valued"):
        head.generate_predicted_boxes(pts, [cls], box)
    head, (B, rois, cls, box) = call(roi)
    with pytest.raises(NotImplementedError, match="list-valued"):
        head.generate_predicted_boxes(B, rois, cls, [box])
    # the coder
    for case in (anchor, point, roi):
        for name in ("PreviousResidualDecoder", "PreviousResidualRoIDecoder", "MyCoder"):
            head, args = call(case, box_coder=seq.coder_stub(name, code_size=7))
            with pytest.raises(NotImplementedError, match=f"box_coder = {name}"):
                head.generate_predicted_boxes(*args)
    head, args = call(point, box_coder=seq.coder_stub("ResidualCoder", code_size=8))
    with pytest.raises(NotImplementedError, match="PointResidualCoder only"):
        head.generate_predicted_boxes(*args)
    head, args = call(anchor, box_coder=seq.coder_stub("PointResidualCoder", code_size=8))
    with pytest.raises(NotImplementedError, match="ResidualCoder only"):
        head.generate_predicted_boxes(*args)
    head, args = call(roi, box_coder=seq.coder_stub("ResidualCoder", code_size=8, encode_angle_by_sincos=True))
    with pytest.raises(NotImplementedError, match="encode_angle_by_sincos on a RoI head"):
        head.generate_predicted_boxes(*args)
    # predictions that are not float32
    head, (B, cls, box, dirp) = call(anchor)
    with pytest.raises(NotImplementedError, match="box_preds of torch.float16"):
        head.generate_predicted_boxes(B, cls, box.half(), dirp)
    with pytest.raises(NotImplementedError, match="dir_cls_preds of torch.float16"):
        head.generate_predicted_boxes(B, cls, box, dirp.half())
    head, (pts, cls, box) = call(point)
    with pytest.raises(NotImplementedError, match="point_box_preds of torch.bfloat16"):
        head.generate_predicted_boxes(pts, cls, box.bfloat16())
    with pytest.raises(NotImplementedError, match="point_cls_preds of torch.float16"):
        head.generate_predicted_boxes(pts, cls.detach().half(), box)
    head, (B, rois, cls, box) = call(roi)
    with pytest.raises(NotImplementedError, match="box_preds of torch.float64"):
        head.generate_predicted_boxes(B, rois, cls, box.double())


def test_every_limit_raises_one_step_past_it():
    assert (ops.BOX_DECODE_MAX_CODE, ops.BOX_DECODE_MAX_BINS, ops.BOX_DECODE_MAX_CLASS, ops.BOX_DECODE_MAX_ROWS) == (16, 8, 32, (1 << 31) - 1)
    assert (seq.MAX_CODE, seq.MAX_BINS, seq.MAX_CLASS, seq.MAX_ROWS) == (16, 8, 32, (1 << 31) - 1)
    past = ops.BOX_DECODE_MAX_ROWS + 1
    # ---- anchor head: code 17 (10 extra columns), bins 0 and 9, rows
    head, args = call(seq.make_anchor(1, B=1, N=24, extra=10, bins=2))
    with pytest.raises(ValueError, match="code size = 17 is outside the limit of 7 .. 16"):
        head.generate_predicted_boxes(*args)
    for bins in (0, 9):
        head, (B, cls, box, dirp) = call(seq.make_anchor(1, B=1, N=24, bins=2))
        head.model_cfg["NUM_DIR_BINS"] = bins
        with pytest.raises(ValueError, match=f"NUM_DIR_BINS = {bins} is outside the limit of 1 .. 8"):
            head.generate_predicted_boxes(B, cls, box, dirp)
    head, (B, cls, box, dirp) = call(seq.make_anchor(1, B=1, N=24, bins=2))
    head.model_cfg["NUM_DIR_BINS"] = 3
    with pytest.raises(ValueError, match="dir_cls_preds has 48 elements, expected 1 \\* 24 rows of NUM_DIR_BINS = 3"):
        head.generate_predicted_boxes(B, cls, box, dirp)
    with pytest.raises(ValueError, match="code size = 6 does not go with anchors of 7 columns"):
        head.generate_predicted_boxes(B, cls, box[:, :144], None)
    B = -(-past // 24)
    with pytest.raises(ValueError, match=f"box_preds has {B * 24} rows, above the limit of {ops.BOX_DECODE_MAX_ROWS}"):
        head.generate_predicted_boxes(B, cls, torch.zeros(1, 1).expand(B, 24 * 7), None)
    # ---- point head: code 7 and 17, K 0 and 33, rows, a mean size without a row for a class
    for extra, code in ((-1, 7), (9, 17)):
        case = seq.make_point(2, N=30, extra=max(extra, 0))
        head, (pts, cls, box) = call(case)
        box = box[:, :7] if extra < 0 else box
        with pytest.raises(ValueError, match=f"code size = {code} is outside the limit of 8 .. 16"):
            head.generate_predicted_boxes(pts, cls, box)
    head, (pts, cls, box) = call(seq.make_point(2, N=30))
    for K in (0, 33):
        with pytest.raises(ValueError, match=f"num_class = {K} is outside the limit of 1 .. 32"):
            head.generate_predicted_boxes(pts, torch.zeros((30, K)), box)
    with pytest.raises(ValueError, match="mean_size \\(3, 3\\) has no row for each of the 4 classes"):
        head.generate_predicted_boxes(pts, torch.zeros((30, 4)), box)
    with pytest.raises(ValueError, match=f"point_box_preds has {past} rows, above the limit of {ops.BOX_DECODE_MAX_ROWS}"):
        head.generate_predicted_boxes(pts, torch.zeros(1, 1).expand(past, 3), torch.zeros(1, 1).expand(past, 8))
    # ---- RoI head: code 6 and 17, rows, rois of another width
    for code in (6, 17):
        head, (B, rois, cls, box) = call(seq.make_roi(3, B=2, M=5))
        head.box_coder.code_size = code
        with pytest.raises(ValueError, match=f"code size = {code} is outside the limit of 7 .. 16"):
            head.generate_predicted_boxes(B, rois, cls, box)
    head, (B, rois, cls, box) = call(seq.make_roi(3, B=2, M=5))
    with pytest.raises(ValueError, match="must hold the same rows of the code size 7"):
        head.generate_predicted_boxes(B, rois[:, :4], cls, box)
    with pytest.raises(ValueError, match=f"box_preds has {past} rows, above the limit of {ops.BOX_DECODE_MAX_ROWS}"):
        head.generate_predicted_boxes(1, torch.zeros(1, 1, 1).expand(1, past, 7), cls, torch.zeros(1, 1).expand(past, 7))
    # ---- everything in order but the device: the refusal is the op's, and the inputs are left as found
    for case in (seq.make_anchor(1, B=1, N=24, bins=2), seq.make_point(2, N=30), seq.make_roi(3, B=2, M=5)):
        head, args = call(case)
        before = [a.clone() if torch.is_tensor(a) else a for a in args]
        with pytest.raises(ValueError, match="must be a device tensor"):
            head.generate_predicted_boxes(*args)
        assert all(torch.equal(a, b) for a, b in zip(args, before) if torch.is_tensor(a))
