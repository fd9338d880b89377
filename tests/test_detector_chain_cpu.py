"""CPU: the detector chains of tests/detector_chain.py on the restatements alone.  The free-running chains run on both scenes;
the three round trips hold in numpy inside their derived bounds; and the conditions that keep tests/test_gpu_detector_chain.py
from passing vacuously are checked here, on the reference, so that the scenes are fixed by this file and not by what a device
gives: positives of every class, an empty sample, all three point labels, every RoI list, an NMS that suppresses and reaches
its limit, both values of reg_valid_mask, a recall counter strictly inside, final boxes.  Also every ``bind_*`` of
``pcdet_bind`` together with ``install(...)`` against ONE set of fake pcdet modules: every method lands on its template class,
a second round changes nothing, and the modules bound together are the union of what each binder binds alone."""
import sys
import types

import numpy as np
import pytest

import anchor_loss_seq as al
import box_decode_seq as bd
import detector_chain as dc
import proposals_seq as ps

F = np.float32


@pytest.fixture(scope="module")
def chain_a():
    return dc.free_chain_a()


@pytest.fixture(scope="module", params=[(0, "cls"), (0, "roi_iou"), (1, "cls")], ids=lambda p: f"scene{p[0]}-{p[1]}")
def chain_b(request):
    return dc.free_chain_b(*request.param)


# ---------------------------------------------------------------------------------------------------- chain A
def test_chain_a_is_not_vacuous(chain_a):
    r = chain_a
    labels, gt = r["targets"]["box_cls_labels"], r["gt"]
    assert labels.shape == (3, 576) and r["targets"]["box_reg_targets"].shape == (3, 576, 7)
    assert [int(g[:, 3].astype(bool).sum()) for g in gt] == [5, 0, 8] and gt.shape == (3, 8, 8)
    assert all((labels == c).sum() >= 2 for c in (1, 2, 3)), "every class has at least 2 positive anchors"
    assert not labels[1].any() and not r["targets"]["box_reg_targets"][1].any(), "the empty sample has no positive and no ignored anchor"
    assert (labels < 0).any()
    assert np.isfinite(r["loss"]["losses"]).all() and (r["loss"]["losses"] > 0).all()
    assert all(np.abs(r["loss"][k]).max() > 0 for k in ("grad_cls", "grad_box", "grad_dir"))
    preds, recall = r["final"]
    assert len(preds[0][0]) and len(preds[2][0]), "final boxes for the samples that have gts"
    passing = int((dc.pp.sigmoid(ps.score_label(r["preds"]["cls"].reshape(-1, 3))[0]) >= F(dc.A_POST["SCORE_THRESH"])).sum())
    assert sum(len(p[0]) for p in preds) < passing < labels.size      # SCORE_THRESH took rows out, and the NMS more
    assert any(0 < v < recall["gt"] for v in recall["rcnn"]), recall


def test_chain_a_is_deterministic(chain_a):
    again = dc.free_chain_a()
    assert dc.pp.same(again["final"], chain_a["final"])
    assert all(np.array_equal(again["preds"][k], chain_a["preds"][k]) for k in ("cls", "box", "dir"))


def test_anchor_round_trip_in_numpy(chain_a):
    """the assigner's restatement and the decoder's, each with its own statement of the anchors' row order, give every
    positive anchor's gt back; with two classes' anchor tensors swapped they do not, and the loss changes"""
    r = chain_a
    labels, targets = r["targets"]["box_cls_labels"], r["targets"]["box_reg_targets"]
    matched = dc.matched_gt_a(r["details"], r["gt"])
    why = dc.anchor_round_trip(bd.anchor_decode(targets, dc.a_flat()), labels, matched)
    assert not why, why
    # box_preds == box_reg_targets: every difference is x - x
    inp = dc.a_loss_inputs(dict(r["preds"], box=targets), labels, targets)
    zero = al.restate(inp, dc.A_LOSS)
    assert zero["losses"][1] == 0.0 and not zero["grad_box"].any()
    # the swap the chain must notice
    swapped = list(dc.a_anchors())
    swapped[0], swapped[1] = swapped[1], swapped[0]
    flat = bd.flat_anchors(swapped)
    assert dc.anchor_round_trip(bd.anchor_decode(targets, flat), labels, matched)
    full = dc.a_loss_inputs(r["preds"], labels, targets)
    assert al.report(al.restate(dict(full, anchors=flat), dc.A_LOSS), r["loss"])


# ---------------------------------------------------------------------------------------------------- chain B
def test_chain_b_is_not_vacuous(chain_b):
    r = chain_b
    sc, cfg = r["scene"], r["cfg"]
    off = dc.offsets_of(sc["counts"])
    lab = r["ptargets"]["point_cls_labels"]
    gts = [int(g[:, 3].astype(bool).sum()) for g in sc["gt_boxes"]]
    for b in range(sc["B"]):
        mine = lab[off[b]:off[b + 1]]
        if gts[b]:
            assert (mine > 0).any() and (mine < 0).any() and (mine == 0).any(), f"sample {b}: all three point labels"
        else:
            assert not mine.any()
    assert set(np.unique(lab[lab > 0])) == {1, 2, 3}
    counts = r["rdetails"]["counts"]
    assert (counts > 0).any(axis=0).all(), f"each of the fg / hard / easy lists is non-empty in some sample: {counts.tolist()}"
    for b in range(sc["B"]):
        if not gts[b]:
            assert counts[b].tolist() == [0, 0, r["props"][0].shape[1]], "the empty-gt sample is all easy"
    # the NMS of the training proposals binds: it reaches NMS_POST_MAXSIZE and its survivors are not the first candidates
    rois = r["props"][0]
    post = dc.B_TRAIN_NMS["NMS_POST_MAXSIZE"]
    full = (rois[..., 3] != 0).sum(axis=1) == post
    assert full.any()
    score, _ = ps.score_label(r["ppreds"]["cls"])
    cand = ps.candidates(score, ps.sample_of(sc["points"][:, 0], len(score), sc["B"]), sc["B"], dc.B_TRAIN_NMS["NMS_PRE_MAXSIZE"])
    assert any(len(c) > post and not np.array_equal(r["pboxes"][c[:post]], rois[b]) for b, c in enumerate(cand)), "NMS suppresses a box"
    mask = r["rtargets"]["reg_valid_mask"]
    assert mask.shape == (sc["B"], cfg["ROI_PER_IMAGE"]) and set(np.unique(mask)) == {0, 1}
    labels = r["rtargets"]["rcnn_cls_labels"]
    assert labels.dtype == (np.int64 if cfg["CLS_SCORE_TYPE"] == "cls" else np.float32)
    if cfg["CLS_SCORE_TYPE"] == "cls":
        assert set(np.unique(labels)) == {-1, 0, 1}
    else:
        assert ((labels > 0) & (labels < 1)).any() and (labels == 0).any() and (labels == 1).any()
    assert r["rtargets"]["gt_of_rois"].shape[-1] == 8 and r["rtargets"]["roi_labels"].dtype == np.int64
    assert all(p[0].shape == (1, cfg["ROI_PER_IMAGE"], dc.POOL_POINTS, 6) for p in r["pooled"])
    assert np.isfinite(r["ploss"]["table"]).all() and np.isfinite(r["rloss"]["table"]).all() and r["rloss"]["table"][2] > 0
    preds, recall = r["final"]
    assert all(len(preds[b][0]) for b in range(sc["B"]) if gts[b]), "final boxes for the samples that have gts"
    assert any(0 < v < recall["gt"] for v in recall["rcnn"] + recall["roi"]), recall


def test_point_round_trip_in_numpy(chain_b):
    r = chain_b
    sc = r["scene"]
    lab = r["ptargets"]["point_cls_labels"]
    onehot = np.full((len(lab), 3), -5.0, dtype=F)
    fg = lab > 0
    onehot[fg, lab[fg] - 1] = 5.0
    dec = bd.point_decode(r["ptargets"]["point_box_labels"], sc["points"][:, 1:4], onehot, dc.mean_size())
    why = dc.point_round_trip(dec, lab, sc["points"], sc["gt_boxes"], r["member"][1])
    assert not why, why
    wrong = np.roll(onehot, 1, axis=1)            # the mean size of another class: the sizes do not come back
    assert dc.point_round_trip(bd.point_decode(r["ptargets"]["point_box_labels"], sc["points"][:, 1:4], wrong, dc.mean_size()),
                               lab, sc["points"], sc["gt_boxes"], r["member"][1])


def test_roi_round_trip_in_numpy(chain_b):
    t = chain_b["rtargets"]
    reg = dc.roi_encode64(t["gt_of_rois"], t["rois"]).reshape(-1, 7)
    why = dc.roi_round_trip(bd.roi_decode(t["rois"], reg), t)
    assert not why, why
    back = np.array(t["rois"])
    back[..., 6] = -back[..., 6]                  # turned back by -ra instead of +ra: the centres do not come back
    assert dc.roi_round_trip(bd.roi_decode(back, reg), t)


def test_the_second_scene_outgrows_the_first():
    a, b = dc.scene_b(0), dc.scene_b(1)
    assert b["B"] > a["B"] and b["target_cfg"]["ROI_PER_IMAGE"] > a["target_cfg"]["ROI_PER_IMAGE"] and len(b["points"]) < len(a["points"])
    words = [2 * s["B"] * s["target_cfg"]["ROI_PER_IMAGE"] for s in (a, b)]      # the picks table: past pinned_table's floor of 16, and growing
    assert 16 < words[0] < words[1]


# ---------------------------------------------------------------------------------------------------- every binder together
TEMPLATES = {"pcdet.models.dense_heads.anchor_head_template": "AnchorHeadTemplate",
             "pcdet.models.dense_heads.point_head_template": "PointHeadTemplate",
             "pcdet.models.roi_heads.roi_head_template": "RoIHeadTemplate",
             "pcdet.models.detectors.detector3d_template": "Detector3DTemplate",
             "pcdet.models.dense_heads.point_head_box": "PointHeadBox",
             "pcdet.models.dense_heads.point_head_simple": "PointHeadSimple",
             "pcdet.models.dense_heads.point_intra_part_head": "PointIntraPartOffsetHead"}


def binders():
    from modest_amd.utils import pcdet_bind as pb
    return {"install": lambda: pb.install(anchor_targets=True, point_targets=True, proposal_layer=True),
            "roi_targets": pb.bind_roi_targets, "post_processing": pb.bind_post_processing, "anchor_loss": pb.bind_anchor_loss,
            "roi_loss": pb.bind_roi_loss, "point_loss": pb.bind_point_loss, "box_decode": pb.bind_box_decode}


def fresh_fakes():
    """one set of fake pcdet modules: every template class with a method of the reference's for each drop-in"""
    ref = lambda *a, **k: "reference"      # noqa: E731
    methods = {"AnchorHeadTemplate": ("get_loss", "generate_predicted_boxes", "get_cls_layer_loss", "get_box_reg_layer_loss"),
               "PointHeadTemplate": ("assign_stack_targets", "generate_predicted_boxes"),
               "RoIHeadTemplate": ("proposal_layer", "assign_targets", "get_loss", "generate_predicted_boxes", "get_box_reg_layer_loss",
                                   "get_box_cls_layer_loss"),
               "Detector3DTemplate": ("post_processing",),
               "PointHeadBox": ("get_loss",), "PointHeadSimple": ("get_loss",), "PointIntraPartOffsetHead": ("get_loss",)}
    fakes = {}
    for name, cls_name in TEMPLATES.items():
        mod = types.ModuleType(name)
        setattr(mod, cls_name, type(cls_name, (), {m: ref for m in methods[cls_name]}))
        fakes[name] = mod
    return fakes


def clean_state():
    """sys.modules without anything a binder binds, with one fresh set of fakes in it -> the fakes"""
    from modest_amd.utils import pcdet_bind as pb
    for k in list(pb.SHIMS) + list(pb.STAND_INS) + ["spconv.utils", pb.ANCHOR_TARGETS_NAME] + list(TEMPLATES):
        sys.modules.pop(k, None)
    fakes = fresh_fakes()
    sys.modules.update(fakes)
    return fakes


def methods_of(fakes):
    return {(name, m): f for name, cls_name in TEMPLATES.items() for m, f in vars(getattr(fakes[name], cls_name)).items() if callable(f)}


def test_every_binder_together_on_one_set_of_fake_modules():
    from modest_amd.utils import (anchor_head_loss, box_decode, pcdet_bind as pb, point_head_loss, point_head_targets, post_processing,
                                  proposal_layer, roi_head_loss, roi_targets, target_assigner)
    names = list(pb.SHIMS) + list(pb.STAND_INS) + ["spconv.utils", pb.ANCHOR_TARGETS_NAME] + list(TEMPLATES)
    saved = {k: sys.modules.get(k) for k in names}
    try:
        clean_state()
        for fn in binders().values():                 # once, so that every module of ours that a binder imports is imported
            fn()
        alone = {}
        for key, fn in binders().items():
            clean_state()
            before = set(sys.modules)
            fn()
            alone[key] = set(sys.modules) - before
        fakes = clean_state()
        before = set(sys.modules)
        for fn in binders().values():
            fn()
        assert set(sys.modules) - before == set().union(*alone.values())
        assert alone["install"] >= set(pb.SHIMS) | {pb.ANCHOR_TARGETS_NAME} and not any(alone[k] for k in alone if k != "install")
        assert sys.modules[pb.ANCHOR_TARGETS_NAME] is target_assigner
        cls = {c: getattr(fakes[n], c) for n, c in TEMPLATES.items()}
        want = {("AnchorHeadTemplate", "get_loss"): anchor_head_loss.get_loss,
                ("AnchorHeadTemplate", "generate_predicted_boxes"): box_decode.anchor_generate_predicted_boxes,
                ("PointHeadTemplate", "assign_stack_targets"): point_head_targets.assign_stack_targets,
                ("PointHeadTemplate", "generate_predicted_boxes"): box_decode.point_generate_predicted_boxes,
                ("RoIHeadTemplate", "proposal_layer"): proposal_layer.proposal_layer,
                ("RoIHeadTemplate", "assign_targets"): roi_targets.assign_targets,
                ("RoIHeadTemplate", "get_loss"): roi_head_loss.get_loss,
                ("RoIHeadTemplate", "generate_predicted_boxes"): box_decode.roi_generate_predicted_boxes,
                ("Detector3DTemplate", "post_processing"): post_processing.post_processing,
                ("PointHeadBox", "get_loss"): point_head_loss.get_loss, ("PointHeadSimple", "get_loss"): point_head_loss.get_loss,
                ("PointIntraPartOffsetHead", "get_loss"): point_head_loss.get_loss}
        for (c, m), f in want.items():
            assert vars(cls[c])[m] is f, f"{c}.{m} is not the drop-in"
        for c, m in (("AnchorHeadTemplate", "get_cls_layer_loss"), ("RoIHeadTemplate", "get_box_reg_layer_loss")):
            assert vars(cls[c])[m]() == "reference"                                    # nothing else is touched
        # a second round of all of them changes nothing: the methods, what each replaced, and the modules
        methods, modules = methods_of(fakes), dict(sys.modules)
        originals = [dict(m._ORIGINAL) for m in (anchor_head_loss, roi_head_loss, point_head_loss, box_decode)]
        for fn in binders().values():
            fn()
        assert methods_of(fakes) == methods and dict(sys.modules) == modules
        assert originals == [dict(m._ORIGINAL) for m in (anchor_head_loss, roi_head_loss, point_head_loss, box_decode)]
        assert anchor_head_loss._ORIGINAL[cls["AnchorHeadTemplate"]]() == "reference"      # what bind() replaced is still the reference's
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_the_stand_in_heads_carry_every_drop_in():
    from modest_amd.utils import (anchor_head_loss, box_decode, point_head_loss, point_head_targets, post_processing, proposal_layer,
                                  roi_head_loss, roi_targets)
    c = dc.head_classes()
    assert c.anchor.get_loss is anchor_head_loss.get_loss and c.anchor.generate_predicted_boxes is box_decode.anchor_generate_predicted_boxes
    assert c.point.assign_stack_targets is point_head_targets.assign_stack_targets and c.point.get_loss is point_head_loss.get_loss
    assert c.point.generate_predicted_boxes is box_decode.point_generate_predicted_boxes
    assert (c.roi.proposal_layer, c.roi.assign_targets, c.roi.get_loss, c.roi.generate_predicted_boxes) == (
        proposal_layer.proposal_layer, roi_targets.assign_targets, roi_head_loss.get_loss, box_decode.roi_generate_predicted_boxes)
    assert c.detector.post_processing is post_processing.post_processing
