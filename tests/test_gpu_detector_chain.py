"""GPU: the detector ops chained, each fed by the op before it (tests/detector_chain.py): an anchor detector from
assign_targets to post_processing, and PointRCNN's training step and test-time forward on one set of heads.  Stage k runs on
the device on stage k - 1's device tensors as they are -- views, strides, dtypes -- and is compared with stage k's restatement
applied to the host copy of those same tensors, by that op's own report function: targets, proposals, RoI targets, pooling,
decoding and post-processing bit for bit, the losses inside their derived bound and bit for bit against the restatement.  So
a mismatch names the stage.  After every stage the tensors it was given still hold their bits.  Last, the free-running chain
of restatements alone gives the device's final pred_dicts and recall_dict bit for bit.

Where a restatement evaluates cos / sin or the sigmoid in double on the host, the stage first asserts that the device's
double functions round to the same float32 on the values at hand (what the ops' own tests count and take out): nothing is
taken out of a chain, so such a value fails the stage by name.

The three round trips hold the conventions of encode and decode against each other inside bounds that count roundings (the
docstring of tests/detector_chain.py); tests/test_detector_chain_cpu.py holds the same in numpy and shows what breaks them."""
import numpy as np
import pytest
import torch

import anchor_loss_seq as al
import anchor_targets_seq as at
import box_decode_seq as bd
import detector_chain as dc
import point_loss_seq as pl
import point_targets_seq as pt
import post_process_seq as pp
import proposals_seq as ps
import roi_loss_seq as rl
import roi_targets_seq as rt
from test_gpu_roi_targets import trig_differs

pytestmark = pytest.mark.gpu
F = np.float32
_runs = {}


def up(a, gpu, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(gpu).requires_grad_(grad)


def host(t):
    return t.detach().cpu().numpy()


def raw(t):
    t = t.detach()
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def snapshot(**tensors):
    return [(k, t, raw(t).clone()) for k, t in tensors.items() if torch.is_tensor(t)]


def unchanged(snap, stage):
    for name, t, before in snap:
        assert torch.equal(raw(t), before), f"{stage} wrote into its input {name}"


def same_trig(stage, **headings):
    for name, h in headings.items():
        bad = trig_differs(h)
        assert not bad.any(), f"{stage}: the device's double cos / sin of {name} {np.asarray(h).reshape(-1)[bad][:4]} round differently from the host's"


def same_sigmoid(stage, x):
    x = np.ascontiguousarray(x, F).reshape(-1)
    dev = (1 / (1 + torch.exp(-torch.from_numpy(x.copy()).cuda().double()))).float().cpu().numpy()
    on_host = pp.sigmoid(x)
    bad = (dev.view(np.uint32) != on_host.view(np.uint32)) & ~(np.isnan(dev) & np.isnan(on_host))
    assert not bad.any(), f"{stage}: the device's double sigmoid of {x[bad][:4]} rounds differently from the host's"


def final_of(pred_dicts, recall_dict):
    return [(host(p["pred_boxes"]), host(p["pred_scores"]), host(p["pred_labels"])) for p in pred_dicts], recall_dict


def kept(owner):
    return {k: v for k, v in vars(owner).items() if k.startswith("_modest_") and torch.is_tensor(v)}


# ---------------------------------------------------------------------------------------------------- chain A
def anchor_losses(tb):
    return np.array([tb["rpn_loss_cls"], tb["rpn_loss_loc"], tb["rpn_loss_dir"], tb["rpn_loss"]], dtype=F)


def a_stage_targets(head, gt_dev):
    """stage 1 -> (the assigner's device dict, its host copy, the restatement's details)"""
    out = head.target_assigner.assign_targets(head.anchors, gt_dev)
    got = {k: host(v) for k, v in out.items()}
    want, details = dc.ref_a_targets(host(gt_dev))
    why = at.report(got, want, dc.A_CFG, dc.a_anchors(), host(gt_dev))
    assert not why, f"chain A stage 1, assign_targets\n{why}"
    return out, got, details


def a_stage_loss(head, preds, targets, got_targets, stage):
    """get_loss on the assigner's own tensors and (B, H, W, A K) predictions, then backward -> (tb_dict, the gradients)"""
    head.forward_ret_dict = dict(cls_preds=preds["cls"], box_preds=preds["box"], dir_cls_preds=preds["dir"], **targets)
    snap = snapshot(**targets)
    loss, tb = head.get_loss()
    loss.backward()
    got = {"losses": anchor_losses(tb), "grad_cls": host(preds["cls"].grad).reshape(dc.A_B, dc.A_N, 3),
           "grad_box": host(preds["box"].grad).reshape(dc.A_B, dc.A_N, 7), "grad_dir": host(preds["dir"].grad).reshape(dc.A_B, dc.A_N, 2)}
    inp = dc.a_loss_inputs({k: host(v) for k, v in preds.items()}, got_targets["box_cls_labels"], got_targets["box_reg_targets"])
    want, ex = dc.ref_a_loss(inp, 2)
    why, _ = al.bound_report(got, ex, "the device")
    assert not why, f"{stage} against exact()\n{why}"
    why = al.report(got, want)
    assert not why, f"{stage} against the restatement\n{why}"
    unchanged(snap, stage)
    return tb, got, want


def run_chain_a(gpu, head=None, det=None):
    head = head or dc.anchor_head(gpu)
    det = det or dc.detector(dc.A_POST)
    gt_dev = up(dc.scene_a(), gpu)
    targets, got1, _ = a_stage_targets(head, gt_dev)
    assert targets["box_cls_labels"].dtype == torch.int32
    # stage 2: the loss and its backward
    net = dc.net_anchor(got1["box_cls_labels"], got1["box_reg_targets"])
    preds = {k: up(dc.a_layout(v), gpu, grad=True) for k, v in net.items()}
    assert preds["box"].shape == (3, 8, 12, 42)
    _, got2, _ = a_stage_loss(head, preds, targets, got1, "chain A stage 2, get_loss")
    # stage 3: decoding, with the direction bins
    snap = snapshot(**preds, **targets)
    cls_out, boxes = head.generate_predicted_boxes(dc.A_B, preds["cls"], preds["box"], preds["dir"])
    why = bd.report(host(boxes), dc.ref_a_decode(host(preds["box"]), host(preds["dir"])), "chain A stage 3, generate_predicted_boxes:")
    assert not why, why
    assert cls_out.shape == (3, 576, 3) and cls_out.requires_grad and cls_out.data_ptr() == preds["cls"].data_ptr() and not boxes.requires_grad
    unchanged(snap, "chain A stage 3")
    # stage 4: post-processing with recall
    same_trig("chain A stage 4", boxes=host(boxes)[..., 6], gt=host(gt_dev)[..., 6])
    same_sigmoid("chain A stage 4", host(cls_out).max(axis=-1))
    snap = snapshot(boxes=boxes, cls=cls_out, gt=gt_dev)
    final = final_of(*det.post_processing(dict(batch_size=dc.A_B, batch_cls_preds=cls_out, batch_box_preds=boxes, cls_preds_normalized=False,
                                               gt_boxes=gt_dev)))
    want_preds, want_recall = dc.ref_a_post(host(boxes), host(cls_out), host(gt_dev))
    why = pp.describe(final, (want_preds, pp.recall_dict(want_recall, dc.A_POST["RECALL_THRESH_LIST"])))
    assert not why, "chain A stage 4, post_processing\n" + "\n".join(why)
    unchanged(snap, "chain A stage 4")
    return dict(head=head, det=det, targets=got1, loss=got2, boxes=host(boxes), final=final)


def assert_final_is_free_running(final, free, thresh_list, chain):
    want_preds, want_recall = free["final"]
    why = pp.describe(final, (want_preds, pp.recall_dict(want_recall, thresh_list)))
    assert not why, f"{chain}: the free-running chain of restatements gives another result\n" + "\n".join(why)


def test_chain_a(gpu):
    r = run_chain_a(gpu)
    _runs["a"] = r
    assert_final_is_free_running(r["final"], dc.free_chain_a(), dc.A_POST["RECALL_THRESH_LIST"], "chain A")
    names = {**kept(r["head"]), **{"assigner " + k: v for k, v in r["head"].target_assigner._tables.items() if torch.is_tensor(v)},
             **kept(r["det"])}
    assert {"_modest_anchor_loss_workspace", "_modest_anchor_loss_table", "_modest_anchor_loss_anchors", "_modest_post_process_workspace",
            "_modest_post_process_table"} <= set(names)
    assert_distinct(names)


def assert_distinct(named):
    """the tensors kept on heads and detector: pairwise distinct objects over distinct memory"""
    items = list(named.items())
    for i, (ka, a) in enumerate(items):
        for kb, b in items[i + 1:]:
            assert a is not b and (a.numel() == 0 or b.numel() == 0 or a.data_ptr() != b.data_ptr()), f"{ka} and {kb} are one buffer"


def test_chain_a_on_a_side_stream(gpu):
    first = _runs.get("a") or run_chain_a(gpu)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        again = run_chain_a(gpu)
    side.synchronize()
    assert not pp.describe(again["final"], first["final"])
    assert bd.same_bits(again["boxes"], first["boxes"]) and not al.report(again["loss"], first["loss"], "the side stream")
    assert not at.mismatches(again["targets"], first["targets"])


def test_anchor_round_trip(gpu):
    """anchor_decode of the assigner's own box_reg_targets over the head's list of anchors gives every positive row its matched
    gt back: centre 9 u |xg - xa| + u |xg|, z 3 u |zg - za| + u |zg|, sizes (4 + 2 |t|) u, heading u |rg - ra| + u |rg| modulo
    2 pi, each times 1.01 (the counts: tests/detector_chain.py).  It fails if the assigner's row order and flat_anchors
    disagree.  With those targets as predictions every regression difference is x - x: rpn_loss_loc is exactly 0.0 in the
    restatement and on the device, and the box gradient is all zeros."""
    head = dc.anchor_head(gpu)
    gt_dev = up(dc.scene_a(), gpu)
    targets, got1, details = a_stage_targets(head, gt_dev)
    snap = snapshot(**targets)
    cls = torch.zeros((dc.A_B, dc.A_N * 3), device=gpu)
    _, boxes = head.generate_predicted_boxes(dc.A_B, cls, targets["box_reg_targets"], None)
    why = dc.anchor_round_trip(host(boxes), got1["box_cls_labels"], dc.matched_gt_a(details, dc.scene_a()))
    assert not why, why
    unchanged(snap, "the decoding")
    net = dc.net_anchor(got1["box_cls_labels"], got1["box_reg_targets"])
    inp = dc.a_loss_inputs(dict(net, box=got1["box_reg_targets"]), got1["box_cls_labels"], got1["box_reg_targets"])
    assert al.restate(inp, dc.A_LOSS)["losses"][1] == 0.0
    preds = {k: up(dc.a_layout(v), gpu, grad=True) for k, v in net.items()}
    preds["box"] = targets["box_reg_targets"].detach().clone().view(3, 8, 12, 42).requires_grad_(True)
    tb, got, want = a_stage_loss(head, preds, targets, got1, "the loss of the targets themselves")
    assert want["losses"][1] == 0.0 and tb["rpn_loss_loc"] == 0.0 and not got["grad_box"].any()


# ---------------------------------------------------------------------------------------------------- chain B
def roi_table(tb, head):
    pinned = head._modest_roi_loss_table
    return np.array([tb["rcnn_loss_cls"], tb["rcnn_loss_reg"], tb.get("rcnn_loss_corner", 0.0), tb["rcnn_loss"], float(pinned[4]),
                     float(pinned[5])], dtype=F)


def proposals_stage(rhead, gpu, cls_out, pboxes, coords, B, nms, stage):
    """proposal_layer on the batch_index path: the strided float column, class logits that keep their graph"""
    batch = dict(batch_size=B, batch_cls_preds=cls_out, batch_box_preds=pboxes, batch_index=coords[:, 0], cls_preds_normalized=False)
    assert not batch["batch_index"].is_contiguous() and batch["batch_index"].dtype == torch.float32
    same_trig(stage, boxes=host(pboxes)[:, 6])
    snap = snapshot(cls=cls_out, boxes=pboxes, coords=coords)
    out = rhead.proposal_layer(batch, nms_config=dc.Cfg(nms))
    assert out is batch and "batch_index" not in batch and batch["has_class_labels"] is True and batch["roi_labels"].dtype == torch.int64
    got = tuple(host(batch[k]) for k in ("rois", "roi_scores", "roi_labels"))
    want = dc.ref_b_proposals(host(pboxes), host(cls_out), host(coords)[:, 0], B, nms["NMS_POST_MAXSIZE"], nms["NMS_THRESH"])
    why = ps.describe(got, want)
    assert not why, f"{stage}, proposal_layer\n" + "\n".join(why)
    unchanged(snap, stage)
    return batch, got


def run_chain_b(gpu, heads, variant=0, score_type="cls"):
    from modest_amd.utils.roipoint_pool3d.roipoint_pool3d_utils import RoIPointPool3d
    phead, rhead, det = heads
    sc = dc.scene_b(variant)
    cfg = dict(sc["target_cfg"], CLS_SCORE_TYPE=score_type)
    rhead.model_cfg["TARGET_CONFIG"] = dc.Cfg(cfg)
    B, M = sc["B"], cfg["ROI_PER_IMAGE"]
    coords, gt = up(sc["points"], gpu), up(sc["gt_boxes"], gpu)
    ext = gt.clone()
    ext[..., 3:6] += gt.new_tensor(dc.EXTEND)                      # box_utils.enlarge_box3d, on the device as the head does it
    bits = {}
    # ---- the training step.  1: point targets
    snap = snapshot(coords=coords, gt=gt, ext=ext)
    ptargets = phead.assign_stack_targets(points=coords, gt_boxes=gt, extend_gt_boxes=ext, ret_box_labels=True)
    got_pt = {k: None if v is None else host(v) for k, v in ptargets.items()}
    want, _ = dc.ref_b_point_targets(host(coords), host(gt), host(ext))
    why = pt.mismatches(got_pt, want)
    assert not why, "chain B stage 1, assign_stack_targets\n" + "\n".join(why)
    unchanged(snap, "chain B stage 1")
    bits["ptargets"] = got_pt
    # 2: the point loss (its backward comes with the RoI loss's)
    net = dc.net_point(got_pt["point_cls_labels"], got_pt["point_box_labels"])
    ppreds = {k: up(v, gpu, grad=True) for k, v in net.items()}
    phead.forward_ret_dict = dict(point_cls_preds=ppreds["cls"], point_box_preds=ppreds["box"], point_cls_labels=ptargets["point_cls_labels"],
                                  point_box_labels=ptargets["point_box_labels"])
    snap_loss = snapshot(labels=ptargets["point_cls_labels"], box_labels=ptargets["point_box_labels"])
    loss_point, tb_point = phead.get_loss()
    # 3: point decoding from the view point_coords[:, 1:4]
    snap = snapshot(coords=coords, **ppreds)
    cls_out, pboxes = phead.generate_predicted_boxes(points=coords[:, 1:4], point_cls_preds=ppreds["cls"], point_box_preds=ppreds["box"])
    why = bd.report(host(pboxes), dc.ref_b_point_decode(host(ppreds["box"]), host(coords)[:, 1:4], host(ppreds["cls"])),
                    "chain B stage 3, generate_predicted_boxes:")
    assert not why, why
    assert cls_out is ppreds["cls"] and not pboxes.requires_grad
    unchanged(snap, "chain B stage 3")
    bits["pboxes"] = host(pboxes)
    # 4: proposals
    batch, got_props = proposals_stage(rhead, gpu, cls_out, pboxes, coords, B, dc.B_TRAIN_NMS, "chain B stage 4")
    bits["props"] = got_props
    # 5: RoI targets under the seeds the restatement is given
    same_trig("chain B stage 5", rois=got_props[0][..., 6], ry=rt.rem(got_props[0][..., 6], rt.TWO_PI), gt=host(gt)[..., 6])
    snap = snapshot(gt=gt, **{k: batch[k] for k in ("rois", "roi_scores", "roi_labels")})
    dc.seed_draws()
    rtargets = rhead.assign_targets(dict(batch_size=B, rois=batch["rois"], roi_scores=batch["roi_scores"], roi_labels=batch["roi_labels"],
                                         gt_boxes=gt))
    got_rt = {k: host(v) for k, v in rtargets.items()}
    want, _ = dc.ref_b_roi_targets(got_props[0], got_props[1], got_props[2], host(gt), cfg)
    why = rt.describe(got_rt, want)
    assert not why, "chain B stage 5, assign_targets\n" + "\n".join(why)
    assert rtargets["rcnn_cls_labels"].dtype == (torch.int64 if score_type == "cls" else torch.float32)
    assert rtargets["gt_of_rois"].shape == (B, M, 8) and rtargets["rois"].shape == (B, M, 7)
    unchanged(snap, "chain B stage 5")
    bits["rtargets"] = got_rt
    # 6: RoI point pooling on the sampled rois, a sample at a time (the samples differ in their number of points)
    pool = RoIPointPool3d(num_sampled_points=dc.POOL_POINTS, pool_extra_width=dc.POOL_EXTRA)
    off = dc.offsets_of(sc["counts"])
    same_trig("chain B stage 6", rois=got_rt["rois"][..., 6])
    snap = snapshot(coords=coords, cls=ppreds["cls"], rois=rtargets["rois"])
    bits["pooled"] = []
    for b in range(B):
        xyz, feat = coords[off[b]:off[b + 1], 1:4].unsqueeze(0), ppreds["cls"].detach()[off[b]:off[b + 1]].unsqueeze(0)
        pooled, flag = pool(xyz, feat, rtargets["rois"][b:b + 1])
        want_pooled, want_flag = dc.ref_b_pool(host(xyz[0]), got_rt["rois"][b], host(feat[0]))
        assert flag.dtype == torch.int32 and np.array_equal(host(flag), want_flag), f"chain B stage 6, pooling: the empty flags of sample {b}"
        rows = np.argwhere((host(pooled).view(np.uint32) != want_pooled.view(np.uint32)).any(axis=(2, 3)))
        assert len(rows) == 0, f"chain B stage 6, pooling: sample {b}, rois {rows[:8, 1].tolist()} differ"
        bits["pooled"].append(host(pooled))
    unchanged(snap, "chain B stage 6")
    # 7: the RoI loss on assign_targets' own dict
    net = dc.net_roi(got_rt)
    rpreds = {k: up(v, gpu, grad=True) for k, v in net.items()}
    rhead.forward_ret_dict = dict(rtargets, rcnn_cls=rpreds["cls"], rcnn_reg=rpreds["reg"])
    snap_rloss = snapshot(**rtargets)
    loss_rcnn, tb_rcnn = rhead.get_loss()
    # 8: ONE backward through both losses
    assert loss_point.grad_fn is not None and loss_rcnn.grad_fn is not None and loss_point.grad_fn is not loss_rcnn.grad_fn
    (loss_point + loss_rcnn).backward()
    got = pl.outputs_of(loss_point.item(), tb_point, ppreds)
    want, ex = dc.ref_b_point_loss(dc.point_loss_inputs({k: host(v) for k, v in ppreds.items()}, got_pt["point_cls_labels"],
                                                        got_pt["point_box_labels"]))
    why, _ = pl.bound_report(got, ex, "the device")
    assert not why, f"chain B stage 2, the point loss against exact()\n{why}"
    why = pl.report(got, want)
    assert not why, f"chain B stage 2, the point loss against the restatement\n{why}"
    unchanged(snap_loss, "chain B stage 2")
    bits["ploss"] = got
    got = {"table": roi_table(tb_rcnn, rhead), "grad_cls": host(rpreds["cls"].grad).reshape(-1), "grad_reg": host(rpreds["reg"].grad)}
    want, ex = dc.ref_b_roi_loss(dc.roi_loss_inputs({k: host(v) for k, v in rpreds.items()}, got_rt), B, M)
    why, _ = rl.bound_report(got, ex, "the device")
    assert not why, f"chain B stage 7, the RoI loss against exact()\n{why}"
    why = rl.report(got, want)
    assert not why, f"chain B stage 7, the RoI loss against the restatement\n{why}"
    assert ("rcnn_loss_corner" in tb_rcnn) == (got["table"][4] > 0)
    unchanged(snap_rloss, "chain B stage 7")
    bits["rloss"] = got
    # ---- the test-time forward on the same heads
    with torch.no_grad():
        tbatch, got_tp = proposals_stage(rhead, gpu, cls_out, pboxes, coords, B, dc.B_TEST_NMS, "chain B test stage 1")
        net = dc.net_rcnn_test(got_tp[0], got_tp[1])
        tpreds = {k: up(v, gpu, grad=True) for k, v in net.items()}
        snap = snapshot(rois=tbatch["rois"], **tpreds)
        batch_cls, batch_box = rhead.generate_predicted_boxes(batch_size=B, rois=tbatch["rois"], cls_preds=tpreds["cls"], box_preds=tpreds["reg"])
        why = bd.report(host(batch_box), dc.ref_b_roi_decode(got_tp[0], host(tpreds["reg"])), "chain B test stage 2, generate_predicted_boxes:")
        assert not why, why
        assert batch_cls.shape == (B, dc.B_TEST_NMS["NMS_POST_MAXSIZE"], 1) and batch_cls.data_ptr() == tpreds["cls"].data_ptr()
        unchanged(snap, "chain B test stage 2")
        same_trig("chain B test stage 3", boxes=host(batch_box)[..., 6], rois=got_tp[0][..., 6], gt=host(gt)[..., 6])
        same_sigmoid("chain B test stage 3", host(batch_cls))
        tbatch.update(batch_cls_preds=batch_cls, batch_box_preds=batch_box, cls_preds_normalized=False, gt_boxes=gt)
        snap = snapshot(**{k: tbatch[k] for k in ("batch_cls_preds", "batch_box_preds", "gt_boxes", "rois", "roi_labels")})
        final = final_of(*det.post_processing(tbatch))
        want_preds, want_recall = dc.ref_b_post(host(batch_box), host(batch_cls), got_tp[2], host(gt), got_tp[0], B)
        why = pp.describe(final, (want_preds, pp.recall_dict(want_recall, dc.B_POST["RECALL_THRESH_LIST"])))
        assert not why, "chain B test stage 3, post_processing\n" + "\n".join(why)
        unchanged(snap, "chain B test stage 3")
    bits.update(tprops=got_tp, tboxes=host(batch_box), final=final)
    return dict(bits=bits, rtargets=rtargets, cfg=cfg, scene=sc)


def heads_b(gpu):
    return dc.point_head(gpu), dc.roi_head(gpu, dc.scene_b(0)["target_cfg"]), dc.detector(dc.B_POST)


def same_run(a, b):
    """every stage's host copy of two runs, bit for bit"""
    def flat(v, out):
        if isinstance(v, dict):
            for k in sorted(v):
                flat(v[k], out)
        elif isinstance(v, (list, tuple)):
            for x in v:
                flat(x, out)
        elif isinstance(v, np.ndarray):
            out.append(v.tobytes())
        else:
            out.append(repr(v).encode())
        return out
    return flat(a, []) == flat(b, [])


@pytest.mark.parametrize("score_type", ["cls", "roi_iou"])
def test_chain_b(gpu, score_type):
    """CLS_SCORE_TYPE cls hands the RoI loss int64 rcnn_cls_labels, roi_iou float32 ones"""
    heads = heads_b(gpu)
    r = run_chain_b(gpu, heads, 0, score_type)
    _runs[("b", score_type)] = (r, heads)
    assert_final_is_free_running(r["bits"]["final"], dc.free_chain_b(0, score_type), dc.B_POST["RECALL_THRESH_LIST"], "chain B")
    phead, rhead, det = heads
    named = {**kept(phead), **kept(phead.box_coder), **kept(rhead), **kept(det)}
    named["_modest_mean_size"] = phead.box_coder._modest_mean_size[2]
    assert {"_modest_point_loss_workspace", "_modest_point_loss_table", "_modest_proposals_workspace", "_modest_roi_targets_workspace",
            "_modest_roi_targets_counts", "_modest_roi_targets_picks", "_modest_roi_loss_workspace", "_modest_roi_loss_table",
            "_modest_post_process_workspace", "_modest_post_process_table"} <= set(named)
    assert_distinct(named)


def chain_b_run(gpu, score_type="cls"):
    if ("b", score_type) not in _runs:
        heads = heads_b(gpu)
        _runs[("b", score_type)] = (run_chain_b(gpu, heads, 0, score_type), heads)
    return _runs[("b", score_type)]


def test_state_kept_on_the_heads(gpu):
    """the training step and the test-time forward three times on the same head objects: the scene, then one with fewer points
    but B = 4 and ROI_PER_IMAGE 64, under which every kept workspace and pinned table of the RoI head grows (the picks table
    through its own growth path), then the first scene again, which reproduces its first bits"""
    heads = heads_b(gpu)
    first = run_chain_b(gpu, heads, 0)
    before = kept(heads[1])
    run_chain_b(gpu, heads, 1)
    after = kept(heads[1])
    assert after["_modest_roi_targets_picks"] is not before["_modest_roi_targets_picks"]
    assert after["_modest_roi_targets_picks"].numel() >= 2 * 4 * 64 > before["_modest_roi_targets_picks"].numel()
    assert all(after[k].numel() >= v.numel() for k, v in before.items())      # a kept buffer never shrinks
    again = run_chain_b(gpu, heads, 0)
    assert same_run(again["bits"], first["bits"])
    assert all(kept(heads[1])[k] is v for k, v in after.items())      # nothing shrinks or is replaced on the way back
    assert_distinct({**kept(heads[0]), **kept(heads[1]), **kept(heads[2])})


def test_point_round_trip(gpu):
    """point_decode of the targets' own point_box_labels, with logits one-hot at point_cls_labels - 1, gives every foreground
    point the gt box that holds it back: centre 9 u |xg - xp| + u |xg|, z 3 u |zg - zp| + u |zg|, sizes (4 + 2 |t|) u against
    the mean size the decoder picks by its own argmax, heading (2 + 2 pi) u modulo 2 pi, each times 1.01 (the counts:
    tests/detector_chain.py)"""
    sc = dc.scene_b(0)
    phead = dc.point_head(gpu)
    coords, gt = up(sc["points"], gpu), up(sc["gt_boxes"], gpu)
    ext = up(dc.extend_of(sc["gt_boxes"]), gpu)
    out = phead.assign_stack_targets(points=coords, gt_boxes=gt, extend_gt_boxes=ext, ret_box_labels=True)
    labels = out["point_cls_labels"]
    want, member = dc.ref_b_point_targets(sc["points"], sc["gt_boxes"], dc.extend_of(sc["gt_boxes"]))
    assert np.array_equal(host(labels), want["point_cls_labels"])
    logits = torch.full((len(labels), 3), -5.0, device=gpu)
    fg = labels > 0
    logits[fg, labels[fg] - 1] = 5.0
    snap = snapshot(box=out["point_box_labels"], coords=coords)
    _, boxes = phead.generate_predicted_boxes(points=coords[:, 1:4], point_cls_preds=logits, point_box_preds=out["point_box_labels"])
    why = dc.point_round_trip(host(boxes), host(labels), sc["points"], sc["gt_boxes"], member[1])
    assert not why, why
    unchanged(snap, "the decoding")


@pytest.mark.parametrize("score_type", ["cls", "roi_iou"])
def test_roi_round_trip(gpu, score_type):
    """roi_decode(rois, the float64 encode of gt_of_rois against the roi centred at zero) gives the rows with reg_valid_mask == 1
    centre and size of gt_of_rois_src back, and its heading modulo pi where the canonical heading lies strictly inside
    (-pi/2, pi/2): rt_sample turns by -ry, bd_roi back by +ra.  Centre 36 u L + u |xg| with L = |xg - xr| + |yg - yr|, z
    3 u |zg - zr| + u |zg|, sizes (4 + 2 |t|) u, heading (10 pi + |g| + |r|) u, each times 1.01 (the counts:
    tests/detector_chain.py)"""
    r, heads = chain_b_run(gpu, score_type)
    rtargets, got = r["rtargets"], r["bits"]["rtargets"]
    B, M = got["reg_valid_mask"].shape
    reg = up(dc.roi_encode64(got["gt_of_rois"], got["rois"]).reshape(-1, 7), gpu)
    cls = torch.zeros((B * M, 1), device=gpu)
    snap = snapshot(rois=rtargets["rois"], reg=reg)
    _, boxes = heads[1].generate_predicted_boxes(batch_size=B, rois=rtargets["rois"], cls_preds=cls, box_preds=reg)
    why = dc.roi_round_trip(host(boxes), got)
    assert not why, why
    unchanged(snap, "the decoding")
