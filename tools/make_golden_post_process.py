"""Golden post-processing results for modest_amd.utils.post_processing (BUILD CONTAINER ONLY -- needs /root/reference and
oracle/_ref/iou3d_ref.so, which `python __graft_entry__.py` builds there).

Runs the reference's own ``Detector3DTemplate.post_processing``, ``class_agnostic_nms`` and ``generate_recall_record``
(imported from where they lie, nothing copied) on the CPU in a child process.  The child binds empty package modules that
keep their ``__path__`` (so ``pcdet/models/__init__.py`` is never executed), empty modules for the sub-packages
``detector3d_template.py`` imports and never uses here, and this project's shims for the extension modules.  It substitutes,
as tools/make_golden_proposals.py and tools/make_golden_roi_targets.py do:
  * ``iou3d_nms_utils.nms_gpu`` becomes a greedy walk over the reference's own ``boxes_iou_bev_cpu``
    (oracle/_ref/iou3d_ref.so), resolved as src/iou3d_nms.cpp:116-135 resolves its mask;
  * the shim's ``boxes_overlap_bev_gpu`` becomes oracle.labels.boxes_iou_bev(overlap_only=True, arith="f64"), the twin the
    device kernels equal bit for bit, and ``torch.cuda.FloatTensor`` (iou3d_nms_utils.py:66) becomes ``torch.FloatTensor``.

Recorded in tests/golden/post_process.npz per scene: the config as JSON, the inputs, per sample the three outputs, the recall
dict as JSON (its key order is the reference's).  Three scenes:
  one_stage   dense, B = 2, raw logits with K = 3, C = 2, gts: an anchor head's output (cls_preds_normalized False);
  two_stage   dense, B = 2, 100 rows, K = 1, raw logits, ``rois``, ``roi_labels`` and ``has_class_labels``: "rcnn" counts over
              all rows, "roi" over the rois, labels are the given ones;
  empty_raw   stacked, B = 3, batch_index float32 interleaved, OUTPUT_RAW_SCORE; sample 1 has no row above the threshold
              but has gts.
The tool asserts that no order is open -- normalised scores pairwise distinct within a sample, class values distinct within
a row, every pair the walk compares farther from NMS_THRESH than ten derived bounds (tests/iou3d_cases.py), the three
arithmetics keeping the same boxes --, that no normalised score lies within 2 ulp of SCORE_THRESH, that every gt's maximum
lies farther from every recall threshold than ten bounds, that torch's cos / sin of every heading equal the double
functions rounded once, and that the restatement (tests/post_process_seq.py, both walks) reproduces the reference: boxes,
labels, counts and the recall dict bit for bit, scores bit for bit where no sigmoid is taken.  Torch's CPU float32 sigmoid
need not equal the double function rounded once: the largest distance in ulp over the rows of the non-normalised scenes is
measured, printed and stored as ``sigmoid_ulp``; the tests compare those scenes' scores within it.

Usage:  python tools/make_golden_post_process.py
"""
import json
import os
import pickle
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
REF = "/root/reference/downstream/OpenPCDet"
GOLD = os.path.join(ROOT, "tests", "golden", "post_process.npz")
F = np.float32

_CHILD = r"""
import os, pickle, sys, types
import numpy as np
import torch
ref, root, job = sys.argv[1], sys.argv[2], pickle.load(open(sys.argv[3], "rb"))
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "oracle", "_ref"))
for name in ("pcdet", "pcdet.models", "pcdet.models.detectors", "pcdet.models.model_utils", "pcdet.utils", "pcdet.ops",
             "pcdet.ops.iou3d_nms", "pcdet.ops.roiaware_pool3d"):
    m = types.ModuleType(name)
    m.__path__ = [os.path.join(ref, *name.split("."))]
    sys.modules[name] = m
# what detector3d_template.py imports to build a network, never used by post_processing
for name in ("backbones_2d", "backbones_3d", "dense_heads", "roi_heads"):
    m = sys.modules["pcdet.models." + name] = types.ModuleType("pcdet.models." + name)
    setattr(sys.modules["pcdet.models"], name, m)
sys.modules["pcdet.models.backbones_2d"].map_to_bev = types.ModuleType("map_to_bev")
sys.modules["pcdet.models.backbones_3d"].pfe = types.ModuleType("pfe")
sys.modules["pcdet.models.backbones_3d"].vfe = types.ModuleType("vfe")
from modest_amd.utils import pcdet_bind
pcdet_bind.install(stand_ins=False)
import iou3d_ref
from oracle import labels as ol
from pcdet.ops.iou3d_nms import iou3d_nms_utils
from pcdet.models.model_utils import model_nms_utils
from pcdet.models.detectors import detector3d_template
Detector3DTemplate = detector3d_template.Detector3DTemplate
assert detector3d_template.__file__.startswith(ref) and iou3d_nms_utils.__file__.startswith(ref)
assert model_nms_utils.__file__.startswith(ref) and model_nms_utils.iou3d_nms_utils is iou3d_nms_utils
assert detector3d_template.iou3d_nms_utils is iou3d_nms_utils and detector3d_template.model_nms_utils is model_nms_utils

def nms_gpu(boxes, scores, thresh, pre_maxsize=None, **kwargs):
    assert boxes.shape[1] == 7
    order = scores.sort(0, descending=True)[1]
    if pre_maxsize is not None:
        order = order[:pre_maxsize]
    b = boxes[order].contiguous()
    iou = torch.zeros((len(b), len(b)), dtype=torch.float32)
    iou3d_ref.boxes_iou_bev_cpu(b, b, iou)
    iou = iou.numpy()
    dead = np.zeros(len(b), bool)
    keep = []
    for i in range(len(b)):
        if dead[i]:
            continue
        keep.append(i)
        dead[i + 1:] |= iou[i, i + 1:] > np.float32(thresh)
    return order[torch.tensor(keep, dtype=torch.long)].contiguous(), None
iou3d_nms_utils.nms_gpu = nms_gpu
torch.cuda.FloatTensor = torch.FloatTensor
def boxes_overlap_bev_gpu(a, b, out):
    out.copy_(torch.from_numpy(ol.boxes_iou_bev(a.numpy(), b.numpy(), overlap_only=True, arith="f64")))
iou3d_nms_utils.iou3d_nms_cuda = types.SimpleNamespace(boxes_overlap_bev_gpu=boxes_overlap_bev_gpu)

class Cfg(dict):
    __getattr__ = dict.__getitem__

res = {}
for name, (cfg, a) in job.items():
    nms = Cfg({k: cfg[k] for k in ("NMS_TYPE", "MULTI_CLASSES_NMS", "NMS_PRE_MAXSIZE", "NMS_POST_MAXSIZE", "NMS_THRESH")})
    post = Cfg(NMS_CONFIG=nms, SCORE_THRESH=cfg["SCORE_THRESH"], OUTPUT_RAW_SCORE=cfg["OUTPUT_RAW_SCORE"],
               RECALL_THRESH_LIST=cfg["RECALL_THRESH_LIST"])
    det = types.SimpleNamespace(model_cfg=Cfg(POST_PROCESSING=post), num_class=cfg["num_class"],
                                generate_recall_record=Detector3DTemplate.generate_recall_record)
    d = dict(batch_size=cfg["batch_size"], batch_box_preds=torch.from_numpy(a["box"].copy()),
             batch_cls_preds=torch.from_numpy(a["cls"].copy()), cls_preds_normalized=cfg["cls_preds_normalized"])
    if a["batch_index"] is not None:
        d["batch_index"] = torch.from_numpy(a["batch_index"].copy())
    if a["gt_boxes"] is not None:
        d["gt_boxes"] = torch.from_numpy(a["gt_boxes"].copy())
    if cfg["rois_in_batch"]:
        d["rois"] = torch.from_numpy(a["rois"].copy())
    if cfg["has_class_labels"]:
        d["has_class_labels"] = True
        d["roi_labels"] = torch.from_numpy(a["labels"].copy())
    pred_dicts, recall = Detector3DTemplate.post_processing(det, d)
    raw = torch.from_numpy(a["cls"].copy()).reshape(-1, a["cls"].shape[-1]).max(1)[0]
    res[name] = dict(preds=[{k: v.numpy() for k, v in p.items()} for p in pred_dicts], recall=dict(recall), keys=list(recall),
                     torch_sigmoid=torch.sigmoid(raw).numpy())
pickle.dump(res, open(sys.argv[4], "wb"))
"""

RECALL = [0.3, 0.5, 0.7]


def sample(rs, n_obj, per, centre, nms_thresh, post, score, passes):
    """n_obj * per clustered boxes (tools/make_golden_proposals.py:draw_box) whose every pair compared by the walk over the
    rows that pass the score threshold, in the order of `score`, is far from the NMS threshold -> (boxes, objects)"""
    import make_golden_proposals as gp
    import proposals_seq as ps
    obj = gp.objects(rs, n_obj, centre)
    src = np.repeat(np.arange(n_obj), per)
    box = np.stack([gp.draw_box(rs, obj[k]) for k in src])
    rows = np.flatnonzero(passes)
    order = rows[np.argsort(ps.descending_bits(score[rows]), kind="stable")]
    for _ in range(50):
        bad = gp.far_from_threshold(box[order], nms_thresh, post)
        if not bad:
            return box, obj
        for pos in bad:
            gp.DRAWS["dropped"] += 1
            box[order[pos]] = gp.draw_box(rs, obj[src[order[pos]]])
    raise RuntimeError("no sample found")


def recall_far(lists, gt7):
    """every gt's exact maximum 3-D IoU over each list lies farther from every recall threshold than ten times the largest
    derived bound of its column (tools/make_golden_roi_targets.py:margins)"""
    import make_golden_roi_targets as gr
    ok = np.ones(len(gt7), bool)
    for boxes in lists:
        if len(boxes) == 0:
            continue
        ex, bound = gr.margins(np.ascontiguousarray(boxes[:, :7], F), np.ascontiguousarray(gt7, F))
        for t in RECALL:
            ok &= np.abs(ex.max(0) - t) > 10 * bound.max(0)
    return ok


def gts_for(rs, obj, n, rows, cols, lists_of):
    """n gts near the first objects, each far from every recall threshold against the lists `lists_of()` returns, padded
    with zero rows to (rows, cols + 1)"""
    import make_golden_proposals as gp
    out = np.zeros((rows, cols + 1), F)
    for k in range(n):
        for _ in range(200):
            g = gp.draw_box(rs, obj[k % len(obj)])
            g[2] += F(rs.normal(0, 0.1))
            g[5] *= F(rs.normal(1, 0.05))
            g[:2] += rs.normal(0, 0.3, 2).astype(F)
            if recall_far(lists_of(), g[None, :7])[0]:
                break
            gp.DRAWS["dropped"] += 1
        else:
            raise RuntimeError("no gt found")
        out[k, :7], out[k, -1] = g, rs.randint(1, 4)
    return out


def distinct(rs, n, lo, hi):
    return (rs.permutation(n).astype(F) / F(n) * F(hi - lo) + F(lo)).astype(F)


def final_boxes(cfg, a):
    import post_process_seq as seq
    return seq.post_process(a["box"], a["cls"], cfg["batch_size"], cfg["NMS_PRE_MAXSIZE"], cfg["NMS_POST_MAXSIZE"], cfg["NMS_THRESH"],
                            score_thresh=cfg["SCORE_THRESH"], normalized=cfg["cls_preds_normalized"], batch_index=a["batch_index"])[0]


def build_scenes():
    import post_process_seq as seq
    rs = np.random.RandomState(20261023)
    base = dict(NMS_TYPE="nms_gpu", MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=4096, NMS_POST_MAXSIZE=500, NMS_THRESH=0.1,
                SCORE_THRESH=0.1, OUTPUT_RAW_SCORE=False, RECALL_THRESH_LIST=RECALL, cls_preds_normalized=False,
                has_class_labels=False, rois_in_batch=False, num_class=3)
    none = dict(batch_index=None, labels=None, gt_boxes=None, rois=None)
    out = {}
    # one_stage: dense, B = 2, 150 rows, K = 3, C = 2, raw logits; about two thirds pass the threshold
    cfg = dict(base, batch_size=2)
    boxes, clss, objs = [], [], []
    for b in range(2):
        x = distinct(rs, 150, -4.0, 4.0)
        bx, obj = sample(rs, 15, 10, 40.0 * b, cfg["NMS_THRESH"], cfg["NMS_POST_MAXSIZE"], seq.sigmoid(x), seq.sigmoid(x) >= F(0.1))
        c = x[:, None] - (rs.permutation(3 * 150).reshape(150, 3).astype(F) + F(1)) / F(64)      # below the maximum, distinct
        c[np.arange(150), rs.randint(0, 3, 150)] = x
        boxes.append(np.concatenate([bx, rs.uniform(-1, 1, (150, 2)).astype(F)], 1)), clss.append(c), objs.append(obj)
    a = dict(none, box=np.stack(boxes).astype(F), cls=np.stack(clss).astype(F))
    fin = final_boxes(cfg, a)
    a["gt_boxes"] = np.stack([gts_for(rs, objs[b], 9 + b, 12, 9, lambda b=b: [fin[b][0]]) for b in range(2)])
    out["one_stage"] = (cfg, a)
    # two_stage: dense, B = 2, 100 rows, K = 1, logits; rois are the boxes before refinement
    cfg = dict(base, batch_size=2, has_class_labels=True, rois_in_batch=True, NMS_POST_MAXSIZE=100)
    boxes, clss, rois, objs = [], [], [], []
    import make_golden_proposals as gp
    for b in range(2):
        x = distinct(rs, 100, -3.0, 5.0)
        bx, obj = sample(rs, 10, 10, -40.0 * b, cfg["NMS_THRESH"], 100, seq.sigmoid(x), seq.sigmoid(x) >= F(0.1))
        src = np.repeat(np.arange(10), 10)
        boxes.append(bx), clss.append(x[:, None]), objs.append(obj)
        rois.append(np.stack([gp.draw_box(rs, obj[k]) for k in src]))
    a = dict(none, box=np.stack(boxes).astype(F), cls=np.stack(clss).astype(F), rois=np.stack(rois).astype(F),
             labels=rs.randint(1, 4, (2, 100)).astype(np.int64))
    a["gt_boxes"] = np.stack([gts_for(rs, objs[b], 7 + 2 * b, 11, 7, lambda b=b: [a["box"][b], a["rois"][b]]) for b in range(2)])
    out["two_stage"] = (cfg, a)
    # empty_raw: stacked, B = 3, interleaved; sample 1 entirely below the threshold; OUTPUT_RAW_SCORE
    cfg = dict(base, batch_size=3, OUTPUT_RAW_SCORE=True, num_class=1, NMS_POST_MAXSIZE=20)
    parts, objs = [], []
    for b, (lo, hi) in enumerate(((-4.0, 4.0), (-6.0, -2.5), (-3.0, 3.0))):
        x = distinct(rs, 80, lo, hi)
        bx, obj = sample(rs, 8, 10, 50.0 * b, cfg["NMS_THRESH"], 20, seq.sigmoid(x), seq.sigmoid(x) >= F(0.1))
        parts.append((bx, x)), objs.append(obj)
    box, cls = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])[:, None]
    bidx = np.repeat(np.arange(3), 80).astype(F)
    perm = rs.permutation(len(box))
    a = dict(none, box=np.ascontiguousarray(box[perm]), cls=np.ascontiguousarray(cls[perm]), batch_index=np.ascontiguousarray(bidx[perm]))
    fin = final_boxes(cfg, a)
    a["gt_boxes"] = np.stack([gts_for(rs, objs[b], 5 + b, 8, 7, lambda b=b: [fin[b][0]]) for b in range(3)])
    out["empty_raw"] = (cfg, a)
    return out


def ulp_distance(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def record(job):
    import make_golden_proposals as gp
    import post_process_seq as seq
    import proposals_seq as ps
    from oracle import labels as ol
    print("drawn by rejection: %(candidates)d candidates, %(dropped)d dropped" % gp.DRAWS)
    assert gp.DRAWS["dropped"] * 4 <= gp.DRAWS["candidates"], gp.DRAWS
    with tempfile.TemporaryDirectory() as work:
        pickle.dump(job, open(os.path.join(work, "job.pkl"), "wb"))
        open(os.path.join(work, "child.py"), "w").write(_CHILD)
        subprocess.run([sys.executable, os.path.join(work, "child.py"), REF, ROOT, os.path.join(work, "job.pkl"),
                        os.path.join(work, "res.pkl")], check=True)
        res = pickle.load(open(os.path.join(work, "res.pkl"), "rb"))
    rec = {"scenes": np.array(json.dumps(list(job)))}
    worst = 0
    for name, (cfg, a) in job.items():
        assert not cfg["cls_preds_normalized"]
        B, pre, post, thresh = cfg["batch_size"], cfg["NMS_PRE_MAXSIZE"], cfg["NMS_POST_MAXSIZE"], cfg["NMS_THRESH"]
        fb, fc, per = ps._flat(a["box"], a["cls"], a["batch_index"])
        raw, _ = ps.score_label(fc)
        score = seq.sigmoid(raw)
        smp = ps.sample_of(a["batch_index"], len(fb), B, per)
        # no order is open
        assert all(len(np.unique(score[smp == s])) == (smp == s).sum() for s in range(B)), f"{name}: equal scores"
        assert fc.shape[1] == 1 or not (np.diff(np.sort(seq.sigmoid(fc), 1), axis=1) == 0).any(), f"{name}: equal class values"
        assert gp.heading_ok(fb[:, 6]) and gp.heading_ok(a["gt_boxes"][..., 6].reshape(-1)), f"{name}: a heading differs"
        assert a["rois"] is None or gp.heading_ok(a["rois"][..., 6].reshape(-1)), f"{name}: a roi heading differs"
        t = F(cfg["SCORE_THRESH"])
        assert (ulp_distance(score, np.full_like(score, t)) > 2).all(), f"{name}: a score within 2 ulp of SCORE_THRESH"
        torch_sig = res[name]["torch_sigmoid"]
        assert ((torch_sig >= t) == (score >= t)).all(), f"{name}: torch's sigmoid and the double rule pass different rows"
        worst = max(worst, int(ulp_distance(torch_sig, score).max()))
        kept = []
        for s in range(B):
            rows = np.flatnonzero((smp == s) & (score >= t))
            rows = rows[ps.candidates(score[rows], np.zeros(len(rows), np.int64), 1, pre)[0]]
            b = np.ascontiguousarray(fb[rows, :7])
            if len(b) == 0:
                kept.append(0)
                continue
            walks = [gp.reference_arithmetic_walk(b, thresh), ol.nms(b, F(thresh), rotated=True, arith="f64"),
                     ol.nms(b, F(thresh), rotated=True, arith="glibc")]
            assert all(np.array_equal(walks[0], w) for w in walks[1:]), f"{name}: the three arithmetics keep different boxes"
            assert not gp.far_from_threshold(b, thresh, post), f"{name}: a compared pair lies within ten bounds of the threshold"
            kept.append(len(walks[0]))
        r = res[name]
        args = dict(rotated=True, score_thresh=cfg["SCORE_THRESH"], normalized=False, output_raw_score=cfg["OUTPUT_RAW_SCORE"],
                    labels=a["labels"] if cfg["has_class_labels"] else None, batch_index=a["batch_index"], gt_boxes=a["gt_boxes"],
                    rois=a["rois"] if cfg["rois_in_batch"] else None, recall_thresh=cfg["RECALL_THRESH_LIST"])
        for walk in (ps.parent_walk, ps.chunked_walk):
            preds, recall = seq.post_process(a["box"], a["cls"], B, pre, post, thresh, walk=walk, **args)
            want = seq.recall_dict(recall, cfg["RECALL_THRESH_LIST"])
            assert want == r["recall"] and list(want) == r["keys"], f"{name}: recall {want} against the reference's {r['recall']}"
            assert all(type(v) is int for v in r["recall"].values())
            for b, (g, w) in enumerate(zip(preds, r["preds"])):
                assert w["pred_boxes"].dtype == F and w["pred_scores"].dtype == F and w["pred_labels"].dtype == np.int64
                assert g[0].shape == w["pred_boxes"].shape and np.array_equal(seq.bits(g[0]), seq.bits(w["pred_boxes"])), (name, b)
                assert np.array_equal(g[2], w["pred_labels"]), (name, b)
                if cfg["OUTPUT_RAW_SCORE"]:
                    assert np.array_equal(seq.bits(g[1]), seq.bits(w["pred_scores"])), (name, b)
                else:
                    assert (ulp_distance(g[1], w["pred_scores"]) <= worst).all(), (name, b)
            for b in range(B):      # the recall decisions
                gt = a["gt_boxes"][b]
                gt = gt[:seq.trim(gt)]
                lists = [preds[b][0]] if not cfg["rois_in_batch"] else [a["box"][b], a["rois"][b]]
                assert recall_far(lists, gt[:, :7]).all(), f"{name}[{b}]: a maximum within ten bounds of a recall threshold"
        rec[name + "_cfg"] = np.array(json.dumps(cfg))
        for k in seq.ARRAYS:
            if a[k] is not None:
                rec[f"{name}_{k}"] = a[k]
        for b, w in enumerate(r["preds"]):
            for k in ("pred_boxes", "pred_scores", "pred_labels"):
                rec[f"{name}_{k}_{b}"] = w[k]
        rec[name + "_recall"] = np.array(json.dumps(r["recall"]))
        print(name, "box", a["box"].shape, "survivors of the uncapped walk", kept, "final", [len(w["pred_boxes"]) for w in r["preds"]],
              "recall", r["recall"])
    rec["sigmoid_ulp"] = np.array(worst, np.int64)
    print(f"torch's CPU float32 sigmoid against the double function rounded once: at most {worst} ulp over the scenes' rows")
    return rec


def main():
    import make_golden_proposals as gp
    rec = record(build_scenes())
    import post_process_seq as seq
    empty = seq.recorded(rec, "empty_raw")[0]
    assert len(empty[1][0]) == 0 and len(empty[0][0]) > 0 and empty[1][0].shape == (0, 7)
    gp.save(GOLD, rec, 64 * 1024)


if __name__ == "__main__":
    main()
