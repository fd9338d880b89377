"""Golden RoI proposals for modest_amd.utils.proposal_layer (BUILD CONTAINER ONLY -- needs /root/reference and
oracle/_ref/iou3d_ref.so, which `python __graft_entry__.py` builds there).

Runs the reference's own ``RoIHeadTemplate.proposal_layer`` and ``class_agnostic_nms`` (imported from where they lie,
nothing copied) on the CPU in a child process.  The child binds empty package modules that keep their ``__path__`` (so
``pcdet/models/__init__.py`` is never executed) and this project's shims for the extension modules
(``pcdet_bind.install``), and replaces ``iou3d_nms_utils.nms_gpu`` there by a greedy walk over the reference's own
``boxes_iou_bev_cpu`` (oracle/_ref/iou3d_ref.so): the descending sort of the scores, then box i survives unless an earlier
survivor's IoU with it is > thresh, as src/iou3d_nms.cpp:116-135 resolves its mask.

Recorded in tests/golden/proposals.npz per scene: the config as JSON (plain values), box and class predictions, the batch
index of a stacked scene, and the three outputs.  Three scenes:
  stacked   B = 3, about 300 rows in the stacked form, batch_index float32 and interleaved, K = 1, C = 0;
  dense     B = 2, 120 rows each in the dense form, K = 3, C = 2;
  post      stacked, B = 2: sample 0 reaches NMS_POST_MAXSIZE, sample 1 does not.
Scores and class values are pairwise distinct, so no order the reference leaves open is recorded.  Boxes are clustered
like tests/iou3d_cases.py:proposals and drawn by rejection.  The tool asserts
  * that the walk in the reference's arithmetic, the f64 twin and the glibc oracle (oracle.labels.nms) give the same keep
    list on every sample of every scene;
  * that every pair the walk compares (an earlier survivor against a later candidate) has an exact IoU
    (tests/rect_exact.py) farther from the threshold than ten times that pair's derived bound (tests/iou3d_cases.py);
  * that torch's CPU cos / sin of every heading equals the double function rounded once;
  * that the numpy restatement (tests/proposals_seq.py, both walks) reproduces every recorded output bit for bit, and the
    fixture's size (64 KB).
A fixture whose arrays are all unchanged is left alone on disk (a zip archive carries the time of writing).

Usage:  python tools/make_golden_proposals.py
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
REF = "/root/reference/downstream/OpenPCDet"
GOLD = os.path.join(ROOT, "tests", "golden", "proposals.npz")
F = np.float32

_CHILD = r"""
import os, pickle, sys, types
import numpy as np
import torch
ref, root, job = sys.argv[1], sys.argv[2], pickle.load(open(sys.argv[3], "rb"))
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "oracle", "_ref"))
for name in ("pcdet", "pcdet.models", "pcdet.models.roi_heads", "pcdet.models.roi_heads.target_assigner",
             "pcdet.models.model_utils", "pcdet.utils", "pcdet.ops", "pcdet.ops.iou3d_nms", "pcdet.ops.roiaware_pool3d"):
    m = types.ModuleType(name)
    m.__path__ = [os.path.join(ref, *name.split("."))]
    sys.modules[name] = m
from modest_amd.utils import pcdet_bind
pcdet_bind.install(stand_ins=False)
import iou3d_ref
from pcdet.ops.iou3d_nms import iou3d_nms_utils
from pcdet.models.model_utils import model_nms_utils
from pcdet.models.roi_heads.roi_head_template import RoIHeadTemplate
assert RoIHeadTemplate.__module__.startswith("pcdet.") and iou3d_nms_utils.__file__.startswith(ref)
assert model_nms_utils.__file__.startswith(ref) and model_nms_utils.iou3d_nms_utils is iou3d_nms_utils

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

class Cfg(dict):
    __getattr__ = dict.__getitem__

res = {}
for name, (cfg, box, cls, bidx) in job.items():
    d = dict(batch_size=cfg["batch_size"], batch_box_preds=torch.from_numpy(box.copy()), batch_cls_preds=torch.from_numpy(cls.copy()))
    if bidx is not None:
        d["batch_index"] = torch.from_numpy(bidx.copy())
    nms = Cfg({k: v for k, v in cfg.items() if k != "batch_size"})
    out = RoIHeadTemplate.proposal_layer(types.SimpleNamespace(), d, nms)
    assert "batch_index" not in out
    res[name] = dict(rois=out["rois"].numpy(), roi_scores=out["roi_scores"].numpy(), roi_labels=out["roi_labels"].numpy(),
                     has_class_labels=bool(out["has_class_labels"]))
pickle.dump(res, open(sys.argv[4], "wb"))
"""

DRAWS = {"candidates": 0, "dropped": 0}


def heading_ok(v):
    import torch
    import point_targets_seq as pts
    v = np.atleast_1d(np.asarray(v, F))
    t = torch.from_numpy(np.concatenate([v, -v]).copy())
    return bool(np.array_equal(torch.cos(t).numpy().view(np.uint32), pts.f32_of_double(np.cos, t.numpy()).view(np.uint32))
                and np.array_equal(torch.sin(t).numpy().view(np.uint32), pts.f32_of_double(np.sin, t.numpy()).view(np.uint32)))


def draw_box(rs, obj):
    """a jittered copy of object row `obj` whose heading torch and the rounded double functions agree on"""
    for _ in range(200):
        DRAWS["candidates"] += 1
        b = obj.copy()
        b[:2] += rs.normal(0, 0.25, 2)
        b[3:5] *= rs.normal(1, 0.06, 2)
        b[6] += rs.normal(0, 0.08) + np.pi * (rs.random_sample() < 0.2)
        b = b.astype(F)
        if heading_ok(b[6]):
            return b
        DRAWS["dropped"] += 1
    raise RuntimeError("no box found")


def objects(rs, n, centre):
    return np.c_[centre + rs.uniform(-30, 30, n), rs.uniform(-30, 30, n), rs.uniform(-1.5, 0.5, n), rs.uniform(3.2, 4.8, n),
                 rs.uniform(1.5, 2.0, n), rs.uniform(1.4, 1.7, n), rs.uniform(-3.2, 3.2, n)]


def far_from_threshold(boxes_sorted, thresh, post):
    """rows (positions in the sorted list) of the later box of every compared pair whose exact IoU lies within ten
    derived bounds of the threshold; the walk is the exact one"""
    import iou3d_cases as ic
    e = ic.Exact.all_pairs(boxes_sorted[:, :7], boxes_sorted[:, :7])
    close = np.abs(e.iou - thresh) <= 10 * e.iou_bound
    dead = np.zeros(len(boxes_sorted), bool)
    bad, kept = set(), 0
    for i in range(len(boxes_sorted)):
        if dead[i]:
            continue
        kept += 1
        if kept > post:
            break
        later = np.arange(len(boxes_sorted)) > i
        bad |= set(np.flatnonzero(close[i] & later & ~dead).tolist())
        dead |= later & (e.iou[i] > thresh)
    return sorted(bad)


def make_sample(rs, n_obj, per, centre, thresh, post):
    """n_obj * per clustered boxes with pairwise distinct scores whose every compared pair is far from the threshold"""
    import proposals_seq as seq
    obj = objects(rs, n_obj, centre)
    src = np.repeat(np.arange(n_obj), per)
    box = np.stack([draw_box(rs, obj[k]) for k in src])
    score = rs.permutation(len(box)).astype(F) / F(len(box)) * F(0.98) + F(0.01)      # distinct by construction
    for _ in range(50):
        order = np.argsort(seq.descending_bits(score), kind="stable")
        bad = far_from_threshold(box[order], thresh, post)
        if not bad:
            return box, score
        for pos in bad:
            DRAWS["dropped"] += 1
            box[order[pos]] = draw_box(rs, obj[src[order[pos]]])
    raise RuntimeError("no sample found")


def build_scenes():
    rs = np.random.RandomState(20261021)
    out = {}
    # stacked: B = 3, 140 + 100 + 60 rows, interleaved
    cfg = dict(batch_size=3, NMS_TYPE="nms_gpu", MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=9000, NMS_POST_MAXSIZE=100, NMS_THRESH=0.8)
    parts = [make_sample(rs, 14, 10, 0.0, 0.8, 100), make_sample(rs, 10, 10, 60.0, 0.8, 100), make_sample(rs, 6, 10, -60.0, 0.8, 100)]
    box = np.concatenate([p[0] for p in parts])
    cls = np.concatenate([p[1] for p in parts])[:, None]
    bidx = np.concatenate([np.full(len(p[0]), k, F) for k, p in enumerate(parts)])
    perm = rs.permutation(len(box))
    out["stacked"] = (cfg, np.ascontiguousarray(box[perm]), np.ascontiguousarray(cls[perm]), np.ascontiguousarray(bidx[perm]))
    # dense: B = 2, 120 rows, K = 3, C = 2; PRE below the rows
    cfg = dict(batch_size=2, NMS_TYPE="nms_gpu", MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=100, NMS_POST_MAXSIZE=64, NMS_THRESH=0.7)
    boxes, clss = [], []
    for k in range(2):
        # the walk sees the 100 best only: draw against the full list, which holds every pair of that prefix
        b, s = make_sample(rs, 12, 10, 30.0 * k, 0.7, 120)
        other = rs.permutation(3 * len(b)).reshape(len(b), 3).astype(F) / F(3 * len(b)) * F(0.009)   # below every score, distinct
        c = other.copy()
        c[np.arange(len(b)), rs.randint(0, 3, len(b))] = s
        boxes.append(np.concatenate([b, rs.uniform(-1, 1, (len(b), 2)).astype(F)], 1))
        clss.append(c)
    out["dense"] = (cfg, np.stack(boxes).astype(F), np.stack(clss).astype(F), None)
    # post: sample 0 reaches POST = 16, sample 1 (3 objects) does not
    cfg = dict(batch_size=2, NMS_TYPE="nms_gpu", MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=9000, NMS_POST_MAXSIZE=16, NMS_THRESH=0.5)
    parts = [make_sample(rs, 20, 5, 0.0, 0.5, 16), make_sample(rs, 3, 30, 80.0, 0.5, 16)]
    box = np.concatenate([p[0] for p in parts])
    cls = np.concatenate([p[1] for p in parts])[:, None]
    bidx = np.concatenate([np.full(len(p[0]), k, F) for k, p in enumerate(parts)])
    out["post"] = (cfg, box, cls, bidx)                       # grouped by sample, as a batch normally is
    return out


def reference_arithmetic_walk(boxes_sorted, thresh):
    from oracle import labels as ol
    iou = ol.boxes_iou_bev_reference(boxes_sorted, boxes_sorted)
    assert iou is not None, "oracle/_ref/iou3d_ref.so is not built: run python __graft_entry__.py"
    dead = np.zeros(len(iou), bool)
    keep = []
    for i in range(len(iou)):
        if not dead[i]:
            keep.append(i)
            dead[i + 1:] |= iou[i, i + 1:] > F(thresh)
    return np.asarray(keep, np.int64)


def record(job):
    import proposals_seq as seq
    from oracle import labels as ol
    print("drawn by rejection: %(candidates)d candidates, %(dropped)d dropped" % DRAWS)
    assert DRAWS["dropped"] * 4 <= DRAWS["candidates"], DRAWS
    with tempfile.TemporaryDirectory() as work:
        pickle.dump(job, open(os.path.join(work, "job.pkl"), "wb"))
        open(os.path.join(work, "child.py"), "w").write(_CHILD)
        subprocess.run([sys.executable, os.path.join(work, "child.py"), REF, ROOT, os.path.join(work, "job.pkl"),
                        os.path.join(work, "res.pkl")], check=True)
        res = pickle.load(open(os.path.join(work, "res.pkl"), "rb"))
    rec = {"scenes": np.array(json.dumps(list(job)))}
    for name, (cfg, box, cls, bidx) in job.items():
        B, pre, post, thresh = cfg["batch_size"], cfg["NMS_PRE_MAXSIZE"], cfg["NMS_POST_MAXSIZE"], cfg["NMS_THRESH"]
        fb, fc, per = seq._flat(box, cls, bidx)
        score, _ = seq.score_label(fc)
        smp = seq.sample_of(bidx, len(fb), B, per)
        assert all(len(np.unique(score[smp == s])) == (smp == s).sum() for s in range(B)), f"{name}: equal scores"
        assert fc.shape[1] == 1 or not (np.diff(np.sort(fc, 1), axis=1) == 0).any(), f"{name}: equal class values"
        assert heading_ok(fb[:, 6]), f"{name}: a heading differs"
        kept = []
        for rows in seq.candidates(score, smp, B, pre):
            b = np.ascontiguousarray(fb[rows, :7])
            if len(b) == 0:
                kept.append(0)
                continue
            walks = [reference_arithmetic_walk(b, thresh), ol.nms(b, F(thresh), rotated=True, arith="f64"),
                     ol.nms(b, F(thresh), rotated=True, arith="glibc")]
            assert all(np.array_equal(walks[0], w) for w in walks[1:]), f"{name}: the three arithmetics keep different boxes"
            assert not far_from_threshold(b, thresh, post), f"{name}: a compared pair lies within ten bounds of the threshold"
            kept.append(len(walks[0]))
        r = res[name]
        ref = (r["rois"], r["roi_scores"], r["roi_labels"])
        assert ref[0].dtype == F and ref[1].dtype == F and ref[2].dtype == np.int64
        assert r["has_class_labels"] == (fc.shape[1] > 1)
        for fn in (seq.proposals, seq.proposals_chunked):
            ours = fn(box, cls, B, pre, post, thresh, True, bidx)
            assert seq.same(ours, ref), f"{name}: {fn.__name__} differs from the reference\n" + "\n".join(seq.describe(ours, ref))
        rec[name + "_cfg"] = np.array(json.dumps(cfg))
        rec[name + "_box"], rec[name + "_cls"] = box, cls
        if bidx is not None:
            rec[name + "_batch_index"] = bidx
        rec[name + "_rois"], rec[name + "_roi_scores"], rec[name + "_roi_labels"] = ref
        print(name, "box", box.shape, "cls", cls.shape, "survivors of the uncapped walk", kept, "POST", post)
    return rec


def save(path, rec, limit):
    have = dict(np.load(path)) if os.path.exists(path) else {}
    if sorted(have) == sorted(rec) and all(have[k].dtype == np.asarray(v).dtype and have[k].shape == np.asarray(v).shape
                                           and have[k].tobytes() == np.asarray(v).tobytes() for k, v in rec.items()):
        print(path, "holds these arrays already: left as it is")
    else:
        np.savez_compressed(path, **rec)
    size_ = os.path.getsize(path)
    assert size_ <= limit, size_
    print(path, size_, "bytes")


def main():
    rec = record(build_scenes())
    import proposals_seq as seq
    cfgs = {n: seq.scene_inputs(rec, n)[0] for n in seq.scenes(rec)}
    post = seq.recorded(rec, "post")[2]
    assert (seq.recorded(rec, "post")[1][0] != 0).all() and (seq.recorded(rec, "post")[1][1] == 0).any() and post.shape == (2, cfgs["post"]["NMS_POST_MAXSIZE"])
    save(GOLD, rec, 64 * 1024)


if __name__ == "__main__":
    main()
