"""Golden RoI targets for modest_amd.utils.roi_targets (BUILD CONTAINER ONLY -- needs /root/reference).

Runs the reference's own ``ProposalTargetLayer.forward`` and ``RoIHeadTemplate.assign_targets`` (imported from where they
lie, nothing copied) on the CPU in a child process, after ``np.random.seed`` / ``torch.manual_seed`` per scene.  The child
binds empty package modules that keep their ``__path__`` (so ``pcdet/models/__init__.py`` is never executed) and this
project's shims for the extension modules (``pcdet_bind.install``).  It substitutes two things and nothing else:
  * ``torch.cuda.FloatTensor`` (iou3d_nms_utils.py:66) becomes ``torch.FloatTensor``, the CPU type;
  * the shim's ``boxes_overlap_bev_gpu`` becomes oracle.labels.boxes_iou_bev(overlap_only=True, arith="f64"), the twin the
    device kernels equal bit for bit.

Recorded in tests/golden/roi_targets.npz per scene: the config as JSON, the two seeds, the four inputs, the eight outputs.
  cls        PointRCNN's thresholds (0.55 / 0.6 / 0.45 / 0.1 / 0.8, FG_RATIO 0.5), M = 16, B = 4: sample 0 takes the
             fg-and-bg branch with both bg lists, 1 fg and bg with only hard, 2 bg with only hard, 3 (all gts zero) bg with
             only easy; every sample has another number of trailing zero rows.  The fg-only branch cannot be recorded: the
             reference ends it in torch.cat((fg_inds, [])) (proposal_target_layer.py:148, 161), a TypeError in this torch;
             tests/roi_targets_cases.py covers it against the restatement;
  roi_iou    PV-RCNN's thresholds (0.55 / 0.75 / 0.25 / 0.1), labels 1 - 3, a roi class without a gt, M above the rois.  C = 0:
             the reference's boxes_iou3d_gpu asserts 7 columns on the rois it is handed whole (iou3d_nms_utils.py:57), so its
             assign_targets cannot run with C > 0; C = 2 is covered by tests/roi_targets_cases.py against the restatement;
  any_class  SAMPLE_ROI_BY_EACH_CLASS off.
The tool asserts
  * that the glibc oracle and the f64 twin give the same three lists and the same assignments;
  * that no positive maximum is attained by two gts;
  * that every maximum lies farther from every threshold it is compared with than ten times the pair's derived bound: the
    BEV overlap bound of tests/iou3d_cases.py times the exact height overlap, twice over the exact union, plus 1e-6;
  * that torch's CPU cos / sin of every -ry (and ry) equal the double function rounded once -- rois are drawn by
    rejection, at most a quarter dropped;
  * that the restatement (tests/roi_targets_seq.py) reproduces every recorded output bit for bit from the seeds alone, and
    the fixture's size (64 KB).

Usage:  python tools/make_golden_roi_targets.py
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
GOLD = os.path.join(ROOT, "tests", "golden", "roi_targets.npz")
F = np.float32

_CHILD = r"""
import os, pickle, sys, types
import numpy as np
import torch
ref, root, job = sys.argv[1], sys.argv[2], pickle.load(open(sys.argv[3], "rb"))
sys.path.insert(0, root)
for name in ("pcdet", "pcdet.models", "pcdet.models.roi_heads", "pcdet.models.roi_heads.target_assigner",
             "pcdet.models.model_utils", "pcdet.utils", "pcdet.ops", "pcdet.ops.iou3d_nms", "pcdet.ops.roiaware_pool3d"):
    m = types.ModuleType(name)
    m.__path__ = [os.path.join(ref, *name.split("."))]
    sys.modules[name] = m
from modest_amd.utils import pcdet_bind
pcdet_bind.install(stand_ins=False)
from oracle import labels as ol
from pcdet.ops.iou3d_nms import iou3d_nms_utils
from pcdet.models.roi_heads.roi_head_template import RoIHeadTemplate
from pcdet.models.roi_heads.target_assigner.proposal_target_layer import ProposalTargetLayer
assert RoIHeadTemplate.__module__.startswith("pcdet.") and iou3d_nms_utils.__file__.startswith(ref)
assert sys.modules[ProposalTargetLayer.__module__].__file__.startswith(ref)

# the two substitutions
torch.cuda.FloatTensor = torch.FloatTensor
def boxes_overlap_bev_gpu(a, b, out):
    out.copy_(torch.from_numpy(ol.boxes_iou_bev(a.numpy(), b.numpy(), overlap_only=True, arith="f64")))
iou3d_nms_utils.iou3d_nms_cuda = types.SimpleNamespace(boxes_overlap_bev_gpu=boxes_overlap_bev_gpu)

class Cfg(dict):
    __getattr__ = dict.__getitem__

res = {}
for name, (cfg, seeds, rois, scores, labels, gt) in job.items():
    head = types.SimpleNamespace(proposal_target_layer=ProposalTargetLayer(roi_sampler_cfg=Cfg(cfg)))
    def batch():
        return dict(batch_size=len(rois), rois=torch.from_numpy(rois.copy()), roi_scores=torch.from_numpy(scores.copy()),
                    roi_labels=torch.from_numpy(labels.copy()), gt_boxes=torch.from_numpy(gt.copy()))
    np.random.seed(seeds[0]); torch.manual_seed(seeds[1])
    out = RoIHeadTemplate.assign_targets(head, batch())
    np.random.seed(seeds[0]); torch.manual_seed(seeds[1])
    fwd = head.proposal_target_layer.forward(batch())
    assert list(fwd) == list(out)[:7] and all(torch.equal(fwd[k], out[k]) for k in fwd if k != "gt_of_rois")
    assert torch.equal(fwd["gt_of_rois"], out["gt_of_rois_src"])
    res[name] = (list(out), {k: v.numpy() for k, v in out.items()})
pickle.dump(res, open(sys.argv[4], "wb"))
"""

DRAWS = {"candidates": 0, "dropped": 0}
POINTRCNN = dict(ROI_PER_IMAGE=16, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True, CLS_SCORE_TYPE="cls", CLS_FG_THRESH=0.6,
                 CLS_BG_THRESH=0.45, CLS_BG_THRESH_LO=0.1, HARD_BG_RATIO=0.8, REG_FG_THRESH=0.55)
PVRCNN = dict(ROI_PER_IMAGE=16, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True, CLS_SCORE_TYPE="roi_iou", CLS_FG_THRESH=0.75,
              CLS_BG_THRESH=0.25, CLS_BG_THRESH_LO=0.1, HARD_BG_RATIO=0.8, REG_FG_THRESH=0.55)


def thresholds(cfg):
    return [cfg[k] for k in ("REG_FG_THRESH", "CLS_FG_THRESH", "CLS_BG_THRESH", "CLS_BG_THRESH_LO")]


def heading_ok(v):
    """torch's CPU cos / sin of v and -v equal the double functions rounded once"""
    import torch
    import roi_targets_seq as seq
    v = np.atleast_1d(np.asarray(v, F))
    t = torch.from_numpy(np.concatenate([v, -v]).copy())
    return bool(np.array_equal(torch.cos(t).numpy().view(np.uint32), seq.f32_trig(np.cos, t.numpy()).view(np.uint32))
                and np.array_equal(torch.sin(t).numpy().view(np.uint32), seq.f32_trig(np.sin, t.numpy()).view(np.uint32)))


def margins(rois7, gts7):
    """(exact 3-D IoU, its derived bound) of every pair, in float64"""
    import iou3d_cases as ic
    e = ic.Exact.all_pairs(np.ascontiguousarray(rois7, F), np.ascontiguousarray(gts7, F))
    a, b = rois7.astype(np.float64), gts7.astype(np.float64)
    h = np.clip(np.minimum((a[:, 2] + a[:, 5] / 2)[:, None], (b[:, 2] + b[:, 5] / 2)[None]) -
                np.maximum((a[:, 2] - a[:, 5] / 2)[:, None], (b[:, 2] - b[:, 5] / 2)[None]), 0, None)
    o3 = e.overlap * h
    union = np.maximum(a[:, 3:6].prod(1)[:, None] + b[:, 3:6].prod(1)[None] - o3, 1e-6)
    return o3 / union, 2 * e.overlap_bound * h / union + 1e-6


def objects(rs, n, x0, classes):
    """n objects 9 m apart (no roi reaches two of them) -> (n, 8) with the class in the last column"""
    return np.c_[x0 + 9.0 * np.arange(n), rs.uniform(-20, 20, n), rs.uniform(-1.5, 0.5, n), rs.uniform(3.2, 4.8, n),
                 rs.uniform(1.5, 2.0, n), rs.uniform(1.4, 1.7, n), rs.uniform(-3.2, 3.2, n), rs.choice(classes, n)].astype(F)


def draw_roi(rs, obj, kind):
    """a copy of the object moved so that its IoU tends to the list `kind`"""
    shift = {"fg": 0.08, "hard": 0.55, "easy": 1.6}[kind]
    b = obj[:7].astype(np.float64).copy()
    ang = rs.uniform(0, 2 * np.pi)
    b[:2] += shift * rs.uniform(0.6, 1.4) * np.array([np.cos(ang), np.sin(ang)])
    b[2] += rs.normal(0, 0.03)
    b[3:6] *= rs.normal(1, 0.03, 3)
    b[6] += rs.normal(0, 0.05) + np.pi * (rs.random_sample() < 0.3) + 2 * np.pi * rs.randint(-1, 2)
    return b.astype(F)


def make_sample(rs, cfg, gts, want, extra_cols=0, wrong_label=0, by_class=True):
    """rois whose maxima fall into the lists `want` names (a dict kind -> count), far from every threshold, with headings
    torch and the rounded double functions agree on -> (rois (n, 7 + C), labels (n,))"""
    import roi_targets_seq as seq
    valid = gts[:seq.trim(gts)]
    rois, labels = [], []
    for kind, count in want.items():
        have = 0
        while have < count:
            DRAWS["candidates"] += 1
            k = rs.randint(len(valid))
            r = draw_roi(rs, valid[k], kind)
            lab = np.int64(valid[k, -1])
            if not (heading_ok(r[6]) and heading_ok(seq.rem(r[6], seq.TWO_PI))):
                DRAWS["dropped"] += 1
                continue
            best, at, _ = seq.match(r[None], np.array([lab]), gts, by_class)
            ls = seq.lists(best, cfg)
            ex, bound = margins(r[None, :7], valid[:, :7])
            hit = [len(ls[0]) == 1 and len(ls[1]) == 0, len(ls[1]) == 1 and len(ls[0]) == 0, len(ls[2]) == 1][("fg", "hard", "easy").index(kind)]
            far = all(abs(ex[0, at[0]] - t) > 10 * bound[0, at[0]] for t in thresholds(cfg))
            if not (hit and far):
                DRAWS["dropped"] += 1 if hit else 0      # a miss of the list is no rejected box: it is aimed again
                continue
            rois.append(np.concatenate([r, rs.uniform(-1, 1, extra_cols).astype(F)]))
            labels.append(lab)
            have += 1
    for _ in range(wrong_label):       # rois of a class no gt has: maximum 0, assignment 0
        DRAWS["candidates"] += 1
        r = draw_roi(rs, valid[rs.randint(len(valid))], "fg")
        while not (heading_ok(r[6]) and heading_ok(seq.rem(r[6], seq.TWO_PI))):
            DRAWS["dropped"] += 1
            r = draw_roi(rs, valid[rs.randint(len(valid))], "fg")
        rois.append(np.concatenate([r, rs.uniform(-1, 1, extra_cols).astype(F)]))
        labels.append(np.int64(7))
    perm = rs.permutation(len(rois))
    return np.stack(rois)[perm].astype(F), np.asarray(labels, np.int64)[perm]


def pad(gts, rows, cols):
    out = np.zeros((rows, cols), F)
    out[:len(gts), :7], out[:len(gts), -1] = gts[:, :7], gts[:, -1]
    return out


def build_scenes():
    rs = np.random.RandomState(20261022)
    out = {}
    # cls: B = 4, 24 rois, gts padded to 9 rows
    cfg = dict(POINTRCNN)
    gts = [pad(objects(rs, 5, 0.0, [1, 2, 3]), 9, 8), pad(objects(rs, 3, 60.0, [1, 2, 3]), 9, 8), pad(objects(rs, 7, -80.0, [1, 2, 3]), 9, 8),
           np.zeros((9, 8), F)]
    wants = [dict(fg=9, hard=8, easy=7), dict(fg=5, hard=19), dict(hard=24), None]
    rois, labels = [], []
    for g, w in zip(gts[:3], wants[:3]):
        r, l = make_sample(rs, cfg, g, w)
        rois.append(r), labels.append(l)
    r, l = make_sample(rs, cfg, gts[0], dict(fg=10, hard=14))      # sample 3: real rois against gts that are all zero
    rois.append(r), labels.append(l)
    scores = rs.random_sample((4, 24)).astype(F)
    out["cls"] = (cfg, (11, 12), np.stack(rois), scores, np.stack(labels), np.stack(gts))
    # roi_iou: labels 1 - 3, three rois per sample of a class without a gt, M = 16 above the 12 rois
    cfg = dict(PVRCNN)
    gts, rois, labels = [], [], []
    for b in range(2):
        g = pad(objects(rs, 4 + b, 30.0 * b, [1, 2, 3]), 8, 8)
        r, l = make_sample(rs, cfg, g, dict(fg=4, hard=3, easy=2), wrong_label=3)
        gts.append(g), rois.append(r), labels.append(l)
    out["roi_iou"] = (cfg, (21, 22), np.stack(rois), rs.random_sample((2, 12)).astype(F), np.stack(labels), np.stack(gts))
    # any_class: the class restriction off, labels that match no gt
    cfg = dict(POINTRCNN, SAMPLE_ROI_BY_EACH_CLASS=False)
    gts, rois, labels = [], [], []
    for b in range(2):
        g = pad(objects(rs, 3 + 2 * b, -40.0 * b, [1, 2, 3]), 7, 8)
        r, l = make_sample(rs, cfg, g, dict(fg=6, hard=7, easy=7), by_class=False)
        gts.append(g), rois.append(r), labels.append(rs.randint(1, 4, len(l)).astype(np.int64))
    out["any_class"] = (cfg, (31, 32), np.stack(rois), rs.random_sample((2, 20)).astype(F), np.stack(labels), np.stack(gts))
    return out


def record(job):
    import torch
    import roi_targets_seq as seq
    print("drawn by rejection: %(candidates)d candidates, %(dropped)d dropped" % DRAWS)
    assert DRAWS["dropped"] * 4 <= DRAWS["candidates"], DRAWS
    with tempfile.TemporaryDirectory() as work:
        pickle.dump(job, open(os.path.join(work, "job.pkl"), "wb"))
        open(os.path.join(work, "child.py"), "w").write(_CHILD)
        subprocess.run([sys.executable, os.path.join(work, "child.py"), REF, ROOT, os.path.join(work, "job.pkl"),
                        os.path.join(work, "res.pkl")], check=True)
        res = pickle.load(open(os.path.join(work, "res.pkl"), "rb"))
    rec = {"scenes": np.array(json.dumps(list(job)))}
    for name, (cfg, seeds, rois, scores, labels, gt) in job.items():
        by_class = cfg["SAMPLE_ROI_BY_EACH_CLASS"]
        branches = []
        for b in range(len(rois)):
            found = {}
            for arith in ("f64", "glibc"):
                best, at, n = seq.match(rois[b], labels[b], gt[b], by_class, arith=arith)
                found[arith] = (at, seq.lists(best, cfg))
            assert np.array_equal(found["f64"][0], found["glibc"][0]), f"{name}[{b}]: the two arithmetics assign differently"
            assert all(np.array_equal(x, y) for x, y in zip(found["f64"][1], found["glibc"][1])), f"{name}[{b}]: lists differ"
            best, at, n = seq.match(rois[b], labels[b], gt[b], by_class)
            valid = gt[b][:n]
            iou = seq.iou3d(rois[b][:, :7], valid[:, :7])
            comp = (labels[b][:, None] == valid[None, :, -1].astype(np.int64)) if by_class else np.ones(iou.shape, bool)
            twice = ((iou == best[:, None]) & comp).sum(1) > 1
            assert not (twice & (best > 0)).any(), f"{name}[{b}]: a positive maximum is attained twice"
            ex, bound = margins(rois[b][:, :7], valid[:, :7])
            rows = np.flatnonzero(comp.any(1))
            for t in thresholds(cfg):
                assert (np.abs(ex[rows, at[rows]] - t) > 10 * bound[rows, at[rows]]).all(), f"{name}[{b}]: a maximum near {t}"
            ry = seq.rem(rois[b][:, 6], seq.TWO_PI)
            assert heading_ok(ry) and heading_ok(rois[b][:, 6]), f"{name}[{b}]: a heading differs"
            branches.append(tuple(len(l) for l in found["f64"][1]))
        keys, ref = res[name]
        assert tuple(keys) == seq.KEYS, keys
        np.random.seed(seeds[0])
        torch.manual_seed(seeds[1])
        ours = seq.assign_targets(rois, scores, labels, gt, cfg)
        assert seq.same(ours, ref), f"{name}: the restatement differs from the reference\n" + "\n".join(seq.describe(ours, ref))
        rec[name + "_cfg"] = np.array(json.dumps(cfg))
        rec[name + "_seeds"] = np.asarray(seeds, np.int64)
        rec[name + "_in_rois"], rec[name + "_in_roi_scores"], rec[name + "_in_roi_labels"] = rois, scores, labels
        rec[name + "_gt_boxes"] = gt
        for k in seq.KEYS:
            rec[name + "_" + k] = ref[k]
        print(name, "rois", rois.shape, "gt", gt.shape, "(fg, hard, easy) per sample", branches)
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
    save(GOLD, rec, 64 * 1024)


if __name__ == "__main__":
    main()
