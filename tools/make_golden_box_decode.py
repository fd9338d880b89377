"""Golden decoded boxes for modest_amd.utils.box_decode (BUILD CONTAINER ONLY -- needs /root/reference).

Runs the reference's own ``AnchorHeadTemplate`` / ``PointHeadTemplate`` / ``RoIHeadTemplate`` ``.generate_predicted_boxes`` with
its ``ResidualCoder`` / ``PointResidualCoder`` (imported from where they lie, nothing copied) on the CPU in a child process.
The child binds empty package modules that keep their ``__path__`` (so ``pcdet/models/__init__.py`` is never executed) and this
project's shims for the extension modules (``pcdet_bind.install``), and makes ``Tensor.cuda`` the identity (PointResidualCoder
calls it on its table).

Recorded in tests/golden/box_decode.npz per scene: the settings as JSON (plain values), the inputs and the decoded boxes.
  anchor head  a 2 x 3 grid with 2 classes x 2 rotations (N = 24), B = 2: code 7 with the direction classifier; code 9; without
               the direction classifier; the sincos coder (with the direction classifier)
  point head   PointRCNN-like with K = 3; K = 1; no mean size
  RoI head     2 x 3 rois; 4 x 100 rois
The tool asserts, per scene, what tests/test_box_decode_cpu.py asserts again: the restatement (tests/box_decode_seq.py) equals
the recording bit for bit on the columns made of + - * / floor only, both lie within the derived bound of the exact value
elsewhere, and the NaN / inf / zero patterns are equal.  It prints the largest error over bound of either, and the fixture's size.

Usage:  python tools/make_golden_box_decode.py
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
GOLD = os.path.join(ROOT, "tests", "golden", "box_decode.npz")
F = np.float32

_CHILD = r"""
import os, pickle, sys, types
import numpy as np
import torch
ref, root, job = sys.argv[1], sys.argv[2], pickle.load(open(sys.argv[3], "rb"))
sys.path.insert(0, root)
for name in ("pcdet", "pcdet.models", "pcdet.models.dense_heads", "pcdet.models.dense_heads.target_assigner",
             "pcdet.models.roi_heads", "pcdet.models.roi_heads.target_assigner", "pcdet.models.model_utils", "pcdet.utils",
             "pcdet.ops", "pcdet.ops.iou3d_nms", "pcdet.ops.roiaware_pool3d"):
    m = types.ModuleType(name)
    m.__path__ = [os.path.join(ref, *name.split("."))]
    sys.modules[name] = m
from modest_amd.utils import pcdet_bind
pcdet_bind.install(stand_ins=False)
torch.Tensor.cuda = lambda self, *a, **k: self
from pcdet.models.dense_heads.anchor_head_template import AnchorHeadTemplate
from pcdet.models.dense_heads.point_head_template import PointHeadTemplate
from pcdet.models.roi_heads.roi_head_template import RoIHeadTemplate
from pcdet.utils.box_coder_utils import PointResidualCoder, ResidualCoder
for c in (AnchorHeadTemplate, PointHeadTemplate, RoIHeadTemplate, ResidualCoder):
    assert c.__module__.startswith("pcdet.") and sys.modules[c.__module__].__file__.startswith(ref)
class Cfg(dict):
    __getattr__ = dict.__getitem__
t = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy())
res = {}
for name, (case, per_class) in job.items():
    kind = case["kind"]
    if kind == "anchor":
        B, N, code = case["box"].shape
        sincos = bool(case["sincos"])
        head = types.SimpleNamespace(anchors=[t(a) for a in per_class], use_multihead=False,
                                     box_coder=ResidualCoder(code_size=code - (1 if sincos else 0), encode_angle_by_sincos=sincos))
        if case["dir"] is not None:
            head.model_cfg = Cfg(DIR_OFFSET=case["dir_offset"], DIR_LIMIT_OFFSET=case["dir_limit_offset"],
                                 NUM_DIR_BINS=case["dir"].shape[-1])
        assert head.box_coder.code_size == code
        box, dirp = t(case["box"]), None if case["dir"] is None else t(case["dir"])
        cls = torch.zeros((B, N * 2))
        cls_out, out = AnchorHeadTemplate.generate_predicted_boxes(head, B, cls, box.view(B, -1), None if dirp is None else dirp.view(B, -1))
        assert cls_out.shape == (B, N, 2) and np.array_equal(box.numpy().view(np.uint32), case["box"].view(np.uint32))
    elif kind == "point":
        kw = {} if case["mean"] is None else dict(mean_size=case["mean"].astype(np.float64).tolist())
        head = types.SimpleNamespace(box_coder=PointResidualCoder(code_size=case["box"].shape[1], use_mean_size=case["mean"] is not None, **kw))
        if case["mean"] is not None:
            assert np.array_equal(head.box_coder.mean_size.numpy(), case["mean"])
        coords, cls = t(case["coords"]), t(case["cls"])
        cls_out, out = PointHeadTemplate.generate_predicted_boxes(head, coords[:, 1:4], cls, t(case["box"]))
        assert cls_out is cls
    else:
        B, M, code = case["rois"].shape
        head = types.SimpleNamespace(box_coder=ResidualCoder(code_size=code))
        rois = t(case["rois"])
        cls_out, out = RoIHeadTemplate.generate_predicted_boxes(head, B, rois, torch.zeros((B * M, 1)), t(case["box"]))
        assert cls_out.shape == (B, M, 1) and out.shape == (B, M, code)
        assert np.array_equal(rois.numpy().view(np.uint32), case["rois"].view(np.uint32)), "the reference changed its input"
    res[name] = out.detach().numpy().astype(np.float32)
pickle.dump(res, open(sys.argv[4], "wb"))
"""


def build_scenes():
    """-> {name: (case, per-class anchor arrays or None)}"""
    import box_decode_seq as seq
    out = {}

    def anchor(name, seed, extra=0, bins=2, sincos=False):
        per_class = seq.anchor_grid(extra=extra, seed=seed)
        flat = seq.flat_anchors(per_class)
        assert flat.shape == (24, 7 + extra)
        case = seq.make_anchor(seed, B=2, N=24, extra=extra, bins=bins, sincos=sincos, dir_offset=0.78539, dir_limit_offset=0.0,
                               anchors=flat)
        out[name] = (case, per_class)

    anchor("anchor_code7_dir", 1)
    anchor("anchor_code9_dir", 2, extra=2)
    anchor("anchor_code7", 3, bins=0)
    anchor("anchor_sincos", 4, sincos=True)
    out["point_k3"] = (seq.make_point(5, N=300, K=3), None)
    out["point_k1"] = (seq.make_point(6, N=70, K=1), None)
    out["point_no_mean"] = (seq.make_point(7, N=70, K=3, mean=False), None)
    out["roi_2x3"] = (seq.make_roi(8, B=2, M=3), None)
    big = seq.make_roi(9, B=4, M=100)
    # a few of the edges among the 400: an infinite z encoding, an infinite x encoding, a roi with dx = dy = 0, headings at +-pi
    big["box"][5, 2] = np.inf
    big["box"][6, 0] = -np.inf
    big["box"][7, 3] = 89.0
    big["rois"][0, 8, 3:5] = 0.0
    big["rois"][0, 9, 6], big["rois"][0, 10, 6] = np.pi, -np.pi
    out["roi_4x100"] = (big, None)
    return out


def main():
    import box_decode_seq as seq
    job = build_scenes()
    with tempfile.TemporaryDirectory() as work:
        pickle.dump(job, open(os.path.join(work, "job.pkl"), "wb"))
        open(os.path.join(work, "child.py"), "w").write(_CHILD)
        subprocess.run([sys.executable, os.path.join(work, "child.py"), REF, ROOT, os.path.join(work, "job.pkl"),
                        os.path.join(work, "res.pkl")], check=True)
        res = pickle.load(open(os.path.join(work, "res.pkl"), "rb"))
    rec = {"scenes": np.array(json.dumps(list(job)))}
    worst = {"ours": 0.0, "the reference": 0.0}
    for name, (case, _) in job.items():
        ref = res[name]
        ours = seq.restate(case)
        assert ref.reshape(ours.shape).shape == ours.shape and ref.dtype == F, name
        ref = ref.reshape(ours.shape)
        ex = seq.exact(case)
        for who, got in (("ours", ours), ("the reference", ref)):
            why, ratio = seq.bound_report(got, ex, f"{name}: {who}")
            assert not why, why
            worst[who] = max(worst[who], ratio)
        why = seq.pattern_report(ours, ref, name)
        assert not why, why
        cols = seq.exact_columns(case)
        why = seq.report(ours[..., cols], ref[..., cols], f"{name}: columns {cols}")
        assert not why, why
        unequal = int((seq.bits(ours) != seq.bits(ref)).sum())
        print(f"{name}: {ours.shape}, bit for bit on columns {cols}, {unequal} of {ours.size} elements differ elsewhere")
        cfg = {k: v for k, v in case.items() if not isinstance(v, np.ndarray) and v is not None}
        rec[name + "_cfg"] = np.array(json.dumps(cfg))
        for f in seq.FIELDS[case["kind"]]:
            if case.get(f) is not None:
                rec[f"{name}_{f}"] = case[f]
        rec[name + "_out"] = ref
    print("largest error / bound:", worst)
    np.savez_compressed(GOLD, **rec)
    back = seq.scenes(dict(np.load(GOLD)))
    assert [n for n, _, _ in back] == list(job)
    size = os.path.getsize(GOLD)
    assert size <= 128 * 1024, size
    print(GOLD, size, "bytes")


if __name__ == "__main__":
    main()
