"""Golden RoI-head losses for modest_amd.utils.roi_head_loss (BUILD CONTAINER ONLY -- needs /root/reference).

Runs the reference's own ``RoIHeadTemplate.get_loss`` (imported from where it lies, nothing copied) with ``backward()`` on the
CPU in a child process, on a bare instance that carries only the attributes the method reads: its own ``ResidualCoder`` and
``WeightedSmoothL1Loss``.  The child binds empty package modules that keep their ``__path__`` (so ``pcdet/models/__init__.py``
is never executed), this project's shims for the extension modules (``pcdet_bind.install``), and makes ``Tensor.cuda`` the
identity.

One substitution, for the scenes with ignored rows (labels of -1) only: torch's CPU ``binary_cross_entropy`` raises on a
target outside [0, 1] where the device kernel does not, so the child wraps ``torch.nn.functional.binary_cross_entropy`` to
pass ``target.clamp(min=0)``.  The reference takes its valid mask from the unclamped labels, so those rows still enter its
sum as ``finite * 0`` and its gradient as 0.  Scenes with soft ``roi_iou`` labels run unwrapped.

Recorded in tests/golden/roi_loss.npz per scene: the config as JSON (the inputs are regenerated from its seed and its specials
by tests/roi_loss_seq.py:make_inputs), the table (the three or four scalars of tb_dict, rcnn_loss_corner 0 where the reference
has no such key, fg_sum and the count of valid class rows) and the two autograd gradients.  Before it writes, the tool asserts
that the restatement and the recorded values lie within the derived bound of ``exact()`` in every element with NaNs in the
same places, that the zero patterns of the gradients agree, that fg_sum agrees and that the reference left the sizes of
gt_of_rois clamped in place (the visible difference), and prints the largest error-to-bound ratio per output (DESIGN.md
section 7q).

A second config set (``roi_loss_seq.edge_scene_cfgs``: NaN and infinite values in rcnn_reg and in a gt on foreground rows,
infinite logits, huge finite values, each with and without the corner term) goes into tests/golden/roi_loss_edges.npz, under
the same assertions.

Usage:  python tools/make_golden_roi_loss.py        (writes tests/golden/roi_loss.npz)
        python tools/make_golden_roi_loss.py edges  (writes tests/golden/roi_loss_edges.npz)
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
GOLD = os.path.join(ROOT, "tests", "golden")

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
torch.Tensor.cuda = lambda self, *a, **k: self
from pcdet.models.roi_heads.roi_head_template import RoIHeadTemplate
from pcdet.utils import box_coder_utils, loss_utils
assert RoIHeadTemplate.__module__.startswith("pcdet.") and sys.modules[RoIHeadTemplate.__module__].__file__.startswith(ref)
class Cfg(dict):
    __getattr__ = dict.__getitem__
bce = torch.nn.functional.binary_cross_entropy
def bce_clamped(input, target, *a, **k):
    return bce(input, target.clamp(min=0), *a, **k)
res = {}
for name, (cfg, inp) in job.items():
    head = RoIHeadTemplate.__new__(RoIHeadTemplate)
    torch.nn.Module.__init__(head)
    head.model_cfg = Cfg(LOSS_CONFIG=Cfg(CLS_LOSS="BinaryCrossEntropy", REG_LOSS="smooth-l1",
                                         CORNER_LOSS_REGULARIZATION=bool(cfg["corner"]),
                                         LOSS_WEIGHTS=dict(rcnn_cls_weight=cfg["cls_weight"], rcnn_reg_weight=cfg["reg_weight"],
                                                           rcnn_corner_weight=cfg["corner_weight"], code_weights=cfg["code_weights"])))
    head.box_coder = box_coder_utils.ResidualCoder(code_size=cfg["code"])
    head.reg_loss_func = loss_utils.WeightedSmoothL1Loss(code_weights=cfg["code_weights"])
    head.reg_loss_func.beta = cfg["beta"]
    B, M, code = cfg["B"], cfg["M"], cfg["code"]
    assert cfg["gt_cols"] == code          # the reference views gt_of_rois[..., 0:code] as (R, code)
    preds = {"cls": torch.from_numpy(inp["cls"].copy()).view(-1, 1).requires_grad_(True),
             "reg": torch.from_numpy(inp["reg"].copy()).requires_grad_(True)}
    t = lambda a, *shape: torch.from_numpy(a.copy()).view(*shape)
    head.forward_ret_dict = dict(rcnn_cls=preds["cls"], rcnn_reg=preds["reg"], rcnn_cls_labels=t(inp["labels"], B, M),
                                 reg_valid_mask=t(inp["mask"], B, M), gt_of_rois=t(inp["gt"], B, M, code),
                                 gt_of_rois_src=t(inp["src"], B, M, code), rois=t(inp["rois"], B, M, code))
    wrapped = bool((inp["labels"] < 0).any())
    torch.nn.functional.binary_cross_entropy = bce_clamped if wrapped else bce
    loss, tb = head.get_loss()
    torch.nn.functional.binary_cross_entropy = bce
    loss.backward()
    fg = int((inp["mask"] > 0).sum())
    assert ("rcnn_loss_corner" in tb) == (bool(cfg["corner"]) and fg > 0), (name, sorted(tb))
    out = dict(table=np.array([tb["rcnn_loss_cls"], tb["rcnn_loss_reg"], tb.get("rcnn_loss_corner", 0.0), tb["rcnn_loss"], fg,
                               int((inp["labels"] >= 0).sum())], dtype=np.float32),
               grad_cls=preds["cls"].grad.numpy().reshape(-1), grad_reg=preds["reg"].grad.numpy(),
               gt_after=head.forward_ret_dict["gt_of_rois"].numpy().reshape(B * M, code), wrapped=wrapped)
    assert np.float32(loss.item()) == out["table"][3] or np.isnan(out["table"][3])
    res[name] = out
pickle.dump(res, open(sys.argv[4], "wb"))
"""


def configs(seq):
    c = seq.base_cfg
    return {
        "pointrcnn": c(B=2, M=128, seed=21, labels="cls", fg=0.3),
        "pvrcnn": c(B=3, M=64, seed=22, labels="iou", samples=["mixed", "nofg", "allfg"], mask_dtype="int32"),
        "nofg": c(B=2, M=64, seed=23, labels="cls", samples=["nofg", "nofg"]),
        "nocorner": c(B=2, M=64, seed=24, labels="iou", corner=False),
        "wide": c(B=1, M=130, code=9, seed=25, labels="cls", label_dtype="int32", cls_weight=1.5, reg_weight=0.75,
                  corner_weight=2.0, code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.5]),
        "edge": c(B=2, M=64, seed=26, labels="iou", samples=["mixed", "mixed"], specials=list(seq.EDGE_RECORDED)),
    }


def run_reference(job):
    with tempfile.TemporaryDirectory() as tmp:
        src, dst, prog = (os.path.join(tmp, n) for n in ("job.pkl", "res.pkl", "child.py"))
        pickle.dump(job, open(src, "wb"))
        open(prog, "w").write(_CHILD)
        env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
        subprocess.run([sys.executable, prog, REF, ROOT, src, dst], check=True, env=env)
        return pickle.load(open(dst, "rb"))


def main(which="scenes"):
    import roi_loss_seq as seq
    assert which in ("scenes", "edges"), which
    cfgs = configs(seq) if which == "scenes" else seq.edge_scene_cfgs()
    job = {n: (cfg, seq.make_inputs(cfg)) for n, cfg in cfgs.items()}
    ref = run_reference(job)
    store = {"scenes": np.array(json.dumps(list(cfgs)))}
    worst = {}
    for name, (cfg, inp) in job.items():
        ours, ex = seq.restate(inp, cfg), seq.exact(inp, cfg)
        rec = {k: ref[name][k] for k in seq.OUTPUTS}
        for who, got in (("ours", ours), ("reference", rec)):
            why, ratios = seq.bound_report(got, ex, who)
            assert not why, f"{name}\n{why}"
            for k, v in ratios.items():
                worst[(who, k)] = max(worst.get((who, k), 0.0), v)
        why = seq.zero_report(ours, rec)
        assert not why, f"{name}\n{why}"
        assert ours["table"][4] == rec["table"][4] and ours["table"][5] == rec["table"][5], name
        gt, after = inp["gt"][:, :cfg["code"]], ref[name]["gt_after"]
        clamped = np.where(np.arange(cfg["code"])[None, :] // 3 == 1, np.maximum(gt, np.float32(1e-5)), gt)
        assert np.array_equal(after, clamped, equal_nan=True), f"{name}: the reference left gt_of_rois otherwise than clamped"
        print(f"{name}: R = {cfg['B'] * cfg['M']}, fg_sum = {int(rec['table'][4])}, bce wrapped = {ref[name]['wrapped']}, "
              f"gt sizes clamped in place by the reference = {int((after != gt).sum() - np.isnan(gt).sum())}")
        store[f"{name}/cfg"] = np.array(json.dumps(cfg))
        for k, v in rec.items():
            store[f"{name}/{k}"] = v
    if which == "scenes":
        assert not np.isnan(ref["edge"]["table"]).any() and ref["nofg"]["table"][4] == 0
    path = os.path.join(GOLD, "roi_loss.npz" if which == "scenes" else "roi_loss_edges.npz")
    np.savez_compressed(path, **store)
    for (who, k), v in sorted(worst.items()):
        print(f"largest error / bound, {who:9s} {k:9s} {v:.3f}")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(*sys.argv[1:2])
