"""Golden anchor-head losses for modest_amd.utils.anchor_head_loss (BUILD CONTAINER ONLY -- needs /root/reference).

Runs the reference's own ``AnchorHeadTemplate.get_loss`` (imported from where it lies, nothing copied) with ``backward()`` on
the CPU in a child process, on a bare instance that carries only the attributes the method reads.  The child binds empty
package modules that keep their ``__path__`` (so ``pcdet/models/__init__.py`` is never executed), this project's shims for
the extension modules ``box_utils`` and ``iou3d_nms_utils`` pull in (``pcdet_bind.install``), and makes ``Tensor.cuda`` the
identity.

Recorded in tests/golden/anchor_loss.npz per scene: the config as JSON (the inputs are regenerated from its seed and its
specials by tests/anchor_loss_seq.py:make_inputs), the four scalars and the three autograd gradients.  Before it writes, the
tool asserts that the restatement and the recorded values lie within the derived bound of ``exact()`` in every element, that
the zero patterns of the gradients agree, and prints the largest error-to-bound ratio per output.

A second config set (``anchor_loss_seq.edge_scene_cfgs``: headings at every direction-bin edge and its float32 neighbours,
saturating and non-finite direction logits, non-finite and huge box values and class logits, the head's real layout of
three anchor tensors) goes into tests/golden/anchor_loss_edges.npz, under the same assertions.

Usage:  python tools/make_golden_anchor_loss.py        (writes tests/golden/anchor_loss.npz)
        python tools/make_golden_anchor_loss.py edges  (writes tests/golden/anchor_loss_edges.npz)
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
sys.path.insert(0, os.path.join(root, "tests"))
for name in ("pcdet", "pcdet.models", "pcdet.models.dense_heads", "pcdet.models.dense_heads.target_assigner", "pcdet.utils",
             "pcdet.ops", "pcdet.ops.iou3d_nms", "pcdet.ops.roiaware_pool3d"):
    m = types.ModuleType(name)
    m.__path__ = [os.path.join(ref, *name.split("."))]
    sys.modules[name] = m
from modest_amd.utils import pcdet_bind
pcdet_bind.install(stand_ins=False)
torch.Tensor.cuda = lambda self, *a, **k: self
from pcdet.models.dense_heads.anchor_head_template import AnchorHeadTemplate
from pcdet.utils import loss_utils
assert AnchorHeadTemplate.__module__.startswith("pcdet.") and "pcdet.models.backbones_3d" not in sys.modules
class Cfg(dict):
    __getattr__ = dict.__getitem__
res = {}
for name, (cfg, inp) in job.items():
    head = AnchorHeadTemplate.__new__(AnchorHeadTemplate)
    torch.nn.Module.__init__(head)
    head.model_cfg = Cfg(LOSS_CONFIG=Cfg(LOSS_WEIGHTS=dict(cls_weight=cfg["cls_weight"], loc_weight=cfg["loc_weight"],
                                                           dir_weight=cfg["dir_weight"], code_weights=cfg["code_weights"])),
                         DIR_OFFSET=cfg["dir_offset"], NUM_DIR_BINS=cfg["bins"], USE_MULTIHEAD=False)
    head.num_class, head.num_anchors_per_location, head.use_multihead = cfg["num_class"], 1, False
    head.anchors = [torch.from_numpy(inp["anchors"].copy()).view(1, 1, -1, 1, 1, inp["anchors"].shape[-1])]
    shape = lambda k: inp[k].shape
    if cfg.get("layout"):      # the head's real layout: three anchor tensors, six anchors per location, (B, H, W, 6 * columns)
        import anchor_loss_seq
        H, W = cfg["layout"]
        head.num_anchors_per_location = 6
        head.anchors = [torch.from_numpy(t) for t in anchor_loss_seq.anchor_tensors(cfg, inp["anchors"])]
        shape = lambda k: (inp[k].shape[0], H, W, 6 * inp[k].shape[2])
    head.cls_loss_func = loss_utils.SigmoidFocalClassificationLoss(alpha=0.25, gamma=2.0)
    if cfg["beta"] == 0:
        head.reg_loss_func = loss_utils.WeightedL1Loss(code_weights=cfg["code_weights"])
    else:
        head.reg_loss_func = loss_utils.WeightedSmoothL1Loss(beta=cfg["beta"], code_weights=cfg["code_weights"])
    head.dir_loss_func = loss_utils.WeightedCrossEntropyLoss()
    preds = {k: torch.from_numpy(inp[k].copy().reshape(shape(k))).requires_grad_(True) for k in ("cls", "box", "dir")
             if inp[k] is not None}
    head.forward_ret_dict = dict(cls_preds=preds["cls"], box_preds=preds["box"],
                                 box_cls_labels=torch.from_numpy(inp["labels"].copy()),
                                 box_reg_targets=torch.from_numpy(inp["tg"].copy()))
    if "dir" in preds:
        head.forward_ret_dict["dir_cls_preds"] = preds["dir"]
    loss, tb = head.get_loss()
    loss.backward()
    out = dict(losses=np.array([tb["rpn_loss_cls"], tb["rpn_loss_loc"], tb.get("rpn_loss_dir", 0.0), tb["rpn_loss"]], dtype=np.float32),
               grad_cls=preds["cls"].grad.numpy().reshape(inp["cls"].shape), grad_box=preds["box"].grad.numpy().reshape(inp["box"].shape))
    assert np.float32(loss.item()) == out["losses"][3] or np.isnan(out["losses"][3])
    if "dir" in preds:
        out["grad_dir"] = preds["dir"].grad.numpy().reshape(inp["dir"].shape)
    res[name] = out
pickle.dump(res, open(sys.argv[4], "wb"))
"""


def configs(seq):
    c = seq.base_cfg
    return {
        "kitti": c(B=2, N=520, num_class=3, seed=11, pos=0.04),
        "lyft": c(B=3, N=257, num_class=1, label_max=3, samples=["mixed", "none", "all"], seed=12, dir_offset=0.78539,
                  cls_weight=1.0, loc_weight=2.0, dir_weight=0.2),
        "wide": c(B=1, N=257, num_class=10, code=9, bins=4, dir_offset=0.0, seed=13, int64=True, pos=0.1,
                  code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2], loc_weight=0.25),
        "edge": c(B=3, N=70, num_class=3, code=8, bins=0, samples=["mixed", "ignore", "none"], seed=14,
                  specials=["logits", "beta", "nan2"]),
        "l1": c(B=1, N=70, num_class=3, beta=0.0, seed=15, pos=0.2),
        "nan6": c(B=2, N=70, num_class=1, seed=16, pos=0.2, specials=["nan6"]),
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
    import anchor_loss_seq as seq
    assert which in ("scenes", "edges"), which
    cfgs = configs(seq) if which == "scenes" else seq.edge_scene_cfgs()
    job = {n: (cfg, seq.make_inputs(cfg)) for n, cfg in cfgs.items()}
    ref = run_reference(job)
    store = {"scenes": np.array(json.dumps(list(cfgs)))}
    worst = {}
    for name, (cfg, inp) in job.items():
        ours, ex = seq.restate(inp, cfg), seq.exact(inp, cfg)
        for who, got in (("ours", ours), ("reference", ref[name])):
            why, ratios = seq.bound_report(got, ex, who)
            assert not why, f"{name}\n{why}"
            for k, v in ratios.items():
                worst[(who, k)] = max(worst.get((who, k), 0.0), v)
        why = seq.zero_report(ours, ref[name])
        assert not why, f"{name}\n{why}"
        assert set(ours) == set(ref[name])
        store[f"{name}/cfg"] = np.array(json.dumps(cfg))
        for k, v in ref[name].items():
            if k in cfg.get("record", seq.OUTPUTS):      # a direction scene keeps the scalars and grad_dir alone
                store[f"{name}/{k}"] = v
    if which == "scenes":
        assert np.isnan(ref["nan6"]["losses"][[1, 3]]).all() and not np.isnan(ref["edge"]["losses"]).any()
    path = os.path.join(GOLD, "anchor_loss.npz" if which == "scenes" else "anchor_loss_edges.npz")
    np.savez_compressed(path, **store)
    for (who, k), v in sorted(worst.items()):
        print(f"largest error / bound, {who:9s} {k:9s} {v:.3f}")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(*sys.argv[1:2])
