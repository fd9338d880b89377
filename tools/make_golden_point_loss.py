"""Golden point-head losses for modest_amd.utils.point_head_loss (BUILD CONTAINER ONLY -- needs /root/reference).

Runs the reference's own ``PointHeadBox.get_loss``, ``PointIntraPartOffsetHead.get_loss`` and ``PointHeadSimple.get_loss``
(imported from where they lie, nothing copied) with ``backward()`` on the CPU in a child process, on bare instances that carry
only the attributes the methods read: ``model_cfg``, ``num_class``, ``box_layers`` and what the reference's own
``build_losses`` makes of the config (its ``SigmoidFocalClassificationLoss`` and ``WeightedSmoothL1Loss``).  The child binds
empty package modules that keep their ``__path__`` (so ``pcdet/models/__init__.py`` is never executed), this project's shims
for the extension modules (``pcdet_bind.install(stand_ins=False)``), and makes ``Tensor.cuda`` the identity.

Nothing is substituted: the part labels of every scene lie inside [0, 1] (zero off the positives, as the target assignment
leaves them), so torch's CPU ``binary_cross_entropy`` accepts them.

Recorded in tests/golden/point_loss.npz per scene: the config as JSON (the inputs are regenerated from its seed and its
specials by tests/point_loss_seq.py:make_inputs), the table (tb_dict's floats, 0 for a term the head does not have, the loss
itself and point_pos_num) and the autograd gradients of the head's predictions.  Before it writes, the tool asserts that the
restatement and the recorded values lie within the derived bound of ``exact()`` in every element with NaNs in the same places,
that the zero patterns of the gradients agree, that point_pos_num agrees and that tb_dict holds the head's keys in the
reference's order, and prints the largest error-to-bound ratio per output.

A second config set (``point_loss_seq.edge_scene_cfgs``: NaN and infinite box values and labels, infinite focal and part
logits, huge finite values, all on positive rows) goes into tests/golden/point_loss_edges.npz, under the same assertions.

Usage:  python tools/make_golden_point_loss.py        (writes tests/golden/point_loss.npz)
        python tools/make_golden_point_loss.py edges  (writes tests/golden/point_loss_edges.npz)
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
for name in ("pcdet", "pcdet.models", "pcdet.models.dense_heads", "pcdet.utils", "pcdet.ops", "pcdet.ops.iou3d_nms",
             "pcdet.ops.roiaware_pool3d"):
    m = types.ModuleType(name)
    m.__path__ = [os.path.join(ref, *name.split("."))]
    sys.modules[name] = m
from modest_amd.utils import pcdet_bind
pcdet_bind.install(stand_ins=False)
torch.Tensor.cuda = lambda self, *a, **k: self
from pcdet.models.dense_heads.point_head_box import PointHeadBox
from pcdet.models.dense_heads.point_head_simple import PointHeadSimple
from pcdet.models.dense_heads.point_intra_part_head import PointIntraPartOffsetHead
heads = dict(PointHeadBox=PointHeadBox, PointHeadSimple=PointHeadSimple, PointIntraPartOffsetHead=PointIntraPartOffsetHead)
for h in heads.values():
    assert h.__module__.startswith("pcdet.") and sys.modules[h.__module__].__file__.startswith(ref) and "get_loss" in h.__dict__
class Cfg(dict):
    __getattr__ = dict.__getitem__
res = {}
for name, (cfg, inp, terms) in job.items():
    cls = heads[cfg["head"]]
    head = cls.__new__(cls)
    torch.nn.Module.__init__(head)
    loss_cfg = Cfg(LOSS_WEIGHTS=Cfg(point_cls_weight=cfg["cls_weight"], point_part_weight=cfg["part_weight"],
                                    point_box_weight=cfg["box_weight"], code_weights=cfg["code_weights"]))
    if "box" in terms:
        loss_cfg["LOSS_REG"] = "WeightedSmoothL1Loss"
    head.model_cfg = Cfg(LOSS_CONFIG=loss_cfg)
    head.num_class = cfg["num_class"]
    head.build_losses(loss_cfg)                      # the reference's own: the focal loss and the weighted smooth L1
    if "box" in terms:
        assert type(head.reg_loss_func).__name__ == "WeightedSmoothL1Loss"
        head.reg_loss_func.beta = cfg["beta"]
    if cfg["head"] == "PointIntraPartOffsetHead":
        head.box_layers = object() if "box" in terms else None
    t = lambda a: torch.from_numpy(a.copy())
    preds = {k: t(inp[k]).requires_grad_(True) for k in ("cls", "part", "box") if k in inp}
    head.forward_ret_dict = dict(point_cls_preds=preds["cls"], point_cls_labels=t(inp["labels"]))
    if "part" in terms:
        head.forward_ret_dict.update(point_part_preds=preds["part"], point_part_labels=t(inp["part_t"]))
    if "box" in terms:
        head.forward_ret_dict.update(point_box_preds=preds["box"], point_box_labels=t(inp["box_t"]))
    loss, tb = head.get_loss()
    loss.backward()
    out = dict(table=np.array([tb["point_loss_cls"], tb.get("point_loss_part", 0.0), tb.get("point_loss_box", 0.0), loss.item(),
                               tb["point_pos_num"]], dtype=np.float32), keys=list(tb))
    for k, p in preds.items():
        out["grad_" + k] = p.grad.numpy()
    res[name] = out
pickle.dump(res, open(sys.argv[4], "wb"))
"""


def configs(seq):
    c = seq.base_cfg
    box, part, simple = seq.HEADS
    return {
        "pointrcnn": c(head=box, B=2, N=128, num_class=1, code=8, seed=31),
        "pointrcnn3": c(head=box, B=2, N=128, num_class=3, code=8, seed=32, box_weight=2.0),
        "parta2": c(head=part, B=2, N=150, num_class=3, seed=33),
        "parta2_nobox": c(head=part, box_layers=False, B=2, N=150, num_class=3, seed=34, int64=False),
        "pvrcnn": c(head=simple, B=2, N=192, num_class=1, seed=35),
        "nopos": c(head=part, B=2, N=100, num_class=3, samples=["none", "none"], seed=36),
        "edge": c(head=part, B=2, N=130, num_class=3, seed=37, cls_weight=1.5, part_weight=0.75, box_weight=2.0,
                  code_weights=[1.0, 1.0, 1.0, 0.5, 0.5, 0.5, 2.0, 0.2], specials=list(seq.EDGE_RECORDED)),
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
    import point_loss_seq as seq
    assert which in ("scenes", "edges"), which
    cfgs = configs(seq) if which == "scenes" else seq.edge_scene_cfgs()
    job = {n: (cfg, seq.make_inputs(cfg), seq.terms_of(cfg)) for n, cfg in cfgs.items()}
    ref = run_reference(job)
    store = {"scenes": np.array(json.dumps(list(cfgs)))}
    worst = {}
    for name, (cfg, inp, terms) in job.items():
        ours, ex = seq.restate(inp, cfg), seq.exact(inp, cfg)
        rec = {k: ref[name][k] for k in seq.OUTPUTS if k in ref[name]}
        assert set(rec) == set(ours), (name, sorted(rec), sorted(ours))
        for who, got in (("ours", ours), ("reference", rec)):
            why, ratios = seq.bound_report(got, ex, who)
            assert not why, f"{name}\n{why}"
            for k, v in ratios.items():
                worst[(who, k)] = max(worst.get((who, k), 0.0), v)
        why = seq.zero_report(ours, rec)
        assert not why, f"{name}\n{why}"
        assert ours["table"][4] == rec["table"][4] == (inp["labels"] > 0).sum(), name
        want_keys = ["point_loss_cls", "point_pos_num"] + (["point_loss_part"] if "part" in terms else []) + (
            ["point_loss_box"] if "box" in terms else [])
        assert ref[name]["keys"] == want_keys, (name, ref[name]["keys"])
        print(f"{name}: {cfg['head']} {terms}, rows = {cfg['B'] * cfg['N']}, positives = {int(rec['table'][4])}, "
              f"ignored = {int((inp['labels'] < 0).sum())}")
        store[f"{name}/cfg"] = np.array(json.dumps(cfg))
        for k, v in rec.items():
            store[f"{name}/{k}"] = v
    if which == "scenes":
        assert not np.isnan(ref["edge"]["table"]).any() and ref["nopos"]["table"][4] == 0
    path = os.path.join(GOLD, "point_loss.npz" if which == "scenes" else "point_loss_edges.npz")
    np.savez_compressed(path, **store)
    for (who, k), v in sorted(worst.items()):
        print(f"largest error / bound, {who:9s} {k:9s} {v:.3f}")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(*sys.argv[1:2])
