"""Golden optimiser steps for modest_amd.utils.optim_step (BUILD CONTAINER ONLY -- needs /root/reference).

Imports the reference's own ``build_optimizer`` and ``build_scheduler`` (tools/train_utils/optimization) and torch's
``clip_grad_norm_`` from where they lie (nothing copied) and runs the tail of ``train_one_epoch`` on the CPU over small modules
that mix Conv, Linear and BatchNorm, so that both kinds of parameter group exist:

    lr_scheduler.step(it); optimizer.zero_grad(); loss.backward(); clip_grad_norm_(model.parameters(), 10); optimizer.step()

Scenes in tests/golden/optim_step.npz:
  onecycle6   six consecutive OneCycle steps (LR 0.003, MOMS [0.95, 0.85], WEIGHT_DECAY 0.01, GRAD_NORM_CLIP 10): ``side`` gets
              no gradient in step 1, ``frozen.weight`` is frozen after the optimiser was built, the loss scale makes steps 0, 2
              clip and steps 1, 3 not
  nan         two steps, the second with one NaN gradient element; this module has a tensor of more than one chunk
  inf         two steps, the second with one inf gradient element
Per step: lr, mom, wd, max_norm, the raw gradients, torch's total_norm, the clipped gradients, and parameters, exp_avg,
exp_avg_sq and step counts after; the parameters before the first step.  The JSON under ``meta`` names the tensors in the
optimiser's group order and in ``model.parameters()`` order.

It also writes tests/golden/optim_step_shapes.json: names and shapes of the parameter sets the bench and the determinism test
run on, at the Lyft configs -- PointPillars (``PillarVFE`` + ``BaseBEVBackbone``), SECOND (``VoxelBackBone8x`` over this
repository's spconv + ``BaseBEVBackbone``) and PointRCNN (``PointNet2MSG`` over this repository's PointNet++ shim), constructed
from the reference's own classes; the three 1x1 convolutions of ``AnchorHeadSingle`` and the two towers of ``PointHeadBox`` are
added by their shapes.  PointRCNN's RoI head is not in its set.

Usage:  python tools/make_golden_optim_step.py
"""
import json
import os
import sys
import types

import numpy as np
import torch
from torch import nn
from torch.nn.utils import clip_grad_norm_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/downstream/OpenPCDet"
GOLD = os.path.join(ROOT, "tests", "golden", "optim_step.npz")
SHAPES = os.path.join(ROOT, "tests", "golden", "optim_step_shapes.json")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(REF, "tools"))
from train_utils.optimization import build_optimizer, build_scheduler  # noqa: E402

assert sys.modules[build_optimizer.__module__].__file__.startswith(REF)


class Cfg(dict):
    __getattr__ = dict.__getitem__


OPTIM = Cfg(OPTIMIZER="adam_onecycle", LR=0.003, WEIGHT_DECAY=0.01, MOMENTUM=0.9, MOMS=[0.95, 0.85], PCT_START=0.4, DIV_FACTOR=10,
            DECAY_STEP_LIST=[35, 45], LR_DECAY=0.1, LR_CLIP=1e-7, LR_WARMUP=False, WARMUP_EPOCH=1, GRAD_NORM_CLIP=10)


class Net(nn.Module):
    def __init__(self, wide):
        super().__init__()
        self.conv = nn.Conv2d(3, 6, 3, bias=False)
        self.bn = nn.BatchNorm2d(6)
        self.fc = nn.Linear(6, 64 if wide else 5)
        self.bn1 = nn.BatchNorm1d(64 if wide else 5)
        self.side = nn.Linear(6, 64 if wide else 5)
        self.wide = nn.Linear(64, 65) if wide else nn.Identity()
        self.out = nn.Linear(65 if wide else 5, 2)
        self.frozen = nn.Linear(65 if wide else 5, 2)

    def forward(self, x, use_side):
        h = torch.relu(self.bn(self.conv(x))).mean((2, 3))
        y = self.bn1(self.fc(h))
        if use_side:
            y = y + self.side(h)
        y = self.wide(y)
        return self.out(y) + self.frozen(y)


def record(name, wide, scales, no_side=(), poison=None):
    torch.manual_seed({"onecycle6": 1, "nan": 2, "inf": 3}[name])
    model = Net(wide)
    opt = build_optimizer(model, OPTIM)
    sched, _ = build_scheduler(opt, total_iters_each_epoch=10, total_epochs=2, last_epoch=-1, optim_cfg=OPTIM)
    model.frozen.weight.requires_grad = False          # "When some parameters are fixed"
    names = {p: n for n, p in model.named_parameters()}
    groups = opt.opt.param_groups
    params = [dict(name=names[p], shape=list(p.shape), group=gi, bn=bool(gi % 2)) for gi, pg in enumerate(groups) for p in pg["params"]]
    meta = dict(params=params, model_order=[n for n, _ in model.named_parameters()], steps=[], bn_wd=bool(opt.bn_wd),
                true_wd=bool(opt.true_wd))
    arrays = {}
    for pr in params:
        arrays[f"{name}.init.{pr['name']}.p"] = dict(model.named_parameters())[pr["name"]].detach().numpy().copy()
    for k, scale in enumerate(scales):
        sched.step(k)
        model.train()
        opt.zero_grad()
        x = torch.randn(4, 3, 8, 8)
        loss = (model(x, k not in no_side) ** 2).sum() * scale
        loss.backward()
        if poison is not None and k == len(scales) - 1:
            model.fc.weight.grad.view(-1)[3] = poison
        raw = {n: None if p.grad is None else p.grad.detach().numpy().copy() for n, p in model.named_parameters()}
        norm = clip_grad_norm_(model.parameters(), OPTIM.GRAD_NORM_CLIP)
        st = dict(lr=float(opt.lr), mom=float(opt.mom), wd=float(opt.wd), max_norm=float(OPTIM.GRAD_NORM_CLIP),
                  beta2=float(groups[0]["betas"][1]), eps=float(groups[0]["eps"]),
                  frozen=[n for n, p in model.named_parameters() if not p.requires_grad],
                  has_grad=[n for n, p in model.named_parameters() if p.grad is not None])
        assert all(pg["lr"] == st["lr"] and pg["betas"][0] == st["mom"] for pg in groups)
        arrays[f"{name}.{k}.norm"] = norm.detach().numpy().copy()
        for n, p in model.named_parameters():
            if raw[n] is not None:
                arrays[f"{name}.{k}.{n}.g"] = raw[n]
                arrays[f"{name}.{k}.{n}.gc"] = p.grad.detach().numpy().copy()
        opt.step()
        st["t"] = {}
        for n, p in model.named_parameters():
            arrays[f"{name}.{k}.{n}.p"] = p.detach().numpy().copy()
            s = opt.opt.state.get(p)
            if s:
                assert s["step"].dtype == torch.float32 and s["step"].ndim == 0 and s["step"].device.type == "cpu"
                st["t"][n] = float(s["step"])
                arrays[f"{name}.{k}.{n}.m"] = s["exp_avg"].numpy().copy()
                arrays[f"{name}.{k}.{n}.v"] = s["exp_avg_sq"].numpy().copy()
        meta["steps"].append(st)
        print(f"{name} step {k}: lr {st['lr']:.6g} mom {st['mom']:.6g} total_norm {float(norm):.6g}"
              f" ({'clips' if float(norm) > OPTIM.GRAD_NORM_CLIP else 'does not clip'}), without gradient: "
              f"{[n for n in meta['model_order'] if n not in st['has_grad']]}")
    return meta, arrays


def rows_of(prefix, mod):
    norm = (nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d)
    owner = {id(p): isinstance(m, norm) for m in mod.modules() for p in m.parameters(recurse=False)}
    return [dict(name=f"{prefix}.{n}", shape=list(p.shape), bn=owner[id(p)]) for n, p in mod.named_parameters()]


def head_convs(channels, anchors=2):
    """AnchorHeadSingle's three 1x1 convolutions by their shapes: 1 class, `anchors` per location, 7 box values, 2 direction bins"""
    rows = []
    for n, c in (("conv_cls", anchors), ("conv_box", 7 * anchors), ("conv_dir_cls", 2 * anchors)):
        rows += [dict(name=f"dense_head.{n}.weight", shape=[c, channels, 1, 1], bn=False), dict(name=f"dense_head.{n}.bias", shape=[c], bn=False)]
    return rows


def fc_rows(prefix, c_in, fcs, c_out):
    """make_fc_layers of the point heads by its shapes: Linear without bias + BatchNorm1d per entry, then a Linear with bias"""
    rows = []
    for k, c in enumerate(fcs):
        rows += [dict(name=f"{prefix}.{3 * k}.weight", shape=[c, c_in], bn=False),
                 dict(name=f"{prefix}.{3 * k + 1}.weight", shape=[c], bn=True), dict(name=f"{prefix}.{3 * k + 1}.bias", shape=[c], bn=True)]
        c_in = c
    return rows + [dict(name=f"{prefix}.{3 * len(fcs)}.weight", shape=[c_out, c_in], bn=False),
                   dict(name=f"{prefix}.{3 * len(fcs)}.bias", shape=[c_out], bn=False)]


def shape_sets():
    """PointPillars, SECOND and PointRCNN at the Lyft configs: the backbones constructed from the reference's own classes with this
    repository's shims (spconv := modest_amd.utils.spconv, the PointNet++ extension := ours), the heads' layers by their shapes.
    PointRCNN's RoI head (PointRCNNHead) is not in its set: it was not constructed here."""
    from modest_amd.utils import pcdet_bind
    pcdet_bind.install(sparse_conv=True)
    for name in ("pcdet", "pcdet.utils", "pcdet.ops", "pcdet.ops.pointnet2", "pcdet.ops.pointnet2.pointnet2_batch",
                 "pcdet.ops.pointnet2.pointnet2_stack", "pcdet.models", "pcdet.models.backbones_3d", "pcdet.models.backbones_3d.vfe",
                 "pcdet.models.backbones_3d.pfe", "pcdet.models.backbones_2d"):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__path__ = [os.path.join(REF, *name.split("."))]
            sys.modules[name] = m
    from pcdet.models.backbones_3d.vfe.pillar_vfe import PillarVFE
    from pcdet.models.backbones_2d.base_bev_backbone import BaseBEVBackbone
    from pcdet.models.backbones_3d.spconv_backbone import VoxelBackBone8x
    from pcdet.models.backbones_3d.pointnet2_backbone import PointNet2MSG
    for c in (PillarVFE, BaseBEVBackbone, VoxelBackBone8x, PointNet2MSG):
        assert sys.modules[c.__module__].__file__.startswith(REF)
    vfe = PillarVFE(Cfg(USE_NORM=True, WITH_DISTANCE=False, USE_ABSLOTE_XYZ=True, NUM_FILTERS=[64]), num_point_features=4,
                    voxel_size=[0.16, 0.16, 4], point_cloud_range=[0, -39.68, -3, 89.6, 39.68, 1])
    bev = BaseBEVBackbone(Cfg(LAYER_NUMS=[3, 5, 5], LAYER_STRIDES=[2, 2, 2], NUM_FILTERS=[64, 128, 256], UPSAMPLE_STRIDES=[1, 2, 4],
                              NUM_UPSAMPLE_FILTERS=[128, 128, 128]), input_channels=64)
    sets = {"pointpillars_lyft": rows_of("vfe", vfe) + rows_of("backbone_2d", bev) + head_convs(384)}
    # SECOND: MeanVFE and HeightCompression have no parameters; grid (90.4, 80, 4) / (0.05, 0.05, 0.1)
    voxel = VoxelBackBone8x(Cfg(), input_channels=4, grid_size=np.array([1808, 1600, 40]))
    bev2 = BaseBEVBackbone(Cfg(LAYER_NUMS=[5, 5], LAYER_STRIDES=[1, 2], NUM_FILTERS=[128, 256], UPSAMPLE_STRIDES=[1, 2],
                               NUM_UPSAMPLE_FILTERS=[256, 256]), input_channels=256)
    sets["second_lyft"] = rows_of("backbone_3d", voxel) + rows_of("backbone_2d", bev2) + head_convs(512)
    msg = PointNet2MSG(Cfg(SA_CONFIG=Cfg(NPOINTS=[4096, 1024, 256, 64], RADIUS=[[0.1, 0.5], [0.5, 1.0], [1.0, 2.0], [2.0, 4.0]],
                                         NSAMPLE=[[16, 32]] * 4,
                                         MLPS=[[[16, 16, 32], [32, 32, 64]], [[64, 64, 128], [64, 96, 128]],
                                               [[128, 196, 256], [128, 196, 256]], [[256, 256, 512], [256, 384, 512]]]),
                           FP_MLPS=[[128, 128], [256, 256], [512, 512], [512, 512]]), input_channels=4)
    sets["pointrcnn_lyft"] = (rows_of("backbone_3d", msg) + fc_rows("point_head.cls_layers", 128, [256, 256], 1)
                              + fc_rows("point_head.box_layers", 128, [256, 256], 8))
    return sets


def main():
    metas, arrays = {}, {}
    for name, kw in (("onecycle6", dict(wide=False, scales=[50, 0.01, 50, 0.01, 1, 1], no_side=(1,))),
                     ("nan", dict(wide=True, scales=[1, 1], poison=float("nan"))),
                     ("inf", dict(wide=False, scales=[1, 1], poison=float("inf")))):
        metas[name], a = record(name, **kw)
        arrays.update(a)
    norms = [float(arrays[f"onecycle6.{k}.norm"]) for k in range(6)]
    assert any(n > 10 for n in norms) and any(n < 10 for n in norms), norms
    np.savez_compressed(GOLD, meta=np.array(json.dumps(metas)), **arrays)
    sets = shape_sets()
    with open(SHAPES, "w") as f:
        json.dump(sets, f, indent=0)
    for k, rows in sets.items():
        print(k, len(rows), "tensors,", sum(int(np.prod(r["shape"])) for r in rows), "elements")
    print(GOLD, os.path.getsize(GOLD), "bytes;", SHAPES, os.path.getsize(SHAPES), "bytes")


if __name__ == "__main__":
    main()
