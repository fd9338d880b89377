"""Golden PillarVFE / PointPillarScatter results for modest_amd.utils.pillar_vfe (BUILD CONTAINER ONLY -- needs /root/reference).

Runs the reference's own ``PillarVFE`` (pcdet/models/backbones_3d/vfe/pillar_vfe.py) and ``PointPillarScatter``
(pcdet/models/backbones_2d/map_to_bev/pointpillar_scatter.py), imported from where they lie (nothing copied), on the CPU in a
child process that binds empty package modules which keep their ``__path__`` (so no ``__init__.py`` of pcdet is executed).

Recorded in tests/golden/pillar_vfe.npz per scene: the settings as JSON (plain values), the inputs, ``pillar_features``, the
canvas, the running buffers after the last step, and -- in training mode, for the recorded upstream gradient of the canvas
(``pillar_vfe_seq.grad_canvas_of``: the recorded (P, C) gradient in the pillars' cells) -- autograd's dW, dgamma, dbeta and the
gradient of ``pillar_features``.
  abs_c64     P = 12, S = 32, 4 point features, C = 64, USE_ABSLOTE_XYZ, training
  rel_c32     P =  9, S = 20, 5 point features, C = 32, without USE_ABSLOTE_XYZ, training
  dist_c64    P =  7, S = 32, WITH_DISTANCE, training
  eval_c32    P = 10, S = 20, C = 32, eval mode with used running buffers
  two_steps   P =  5, S = 32, C = 64, two training steps in a row: the running buffers after the second
  eval_dist   P =  8, S = 32, 5 point features, without USE_ABSLOTE_XYZ, WITH_DISTANCE, eval mode
The tool asserts, per scene, what tests/test_pillar_vfe_cpu.py asserts again: the restatement (tests/pillar_vfe_seq.py) and the
recording each lie within the derived bound of the exact value in every element, the canvas and the features' gradient equal
the recording bit for bit, the NaN / inf patterns are equal, and every deliberately wrong variant of the restatement leaves the
bound on some scene.  It prints the largest error over bound of either, and the fixture's size.

Usage:  python tools/make_golden_pillar_vfe.py
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
GOLD = os.path.join(ROOT, "tests", "golden", "pillar_vfe.npz")

_CHILD = r"""
import os, pickle, sys, types
import numpy as np
import torch
ref, job = sys.argv[1], pickle.load(open(sys.argv[2], "rb"))
for name in ("pcdet", "pcdet.models", "pcdet.models.backbones_3d", "pcdet.models.backbones_3d.vfe", "pcdet.models.backbones_2d",
             "pcdet.models.backbones_2d.map_to_bev"):
    m = types.ModuleType(name)
    m.__path__ = [os.path.join(ref, *name.split("."))]
    sys.modules[name] = m
from pcdet.models.backbones_3d.vfe.pillar_vfe import PillarVFE
from pcdet.models.backbones_2d.map_to_bev.pointpillar_scatter import PointPillarScatter
for c in (PillarVFE, PointPillarScatter):
    assert sys.modules[c.__module__].__file__.startswith(ref)
class Cfg(dict):
    __getattr__ = dict.__getitem__
t = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy())
res = {}
for name, (case, G) in job.items():
    P, S, Cp = case["voxels"].shape
    C, K = case["W"].shape
    vfe = PillarVFE(Cfg(USE_NORM=True, WITH_DISTANCE=bool(case["parts"] & 8), USE_ABSLOTE_XYZ=bool(case["parts"] & 1), NUM_FILTERS=[C]),
                    num_point_features=Cp, voxel_size=list(case["voxel_size"]), point_cloud_range=list(case["range_lo"]) + [0, 0, 0])
    assert (vfe.x_offset, vfe.y_offset, vfe.z_offset) == tuple(case["offsets"])
    pfn = vfe.pfn_layers[0]
    assert len(vfe.pfn_layers) == 1 and tuple(pfn.linear.weight.shape) == (C, K)
    assert pfn.norm.eps == case["eps"] and pfn.norm.momentum == case["momentum"]
    with torch.no_grad():
        pfn.linear.weight.copy_(t(case["W"])); pfn.norm.weight.copy_(t(case["gamma"])); pfn.norm.bias.copy_(t(case["beta"]))
        pfn.norm.running_mean.copy_(t(case["running_mean"])); pfn.norm.running_var.copy_(t(case["running_var"]))
    sc = PointPillarScatter(Cfg(NUM_BEV_FEATURES=C), grid_size=(case["nx"], case["ny"], 1))
    vfe.train(case["training"])
    for step in range(case["steps"]):
        bd = vfe(dict(voxels=t(case["voxels"]), voxel_num_points=t(case["num"]), voxel_coords=t(case["coords"])))
    feats = bd["pillar_features"]
    assert tuple(feats.shape) == (P, C)
    rec = {}
    if case["training"]:
        feats.retain_grad()
    canvas = sc(bd)["spatial_features"]
    assert tuple(canvas.shape) == (case["batch_size"], C, case["ny"], case["nx"])
    if case["training"]:
        (canvas * t(G)).sum().backward()
        rec.update(dW=pfn.linear.weight.grad, dgamma=pfn.norm.weight.grad, dbeta=pfn.norm.bias.grad, grad_feat=feats.grad)
    rec.update(pillar_features=feats, canvas=canvas, running_mean=pfn.norm.running_mean, running_var=pfn.norm.running_var,
               tracked=pfn.norm.num_batches_tracked)
    res[name] = {k: v.detach().numpy().copy() for k, v in rec.items()}
pickle.dump(res, open(sys.argv[3], "wb"))
"""


def build_scenes():
    import pillar_vfe_seq as seq
    out = {"abs_c64": seq.make_case(11, P=12, S=32, Cp=4, C=64),
           "rel_c32": seq.make_case(12, P=9, S=20, Cp=5, C=32, use_abs=False),
           "dist_c64": seq.make_case(13, P=7, S=32, Cp=4, C=64, with_dist=True),
           "eval_c32": seq.make_case(14, P=10, S=20, Cp=4, C=32, training=False),
           "two_steps": seq.make_case(15, P=5, S=32, Cp=4, C=64, steps=2),
           "eval_dist": seq.make_case(16, P=8, S=32, Cp=5, C=64, use_abs=False, with_dist=True, training=False)}
    for name, case in out.items():
        assert case["coords"][:, 0].max() == case["batch_size"] - 1, name      # the reference takes the batch size from the coords
        case["range_lo"] = tuple(case["offsets"][i] - case["voxel_size"][i] / 2 for i in range(3))
        assert tuple(case["voxel_size"][i] / 2 + case["range_lo"][i] for i in range(3)) == tuple(case["offsets"]), name
    return out


def check_scene(seq, name, case, rec, worst):
    """what the CPU test asserts -> {quantity: whether each wrong variant left the bound}"""
    grad = case["grad"] if case["training"] else None
    ex = seq.exact(case, grad)
    assert not ex["margin"], (name, ex["margin"])
    ours = seq.restate_steps(case)
    got = {"out": ours["out"]}
    theirs = {"out": rec["pillar_features"]}
    if case["training"]:
        dW, dg, db = seq.restate_backward(case, ours, case["grad"])
        got.update(running_mean=ours["running_mean"], running_var=ours["running_var"], dW=dW, dgamma=dg, dbeta=db)
        theirs.update({k: rec[k] for k in ("running_mean", "running_var", "dW", "dgamma", "dbeta")})
        assert int(rec["tracked"]) == ours["tracked"] == case["steps"], name
    else:
        assert seq.same_bits(rec["running_mean"], case["running_mean"]) and seq.same_bits(rec["running_var"], case["running_var"])
    for who, res in (("ours", got), ("the reference", theirs)):
        for k, a in res.items():
            why, ratio = seq.bound_report(a, ex[k][0], ex[k][1], f"{name}: {who}: {k}")
            assert not why, why
            worst[who] = max(worst[who], ratio)
    for k in got:
        why = seq.pattern_report(got[k], theirs[k], f"{name}: {k}")
        assert not why, why
    G = seq.grad_canvas_of(case)
    why = seq.report(seq.scatter(rec["pillar_features"], case["coords"], case["batch_size"], case["ny"], case["nx"]), rec["canvas"], f"{name}: canvas")
    assert not why, why
    if case["training"]:
        why = seq.report(seq.scatter_backward(G, case["coords"]), rec["grad_feat"], f"{name}: grad_feat")
        assert not why, why
        assert seq.same_bits(rec["grad_feat"], case["grad"]), name
    caught = {}
    for wrong in seq.WRONG:
        bad = seq.restate_steps(case, wrong)
        res = {"out": bad["out"]}
        if case["training"]:
            res.update(running_mean=bad["running_mean"], running_var=bad["running_var"])
        caught[wrong] = any(seq.bound_report(a, ex[k][0], ex[k][1])[0] for k, a in res.items())
    return caught


def main():
    import pillar_vfe_seq as seq
    job = build_scenes()
    with tempfile.TemporaryDirectory() as work:
        pickle.dump({n: (c, seq.grad_canvas_of(c)) for n, c in job.items()}, open(os.path.join(work, "job.pkl"), "wb"))
        open(os.path.join(work, "child.py"), "w").write(_CHILD)
        subprocess.run([sys.executable, os.path.join(work, "child.py"), REF, os.path.join(work, "job.pkl"),
                        os.path.join(work, "res.pkl")], check=True)
        res = pickle.load(open(os.path.join(work, "res.pkl"), "rb"))
    rec = {"scenes": np.array(json.dumps(list(job)))}
    worst = {"ours": 0.0, "the reference": 0.0}
    caught = {w: [] for w in seq.WRONG}
    for name, case in job.items():
        for w, hit in check_scene(seq, name, case, res[name], worst).items():
            if hit:
                caught[w].append(name)
        rec.update(seq.pack(name, case, res[name]))
        print(f"{name}: voxels {case['voxels'].shape}, C = {case['W'].shape[0]}, K = {case['W'].shape[1]}")
    print("largest error / bound:", worst)
    for w, names in caught.items():
        print(f"wrong variant {w}: leaves the bound on {names}")
        assert names, w
    np.savez_compressed(GOLD, **rec)
    back = seq.scenes(dict(np.load(GOLD)))
    assert [n for n, _, _ in back] == list(job)
    size = os.path.getsize(GOLD)
    assert size <= 100 * 1024, size
    print(GOLD, size, "bytes")


if __name__ == "__main__":
    main()
