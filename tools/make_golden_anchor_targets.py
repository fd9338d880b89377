"""Golden anchor targets for modest_amd.utils.target_assigner (BUILD CONTAINER ONLY -- needs /root/reference).

Runs the reference's own ``AxisAlignedTargetAssigner``, ``AnchorGenerator`` and ``ResidualCoder`` (imported from where
they lie, nothing copied) on the CPU in a child process.  The child binds empty package modules that keep their
``__path__`` (so ``pcdet/models/__init__.py``, which needs torchvision, is never executed), this project's shims for the
two extension modules ``box_utils`` and ``iou3d_nms_utils`` pull in (``pcdet_bind.install``), and makes ``Tensor.cuda``
the identity.

Recorded in tests/golden/anchor_targets.npz per scene: the config as JSON (plain values), the gt tensor and the three
outputs.  Six scenes: small, big, multi, lyft, and two crowded ones past the kernels' constants (crowd: classes of 2, 6
and 4 anchors per location, 275 gts of one class with a tie and two forcings across position 256; crowd_multi: multihead
classes on grids of their own, 280 gts of one class), built with the helpers of tests/anchor_targets_cases.py.  Anchors are regenerated from the config by tests/anchor_targets_seq.py:make_anchors; this tool asserts the
regenerated anchors equal the reference generator's bit for bit.  It also asserts
  * that the numpy restatement reproduces every recorded output (the sincos columns to the derived bound),
  * that torch's CPU log of every size quotient that reaches an output equals the rounded double log (sizes are redrawn
    by single float steps until it does; a crafted footprint that fails stops the tool),
  * every case of anchor_targets_seq.fixture_cases, and the fixture's size.

Usage:  python tools/make_golden_anchor_targets.py        (writes tests/golden/anchor_targets.npz)
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
F = np.float32

_CHILD = r"""
import os, pickle, sys, types
import numpy as np
import torch
ref, root, job = sys.argv[1], sys.argv[2], pickle.load(open(sys.argv[3], "rb"))
sys.path.insert(0, root)
for name in ("pcdet", "pcdet.models", "pcdet.models.dense_heads", "pcdet.models.dense_heads.target_assigner", "pcdet.utils",
             "pcdet.ops", "pcdet.ops.iou3d_nms", "pcdet.ops.roiaware_pool3d"):
    m = types.ModuleType(name)
    m.__path__ = [os.path.join(ref, *name.split("."))]
    sys.modules[name] = m
from modest_amd.utils import pcdet_bind
pcdet_bind.install(stand_ins=False)
torch.Tensor.cuda = lambda self, *a, **k: self
from pcdet.models.dense_heads.target_assigner.axis_aligned_target_assigner import AxisAlignedTargetAssigner
from pcdet.models.dense_heads.target_assigner.anchor_generator import AnchorGenerator
from pcdet.utils.box_coder_utils import ResidualCoder
assert AxisAlignedTargetAssigner.__module__.startswith("pcdet.") and "pcdet.models.backbones_3d" not in sys.modules
class Cfg(dict):
    __getattr__ = dict.__getitem__
res = {}
for name, (cfg, gt) in job.items():
    gen_cfg = [Cfg(class_name=c["class_name"], anchor_sizes=c["anchor_sizes"], anchor_rotations=c["anchor_rotations"],
                   anchor_bottom_heights=c["anchor_bottom_heights"], align_center=c["align_center"],
                   matched_threshold=c["matched_threshold"], unmatched_threshold=c["unmatched_threshold"]) for c in cfg["classes"]]
    model_cfg = Cfg(ANCHOR_GENERATOR_CONFIG=gen_cfg, USE_MULTIHEAD=cfg["use_multihead"],
                    TARGET_ASSIGNER_CONFIG=Cfg(NAME="AxisAlignedTargetAssigner", POS_FRACTION=-1.0, SAMPLE_SIZE=512,
                                               NORM_BY_NUM_EXAMPLES=False, MATCH_HEIGHT=False))
    coder = ResidualCoder(code_size=cfg["code_size"], encode_angle_by_sincos=cfg["sincos"])
    anchors, _ = AnchorGenerator(anchor_range=cfg["anchor_range"], anchor_generator_config=gen_cfg).generate_anchors(
        [c["grid_size"] for c in cfg["classes"]])
    if coder.code_size != 7:   # what AnchorHeadTemplate.generate_anchors does with anchor_ndim = box_coder.code_size
        anchors = [torch.cat((a, a.new_zeros([*a.shape[0:-1], coder.code_size - 7])), dim=-1) for a in anchors]
    assigner = AxisAlignedTargetAssigner(model_cfg=model_cfg, class_names=cfg["class_names"], box_coder=coder, match_height=False)
    out = assigner.assign_targets(anchors, torch.from_numpy(gt.copy()))
    res[name] = dict(anchors=[a.numpy() for a in anchors], labels=out["box_cls_labels"].numpy(),
                     targets=out["box_reg_targets"].numpy(), weights=out["reg_weights"].numpy())
pickle.dump(res, open(sys.argv[4], "wb"))
"""


def cls_cfg(name, size, z, m, u, grid):
    return dict(class_name=name, anchor_sizes=[size], anchor_rotations=[0, 1.57], anchor_bottom_heights=[z], align_center=False,
                matched_threshold=m, unmatched_threshold=u, grid_size=list(grid))


def configs():
    small = dict(anchor_range=[0, -8, -3, 24, 8, 1], use_multihead=False, code_size=7, sincos=False,
                 class_names=["Car", "Pedestrian", "Cyclist", "Truck"],
                 classes=[cls_cfg("Car", [2.0, 1.0, 1.5], -1.0, 0.5, 0.25, (7, 5)),
                          cls_cfg("Pedestrian", [0.75, 0.5, 1.75], -0.6, 0.5, 0.35, (7, 5)),
                          cls_cfg("Cyclist", [1.75, 0.5, 1.75], -0.6, 0.45, 0.3, (7, 5))])
    big = dict(anchor_range=[0, -39.68, -3, 69.12, 39.68, 1], use_multihead=False, code_size=7, sincos=False,
               class_names=["Car", "Pedestrian", "Cyclist"],
               classes=[cls_cfg("Car", [3.9, 1.6, 1.56], -1.78, 0.6, 0.45, (40, 33)),
                        cls_cfg("Pedestrian", [0.8, 0.6, 1.73], -0.6, 0.5, 0.35, (40, 33)),
                        cls_cfg("Cyclist", [1.76, 0.6, 1.73], -0.6, 0.5, 0.35, (40, 33))])
    multi = dict(small, use_multihead=True, code_size=9, sincos=True, class_names=["Car", "Pedestrian", "Cyclist"])
    lyft = dict(anchor_range=[-40, -33, -3, 40, 33, 1], use_multihead=False, code_size=7, sincos=False, class_names=["Car"],
                classes=[cls_cfg("Car", [4.7, 2.1, 1.7], -1.0, 0.6, 0.45, (40, 33))])
    return dict(small=small, big=big, multi=multi, lyft=lyft)


def box(x, y, z, dx, dy, dz, r, cid, extra=()):
    return [x, y, z, dx, dy, dz, r, *extra, cid]


def search_iou(seq, anchors, centre, target, rs):
    """a gt a x b concentric with the two anchors at `centre` (2 x 1 and, rotated, 1 x 2) whose IoU with the rotated anchor
    has exactly the bits of `target` while the other anchor holds the gt's column maximum: with a >= 1 and b <= 2
    the two IoUs are i / (2 + a b - i), i = min(a, 2) min(b, 1), and b / (2 + a b - b), so b = 2 t / (1 + t - t a) aims at t and
    a walk over neighbouring floats of b finds the bits"""
    target = F(target)
    ra = seq.nearest_bev(anchors)
    here = np.flatnonzero((anchors[:, 0] == centre[0]) & (anchors[:, 1] == centre[1]))
    i = int(here[seq.rot_of(anchors[here, 6]) >= seq.QUARTER][0])
    for _ in range(400):
        a = F(rs.uniform(1.5, 3.0))
        t = np.float64(target)
        b = F(2 * t / (1 + t - t * np.float64(a)))
        steps = np.arange(-4000, 4001).astype(np.int32)
        cand = np.zeros((len(steps), 7), dtype=F)
        cand[:, 0], cand[:, 1], cand[:, 3] = centre[0], centre[1], a
        cand[:, 4] = (np.full(len(steps), b, dtype=F).view(np.int32) + steps).view(F)
        ci = seq.iou_matrix(ra, seq.nearest_bev(cand))
        ok = (ci[i] == target) & (ci[i] < ci.max(axis=0))
        if ok.any():
            return cand[int(np.flatnonzero(ok)[0]), [0, 1, 3, 4]]
    raise RuntimeError(f"no gt found for IoU {target!r}")


def build_scenes(seq):
    cfgs = configs()
    rs = np.random.RandomState(20261018)
    out = {}
    # ---- small: three classes, 70 anchors each, B = 3, M = 14.  x = 0, 4, .., 24; y = -8, -4, .., 8 -------------------
    cfg = cfgs["small"]
    car = seq.flatten(seq.make_anchors(cfg)[0], False)
    m, u = F(0.5), F(0.25)
    M = 14
    s0 = [
        box(8, 4, -0.2, 4, 1, 1.5, 0, 1),                       # concentric aligned 4 x 1 over a 2 x 1 anchor: IoU 0.5
        box(16, 4, -0.3, 2, 2, 1.4, 0, 1),                      # both rotations tie at 0.5
        box(100, 100, 0, 3, 1.5, 1.5, 0.3, 1),                  # outside the anchors: column max 0
        box(9.5, -3.25, -0.2, 1.5, 1, 1.5, 0, 1),               # j: best anchor (8, -4), IoU small
        box(10.25, -4, -0.1, 4, 1, 1.6, 0, 1),                  # k: (8, -4) overlaps it more, its best is (12, -4)
        [0] * 8,                                                # a zero row in the middle
        box(20, -4, -0.25, 2.25, 1.25, 1.5, 0, 1),              # same footprint ...
        box(20, -4, 0.5, 2.25, 1.25, 1.5, 0, 1),                # ... another z: the lower index wins
        box(4, 4, -0.3, 3.0, 1.5, 1.5, 0.1, 4),                 # Truck: a class without anchors
        box(4, 0, -0.3, 3.0, 1.5, 1.5, 0.1, 0),                 # id 0 names Truck here
        box(20, 4, -0.5, 0.75, 0.5, 1e-6, 0, 2),                # dz below 1e-5 (Pedestrian, concentric)
        box(12, 8, -0.5, 1.75, 0.5, 1.75, 7.0, 3),              # heading beyond 2 pi (Cyclist)
        box(4, -8, -0.5, 1.75, 0.5, 1.75, -7.5, 3),             # ... and beyond -2 pi
    ]
    s0 += [[0] * 8] * (M - len(s0))
    quarter = seq.QUARTER
    s1 = [box(4, 4, -0.3, 2.5, 1.0, 1.5, np.nextafter(quarter, F(0)), 1),
          box(12, 4, -0.3, 2.5, 1.0, 1.5, quarter, 1),
          box(20, 4, -0.3, 2.5, 1.0, 1.5, np.nextafter(quarter, F(1)), 1)]
    for centre, t in (((4, -4), m), ((12, -4), np.nextafter(m, F(0))), ((20, -4), np.nextafter(m, F(1)))):
        x, y, dx, dy = search_iou(seq, car, centre, t, rs)
        s1.append(box(x, y, -0.3, dx, dy, 1.5, 0, 1))
    s1 += [[0] * 8] * (M - 2 - len(s1)) + [box(1, -1, 0, 0, 0, 0, 0, 0)] + [[0] * 8]   # a trailing row summing to 0
    s2 = []
    for centre, t in (((4, 0), u), ((12, 0), np.nextafter(u, F(0))), ((20, 0), np.nextafter(u, F(1)))):
        x, y, dx, dy = search_iou(seq, car, centre, t, rs)
        s2.append(box(x, y, -0.3, dx, dy, 1.5, 0, 1))
    s2 += [box(12, 4, -0.6, 0.9, 0.6, 1.8, 0.4, 2), box(20, 4.2, -0.6, 1.9, 0.6, 1.7, -0.2, 3)]
    s2 += [[0] * 8] * (M - len(s2))
    out["small"] = (cfg, np.array([s0, s1, s2], dtype=F), {(0, 0), (0, 1), (0, 3), (0, 4), (0, 6), (0, 7), (0, 10), (1, 0), (1, 1), (1, 2),
                                                          (1, 3), (1, 4), (1, 5), (2, 0), (2, 1), (2, 2)})
    # ---- big: the same kind of head at 33 x 40, 2 640 anchors per class, B = 2 -----------------------------------------
    cfg = cfgs["big"]
    M = 12
    g = np.zeros((2, M, 8), dtype=F)
    sizes = {1: (3.9, 1.6, 1.56), 2: (0.8, 0.6, 1.73), 3: (1.76, 0.6, 1.73)}
    for b, n in enumerate((9, 5)):
        for j in range(n):
            cid = 1 + (j % 3)
            sz = np.array(sizes[cid]) * rs.uniform(0.8, 1.25, 3)
            g[b, j] = [rs.uniform(2, 67), rs.uniform(-38, 38), rs.uniform(-1.5, -0.5), *sz, rs.uniform(-3.5, 3.5) + (7 if j == 0 else 0), cid]
    out["big"] = (cfg, g, set())
    # ---- multi: the small head as USE_MULTIHEAD, code_size 9 + sincos, gt with two velocity columns, B = 1 -------------
    cfg = cfgs["multi"]
    rows = [box(8, 4, -0.2, 4, 1, 1.5, 0.2, 1, (0.5, -0.25)), box(16, 4, -0.3, 2, 2, 1.4, -2.0, 1, (1.5, 2.0)),
            box(12, 0, -0.5, 0.9, 0.6, 1.8, 0.4, 2, (0.1, 0.2)), box(20, 0.2, -0.6, 1.9, 0.6, 1.7, 1.3, 3, (-3.0, 0.0)),
            box(4, -4, -0.6, 1.7, 0.55, 1.7, 0.05, 0, (0.25, 0.75)),       # id 0: the last class, Cyclist
            [0] * 10, [0] * 10]
    out["multi"] = (cfg, np.array([rows], dtype=F), {(0, 0), (0, 1)})
    # ---- lyft: one class, B = 2, the second sample without a gt -------------------------------------------------------
    cfg = cfgs["lyft"]
    M = 10
    g = np.zeros((2, M, 8), dtype=F)
    for j in range(7):
        sz = np.array((4.7, 2.1, 1.7)) * rs.uniform(0.7, 1.3, 3)
        g[0, j] = [rs.uniform(-38, 38), rs.uniform(-31, 31), rs.uniform(-1.2, 0.2), *sz, rs.uniform(-3.2, 3.2), 1 if j else 0]
    out["lyft"] = (cfg, g, set())
    out["crowd"] = crowd_scene(seq, rs)
    out["crowd_multi"] = crowd_multi_scene(seq, rs)
    return out


def crowd_scene(seq, rs):
    """the single head of tests/anchor_targets_cases.py with 2, 6 and 4 anchors per location on two heights, B = 2, M = 300:
    275 Cyclists in sample 0 (none in sample 1), among them, by position in the class, one footprint at 250 and 260 (the
    lower index wins across the tile boundary at 256), a gt at 270 that forces an anchor whose argmax is the gt at 30,
    and the mirror image (40 forces, 265 is the argmax)"""
    import anchor_targets_cases as cases
    cfg = cases.single_cfg()
    flats = [seq.flatten(a, False) for a in seq.make_anchors(cfg)]
    geo = dict(sx=4.0, sy=4.0, x0=0.0, y0=-14.0, a=(1.76, 0.6), cid=3)
    j1, k1 = cases.forcer(2, 2, k_at=1.25, k_len=1.7, **geo)
    j2, k2 = cases.forcer(6, 5, k_at=1.25, k_len=1.7, **geo)
    special = {250: cases.twin(4, 6, -0.25, **geo), 260: cases.twin(4, 6, 0.5, **geo), 30: k1, 270: j1, 40: j2, 265: k2}
    taken = {(4, 6), (2, 2), (3, 2), (6, 5), (7, 5)}
    xy = {(geo["x0"] + 4.0 * ix, geo["y0"] + 4.0 * iy) for ix, iy in taken}
    free = [f[[(float(a[0]), float(a[1])) not in xy for a in f]] for f in flats]
    assert all(len(f) < len(g) for f, g in zip(free, flats))
    M = 300
    g = np.zeros((2, M, 8), dtype=F)
    kinds = [3] * 275 + [1] * 9 + [2] * 12 + [9] * 4
    kinds = [kinds[i] for i in rs.permutation(M)]
    crafted, p = set(), 0
    for j, kind in enumerate(kinds):
        if kind == 9:
            continue
        if kind == 3:
            if p in special:
                g[0, j] = special[p]
                crafted.add((0, j))
            else:
                g[0, j] = cases.near(rs, free[2], 3, 8, far=rs.randint(3) == 0)
            p += 1
        else:
            g[0, j] = cases.near(rs, free[kind - 1], kind, 8)
    for j in range(80):
        c = 2 if j % 4 == 0 else 1
        g[1, j] = cases.near(rs, flats[c - 1], c, 8)
    return cfg, g, crafted


def crowd_multi_scene(seq, rs):
    """the multihead of tests/anchor_targets_cases.py on grids of their own (70, 35, 1 248 and 1 000 rows), 9 columns +
    sincos, B = 2, M = 300: 280 Cyclists in sample 0, none in sample 1"""
    import anchor_targets_cases as cases
    cfg = cases.multi_cfg()
    flats = [seq.flatten(a, True) for a in seq.make_anchors(cfg)]
    M = 300
    g = np.zeros((2, M, 10), dtype=F)
    kinds = [3] * 280 + [1] * 4 + [2] * 4 + [4] * 8
    for j, i in enumerate(rs.permutation(len(kinds))):
        g[0, j] = cases.near(rs, flats[kinds[i] - 1], kinds[i], 10, far=kinds[i] == 3 and rs.randint(5) == 0)
    for j, c in enumerate([1, 2, 4, 4, 1, 2, 4]):
        g[1, j] = cases.near(rs, flats[c - 1], c, 10)
    return cfg, g, set()


def settle_logs(seq, cfg, gt, crafted):
    """nudge gt sizes by single float steps until torch's CPU log of every quotient against the class's anchor sizes equals
    the rounded double log; a crafted footprint (dx, dy of a row in `crafted`) is not touched"""
    import torch
    names = cfg["class_names"]
    nudged = 0
    for b in range(gt.shape[0]):
        for j in range(gt.shape[1]):
            row = gt[b, j]
            if not row[:7].any():
                continue
            k = int(row[-1]) - 1
            k += len(names) if k < 0 else 0
            cl = [c for c in cfg["classes"] if 0 <= k < len(names) and c["class_name"] == names[k]]
            sizes = [size for c in cl for size in c["anchor_sizes"]]
            for d in range(3):      # one value must do for every anchor size of the class
                for _ in range(64):
                    q = np.array([max(row[3 + d], seq.TINY) / max(F(size[d]), seq.TINY) for size in sizes], dtype=F)
                    if np.array_equal(torch.log(torch.from_numpy(q)).numpy(), seq.f32_of_double(np.log, q)):
                        break
                    if d < 2 and (b, j) in crafted:
                        raise RuntimeError(f"crafted gt {b, j}: torch's log of {q!r} is not the rounded double log")
                    row[3 + d] = np.nextafter(row[3 + d], F(np.inf))
                    nudged += 1
                else:
                    raise RuntimeError("no size found")
    return nudged


def main():
    import anchor_targets_seq as seq
    built = build_scenes(seq)
    job = {}
    for name, (cfg, gt, crafted) in built.items():
        print(name, "sizes nudged:", settle_logs(seq, cfg, gt, crafted))
        job[name] = (cfg, gt)
    with tempfile.TemporaryDirectory() as work:
        pickle.dump(job, open(os.path.join(work, "job.pkl"), "wb"))
        open(os.path.join(work, "child.py"), "w").write(_CHILD)
        subprocess.run([sys.executable, os.path.join(work, "child.py"), REF, ROOT, os.path.join(work, "job.pkl"),
                        os.path.join(work, "res.pkl")], check=True)
        res = pickle.load(open(os.path.join(work, "res.pkl"), "rb"))
    rec = {"scenes": np.array(json.dumps(list(job)))}
    for name, (cfg, gt) in job.items():
        r = res[name]
        anchors = seq.make_anchors(cfg)
        assert len(anchors) == len(r["anchors"])
        for a, b in zip(anchors, r["anchors"]):
            assert a.shape == b.shape and np.array_equal(seq.bits(a), seq.bits(b)), f"{name}: regenerated anchors differ"
        ref = {"box_cls_labels": r["labels"], "box_reg_targets": r["targets"], "reg_weights": r["weights"]}
        assert r["labels"].dtype == np.int32 and r["targets"].dtype == F and r["weights"].dtype == F
        ours = seq.assign(cfg, anchors, gt)
        why = seq.report(ours, ref, cfg, anchors, gt, sincos_cols_bounded=bool(cfg["sincos"]))
        assert not why, f"{name}: the restatement differs from the reference\n{why}"
        if cfg["sincos"]:
            d = np.abs(ours["box_reg_targets"][..., 6:8].astype(np.float64) - r["targets"][..., 6:8])
            print(name, "sincos columns: largest difference", d.max(), "bound", seq.SINCOS_BOUND, "unequal", int((d > 0).sum()))
        rec[name + "_cfg"] = np.array(json.dumps(cfg))
        rec[name + "_gt"] = gt
        rec[name + "_labels"], rec[name + "_targets"], rec[name + "_weights"] = r["labels"], r["targets"], r["weights"]
        print(name, "gt", gt.shape, "anchors", [a.shape for a in anchors], "foreground", int((r["labels"] > 0).sum()),
              "ignored", int((r["labels"] < 0).sum()))
    path = os.path.join(GOLD, "anchor_targets.npz")
    np.savez_compressed(path, **rec)
    cases = seq.fixture_cases(dict(np.load(path)))
    missing = [k for k, v in cases.items() if not v]
    assert not missing, f"the fixture lacks: {missing}"
    size = os.path.getsize(path)
    assert size <= os.path.getsize(os.path.join(GOLD, "pointnet2_batch.npz")), size
    print(path, size, "bytes;", len(cases), "cases")


if __name__ == "__main__":
    main()
