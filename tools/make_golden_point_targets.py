"""Golden point-head targets for modest_amd.utils.point_head_targets (BUILD CONTAINER ONLY -- needs /root/reference).

Runs the reference's own ``PointHeadTemplate.assign_stack_targets``, ``PointResidualCoder`` and ``enlarge_box3d``
(imported from where they lie, nothing copied) on the CPU in a child process.  The child binds empty package modules
that keep their ``__path__`` (so ``pcdet/models/__init__.py`` is never executed) and this project's shims for the
extension modules (``pcdet_bind.install``), makes ``Tensor.cuda`` the identity (the coder calls it on its table) and
replaces ``roiaware_pool3d_utils.points_in_boxes_gpu`` by ``roipool_seq.points_in_boxes``, the restatement that
tests/golden/roipool.npz pins to the reference's kernel text.

Recorded in tests/golden/point_targets.npz per scene: the config as JSON (plain values), points, gt boxes, enlarged
boxes, the coder's table and the outputs asked for.  Five scenes, one per way the three heads call the method (box +
part, box, box without mean size, part, labels only), a few hundred points each.  The tool asserts
  * that torch's CPU cos / sin of every heading and log of every size quotient that can reach a box label equals the
    double function rounded once: headings and sizes are drawn by rejection, at most 1 candidate in 4 may be dropped;
  * that the numpy restatement (tests/point_targets_seq.py) reproduces every recorded label and box label bit for bit
    and every part label within the bound of DESIGN.md section 7l, computed from the inputs;
  * every case of point_targets_seq.fixture_cases, and the fixture's size.

A sixth scene, ``crowd``, goes into a file of its own, tests/golden/point_targets_crowd.npz (the first file keeps its
five scenes and its bytes): B = 3, M = 140 rows of which 140 / 100 / 66 are live, 400 shuffled points, box and part
labels, three classes, mean sizes -- past two tiles of the kernel's 64 rows, under the same conditions, and with the
cases of point_targets_seq.crowd_cases.  It is drawn from a random state of its own after the five, so they stay as
they were.  A fixture whose arrays are all unchanged is left alone on disk (a zip archive carries the time of writing).

Usage:  python tools/make_golden_point_targets.py        (writes both files)
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
EXTRA = [0.2, 0.2, 0.2]     # GT_EXTRA_WIDTH of the reference's configs

_CHILD = r"""
import os, pickle, sys, types
import numpy as np
import torch
ref, root, job = sys.argv[1], sys.argv[2], pickle.load(open(sys.argv[3], "rb"))
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
for name in ("pcdet", "pcdet.models", "pcdet.models.dense_heads", "pcdet.utils", "pcdet.ops", "pcdet.ops.iou3d_nms",
             "pcdet.ops.roiaware_pool3d"):
    m = types.ModuleType(name)
    m.__path__ = [os.path.join(ref, *name.split("."))]
    sys.modules[name] = m
from modest_amd.utils import pcdet_bind
pcdet_bind.install(stand_ins=False)
torch.Tensor.cuda = lambda self, *a, **k: self
import roipool_seq
from pcdet.ops.roiaware_pool3d import roiaware_pool3d_utils
from pcdet.models.dense_heads.point_head_template import PointHeadTemplate
from pcdet.utils.box_coder_utils import PointResidualCoder
from pcdet.utils import box_utils
assert PointHeadTemplate.__module__.startswith("pcdet.") and roiaware_pool3d_utils.__file__.startswith(ref)
def points_in_boxes_gpu(points, boxes):
    return torch.from_numpy(roipool_seq.points_in_boxes(boxes.numpy(), points.numpy()))
roiaware_pool3d_utils.points_in_boxes_gpu = points_in_boxes_gpu
res = {}
for name, (cfg, pts, gt, mean) in job.items():
    kw = dict(mean_size=mean.tolist()) if cfg["use_mean_size"] else {}
    head = types.SimpleNamespace(num_class=cfg["num_class"],
                                 box_coder=PointResidualCoder(code_size=8, use_mean_size=cfg["use_mean_size"], **kw))
    g = torch.from_numpy(gt.copy())
    ext = box_utils.enlarge_box3d(g.view(-1, g.shape[-1]), extra_width=cfg["extra_width"]).view(g.shape[0], -1, g.shape[-1])
    out = PointHeadTemplate.assign_stack_targets(head, points=torch.from_numpy(pts.copy()), gt_boxes=g, extend_gt_boxes=ext,
                                                 set_ignore_flag=True, use_ball_constraint=False,
                                                 ret_part_labels=cfg["want_part"], ret_box_labels=cfg["want_box"])
    assert np.array_equal(g.numpy().view(np.uint32), gt.view(np.uint32)), "the reference changed its input"
    res[name] = dict(ext=ext.numpy(), **{k: None if v is None else v.numpy() for k, v in out.items()})
pickle.dump(res, open(sys.argv[4], "wb"))
"""

DRAWS = {"candidates": 0, "dropped": 0}


def agrees(values, np_fn, torch_fn):
    import torch
    import point_targets_seq as seq
    v = np.atleast_1d(np.asarray(values, dtype=F))
    return bool(np.array_equal(torch_fn(torch.from_numpy(v.copy())).numpy().view(np.uint32),
                               seq.f32_of_double(np_fn, v).view(np.uint32)))


def draw(rs, lo, hi, ok):
    """a float32 uniform in [lo, hi) that passes ok, by rejection; every candidate is counted"""
    for _ in range(200):
        v = F(rs.uniform(lo, hi))
        DRAWS["candidates"] += 1
        if ok(v):
            return v
        DRAWS["dropped"] += 1
    raise RuntimeError("no value found")


def heading(rs, lo=-3.5, hi=3.5):
    import torch
    return draw(rs, lo, hi, lambda v: agrees(v, np.cos, torch.cos) and agrees(v, np.sin, torch.sin))


def size(rs, lo, hi, against):
    """a box size whose quotient with every entry of `against` (mean sizes; [1] without) has a log torch agrees on"""
    import torch
    return draw(rs, lo, hi, lambda v: all(agrees(np.maximum(v, F(1e-5)) / F(a), np.log, torch.log) for a in against))


def make_scene(rs, cfg, B, M, n_live, n_points):
    """-> points (N, 4), gt (B, M, 8).  n_live[b] live rows per sample, the rest zero rows; every scene holds: a pair of
    overlapping boxes, a box with dx = 0 around a point, a box with negative dz over a point, points inside the enlarged
    box only, the origin inside zero rows alone (sample 0), points of no sample"""
    mean = np.asarray(cfg["mean_size"], dtype=F).reshape(-1, 3) if cfg["use_mean_size"] else None
    n_cls = cfg["num_class"]

    def against(c, d):
        if not cfg["want_box"]:
            return [1.0]
        if mean is None:
            return [1.0]
        return [mean[(c - 1) % len(mean), d]]

    gt = np.zeros((B, M, 8), dtype=F)
    pts = []
    for b in range(B):
        for j in range(n_live[b]):
            c = 1 + (j % n_cls)
            if j == 1:   # overlaps row 0: the same centre, a little larger
                gt[b, j] = gt[b, 0]
                gt[b, j, 3:6] = [size(rs, 4.0, 5.0, against(c, 0)), size(rs, 2.0, 2.6, against(c, 1)), size(rs, 1.8, 2.2, against(c, 2))]
                gt[b, j, 7] = c
                continue
            ctr = [rs.uniform(5, 60) * (1 if b % 2 == 0 else -1), rs.uniform(-30, 30) + 70 * (j % 2), rs.uniform(-1.5, 0.5)]
            gt[b, j] = [*ctr, size(rs, 3.0, 4.5, against(c, 0)), size(rs, 1.4, 2.0, against(c, 1)),
                        size(rs, 1.3, 1.8, against(c, 2)), heading(rs), c]
        j = n_live[b]
        if b == 0 and n_live[b] + 2 <= M:
            # dx = 0 (the clamp in the log and, with box labels, in the part labels); class 0 names the last mean size
            gt[b, j] = [1.0, 100.0, 0.0, 0.0, size(rs, 1.4, 2.0, against(0, 1)), size(rs, 1.3, 1.8, against(0, 2)), 0.0, 0.0]
            pts += [[b, 1.0, 100.25, 0.1], [b, F(1.0) + F(2.0 ** -18), 99.5, -0.2]]
            # dz < 0: no point is ever inside
            gt[b, j + 1] = [-100.0, -100.0, 0.0, 3.0, 2.0, -1.5, 0.25, 1.0]
            pts += [[b, -100.0, -100.0, 0.0], [b, -100.5, -100.1, 0.3]]
        for j in range(n_live[b]):
            g = gt[b, j]
            k = 10
            u = rs.uniform(-0.62, 0.62, (k, 3))           # beyond +-0.5: in the enlarged box only, or outside both
            u[:2] *= 0.5
            c, s = np.cos(g[6]), np.sin(g[6])
            lx, ly, lz = u[:, 0] * g[3], u[:, 1] * g[4], u[:, 2] * g[5]
            pts += [[b, g[0] + x * c - y * s, g[1] + x * s + y * c, g[2] + z] for x, y, z in zip(lx, ly, lz)]
    pts.append([0, 0.0, 0.0, 0.0])                        # the origin: inside the zero rows of sample 0 and nothing else
    pts += [[B, 1.0, 1.0, 0.0], [-1, 1.0, 1.0, 0.0], [0.5, *gt[0, 0, :3]], [np.nan, *gt[0, 0, :3]]]
    while len(pts) < n_points:
        b = rs.randint(B)
        pts.append([b, rs.uniform(-70, 70), rs.uniform(-40, 110), rs.uniform(-3, 1)])
    pts = np.array(pts, dtype=F)
    order = np.argsort(pts[:, 0], kind="stable")          # grouped by sample as a batch is; the strays first and last
    return np.ascontiguousarray(pts[order]), gt


def make_crowd(rs, cfg, n_points=400, M=140, n_live=(140, 100, 66)):
    """-> points (n_points, 4) shuffled, gt (3, M, 8): the live boxes one per cell of a 12 m grid (none touches another),
    but for one row of the third tile (sample 0) and one of the second (sample 1) that enclose a row of the first; points
    in and around rows of every tile, points 5 cm outside rows of the last tile, the origin (zero rows only), strays"""
    mean = np.asarray(cfg["mean_size"], dtype=F).reshape(-1, 3)
    B = len(n_live)
    gt = np.zeros((B, M, 8), dtype=F)
    around = {0: (131, 10), 1: (70, 3)}       # sample: (the enclosing row, the row it encloses)
    for b in range(B):
        for j in range(n_live[b]):
            c = 1 + j % 3
            against = [[mean[c - 1, d]] for d in range(3)]
            if j == around.get(b, (None,))[0]:
                gt[b, j] = gt[b, around[b][1]]
                gt[b, j, 3:6] = [size(rs, 4.6, 5.2, against[0]), size(rs, 2.1, 2.6, against[1]), size(rs, 1.9, 2.2, against[2])]
                gt[b, j, 7] = c
                continue
            ctr = [-66 + 12 * (j % 12) + rs.uniform(-2, 2), -66 + 12 * (j // 12) + rs.uniform(-2, 2), rs.uniform(-1.5, 0.5)]
            gt[b, j] = [*ctr, size(rs, 3.0, 4.5, against[0]), size(rs, 1.4, 2.0, against[1]), size(rs, 1.3, 1.8, against[2]),
                        heading(rs), c]

    def at(b, j, u):
        g = gt[b, j]
        c, s = np.cos(g[6]), np.sin(g[6])
        x, y, z = u[0] * g[3], u[1] * g[4], u[2] * g[5]
        return [b, g[0] + x * c - y * s, g[1] + x * s + y * c, g[2] + z]

    pts = []
    rows = {0: sorted(set(range(0, 128, 5)) | set(range(128, 140))), 1: sorted(set(range(0, 100, 8)) | {3, 63, 64, 70, 99}),
            2: sorted(set(range(0, 66, 6)) | {63, 64, 65})}
    for b in range(B):
        for j in rows[b]:
            u = rs.uniform(-0.62, 0.62, (4, 3))           # beyond +-0.5: in the enlarged box only, or outside both
            u[:2] *= 0.5
            pts += [at(b, j, v) for v in u]
    for j in range(133, 139):                             # 5 cm outside a row of the last tile: that enlarged row alone holds it
        for sign in (-1, 1):
            pts.append(at(0, j, [sign * (0.5 + 0.05 / gt[0, j, 3]), rs.uniform(-0.4, 0.4), rs.uniform(-0.4, 0.4)]))
    pts += [[1, 0.0, 0.0, 0.0], [2, 0.0, 0.0, 0.0]]       # the origin: inside the zero rows of samples 1 and 2 alone
    pts += [[B, 1.0, 1.0, 0.0], [-1, 1.0, 1.0, 0.0], [0.5, *gt[0, 0, :3]], [np.nan, *gt[0, 0, :3]]]
    assert len(pts) <= n_points, len(pts)
    while len(pts) < n_points:
        pts.append([rs.randint(B), rs.uniform(-75, 75), rs.uniform(-75, 75), rs.uniform(-3, 1)])
    pts = np.array(pts, dtype=F)
    return np.ascontiguousarray(pts[rs.permutation(len(pts))]), gt


def build_crowd():
    rs = np.random.RandomState(20261020)
    kitti = [[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]]
    cfg = dict(extra_width=EXTRA, num_class=3, use_mean_size=True, mean_size=kitti, want_box=True, want_part=True)
    pts, gt = make_crowd(rs, cfg)
    return {"crowd": (cfg, pts, gt, np.asarray(kitti, dtype=F))}


def build_scenes():
    rs = np.random.RandomState(20261019)
    kitti = [[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]]
    base = dict(extra_width=EXTRA)
    cfgs = {
        "box_part": dict(base, num_class=3, use_mean_size=True, mean_size=kitti, want_box=True, want_part=True),
        "box": dict(base, num_class=1, use_mean_size=True, mean_size=kitti[:1], want_box=True, want_part=False),
        "box_no_mean": dict(base, num_class=3, use_mean_size=False, mean_size=None, want_box=True, want_part=False),
        "part": dict(base, num_class=3, use_mean_size=False, mean_size=None, want_box=False, want_part=True),
        "labels": dict(base, num_class=3, use_mean_size=False, mean_size=None, want_box=False, want_part=False),
    }
    shapes = {"box_part": (2, 12, (7, 4), 330), "box": (3, 8, (5, 0, 3), 300), "box_no_mean": (1, 10, (6,), 200),
              "part": (2, 9, (5, 6), 260), "labels": (2, 7, (3, 4), 200)}
    out = {}
    for name, cfg in cfgs.items():
        B, M, live, n = shapes[name]
        pts, gt = make_scene(rs, cfg, B, M, live, n)
        mean = np.asarray(cfg["mean_size"], dtype=F) if cfg["use_mean_size"] else np.zeros((0, 3), dtype=F)
        out[name] = (cfg, pts, gt, mean)
    return out


def record(job):
    """run the reference on the scenes of `job` and check the restatement against it -> the arrays to save"""
    import torch
    import point_targets_seq as seq
    print("drawn by rejection: %(candidates)d candidates, %(dropped)d dropped" % DRAWS)
    assert DRAWS["dropped"] * 4 <= DRAWS["candidates"], DRAWS
    with tempfile.TemporaryDirectory() as work:
        pickle.dump(job, open(os.path.join(work, "job.pkl"), "wb"))
        open(os.path.join(work, "child.py"), "w").write(_CHILD)
        subprocess.run([sys.executable, os.path.join(work, "child.py"), REF, ROOT, os.path.join(work, "job.pkl"),
                        os.path.join(work, "res.pkl")], check=True)
        res = pickle.load(open(os.path.join(work, "res.pkl"), "rb"))
    rec = {"scenes": np.array(json.dumps(list(job)))}
    for name, (cfg, pts, gt, mean) in job.items():
        r = res[name]
        ext = r["ext"]
        assert seq.same_bits(ext, seq.enlarge(gt, cfg["extra_width"])), f"{name}: enlarge_box3d is not size + extra in float32"
        ref = {k: r[k] for k in ("point_cls_labels", "point_box_labels", "point_part_labels")}
        assert ref["point_cls_labels"].dtype == np.int64
        ms = mean if cfg["use_mean_size"] else None
        ours = seq.assign(pts, gt, ext, cfg["num_class"], ms, cfg["want_box"], cfg["want_part"])
        # every quotient and heading that reached a box label: torch's functions equal the rounded double ones
        k, idx, _ = seq.membership(pts, gt, ext)
        rows = gt[k[idx >= 0], idx[idx >= 0]]
        if cfg["want_box"] and len(rows):
            dg = np.maximum(rows[:, 3:6], seq.TINY)
            if ms is not None:
                dg = dg / ms[(np.trunc(rows[:, 7]).astype(np.int64) - 1) % len(ms)]
            assert agrees(dg.reshape(-1), np.log, torch.log), f"{name}: a log differs"
            assert agrees(rows[:, 6], np.cos, torch.cos) and agrees(rows[:, 6], np.sin, torch.sin), f"{name}: a heading differs"
        bound = seq.part_bound(pts, gt, ext, cfg["want_box"]) if cfg["want_part"] else None
        why = seq.mismatches(ours, ref, bound=bound)
        assert not why, f"{name}: the restatement differs from the reference\n" + "\n".join(why)
        if cfg["want_part"]:
            d = np.abs(ours["point_part_labels"].astype(np.float64) - ref["point_part_labels"])
            fin = np.isfinite(d) & (bound > 0) & np.isfinite(bound)
            print(name, "part labels: unequal", int((d[np.isfinite(d)] > 0).sum()), "largest difference / bound",
                  float((d[fin] / bound[fin]).max()) if fin.any() else 0.0)
        rec[name + "_cfg"] = np.array(json.dumps(cfg))
        rec[name + "_points"], rec[name + "_gt"], rec[name + "_ext"], rec[name + "_mean_size"] = pts, gt, ext, mean
        rec[name + "_labels"] = ref["point_cls_labels"]
        if cfg["want_box"]:
            rec[name + "_box"] = ref["point_box_labels"]
        if cfg["want_part"]:
            rec[name + "_part"] = ref["point_part_labels"]
        lab = ref["point_cls_labels"]
        print(name, "points", pts.shape, "gt", gt.shape, "foreground", int((idx >= 0).sum()), "ignored", int((lab == -1).sum()))
    return rec


def save(path, rec, cases_of, limit):
    """write `rec` unless the file holds exactly these arrays already; then check its cases and its size"""
    import point_targets_seq as seq
    have = dict(np.load(path)) if os.path.exists(path) else {}
    if sorted(have) == sorted(rec) and all(have[k].dtype == np.asarray(v).dtype and have[k].shape == np.asarray(v).shape
                                           and have[k].tobytes() == np.asarray(v).tobytes() for k, v in rec.items()):
        print(path, "holds these arrays already: left as it is")
    else:
        np.savez_compressed(path, **rec)
    cases = cases_of(dict(np.load(path)))
    missing = [k for k, v in cases.items() if not v]
    assert not missing, f"the fixture lacks: {missing}"
    size_ = os.path.getsize(path)
    assert size_ <= limit, size_
    print(path, size_, "bytes;", len(cases), "cases")


def main():
    import point_targets_cases
    import point_targets_seq as seq
    save(os.path.join(GOLD, "point_targets.npz"), record(build_scenes()), seq.fixture_cases, 64 * 1024)
    save(os.path.join(GOLD, "point_targets_crowd.npz"), record(build_crowd()),
         lambda rec: seq.crowd_cases(rec, point_targets_cases.TILE), 96 * 1024)


if __name__ == "__main__":
    main()
