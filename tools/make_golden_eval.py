"""Golden AP evaluation for modest_amd.kitti_eval (BUILD CONTAINER ONLY -- needs /root/reference).

Runs the reference's own ``kitti_object_eval_python/eval.py`` (imported, nothing copied) in a child process.  The
child installs a stub ``numba``: ``jit`` and ``cuda.jit`` are identity decorators and ``cuda.local.array`` returns
float32 zeros with room for 24 polygon vertices (the reference's 8-vertex buffer overflows for nested boxes).
``rotate_iou_gpu_eval`` is replaced by a pair loop over the reference's own ``devRotateIoUEval`` on float32 arrays,
with the kernel's argument order (query box first).

Inputs come from ``modest_amd.synth.eval_frames``.  Detections whose BEV box equals a gt box are dropped (the
reference's polygon walk is decided by rounding there; modest_amd gives such pairs their true IoU of 1).  Detections whose BEV or 3-D IoU with any gt box lies within 1e-3
of 0.25, 0.5 or 0.7, or whose overlap with a gt box is within 1e-4 of (but not equal to) another detection's, are
dropped, so that no AP depends on float32 noise.

Recorded: the annos, every frame's (dt, gt) BEV and 3-D IoU blocks, the range-eval string and dict for Dynamic, the
official-eval strings and dicts for Car and for Pedestrian (with aos), and fused_compute_statistics' (tp, fp, fn)
table of one range configuration (Dynamic, 0-80 m, BEV, min overlap 0.7).

Usage:  python tools/make_golden_eval.py        (writes tests/golden/kitti_eval.npz)
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
REF = "/root/reference/downstream/OpenPCDet/pcdet/datasets/kitti"
GOLD = os.path.join(ROOT, "tests", "golden")
KEYS = ("truncated", "occluded", "alpha", "bbox", "dimensions", "location", "rotation_y", "score")

_CHILD = r"""
import pickle, sys, types
import numpy as np
numba = types.ModuleType("numba")
def _jit(*a, **k):
    if len(a) == 1 and callable(a[0]) and not k:
        return a[0]
    return lambda f: f
class _Local:
    @staticmethod
    def array(shape, dtype=None):
        n = shape[0] if isinstance(shape, tuple) else shape
        return np.zeros(48 if n == 16 else n, dtype=np.float32)   # 16-float buffers: 24 vertices
cuda = types.ModuleType("numba.cuda")
cuda.jit, cuda.local, cuda.shared = _jit, _Local, _Local
numba.jit, numba.cuda, numba.float32 = _jit, cuda, np.float32
sys.modules["numba"], sys.modules["numba.cuda"] = numba, cuda
sys.path.insert(0, sys.argv[1])
import kitti_object_eval_python.rotate_iou as ri
import kitti_object_eval_python.eval as ev
_sort = ri.sort_vertex_in_convex_polygon
def _rot(boxes, query_boxes, criterion=-1, device_id=0):
    b = boxes.astype(np.float32)
    q = query_boxes.astype(np.float32)
    out = np.zeros((len(b), len(q)), dtype=np.float32)
    for n in range(len(b)):
        for k in range(len(q)):
            out[n, k] = ri.devRotateIoUEval(q[k], b[n], criterion)
    return out
ev.rotate_iou_gpu_eval = _rot
job = pickle.load(open(sys.argv[2], "rb"))
gt, dt = job["gt"], job["dt"]
res = {}
if job["what"] == "iou":
    res["bev"], res["d3"] = [], []
    for g, d in zip(gt, dt):
        gb = np.concatenate([g["location"][:, [0, 2]], g["dimensions"][:, [0, 2]], g["rotation_y"][:, None]], 1)
        db = np.concatenate([d["location"][:, [0, 2]], d["dimensions"][:, [0, 2]], d["rotation_y"][:, None]], 1)
        g7 = np.concatenate([g["location"], g["dimensions"], g["rotation_y"][:, None]], 1)
        d7 = np.concatenate([d["location"], d["dimensions"], d["rotation_y"][:, None]], 1)
        res["bev"].append(ev.bev_box_overlap(db, gb).astype(np.float64))
        res["d3"].append(ev.d3_box_overlap(d7, g7).astype(np.float64))
else:
    res["range"] = ev.get_range_eval_result(gt, dt, "Dynamic")
    res["car"] = ev.get_official_eval_result(gt, dt, "Car")
    res["ped"] = ev.get_official_eval_result(gt, dt, "Pedestrian")
    # fused_compute_statistics for (Dynamic, 0-80 m, BEV, 0.7), as get_range_eval_result runs it
    gr = [ev.filter_det_range(a, 0, 80) for a in gt]
    dr = [ev.filter_det_range(a, 0, 80) for a in dt]
    overlaps, parted, total_dt_num, total_gt_num = ev.calculate_iou_partly(dr, gr, 1, 100)
    (gdl, ddl, igs, ids, dcs, tdc, nvalid) = ev._prepare_data(gr, dr, 6, 3)
    th = []
    for i in range(len(gr)):
        th += ev.compute_statistics_jit(overlaps[i], gdl[i], ddl[i], igs[i], ids[i], dcs[i], 1, min_overlap=0.7,
                                        thresh=0.0, compute_fp=False)[4].tolist()
    thr = np.array(ev.get_thresholds(np.array(th), nvalid))
    pr = np.zeros([len(thr), 4])
    for i in range(len(gr)):
        for t, s in enumerate(thr):
            tp, fp, fn, _, _ = ev.compute_statistics_jit(overlaps[i], gdl[i], ddl[i], igs[i], ids[i], dcs[i], 1,
                                                         min_overlap=0.7, thresh=s, compute_fp=True)
            pr[t, 0] += tp; pr[t, 1] += fp; pr[t, 2] += fn
    res["pr"], res["thr"] = pr[:, :3].astype(np.int64), thr
pickle.dump(res, open(sys.argv[3], "wb"))
"""


def _child(what, gt, dt):
    with tempfile.TemporaryDirectory() as d:
        job, out, prog = os.path.join(d, "job.pkl"), os.path.join(d, "out.pkl"), os.path.join(d, "child.py")
        pickle.dump({"what": what, "gt": gt, "dt": dt}, open(job, "wb"))
        open(prog, "w").write(_CHILD)
        subprocess.run([sys.executable, prog, REF, job, out], check=True)
        return pickle.load(open(out, "rb"))


def _near(v, marks=(0.25, 0.5, 0.7), eps=1e-3):
    return np.zeros(v.shape, bool) if v.size == 0 else np.any([np.abs(v - m) < eps for m in marks], axis=0)


def clean(gt, dt):
    """drop detections on an IoU threshold or in a near-tie (not an exact tie) with another detection"""
    for _ in range(10):
        iou = _child("iou", gt, dt)
        changed = False
        for f in range(len(gt)):
            bad = np.zeros(len(dt[f]["name"]), bool)
            for m in (iou["bev"][f], iou["d3"][f]):
                bad |= _near(m).any(axis=1) if m.size else False
                for i in range(m.shape[1] if m.size else 0):
                    col = m[:, i]
                    dif = np.abs(col[:, None] - col[None, :])
                    tie = (dif < 1e-4) & (dif > 0) & (col[:, None] > 0.2)
                    bad |= np.triu(tie, 1).any(axis=0)
            for j in range(len(dt[f]["name"])):        # coincident BEV boxes: the reference's result is rounding noise
                bj = np.r_[dt[f]["location"][j, [0, 2]], dt[f]["dimensions"][j, [0, 2]], dt[f]["rotation_y"][j]]
                for i in range(len(gt[f]["name"])):
                    bi = np.r_[gt[f]["location"][i, [0, 2]], gt[f]["dimensions"][i, [0, 2]], gt[f]["rotation_y"][i]]
                    bad[j] |= bool(np.array_equal(bj.astype(np.float32), bi.astype(np.float32)))
            if bad.any():
                keep = np.nonzero(~bad)[0]
                dt[f] = {k: v[keep] for k, v in dt[f].items()}
                changed = True
        if not changed:
            return gt, dt, iou
    raise RuntimeError("could not clean the set")


def main():
    from modest_amd import synth
    gt, dt = synth.eval_frames(7, n_frames=120)
    gt, dt, iou = clean(gt, dt)
    r = _child("eval", gt, dt)
    out = {}
    for tag, annos in (("gt", gt), ("dt", dt)):
        out[f"{tag}_n"] = np.array([len(a["name"]) for a in annos], np.int64)
        out[f"{tag}_name"] = np.concatenate([a["name"].astype("<U16") for a in annos])
        for k in KEYS:
            if k == "score" and tag == "gt":
                continue
            w = {"bbox": (4,), "dimensions": (3,), "location": (3,)}.get(k, ())
            out[f"{tag}_{k}"] = np.concatenate([np.asarray(a[k]).reshape((len(a["name"]),) + w) for a in annos], 0)
    out["bev"] = np.concatenate([m.reshape(-1) for m in iou["bev"]])
    out["d3"] = np.concatenate([m.reshape(-1) for m in iou["d3"]])
    for tag in ("range", "car", "ped"):
        s, d = r[tag]
        out[f"{tag}_str"] = np.array(s)
        out[f"{tag}_keys"] = np.array(list(d.keys()))
        out[f"{tag}_vals"] = np.array([float(v) for v in d.values()], np.float64)
    out["pr_range_bev07"], out["thr_range_bev07"] = r["pr"], r["thr"]
    os.makedirs(GOLD, exist_ok=True)
    path = os.path.join(GOLD, "kitti_eval.npz")
    np.savez_compressed(path, **out)
    print(json.dumps({"frames": len(gt), "gt": int(out["gt_n"].sum()), "dt": int(out["dt_n"].sum()),
                      "bytes": os.path.getsize(path)}))
    print(r["range"][0])
    print(r["car"][0])


if __name__ == "__main__":
    main()
