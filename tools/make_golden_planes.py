"""Golden planes for modest_amd.ground_planes (BUILD CONTAINER ONLY -- needs /root/reference).

Runs the reference's own ``data_preprocessing/RANSAC.py:extract_ransac`` (imported, nothing copied; its
``kitti_util`` imports cv2, which an empty stub module satisfies) on small KITTI-format trees and records the plane
files it writes, in two RNG settings:
  global  -- one run per tree after ``np.random.seed(0)``            (the ``--global_seed 0`` contract);
  frame   -- every frame alone after ``np.random.seed(int(idx))``    (the ``--seed 0`` contract).
Every (tree, window) pair runs in a fresh process.  Per fitted frame the fitted RANSACRegressor's ``n_trials_`` and
``inlier_mask_.sum()`` are recorded with the candidate count and the residual threshold (MAD).

Trees (inputs are stored only where they are not in another fixture):
  nusc   e2e_tree_nusc.npz's 24 frames at 1.3 / 2.0 (2.4-2.6 k candidates each)
  lyft_a e2e_tree.npz's 24 frames at 1.5 / 2.5 (ground at rect y ~ 1.40: every frame takes the default plane)
  lyft_b the same frames at 1.2 / 2.0
  tilt   4 nuScenes frames rolled / pitched by 2-4 degrees, 1.3 / 2.0
  trunc  frames with 0, 4, 5, 120, 299, 300, 301 candidates, 1.3 / 2.0 (sklearn permutes for 0.01 < 3/n < 0.99)

Usage:  python tools/make_golden_planes.py        (writes tests/golden/planes.npz)
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = "/root/reference/data_preprocessing"
GOLD = os.path.join(ROOT, "tests", "golden")

# the child: stub cv2, import the reference, record every RANSACRegressor fit, run extract_ransac
_CHILD = r"""
import contextlib, io, json, sys, types
import numpy as np
sys.modules["cv2"] = types.ModuleType("cv2")
sys.path.insert(0, sys.argv[1])
import RANSAC
rec = []
class Rec(RANSAC.RANSACRegressor):
    def fit(self, X, y, *a, **k):
        r = super().fit(X, y, *a, **k)
        rec.append([int(len(y)), float(np.median(np.abs(y - np.median(y)))), int(self.n_trials_), int(self.inlier_mask_.sum())])
        return r
RANSAC.RANSACRegressor = Rec
calib, lidar, planes, min_h, max_h, mode = sys.argv[2:8]
names = sys.argv[8:]
out = {}
with contextlib.redirect_stdout(io.StringIO()):
    if mode == "global":
        np.random.seed(0)
        RANSAC.extract_ransac(calib, lidar, planes, float(min_h), float(max_h))
    else:
        for i in names:
            split = planes + "_split_" + i
            open(split, "w").write(i + "\n")
            np.random.seed(int(i))
            n0 = len(rec)
            RANSAC.extract_ransac(calib, lidar, planes, float(min_h), float(max_h), split)
            out[i] = rec[n0][:] if len(rec) > n0 else None
print(json.dumps({"rec": rec, "per_frame": out}))
"""


def calib_of(text):
    from modest_amd.ground_planes import calib_mats
    return calib_mats(text)


def write_tree(d, names, frames, calibs):
    os.makedirs(os.path.join(d, "velodyne"))
    os.makedirs(os.path.join(d, "calib"))
    for i, f, c in zip(names, frames, calibs):
        np.ascontiguousarray(f, dtype=np.float32).tofile(os.path.join(d, "velodyne", i + ".bin"))
        open(os.path.join(d, "calib", i + ".txt"), "w").write(c)


def run_ref(d, names, min_h, max_h, mode):
    planes = os.path.join(d, "planes_" + mode)
    r = subprocess.run([sys.executable, "-c", _CHILD, REF, os.path.join(d, "calib"), os.path.join(d, "velodyne"), planes,
                        repr(min_h), repr(max_h), mode, *names], capture_output=True, text=True, cwd=d)
    if r.returncode != 0:
        raise RuntimeError(r.stderr)
    info = json.loads(r.stdout.strip().splitlines()[-1])
    texts = [open(os.path.join(planes, i + ".txt")).read() for i in names]
    return texts, info


def cand_mask(rows, calib, min_h, max_h):
    V2C, R0 = calib_of(calib)
    ref = np.dot(np.hstack((rows[:, :3], np.ones((len(rows), 1)))), V2C.T)
    r = np.dot(R0, ref.T).T
    return (r[:, 1] > min_h) & (r[:, 1] < max_h) & (r[:, 2] > -10) & (r[:, 2] < 70) & (r[:, 0] > -20) & (r[:, 0] < 20)


def rot(roll_deg, pitch_deg):
    a, b = np.radians(roll_deg), np.radians(pitch_deg)
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    return Rx @ Ry


def trees():
    nu = np.load(os.path.join(GOLD, "e2e_tree_nusc.npz"))
    ly = np.load(os.path.join(GOLD, "e2e_tree.npz"))

    def frames(z):
        o = z["bin_offsets"]
        return [z["bins"][o[k]:o[k + 1]] for k in range(len(o) - 1)], [str(c) for c in z["calib"]]

    nf, nc = frames(nu)
    lf, lc = frames(ly)
    names24 = ["%06d" % k for k in range(24)]
    out = {"nusc": (names24, nf, nc, 1.3, 2.0, False), "lyft_a": (names24, lf, lc, 1.5, 2.5, False),
           "lyft_b": (names24, lf, lc, 1.2, 2.0, False)}
    tilt = []
    for k, (ro, pi) in enumerate([(2.0, 0.0), (0.0, -3.0), (3.0, 2.5), (-4.0, 3.5)]):
        f = nf[3 + k].copy()
        f[:, :3] = (f[:, :3].astype(np.float64) @ rot(ro, pi).T).astype(np.float32)
        tilt.append(f)
    out["tilt"] = (["%06d" % (100 + k) for k in range(4)], tilt, nc[3:7], 1.3, 2.0, True)
    trunc, tc = [], []
    base, bc = nf[10], nc[10]
    m = cand_mask(base, bc, 1.3, 2.0)
    cand, other = base[m], base[~m][:40]
    for k in (0, 4, 5, 120, 299, 300, 301):
        trunc.append(np.concatenate([other[:20], cand[:k], other[20:]]))
        tc.append(bc)
    out["trunc"] = (["%06d" % (200 + k) for k in range(7)], trunc, tc, 1.3, 2.0, True)
    return out


def main():
    res = {}
    for name, (names, fr, cal, lo, hi, store) in trees().items():
        with tempfile.TemporaryDirectory() as d:
            write_tree(d, names, fr, cal)
            g_txt, g_info = run_ref(d, names, lo, hi, "global")
            f_txt, f_info = run_ref(d, names, lo, hi, "frame")
        # per-frame statistics: -1 rows for the default frames (no fit)
        gstat = np.full((len(names), 4), -1.0)
        it = iter(g_info["rec"])
        for k, f in enumerate(fr):
            if cand_mask(f, cal[k], lo, hi).sum() >= 5:
                gstat[k] = next(it)
        fstat = np.array([f_info["per_frame"][i] if f_info["per_frame"][i] else [-1.0] * 4 for i in names], dtype=np.float64)
        res[f"{name}_names"] = np.array(names)
        res[f"{name}_window"] = np.array([lo, hi])
        res[f"{name}_global"] = np.array(g_txt)
        res[f"{name}_frame"] = np.array(f_txt)
        res[f"{name}_global_stats"] = gstat
        res[f"{name}_frame_stats"] = fstat
        if store:
            res[f"{name}_bins"] = np.concatenate(fr).astype(np.float32)
            res[f"{name}_offsets"] = np.concatenate([[0], np.cumsum([len(f) for f in fr])]).astype(np.int64)
            res[f"{name}_calib"] = np.array(cal)
        print(name, "n_cand", [int(cand_mask(f, cal[k], lo, hi).sum()) for k, f in enumerate(fr)])
    path = os.path.join(GOLD, "planes.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
