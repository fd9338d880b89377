"""The trees of tests/golden/planes.npz (tools/make_golden_planes.py) as KITTI-format directories."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TREES = ("nusc", "lyft_a", "lyft_b", "tilt", "trunc")
_SOURCE = {"nusc": "e2e_tree_nusc.npz", "lyft_a": "e2e_tree.npz", "lyft_b": "e2e_tree.npz"}


def golden():
    return np.load(os.path.join(GOLD, "planes.npz"))


def tree_frames(name):
    """(names, [(n,4) float32 rows], [calib text], (min_h, max_h))"""
    g = golden()
    src = np.load(os.path.join(GOLD, _SOURCE[name])) if name in _SOURCE else None
    if src is not None:
        bins, offs, cal = src["bins"], src["bin_offsets"], src["calib"]
    else:
        bins, offs, cal = g[f"{name}_bins"], g[f"{name}_offsets"], g[f"{name}_calib"]
    frames = [np.ascontiguousarray(bins[offs[k]:offs[k + 1]]) for k in range(len(offs) - 1)]
    lo, hi = (float(v) for v in g[f"{name}_window"])
    return [str(x) for x in g[f"{name}_names"]], frames, [str(c) for c in cal], (lo, hi)


def write_tree(root, names, frames, calibs):
    """root/velodyne/<idx>.bin, root/calib/<idx>.txt; returns (calib_dir, lidar_dir)"""
    cd, ld = os.path.join(root, "calib"), os.path.join(root, "velodyne")
    os.makedirs(cd, exist_ok=True)
    os.makedirs(ld, exist_ok=True)
    for i, f, c in zip(names, frames, calibs):
        np.ascontiguousarray(f, dtype=np.float32).tofile(os.path.join(ld, i + ".bin"))
        with open(os.path.join(cd, i + ".txt"), "w") as fh:
            fh.write(c)
    return cd, ld


def read_planes(planes_dir, names):
    out = []
    for i in names:
        with open(os.path.join(planes_dir, i + ".txt")) as f:
            out.append(f.read())
    return out
