"""Ground-plane throughput (modest_amd.ground_planes) on a Lyft-shaped synthetic tree.

Writes `--frames` frames of about 35 k rows (ground inside the 1.5 / 2.5 window, three calibrations) under `--root`,
reads them once (warm page cache), then runs extract_ransac in this process on one GPU and prints one JSON line:
end-to-end frames/s with the read / H2D / GPU / write split, GPU ms per batch (HIP events), and the same loop as
RANSAC.py (sklearn RANSACRegressor per frame, one after another) on `--sk_frames` frames of the tree on this host.

    python tools/planes_bench.py --root /tmp/planes_tree --frames 1024 --batch 256
"""
import argparse
import json
import os
import shutil
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_tree(root, n_frames, seed=0):
    from modest_amd import synth
    cd, ld = os.path.join(root, "calib"), os.path.join(root, "velodyne")
    os.makedirs(cd, exist_ok=True)
    os.makedirs(ld, exist_ok=True)
    rng = np.random.default_rng(seed)
    for k in range(n_frames):
        n = int(rng.integers(32000, 38000))
        f = synth.ground_frame(rng, n, height=2.1 + rng.uniform(-0.1, 0.1),
                               tilt=(rng.uniform(-0.004, 0.004), rng.uniform(-0.004, 0.004)), clutter=rng.uniform(0.1, 0.5))
        f.tofile(os.path.join(ld, "%06d.bin" % k))
        with open(os.path.join(cd, "%06d.txt" % k), "w") as fh:
            fh.write(synth.ground_calib_txt(k))
    return cd, ld


def sklearn_loop(cd, ld, names, min_h, max_h):
    """RANSAC.py:24-52 restated: per frame Calibration + project_velo_to_rect + window + RANSACRegressor().fit"""
    from sklearn.linear_model import RANSACRegressor
    from modest_amd.utils.kitti_util import Calibration
    np.random.seed(0)
    t0 = time.perf_counter()
    for i in names:
        calib = Calibration(os.path.join(cd, i + ".txt"))
        pc = np.fromfile(os.path.join(ld, i + ".bin"), dtype=np.float32).reshape(-1, 4)
        r = calib.project_velo_to_rect(pc[:, :3])
        v = (r[:, 1] > min_h) & (r[:, 1] < max_h) & (r[:, 2] > -10) & (r[:, 2] < 70) & (r[:, 0] > -20) & (r[:, 0] < 20)
        r = r[v]
        if len(r) >= 5:
            RANSACRegressor().fit(r[:, [0, 2]], r[:, 1])
    return len(names) / (time.perf_counter() - t0)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--root", default="/tmp/modest_planes_bench")
    p.add_argument("--frames", type=int, default=1024)
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--readers", type=int, default=8)
    p.add_argument("--sk_frames", type=int, default=24)
    p.add_argument("--repeats", type=int, default=2)
    a = p.parse_args()
    from modest_amd.ground_planes import extract_ransac
    cd, ld = make_tree(a.root, a.frames)
    for name in sorted(os.listdir(ld)):   # warm page cache
        with open(os.path.join(ld, name), "rb") as f:
            f.read()
    names = sorted(x[:-4] for x in os.listdir(ld))
    runs = []
    for r in range(a.repeats + 1):   # the first run loads the device code and allocates: not reported
        pd = os.path.join(a.root, "planes")
        shutil.rmtree(pd, ignore_errors=True)
        st = {}
        extract_ransac(cd, ld, pd, 1.5, 2.5, batch=a.batch, readers=a.readers, stats=st)
        if r:
            runs.append(st)
    best = min(runs, key=lambda s: s["wall_s"])
    n_batches = (a.frames + a.batch - 1) // a.batch
    sk_rate = sklearn_loop(cd, ld, names[:a.sk_frames], 1.5, 2.5)
    fps = best["frames"] / best["wall_s"]
    out = {"tool": "planes_bench", "frames": best["frames"], "batch": a.batch, "rows_per_frame": "32k-38k",
           "read_mb": round(best["bytes"] / 1e6, 1), "frames_per_s": round(fps, 1),
           "wall_s": round(best["wall_s"], 4), "read_s": round(best["read_s"], 4), "h2d_s": round(best["h2d_s"], 4),
           "gpu_s": round(best["gpu_s"], 4), "write_s": round(best["write_s"], 4), "host_fits": best["host_fits"],
           "gpu_ms_per_batch": round(1e3 * best["gpu_s"] / n_batches, 3),
           "gpu_us_per_frame": round(1e6 * best["gpu_s"] / best["frames"], 2),
           "sklearn_frames": a.sk_frames, "sklearn_frames_per_s": round(sk_rate, 2), "speedup_vs_sklearn": round(fps / sk_rate, 1),
           "runs_wall_s": [round(s["wall_s"], 4) for s in runs]}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
