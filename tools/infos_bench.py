"""Dataset infos + gt database throughput (modest_amd.kitti_infos) on a Lyft-shaped synthetic tree.

Writes `--scans` scans of 60-120 k rows with 0-12 boxes (every 64th scan: 300) under `--root` (use /dev/shm), reads them
once (warm page cache), then in this process on one GPU: create_kitti_infos end to end (best of `--repeats` after a
warm-up run that loads the device code), its phase clocks, and the host mirror with the reference's four worker threads
on the same tree on the same host (`--mirror_scans N`: on its first N scans only).  Prints one JSON line.

    python tools/infos_bench.py --root /dev/shm/infos_tree --scans 1485
"""
import argparse
import json
import os
import shutil
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUTPUTS = ("kitti_infos_train.pkl", "kitti_infos_val.pkl", "kitti_dbinfos_train.pkl", "gt_database")


def clean(root):
    for f in OUTPUTS:
        p = os.path.join(root, f)
        shutil.rmtree(p, ignore_errors=True) if os.path.isdir(p) else (os.path.exists(p) and os.remove(p))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--root", default="/dev/shm/modest_infos_bench")
    p.add_argument("--scans", type=int, default=1485)
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--readers", type=int, default=8)
    p.add_argument("--repeats", type=int, default=2)
    p.add_argument("--mirror_scans", type=int, default=0, help="scans of the tree the host mirror runs on (0: all)")
    p.add_argument("--keep", action="store_true")
    a = p.parse_args()
    from modest_amd import kitti_infos as ki, synth
    shutil.rmtree(a.root, ignore_errors=True)
    tree = synth.write_infos_tree(a.root, 3, a.scans, big_every=64)
    vd = os.path.join(a.root, "training", "velodyne")
    for name in sorted(os.listdir(vd)):   # warm page cache
        with open(os.path.join(vd, name), "rb") as f:
            f.read()
    cfg = ki.AttrDict(FOV_POINTS_ONLY=True)
    runs = []
    for r in range(a.repeats + 1):
        clean(a.root)
        st = {}
        ki.create_kitti_infos(cfg, None, a.root, a.root, if_val=True, batch=a.batch, readers=a.readers, stats=st)
        if r:
            runs.append(st)
    best = min(runs, key=lambda s: s["wall_s"])
    # the mirror on a second tree of the same files (links), four worker threads as the reference
    sub = a.root + "_mirror"
    shutil.rmtree(sub, ignore_errors=True)
    m = min(a.mirror_scans, a.scans) if a.mirror_scans > 0 else a.scans
    ids = ["%06d" % k for k in range(m)]
    for d in ("velodyne", "label_2", "calib", "image_2"):
        os.makedirs(os.path.join(sub, "training", d))
        ext = {"velodyne": ".bin", "image_2": ".png"}.get(d, ".txt")
        for i in ids:
            os.link(os.path.join(a.root, "training", d, i + ext), os.path.join(sub, "training", d, i + ext))
    synth.write_infos_splits(sub, [i for k, i in enumerate(ids) if k % 5 != 4], [i for k, i in enumerate(ids) if k % 5 == 4])
    hs = {}
    ki.create_kitti_infos_host(cfg, None, sub, sub, if_val=True, workers=4, stats=hs)
    rate, hrate = best["scans"] / best["wall_s"], hs["scans"] / hs["wall_s"]
    out = {"tool": "infos_bench", "scans": best["scans"], "batch": a.batch, "rows": tree["points"], "boxes": best["boxes"],
           "db_points": best["db_points"], "read_mb": round(best["bytes"] / 1e6, 1), "scans_per_s": round(rate, 1),
           "wall_s": round(best["wall_s"], 3)}
    for k in ("read_s", "host_s", "h2d_s", "gpu_s", "hull_host_s", "write_s", "pickle_s"):
        out[k] = round(best[k], 3)
    out.update(gpu_phase_us_per_scan=round(1e6 * best["gpu_s"] / best["scans"], 1),
               gpu_phase_share_of_wall=round(best["gpu_s"] / best["wall_s"], 3),
               h2d_us_per_scan=round(1e6 * best["h2d_s"] / best["scans"], 1), host_boxes=best["host_boxes"],
               undecided_points=best["undecided_points"], overflow_boxes=best["overflow_boxes"],
               mirror_scans=hs["scans"], mirror_workers=4, mirror_scans_per_s=round(hrate, 2),
               mirror_infos_s=round(hs["infos_s"], 2), mirror_db_s=round(hs["db_s"], 2),
               ratio_over_mirror=round(rate / hrate, 1), runs_wall_s=[round(s["wall_s"], 3) for s in runs])
    print(json.dumps(out), flush=True)
    if not a.keep:
        shutil.rmtree(a.root, ignore_errors=True)
        shutil.rmtree(sub, ignore_errors=True)


if __name__ == "__main__":
    main()
