"""AP evaluation on synthetic Lyft-shaped sets (GPU): label trees of N frames (~25 gt, ~60 detections per frame)
written to a temporary folder, read back, evaluated by the range eval (Dynamic) and by the official eval (Car, with
aos).  Prints one JSON line: read/parse seconds, GPU ms of the overlaps and of the statistics (HIP events), end-to-end
seconds of each eval, and the throughput of the sequential pure-Python restatement (tests/kitti_eval_seq.py) on a
200-frame subset, labelled as such (numba is not available to time).

Usage:  python tools/eval_bench.py [--frames 4900] [--seq-frames 200]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def lyft_set(n, seed=0):
    from modest_amd import synth
    rng = np.random.default_rng(seed)
    gts, dts = [], []
    for f in range(n):
        ng = int(rng.integers(15, 36))
        g = synth._eval_anno(rng, ng, ("Dynamic", "Car", "Pedestrian", "DontCare"), False)
        keep = rng.random(ng) < 0.8
        d = {k: v[keep].copy() for k, v in g.items()}
        d["location"] = np.round(d["location"] + rng.normal(0, 0.3, d["location"].shape), 2)
        fp = synth._eval_anno(rng, max(0, 60 - len(d["name"])), ("Dynamic", "Car"), False)
        d = {k: np.concatenate([d[k], fp[k]], 0) for k in d}
        d["name"] = np.where(d["name"] == "DontCare", "Dynamic", d["name"])
        d["score"] = np.round(rng.random(len(d["name"])), 3)
        gts.append(g)
        dts.append(d)
    return gts, dts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4900)
    ap.add_argument("--seq-frames", type=int, default=200)
    a = ap.parse_args()
    import torch
    from modest_amd import kitti_eval as ke
    from modest_amd import synth
    gts, dts = lyft_set(a.frames)
    tmp = tempfile.mkdtemp()
    try:
        for tag, annos, sc in (("gt", gts, False), ("dt", dts, True)):
            os.makedirs(os.path.join(tmp, tag))
            for i, x in enumerate(annos):
                b = {k: v for k, v in x.items() if sc or k != "score"}
                open(os.path.join(tmp, tag, "%06d.txt" % i), "w").write(synth.label_text(b))
        ids = list(range(a.frames))
        ke.get_range_eval_result(gts[:64], dts[:64], "Dynamic")          # warm-up (code objects, allocator)
        t0 = time.perf_counter()
        g = ke.get_label_annos(os.path.join(tmp, "gt"), ids)
        d = ke.get_label_annos(os.path.join(tmp, "dt"), ids)
        t_read = time.perf_counter() - t0
        out = {"frames": a.frames, "gt_boxes": sum(len(x["name"]) for x in g), "dt_boxes": sum(len(x["name"]) for x in d),
               "pairs": int(sum(len(x["name"]) * len(y["name"]) for x, y in zip(g, d))), "read_parse_s": round(t_read, 3)}
        for tag, fn in (("range", lambda: ke.get_range_eval_result(g, d, "Dynamic")),
                        ("official", lambda: ke.get_official_eval_result(g, d, "Car"))):
            ke.reset_timings()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out[f"{tag}_s"] = round(time.perf_counter() - t1, 3)
            out[f"{tag}_gpu_ms"] = {k: round(v, 3) for k, v in ke.last_timings.items()}
        out["end_to_end_range_from_files_s"] = round(t_read + out["range_s"], 3)
        # the sequential restatement on a subset (pure Python: what an evaluator without numba runs)
        import kitti_eval_seq as seq
        n = min(a.seq_frames, a.frames)
        bl = [x[0] for x in ke.frame_overlaps(g[:n], d[:n])]
        frames = list(zip(g[:n], d[:n], bl))
        t2 = time.perf_counter()
        seq.eval_config(frames, 1, 6, 3, 0.5, flags=seq.range_flags(frames, 6, (0, 80)))
        ts = time.perf_counter() - t2
        out["python_restatement"] = {"frames": n, "configs": 1, "seconds": round(ts, 3),
                                     "frames_per_s_per_config": round(n / ts, 1)}
        print(json.dumps(out))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
