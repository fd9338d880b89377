"""``python -m modest_amd.evaluate``: kitti_object_eval_python/evaluate.py on the GPU.

    python -m modest_amd.evaluate [evaluate] --label_path GT_DIR --result_path DT_DIR|result.pkl \\
        --label_split_file SPLIT.txt [--current_class 0|Car|Dynamic] [--score_thresh S] [--range_eval] [--ranges 0,30,50,80]

Prints the reference's result string unchanged, then one JSON line (frames, boxes, pairs, GPU ms per stage, wall
and read/parse seconds).  ``--range_eval`` (the default for Dynamic) runs get_range_eval_result; ``--coco`` raises,
as the reference's COCO path cannot run.  Detections are read for the split's ids; a result.pkl is matched to the
split by frame_id.
"""
import argparse
import json
import os
import pickle
import sys
import time

import numpy as np


def _read_imageset_file(path):
    with open(path, 'r') as f:
        return [int(line) for line in f.readlines()]


def read_detections(result_path, image_ids):
    """a label folder or an OpenPCDet result.pkl -> dt annos in the split's order"""
    from . import kitti_eval as ke
    if os.path.isdir(result_path):
        return ke.get_label_annos(result_path, list(image_ids))
    with open(result_path, "rb") as f:
        det = pickle.load(f)
    by_id = {int(a["frame_id"]): a for a in det}
    missing = [i for i in image_ids if int(i) not in by_id]
    if missing:
        raise KeyError(f"{len(missing)} split ids have no detection entry in {result_path} (first: {missing[0]})")
    return [by_id[int(i)] for i in image_ids]


def _cls(v):
    try:
        return int(v)
    except ValueError:
        return v


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if argv and argv[0] == "evaluate":
        argv = argv[1:]
    p = argparse.ArgumentParser(prog="python -m modest_amd.evaluate")
    p.add_argument("--label_path", required=True)
    p.add_argument("--result_path", required=True)
    p.add_argument("--label_split_file", required=True)
    p.add_argument("--current_class", default="0")
    p.add_argument("--coco", action="store_true")
    p.add_argument("--score_thresh", type=float, default=-1)
    p.add_argument("--range_eval", action="store_true")
    p.add_argument("--ranges", default="0,30,50,80")
    a = p.parse_args(argv)
    from . import kitti_eval as ke
    t0 = time.perf_counter()
    ids = _read_imageset_file(a.label_split_file)
    dt_annos = read_detections(a.result_path, ids)
    if a.score_thresh > 0:
        dt_annos = ke.filter_annos_low_score(dt_annos, a.score_thresh)
    gt_annos = ke.get_label_annos(a.label_path, ids)
    t_read = time.perf_counter() - t0
    cls = _cls(a.current_class)
    ke.reset_timings()
    if a.coco:
        ke.get_coco_eval_result(gt_annos, dt_annos, cls)
    if a.range_eval or cls in ("Dynamic", 6):
        ranges = tuple(int(x) for x in a.ranges.split(","))
        result, _ = ke.get_range_eval_result(gt_annos, dt_annos, cls, ranges=ranges)
    else:
        result, _ = ke.get_official_eval_result(gt_annos, dt_annos, cls)
    print(result)
    ng = sum(len(x["name"]) for x in gt_annos)
    nd = sum(len(x["name"]) for x in dt_annos)
    pairs = int(sum(len(g["name"]) * len(d["name"]) for g, d in zip(gt_annos, dt_annos)))
    print(json.dumps({"frames": len(gt_annos), "gt_boxes": ng, "dt_boxes": nd, "pairs": pairs,
                      "gpu_ms": {k: round(v, 3) for k, v in ke.last_timings.items()},
                      "read_parse_s": round(t_read, 3), "wall_s": round(time.perf_counter() - t0, 3)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
