#!/usr/bin/env python
"""Time the device voxeliser (modest_amd.ops.voxelize) on B = 4 synthetic Lyft-shape clouds with the PointPillars
geometry and its train / test caps (pointpillar_dynamic_obj.yaml: voxels of 0.16 x 0.16 x 4, 32 points per voxel,
16 000 / 40 000 voxels per cloud) against two yardsticks, and write profiles/voxelize_bench.json.

  host   what the reference's data pipeline does: the host generator (modest_amd.utils.spconv_utils, one thread) cloud
         by cloud, collate_batch's concatenation, and the host-to-device copy of the zero-padded voxels, the coordinates
         and the counts.
  torch  a composition of stock PyTorch-ROCm operators written in this file, independent of the code under test:
         torch.unique over the cell keys, the first index of every cell by scatter_reduce, argsort of the first indices
         for the voxel numbers, a stable argsort for the slots, scatters for the outputs.

All three run in this process on the same inputs; each is warmed up; a window is a fixed number of whole batches timed
with the host clock around work that ends in a device synchronise (the op itself synchronises once to size its outputs);
the three alternate window by window (other people's work shares the host); median, minimum and maximum of the windows
are written.  Before any time is reported all three outputs are compared bit for bit and every difference is listed.

    python tools/voxelize_bench.py [--out profiles/voxelize_bench.json] [--windows 7] [--points 100000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from modest_amd import synth  # noqa: E402

VOXEL, RANGE, P = [0.16, 0.16, 4], [0, -39.68, -3, 89.6, 39.68, 1], 32
CAPS = {"train": 16000, "test": 40000}
I32, I64, F32 = torch.int32, torch.int64, torch.float32


def lyft_clouds(b, n):
    world = synth.make_world(0)
    return [synth.sample_frame(world, 1000 + k, n - 977 * k, synth._pose_matrix(5.0 * k, 0.0, 0.01), synth.default_l2e(),
                               mobiles=synth.make_mobiles(k, 5.0 * k)) for k in range(b)]


def stack(clouds):
    return np.concatenate([np.concatenate([np.full((len(c), 1), b, dtype=np.float32), c], axis=1) for b, c in enumerate(clouds)])


# ---- yardstick 1: the host path + collate + H2D ----------------------------------------------------------------------------
def yard_host(clouds, m, dev):
    from modest_amd.utils.spconv_utils import VoxelGeneratorV2
    gen = VoxelGeneratorV2(voxel_size=VOXEL, point_cloud_range=RANGE, max_num_points=P, max_voxels=m)

    def run():
        outs = [gen.generate(c) for c in clouds]
        voxels = np.concatenate([o["voxels"] for o in outs])
        coords = np.concatenate([np.pad(o["coordinates"], ((0, 0), (1, 0)), mode="constant", constant_values=b)
                                 for b, o in enumerate(outs)])
        num = np.concatenate([o["num_points_per_voxel"] for o in outs])
        masks, count = [], 0
        for o, c in zip(outs, clouds):
            v = o["voxel_point_mask"].copy()
            v[v >= 0] += count
            masks.append(v)
            count += len(c)
        mask = np.concatenate(masks)
        counts = np.asarray([o["voxel_num"] for o in outs], dtype=np.int32)
        return (torch.from_numpy(voxels).to(dev), torch.from_numpy(coords).to(dev), torch.from_numpy(num).to(dev),
                torch.from_numpy(mask).to(dev), counts)
    return run


# ---- yardstick 2: stock torch operators ------------------------------------------------------------------------------------
def yard_torch(points, m, batch, voxel=VOXEL, rng=RANGE, p=P):
    dev = points.device
    lo = torch.tensor(np.asarray(rng[:3], dtype=np.float32), device=dev)
    vs = torch.tensor(np.asarray(voxel, dtype=np.float32), device=dev)
    grid_np = np.round((np.asarray(rng[3:], dtype=np.float32) - np.asarray(rng[:3], dtype=np.float32))
                       / np.asarray(voxel, dtype=np.float32)).astype(np.int64)
    grid = torch.tensor(grid_np, device=dev)
    cells = int(np.prod(grid_np))
    n, width = points.shape[0], points.shape[1] - 1

    def run():
        b = points[:, 0].to(I64)
        c = torch.floor((points[:, 1:4] - lo) / vs)
        kept = ((c >= 0) & (c < grid.to(F32))).all(dim=1)
        ci = torch.where(kept[:, None], c, torch.zeros((), device=dev)).to(I64)
        cell = (ci[:, 2] * grid[1] + ci[:, 1]) * grid[0] + ci[:, 0]
        key = torch.where(kept, b * cells + cell, torch.full((), batch * cells, dtype=I64, device=dev))
        uniq, inv = torch.unique(key, return_inverse=True)
        rows_i = torch.arange(n, device=dev)
        first = torch.full((len(uniq),), n, dtype=I64, device=dev).scatter_reduce(0, inv, rows_i, "amin")
        cloud = uniq // cells
        first = torch.where(cloud < batch, first, torch.full((), n, dtype=I64, device=dev))   # the dropped rows' group comes last
        vrank = torch.empty_like(first)
        vrank[torch.argsort(first)] = torch.arange(len(uniq), device=dev)        # cells in the order they were opened
        per_cloud = torch.bincount(cloud, minlength=batch + 1)[:batch]
        rbase = torch.cumsum(per_cloud, 0) - per_cloud
        counts = per_cloud.clamp(max=m)
        obase = torch.cumsum(counts, 0) - counts
        live = cloud < batch
        cl = cloud.clamp(max=batch - 1)
        local = vrank - rbase[cl]
        vok = live & (local < m)
        vrow = obase[cl] + local
        order = torch.argsort(inv, stable=True)                                    # rows grouped by cell, in row order
        sinv = inv[order]
        seg = torch.bincount(inv, minlength=len(uniq))
        slot = torch.arange(n, device=dev) - (torch.cumsum(seg, 0) - seg)[sinv]
        take = vok[sinv] & (slot < p)
        src, row, slot = order[take], vrow[sinv][take], slot[take]
        counts_h = counts.cpu().numpy().astype(np.int32)                           # the synchronise that sizes the outputs
        total = int(counts_h.sum())
        voxels = torch.zeros((total, p, width), dtype=F32, device=dev)
        voxels.view(I32)[row, slot] = points.view(I32)[src, 1:]
        mask = torch.full((total, p), -1, dtype=I32, device=dev)
        mask[row, slot] = src.to(I32)
        num = torch.bincount(row, minlength=total).to(I32)
        coords = torch.empty((total, 4), dtype=I32, device=dev)
        uc = uniq[vok] % cells
        coords[vrow[vok]] = torch.stack([cloud[vok], uc // (grid[0] * grid[1]), (uc // grid[0]) % grid[1], uc % grid[0]], 1).to(I32)
        return voxels, coords, num, mask, counts_h
    return run


def op_device(points, m, batch):
    from modest_amd import ops
    geo = ops.VoxelizeGeometry(VOXEL, RANGE)
    state = {"ws": None, "pin": None}

    def run():
        pl = ops.voxelize_plan(points, None, None, P, m, batch, state["ws"], state["pin"], geo)
        state["ws"], state["pin"] = pl.workspace, pl.counts_pinned
        return (*ops.voxelize_fill(pl), pl.counts)
    return run


NAMES = ("voxels", "voxel_coords", "voxel_num_points", "voxel_point_mask", "counts")


def differences(a, b):
    """names of the outputs on which a and b differ (bit for bit), with the number of differing voxel rows"""
    out = {}
    for name, x, y in zip(NAMES, a, b):
        x = x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
        y = y.cpu().numpy() if isinstance(y, torch.Tensor) else np.asarray(y)
        if x.shape != y.shape or x.dtype != y.dtype:
            out[name] = f"shape / dtype {x.shape} {x.dtype} against {y.shape} {y.dtype}"
            continue
        xb, yb = (x.view(np.uint32), y.view(np.uint32)) if x.dtype == np.float32 else (x, y)
        bad = (xb != yb).reshape(len(xb), -1).any(axis=1) if len(xb) else np.zeros(0, dtype=bool)
        if bad.any():
            out[name] = {"rows_differ": int(bad.sum()), "first_rows": np.nonzero(bad)[0][:16].tolist()}
    return out


def window(fn, batches):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(batches):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / batches


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)),
            "windows_ms": [float(x) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxelize_bench.json"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--points", type=int, default=100_000, help="points of the largest cloud")
    ap.add_argument("--batches-per-window", type=int, default=0, help="0: enough for a window of about 0.3 s, per side")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/voxelize_bench.py needs an MI355X: there is no CPU path")
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    clouds = lyft_clouds(args.batch, args.points)
    points = torch.from_numpy(stack(clouds)).to(dev)
    rows = []
    for mode, m in CAPS.items():
        sides = {"op": op_device(points, m, args.batch), "host": yard_host(clouds, m, dev), "torch": yard_torch(points, m, args.batch)}
        with torch.no_grad():
            res = {k: fn() for k, fn in sides.items()}
        torch.cuda.synchronize()
        counts = res["op"][4]
        row = {"case": f"B={args.batch} {mode} cap {m}",
               "shape": {"points per cloud": [len(c) for c in clouds], "voxels per cloud": counts.tolist(),
                         "padded voxel bytes": int(counts.sum()) * P * 4 * 4, "point bytes": int(points.numel()) * 4},
               "host_vs_op": differences(res["host"], res["op"]), "torch_vs_op": differences(res["torch"], res["op"])}
        per = {}
        for k, fn in sides.items():
            fn()
            t = window(fn, 1)
            per[k] = args.batches_per_window or int(min(500, max(2, np.ceil(300.0 / max(t, 1e-3)))))
        ms = {k: [] for k in sides}
        with torch.no_grad():
            for _ in range(args.windows):          # alternating windows
                for k, fn in sides.items():
                    ms[k].append(window(fn, per[k]))
        for k in sides:
            row[k] = dict(stats(ms[k]), batches_per_window=per[k])
        row["host_over_op"] = row["host"]["median_ms"] / row["op"]["median_ms"]
        row["torch_over_op"] = row["torch"]["median_ms"] / row["op"]["median_ms"]
        print(json.dumps({k: row[k] if not isinstance(row[k], dict) or "median_ms" not in row[k] else
                          {"median_ms": row[k]["median_ms"], "min_ms": row[k]["min_ms"], "max_ms": row[k]["max_ms"]}
                          for k in row}), flush=True)
        rows.append(row)
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "windows": args.windows,
           "note": "milliseconds per batch, host clock around whole batches ending in a device synchronise; op, host path "
                   "(one thread, + collate + H2D of the padded outputs) and the torch composition alternate window by window",
           "cases": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
