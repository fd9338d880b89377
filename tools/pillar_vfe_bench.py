"""PointPillars' front end on one MI355X: the reference's PillarVFE.forward and PointPillarScatter.forward -- their torch
expressions, restated here with torch ops from the semantics of tests/pillar_vfe_seq.py, since pcdet is not importable on the GPU
machine -- against the drop-in methods of modest_amd.utils.pillar_vfe on the same modules and tensors, and
profiles/pillar_vfe_bench.json.

Workloads, at B = 4 on the 560 x 496 grid: the Lyft config's 64 000 pillars (S = 32, 4 -> 64) and the test-time 160 000 pillars.
Per workload and side, a training step (forward and backward of both modules, the canvas's gradient given) and a test-time
forward (eval mode, no_grad): the time of a call (median over --windows windows of events on the stream, each of at least 20 ms,
warm, the two sides alternating), the kernel launches of a call (torch's profiler), the synchronising calls of a call (torch's
sync debug mode), the peak memory a call allocates, and the largest difference between the two sides' canvases and weight
gradients.  For the forward of PillarVFE alone also the achieved bytes per second against its algorithmic traffic (the voxels
read twice in training mode, once in eval mode, out and the winners written) next to a device-to-device copy that moves the same
traffic (half of it read, half written) in the same run.

    python tools/pillar_vfe_bench.py [--out profiles/pillar_vfe_bench.json] [--windows 5]
    python tools/pillar_vfe_bench.py --once --side op      (one call per workload and mode, for a kernel trace)
"""
import argparse
import json
import os
import sys
import types
import warnings

import numpy as np
import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WINDOW_MS = 60.0            # a window is at least this long (and never fewer than 3 calls)
PEAK_BYTES_PER_S = 8e12     # the figure the README uses


# ---- the reference's two forward methods as torch expressions -------------------------------------------------------------------
def yard_vfe(self, batch_dict, **kwargs):
    v, num, coords = batch_dict["voxels"], batch_dict["voxel_num_points"], batch_dict["voxel_coords"]
    xyz = v[:, :, :3]
    mean = xyz.sum(dim=1, keepdim=True) / num.type_as(v).view(-1, 1, 1)
    cluster = xyz - mean
    centre = torch.zeros_like(xyz)
    for j, (col, size, off) in enumerate(((3, self.voxel_x, self.x_offset), (2, self.voxel_y, self.y_offset), (1, self.voxel_z, self.z_offset))):
        centre[:, :, j] = v[:, :, j] - (coords[:, col].to(v.dtype).unsqueeze(1) * size + off)
    parts = [v if self.use_absolute_xyz else v[..., 3:], cluster, centre]
    if self.with_distance:
        parts.append(torch.norm(xyz, 2, 2, keepdim=True))
    f = torch.cat(parts, dim=-1)
    S = f.shape[1]
    mask = num.unsqueeze(1).int() > torch.arange(S, dtype=torch.int, device=num.device).view(1, -1)
    f *= mask.unsqueeze(-1).type_as(v)
    pfn = self.pfn_layers[0]
    part = 50000                                                     # the reference's chunks of the linear layer
    if f.shape[0] > part:
        x = torch.cat([pfn.linear(f[i * part:(i + 1) * part]) for i in range(f.shape[0] // part + 1)], dim=0)
    else:
        x = pfn.linear(f)
    x = pfn.norm(x.permute(0, 2, 1)).permute(0, 2, 1)
    x = TF.relu(x)
    batch_dict["pillar_features"] = torch.max(x, dim=1, keepdim=True)[0].squeeze()
    return batch_dict


def yard_scatter(self, batch_dict, **kwargs):
    feat, coords = batch_dict["pillar_features"], batch_dict["voxel_coords"]
    batch_size = coords[:, 0].max().int().item() + 1
    planes = []
    for b in range(batch_size):
        plane = torch.zeros(self.num_bev_features, self.nz * self.nx * self.ny, dtype=feat.dtype, device=feat.device)
        on = coords[:, 0] == b
        c = coords[on, :]
        index = (c[:, 1] + c[:, 2] * self.nx + c[:, 3]).type(torch.long)
        plane[:, index] = feat[on, :].t()
        planes.append(plane)
    batch_dict["spatial_features"] = torch.stack(planes, 0).view(batch_size, self.num_bev_features * self.nz, self.ny, self.nx)
    return batch_dict


# ---- timing -----------------------------------------------------------------------------------------------------------------
def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def calls_for(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()               # warm-up: code objects loaded, allocator settled
    t = window(fn, 3)
    return int(min(5000, max(3, np.ceil(WINDOW_MS / max(t, 1e-3)))))


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "windows_ms": [float(x) for x in ms]}


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = int(torch.cuda.max_memory_allocated() - base)
    del out
    return peak


def launches(fn):
    """kernel launches and device copies of one call, from torch's profiler; None where it is not available"""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return int(sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")))
    except Exception as err:      # noqa: BLE001
        print("launch count not available:", err, file=sys.stderr)
        return None


def synchronising_calls(fn):
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    return sum("called a synchronizing" in str(w.message) for w in seen)


WORKLOADS = (("Lyft config, 4 x 16 000 pillars", dict(seed=140, P=64000, S=32, Cp=4, C=64, B=4, ny=496, nx=560)),
             ("test time, 160 000 pillars", dict(seed=141, P=160000, S=32, Cp=4, C=64, B=4, ny=496, nx=560)))


def sides(case, dev):
    """-> {side: (vfe, scatter)} on equal parameters, the batch, the canvas's upstream gradient"""
    import pillar_vfe_seq as seq
    ours = seq.bare_modules(case, dev)
    yard = seq.bare_modules(case, dev)
    yard[0].forward = types.MethodType(yard_vfe, yard[0])
    yard[1].forward = types.MethodType(yard_scatter, yard[1])
    G = torch.from_numpy(seq.grad_canvas_of(case)).to(dev)
    return {"op": ours[:2], "yardstick": yard[:2]}, ours[2], G


def step_of(vfe, sc, batch, G):
    """a training step: forward and backward of both modules (the running buffers move, as in training)"""
    def step():
        for p in vfe.parameters():
            p.grad = None
        canvas = sc(vfe(dict(batch)))["spatial_features"]
        torch.autograd.backward(canvas, G)
        return canvas
    return step


def forward_of(vfe, sc, batch):
    def forward():
        with torch.no_grad():
            return sc(vfe(dict(batch)))["spatial_features"]
    return forward


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pillar_vfe_bench.json"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--once", action="store_true", help="run --steps calls of --side per workload and mode and exit (for a kernel trace)")
    ap.add_argument("--side", choices=("both", "op", "yardstick"), default="both", help="with --once: the side to run")
    ap.add_argument("--steps", type=int, default=1, help="with --once: calls per side, workload and mode")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "pillar_vfe_bench needs an MI355X: there is no CPU fallback"
    import pillar_vfe_seq as seq
    from modest_amd import ops
    dev = torch.device("cuda:0")
    rows = []
    for name, cfg in WORKLOADS:
        case = seq.make_case(**cfg)
        mods, batch, G = sides(case, dev)
        for mode in ("training step", "test-time forward"):
            fns = {}
            for side, (vfe, sc) in mods.items():
                vfe.train(mode == "training step")
                fns[side] = step_of(vfe, sc, batch, G) if mode == "training step" else forward_of(vfe, sc, batch)
            if args.once:
                for side, fn in fns.items():
                    if args.side in ("both", side):
                        for _ in range(args.steps):
                            fn()
                torch.cuda.synchronize()
                continue
            mods["yardstick"][0].load_state_dict(mods["op"][0].state_dict())      # equal buffers, however many steps each side ran
            a, b = fns["op"](), fns["yardstick"]()
            diff = {"canvas": float((a.detach().double() - b.detach().double()).abs().max())}
            if mode == "training step":
                ga, gb = (mods[s][0].pfn_layers[0].linear.weight.grad.double() for s in ("op", "yardstick"))
                diff["grad_weight_relative"] = float((ga - gb).abs().max() / gb.abs().max())
            assert diff["canvas"] < 1e-3 and diff.get("grad_weight_relative", 0.0) < 1e-3, (name, mode, diff)
            del a, b
            n = {s: calls_for(fn) for s, fn in fns.items()}
            t = {s: [] for s in fns}
            for _ in range(args.windows):                                  # alternating: both sides see the same neighbours
                for s, fn in fns.items():
                    t[s].append(window(fn, n[s]))
            row = {"case": name, "mode": mode, "settings": cfg, "op": stats(t["op"]), "yardstick": stats(t["yardstick"]),
                   "calls_per_window": n, "yardstick_over_op": float(np.median(t["yardstick"]) / np.median(t["op"])),
                   "launches": {s: launches(fn) for s, fn in fns.items()},
                   "synchronising_calls": {s: synchronising_calls(fn) for s, fn in fns.items()},
                   "peak_bytes": {s: peak_bytes(fn) for s, fn in fns.items()}, "largest_difference": diff}
            # the forward of PillarVFE alone against a copy of its traffic
            P, S, Cp = case["voxels"].shape
            C = case["W"].shape[0]
            train = mode == "training step"
            vfe = mods["op"][0]

            def alone():
                with torch.set_grad_enabled(train):
                    return vfe(dict(batch))["pillar_features"]

            n_alone = calls_for(alone)
            t_alone = [window(alone, n_alone) for _ in range(args.windows)]
            traffic = P * S * Cp * 4 * (2 if train else 1) + P * C * (5 if train else 4)
            src = torch.empty((traffic // 2,), dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            copy = lambda: dst.copy_(src)                                  # noqa: E731  (a device-to-device memcpy on the stream)
            n_copy = calls_for(copy)
            t_copy = [window(copy, n_copy) for _ in range(args.windows)]
            row["vfe_forward"] = dict(stats(t_alone), traffic_bytes=traffic, bytes_per_s=traffic / (np.median(t_alone) * 1e-3))
            row["vfe_forward"]["fraction_of_8TBps"] = row["vfe_forward"]["bytes_per_s"] / PEAK_BYTES_PER_S
            row["copy"] = dict(stats(t_copy), bytes_copied=traffic // 2, bytes_per_s=traffic / (np.median(t_copy) * 1e-3))
            row["vfe_forward_over_copy_rate"] = row["vfe_forward"]["bytes_per_s"] / row["copy"]["bytes_per_s"]
            del src, dst
            rows.append(row)
            print(json.dumps({k: row[k] for k in row if k not in ("op", "yardstick", "settings", "copy", "vfe_forward")}
                             | {"op_ms": row["op"]["median_ms"], "yardstick_ms": row["yardstick"]["median_ms"],
                                "vfe_forward_ms": row["vfe_forward"]["median_ms"], "copy_ms": row["copy"]["median_ms"]}), flush=True)
        del mods, batch, G
        torch.cuda.empty_cache()
    if args.once:
        return
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "window_ms": WINDOW_MS, "windows": args.windows,
           "tree": {"run": ops.pillar_vfe_run(), "group": ops.pillar_vfe_group()}, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
