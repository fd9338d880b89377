"""The tail of a training step on one MI355X: torch's path -- ``clip_grad_norm_``, a ``mul_`` per parameter (the reference's
decoupled decay), ``torch.optim.Adam.step``, restated here in a few lines -- against the drop-ins of
modest_amd.utils.optim_step on equal tensors: the pair ``clip_grad_norm_`` + ``step`` and the fused ``clip_and_step``
(DESIGN.md section 7w).  Reads only tests/golden/optim_step_shapes.json; writes profiles/optim_step_bench.json.

Per shape set (the recorded ones and a synthetic set of 600 tensors of 64 to 4096 elements) and side: the wall time of a step
(median over --windows windows of events on the stream, each of at least 60 ms, warm, the sides alternating), the host's time
to enqueue a step (a host clock around the calls of a window, before its synchronise), the kernel launches and copies of a
step (torch's profiler), its synchronising calls (torch's sync debug mode) and the peak memory it allocates.  For ``step``
alone also the bytes per second of its algorithmic traffic (28 bytes per element: p, g, m, v read, p, m, v written) next to a
device-to-device copy that moves the same traffic in the same run -- the time of the whole call on the stream, table upload
included, not a kernel time.

Kernel times come from a run of their own under the kernel tracer, with no timing in it:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- \
        python tools/optim_step_bench.py --once --set pointpillars_lyft --steps 20

runs, warm, --steps steps each of the pair and of clip_and_step, first with the chunk partials summed by every workgroup of the
consumer and then with the one-workgroup finishing launch (the kernels differ in their template argument, so the statistics
keep them apart).  ``--kernel-stats SET=CSV`` (repeatable) reads such statistics into the JSON: per kernel the calls and the
average, minimum and maximum time, the step kernel's bytes per second against the copy of the same run of this tool, and the
two ways to the coefficient next to each other.

    python tools/optim_step_bench.py [--out profiles/optim_step_bench.json] [--windows 5] [--kernel-stats SET=CSV ...]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WINDOW_MS = 60.0
MAX_NORM, WD = 10.0, 0.01


def window(fn, calls):
    """-> (ms per call on the stream, host ms per call to enqueue)"""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    host = (time.perf_counter() - t0) * 1e3 / calls
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls, host


def calls_for(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t, _ = window(fn, 3)
    return int(min(5000, max(3, np.ceil(WINDOW_MS / max(t, 1e-3)))))


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def launches(fn):
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


def side(rows, dev, seed):
    """a wrapper over fresh copies of the set's tensors with gradients of a norm near 30 -> (wrapper, parameters)"""
    from optim_step_cases import make_wrapper, onecycle
    gen = torch.Generator(device="cpu").manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(r["shape"], generator=gen).to(dev)) for r in rows]
    total = sum(p.numel() for p in params)
    for p in params:
        p.grad = (torch.randn(p.shape, generator=gen) * (30.0 / total ** 0.5)).to(dev)
    w = make_wrapper([p for p, r in zip(params, rows) if not r["bn"]], [p for p, r in zip(params, rows) if r["bn"]], wd=WD,
                     betas=(0.9, 0.99))
    w.hyper(*onecycle(3))
    return w, params


KERNELS = {"optim_grad_norm_kernel": "norm", "optim_norm_finish_kernel": "finish", "optim_clip_kernel<1>": "clip_resum",
           "optim_clip_kernel<2>": "clip_finished", "optim_step_kernel<0>": "step", "optim_step_kernel<1>": "step_fused_resum",
           "optim_step_kernel<2>": "step_fused_finished"}


def kernel_stats(path, elements, copy_bytes_per_s):
    """the kernel statistics of a traced --once run -> per kernel calls and times in us, the step kernel's rate, the two variants"""
    import csv
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            for needle, key in KERNELS.items():
                if needle in row["Name"]:
                    out[key] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3,
                                "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
    avg = lambda *keys: sum(out[k]["average_us"] for k in keys)      # noqa: E731
    res = {"kernels": out, "source": os.path.basename(path)}
    if "step" in out:
        rate = 28 * elements / (out["step"]["average_us"] * 1e-6)
        res["step_kernel"] = {"traffic_bytes": 28 * elements, "bytes_per_s": rate, "over_copy_rate": rate / copy_bytes_per_s}
    if all(k in out for k in ("clip_resum", "clip_finished", "step_fused_resum", "step_fused_finished", "finish", "norm")):
        res["norm_variants_us"] = {"clip, re-summing": avg("norm", "clip_resum"), "clip, finishing launch": avg("norm", "finish", "clip_finished"),
                                   "fused step, re-summing": avg("norm", "step_fused_resum"),
                                   "fused step, finishing launch": avg("norm", "finish", "step_fused_finished")}
    return res


def all_sets():
    from optim_step_cases import shape_sets
    sets = dict(shape_sets())
    rs = np.random.RandomState(7)
    sets["synthetic_600"] = [dict(name=f"t{i}", shape=[int(n)], bn=i % 3 == 2) for i, n in enumerate(rs.randint(64, 4097, size=600))]
    return sets


def once(rows, dev, steps):
    """for a kernel trace: warm, `steps` steps each of the pair and of clip_and_step, with either way to the coefficient"""
    from modest_amd.utils import optim_step as osd
    for finish in (False, True):
        osd.FINISH_LAUNCH = finish
        w, params = side(rows, dev, 11)
        for _ in range(steps):
            osd.clip_grad_norm_(params, MAX_NORM)
            osd.step(w)
        torch.cuda.synchronize()
        w, params = side(rows, dev, 11)
        for _ in range(steps):
            osd.clip_and_step(w, MAX_NORM)
        torch.cuda.synchronize()
    osd.FINISH_LAUNCH = False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_step_bench.json"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--once", action="store_true", help="run --steps steps of each side and variant on --set and exit (for a kernel trace)")
    ap.add_argument("--set", default="pointpillars_lyft")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--kernel-stats", action="append", default=[], metavar="SET=CSV")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "optim_step_bench needs an MI355X: there is no CPU fallback"
    from optim_step_cases import Wrapper
    from modest_amd.utils import optim_step as osd
    dev = torch.device("cuda:0")
    sets = all_sets()
    if args.once:
        once(sets[args.set], dev, args.steps)
        return
    traced = dict(item.split("=", 1) for item in args.kernel_stats)
    out = []
    for name, rows in sets.items():
        made = {s: side(rows, dev, 11) for s in ("torch", "pair", "fused", "step")}

        def torch_path(w=made["torch"][0], params=made["torch"][1]):
            torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
            Wrapper.step(w)                    # a mul_ per parameter, then torch.optim.Adam.step

        def pair(w=made["pair"][0], params=made["pair"][1]):
            osd.clip_grad_norm_(params, MAX_NORM)
            osd.step(w)

        fns = {"torch": torch_path, "pair": pair, "fused": lambda w=made["fused"][0]: osd.clip_and_step(w, MAX_NORM),
               "step": lambda w=made["step"][0]: osd.step(w)}
        n = {s: calls_for(fn) for s, fn in fns.items()}
        t, h = {s: [] for s in fns}, {s: [] for s in fns}
        for _ in range(args.windows):
            for s, fn in fns.items():
                a, b = window(fn, n[s])
                t[s].append(a)
                h[s].append(b)
        elements = sum(int(np.prod(r["shape"])) for r in rows)
        traffic = 28 * elements
        src = torch.empty((traffic // 2,), dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        copy = lambda: dst.copy_(src)          # noqa: E731
        n_copy = calls_for(copy)
        t_copy = [window(copy, n_copy)[0] for _ in range(args.windows)]
        del src, dst
        row = {"set": name, "tensors": len(rows), "elements": elements, "calls_per_window": n,
               "wall_ms": {s: stats(t[s]) for s in fns}, "host_enqueue_ms": {s: stats(h[s]) for s in fns},
               "launches": {s: launches(fn) for s, fn in fns.items()},
               "synchronising_calls": {s: synchronising_calls(fn) for s, fn in fns.items()},
               "peak_bytes": {s: peak_bytes(fn) for s, fn in fns.items()},
               "torch_over_pair": float(np.median(t["torch"]) / np.median(t["pair"])),
               "torch_over_fused": float(np.median(t["torch"]) / np.median(t["fused"])),
               "step_call": {"traffic_bytes": traffic, "bytes_per_s": traffic / (np.median(t["step"]) * 1e-3)},
               "copy": dict(stats(t_copy), bytes_per_s=traffic / (np.median(t_copy) * 1e-3))}
        row["step_call_over_copy_rate"] = row["step_call"]["bytes_per_s"] / row["copy"]["bytes_per_s"]
        if name in traced:
            row["kernel_trace"] = kernel_stats(traced[name], elements, row["copy"]["bytes_per_s"])
        out.append(row)
        print(json.dumps(row), flush=True)
        del made, fns
        torch.cuda.empty_cache()
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "window_ms": WINDOW_MS, "windows": args.windows, "rows": out}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
