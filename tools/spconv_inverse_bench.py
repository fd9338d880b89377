#!/usr/bin/env python
"""Time the inverse sparse convolutions (modest_amd.utils.spconv_inverse on modest_amd/csrc/spconv_inverse.hip) on the
three SparseInverseConv3d layers of PartA2's UNetV2 and write profiles/spconv_inverse_bench.json.

Data: tools/spconv_bench.py's own clouds -- B = 4 synthetic Lyft-shape clouds voxelised on the device at
[0.05, 0.05, 0.1] (sparse shape [41, 1600, 1808]) with both caps, 16 000 and 40 000 voxels per cloud -- and its eight
rulebooks, built beforehand.

Timed: the three layers 64 -> 64 on spconv4, 64 -> 32 on spconv3 and 32 -> 16 on spconv2, each on a fixed random input
on its rulebook's coarse sites, forward and forward + backward, all three per pass; and the class order of the three
rulebooks on its own.

Three sides:
  classes   the class tiles (modest_spconv_gather_gemm_classes), order="classes"
  rows      modest_spconv_gather_gemm on nbr_t, order="rows": the kernel the library had before, and the yardstick
  composed  spconv's own algorithm from stock PyTorch-ROCm operators -- per offset index_select -> mm -> index_add_ --,
            autograd for the backward pass; `compose_forward` is checked on the CPU by tests/test_spconv_inverse_cpu.py
"classes" and "rows" differ in the forward only; the backward is the same launches on either.

All sides run in this process on the same inputs and weights; each is warmed up; a window is a fixed number of whole
passes timed with the host clock around work that ends in one device synchronise; the sides alternate window by window;
median, minimum and maximum of the windows are written.  Before any time is reported the outputs are compared: classes
and rows byte for byte, the composition inside a relative difference that is written down.

    python tools/spconv_inverse_bench.py [--out profiles/spconv_inverse_bench.json] [--windows 7] [--points 100000]
"""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (indice_key, cin, cout): the inverse convolutions of UNetV2, in the order the decoder runs them
LAYERS = [("spconv4", 64, 64), ("spconv3", 64, 32), ("spconv2", 32, 16)]


def compose_pairs(nbr_t):
    """per offset the (coarse rows, fine rows) of the present pairs, from the rulebook's map nbr_t (K, N_fine)"""
    pairs = []
    for k in range(nbr_t.shape[0]):
        i = torch.nonzero(nbr_t[k] >= 0).flatten()
        pairs.append((nbr_t[k, i].long(), i))
    return pairs


def compose_forward(x, weight, bias, pairs, n_fine):
    """spconv's gather -> GEMM -> scatter-add from stock operators; x on the coarse rows, weight (K, Cin, Cout)"""
    out = x.new_zeros((n_fine, weight.shape[2]))
    for k, (o, i) in enumerate(pairs):
        if len(i):
            out = out.index_add(0, i, x.index_select(0, o) @ weight[k])
    return out if bias is None else out + bias


def forward_bench():
    spec = importlib.util.spec_from_file_location("spconv_bench", os.path.join(ROOT, "tools", "spconv_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def window(fn, passes):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(passes):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / passes


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)),
            "windows_ms": [float(x) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spconv_inverse_bench.json"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--points", type=int, default=100_000, help="points of the largest cloud")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/spconv_inverse_bench.py needs an MI355X: there is no CPU path")
    from modest_amd import ops, synth
    fb = forward_bench()
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    world = synth.make_world(0)
    clouds = [synth.sample_frame(world, 1000 + k, args.points - 977 * k, synth._pose_matrix(5.0 * k, 0.0, 0.01), synth.default_l2e(),
                                 mobiles=synth.make_mobiles(k, 5.0 * k)) for k in range(args.batch)]
    points = torch.from_numpy(np.concatenate([np.concatenate([np.full((len(c), 1), b, dtype=np.float32), c], axis=1)
                                              for b, c in enumerate(clouds)])).to(dev)
    rows = []
    for mode, cap in fb.CAPS.items():
        vox, coords, num, _, counts = ops.voxelize(points, fb.VOXEL, fb.RANGE, fb.P, cap, batch_size=args.batch)
        books = fb.build_rulebooks(ops, coords, args.batch)
        gen = torch.Generator().manual_seed(0)
        layers = []
        for key, cin, cout in LAYERS:
            rb = books[key]
            x = torch.randn((rb.n_out, cin), generator=gen).to(dev)
            w = ((torch.rand((rb.kvol, cin, cout), generator=gen) - 0.5) * (2.0 / np.sqrt(rb.kvol * cin))).to(dev)
            dy = torch.randn((rb.n_in, cout), generator=gen).to(dev)
            layers.append(dict(key=key, rb=rb, x=x, w=w, dy=dy, pairs=compose_pairs(rb.nbr_t)))
            ops.spconv_class_order(rb)
        row = {"case": f"B={args.batch} {mode} cap {cap}",
               "shape": {"voxels per cloud": counts.tolist(),
                         "rows per layer (coarse in, fine out)": {l["key"]: [l["rb"].n_out, l["rb"].n_in] for l in layers}}}
        # the outputs first: classes and rows byte for byte, the composition close
        worst = 0.0
        for l in layers:
            a = ops.spconv_inverse_forward(l["x"], l["w"], None, l["rb"], order="classes")
            b = ops.spconv_inverse_forward(l["x"], l["w"], None, l["rb"], order="rows")
            c = compose_forward(l["x"], l["w"], None, l["pairs"], l["rb"].n_in)
            if not torch.equal(a.view(torch.int32), b.view(torch.int32)):
                raise SystemExit(f"{l['key']}: the class tiles and the rows differ")
            worst = max(worst, float((a - c).abs().max()) / max(float(a.abs().max()), 1e-30))
        row["classes_equal_rows_bytes"] = True
        row["composed max_abs_difference_over_max_abs"] = worst

        def fwd(order):
            def run():
                for l in layers:
                    ops.spconv_inverse_forward(l["x"], l["w"], None, l["rb"], order=order)
            return run

        def fwd_bwd(order):
            def run():
                for l in layers:
                    ops.spconv_inverse_forward(l["x"], l["w"], None, l["rb"], order=order)
                    ops.spconv_inverse_backward(l["x"], l["w"], l["dy"], l["rb"], need_bias_grad=False)
            return run

        def composed(backward):
            def run():
                for l in layers:
                    if backward:
                        x, w = l["x"].detach().requires_grad_(True), l["w"].detach().requires_grad_(True)
                        compose_forward(x, w, None, l["pairs"], l["rb"].n_in).backward(l["dy"])
                    else:
                        with torch.no_grad():
                            compose_forward(l["x"], l["w"], None, l["pairs"], l["rb"].n_in)
            return run

        def class_orders():
            for l in layers:
                l["rb"].class_order = None
                ops.spconv_class_order(l["rb"])
        sides = {"class order": class_orders}
        for order in ("classes", "rows"):
            sides[f"{order} forward"] = fwd(order)
            sides[f"{order} forward+backward"] = fwd_bwd(order)
        sides["composed forward"] = composed(False)
        sides["composed forward+backward"] = composed(True)
        per = {}
        for k, fn in sides.items():
            fn()
            t = window(fn, 1)
            per[k] = int(min(200, max(2, np.ceil(200.0 / max(t, 1e-3)))))
        ms = {k: [] for k in sides}
        for _ in range(args.windows):          # alternating windows
            for k, fn in sides.items():
                ms[k].append(window(fn, per[k]))
        for k in sides:
            row[k] = dict(stats(ms[k]), passes_per_window=per[k])
        for what in ("forward", "forward+backward"):
            row[f"rows_over_classes {what}"] = row[f"rows {what}"]["median_ms"] / row[f"classes {what}"]["median_ms"]
            row[f"composed_over_classes {what}"] = row[f"composed {what}"]["median_ms"] / row[f"classes {what}"]["median_ms"]
            row[f"classes windows wholly below rows {what}"] = row[f"classes {what}"]["max_ms"] < row[f"rows {what}"]["min_ms"]
        print(json.dumps({k: ({"median_ms": v["median_ms"], "min_ms": v["min_ms"], "max_ms": v["max_ms"]}
                              if isinstance(v, dict) and "median_ms" in v else v) for k, v in row.items()}), flush=True)
        rows.append(row)
        del layers, books
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "windows": args.windows,
           "note": "milliseconds per pass over the three inverse convolutions of UNetV2 (64->64 on spconv4, 64->32 on spconv3, "
                   "32->16 on spconv2), host clock around whole passes ending in a device synchronise; the sides alternate "
                   "window by window; 'rows' is modest_spconv_gather_gemm on nbr_t, the yardstick; 'class order' builds the "
                   "class order of the three rulebooks",
           "cases": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
