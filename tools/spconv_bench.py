#!/usr/bin/env python
"""Time the sparse 3-D convolutions (modest_amd.utils.spconv on modest_amd/csrc/spconv.hip) on the layer sequence of
SECOND's VoxelBackBone8x and write profiles/spconv_bench.json.

Data: B = 4 synthetic Lyft-shape clouds voxelised on the device at [0.05, 0.05, 0.1] on [0, -40, -3, 90.4, 40, 1]
(second_dynamic_obj.yaml: sparse shape [41, 1600, 1808]) with both caps, 16 000 and 40 000 voxels per cloud; the
features are the voxel means.

Timed: the twelve convolutions with eval-mode BatchNorm1d and ReLU between them, forward and forward + backward, on
rulebooks built beforehand; and, separately, building the eight rulebooks of the sequence.

Yardstick: spconv's own algorithm composed from stock PyTorch-ROCm operators in this file -- per kernel offset
index_select -> mm -> index_add_ on the same rulebook, autograd for the backward pass.  It adds in the order in which
atomics land, so it cannot meet the fixed-order contract; it is what a port without kernels of its own would run.
`compose_forward` is checked on the CPU against float64 sums by tests/test_spconv_cpu.py.

Both sides run in this process on the same inputs and weights; each is warmed up; a window is a fixed number of whole
passes timed with the host clock around work that ends in a device synchronise; the sides alternate window by window;
median, minimum and maximum of the windows are written.  Before any time is reported the two outputs are compared.

    python tools/spconv_bench.py [--out profiles/spconv_bench.json] [--windows 7] [--points 100000]
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

VOXEL, RANGE, P = [0.05, 0.05, 0.1], [0, -40, -3, 90.4, 40, 1], 5
SHAPE = [41, 1600, 1808]
CAPS = {"train": 16000, "test": 40000}
# (subm, cin, cout, kernel, stride, padding, indice_key)
LAYERS = [(True, 4, 16, 3, 1, 1, "subm1"), (True, 16, 16, 3, 1, 1, "subm1"),
          (False, 16, 32, 3, 2, 1, "spconv2"), (True, 32, 32, 3, 1, 1, "subm2"), (True, 32, 32, 3, 1, 1, "subm2"),
          (False, 32, 64, 3, 2, 1, "spconv3"), (True, 64, 64, 3, 1, 1, "subm3"), (True, 64, 64, 3, 1, 1, "subm3"),
          (False, 64, 64, 3, 2, (0, 1, 1), "spconv4"), (True, 64, 64, 3, 1, 1, "subm4"), (True, 64, 64, 3, 1, 1, "subm4"),
          (False, 64, 128, (3, 1, 1), (2, 1, 1), 0, "spconv_down2")]


def compose_pairs(nbr):
    """per offset the (input rows, output rows) of the present neighbours, from the rulebook's map (K, N_out)"""
    pairs = []
    for k in range(nbr.shape[0]):
        o = torch.nonzero(nbr[k] >= 0).flatten()
        pairs.append((nbr[k, o].long(), o))
    return pairs


def compose_forward(x, weight, bias, pairs, n_out):
    """spconv's gather -> GEMM -> scatter-add from stock operators; weight (K, Cin, Cout)"""
    out = x.new_zeros((n_out, weight.shape[2]))
    for k, (i, o) in enumerate(pairs):
        if len(o):
            out = out.index_add(0, o, x.index_select(0, i) @ weight[k])
    return out if bias is None else out + bias


def build_rulebooks(ops, indices, batch):
    """the eight rulebooks of the sequence -> {key: rulebook}"""
    books, shape = {}, SHAPE
    for subm, cin, cout, k, s, p, key in LAYERS:
        if key not in books:
            books[key] = ops.spconv_rulebook(indices, batch, shape, k, s, p, subm)
        indices, shape = books[key].out_indices, books[key].out_shape
    return books


class Chain(torch.nn.Module):
    def __init__(self, books, composed):
        super().__init__()
        self.books, self.composed = books, composed
        self.weights = torch.nn.ParameterList()
        self.bns = torch.nn.ModuleList()
        gen = torch.Generator().manual_seed(0)
        for subm, cin, cout, k, s, p, key in LAYERS:
            kvol = books[key].kvol
            self.weights.append(torch.nn.Parameter((torch.rand((kvol, cin, cout), generator=gen) - 0.5) * (2.0 / np.sqrt(kvol * cin))))
            self.bns.append(torch.nn.BatchNorm1d(cout, eps=1e-3, momentum=0.01))
        self.pairs = {key: compose_pairs(b.nbr) for key, b in books.items()} if composed else None

    def forward(self, x):
        from modest_amd.utils.spconv.conv import _SparseConvFunction
        for (subm, cin, cout, k, s, p, key), w, bn in zip(LAYERS, self.weights, self.bns):
            if self.composed:
                x = compose_forward(x, w, None, self.pairs[key], self.books[key].n_out)
            else:
                x = _SparseConvFunction.apply(x, w, None, self.books[key])
            x = torch.relu(bn(x))
        return x


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spconv_bench.json"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--points", type=int, default=100_000, help="points of the largest cloud")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/spconv_bench.py needs an MI355X: there is no CPU path")
    from modest_amd import ops, synth
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    world = synth.make_world(0)
    clouds = [synth.sample_frame(world, 1000 + k, args.points - 977 * k, synth._pose_matrix(5.0 * k, 0.0, 0.01), synth.default_l2e(),
                                 mobiles=synth.make_mobiles(k, 5.0 * k)) for k in range(args.batch)]
    points = torch.from_numpy(np.concatenate([np.concatenate([np.full((len(c), 1), b, dtype=np.float32), c], axis=1)
                                              for b, c in enumerate(clouds)])).to(dev)
    rows = []
    for mode, cap in CAPS.items():
        vox, coords, num, _, counts = ops.voxelize(points, VOXEL, RANGE, P, cap, batch_size=args.batch)
        feats = (vox.sum(1) / num.float()[:, None]).contiguous()
        books = build_rulebooks(ops, coords, args.batch)
        nets = {"op": Chain(books, False).to(dev).eval(), "composed": Chain(books, True).to(dev).eval()}
        nets["composed"].load_state_dict(nets["op"].state_dict())
        with torch.no_grad():
            res = {k: n(feats) for k, n in nets.items()}
        scale = float(res["op"].abs().max())
        row = {"case": f"B={args.batch} {mode} cap {cap}",
               "shape": {"voxels per cloud": counts.tolist(),
                         "rows per rulebook": {key: [b.n_in, b.n_out] for key, b in books.items()}},
               "max_abs_difference_over_max_abs": float((res["op"] - res["composed"]).abs().max()) / max(scale, 1e-30)}

        def fwd(net):
            def run():
                with torch.no_grad():
                    net(feats)
            return run

        def fwd_bwd(net):
            def run():
                net.zero_grad(set_to_none=True)
                net(feats).sum().backward()
            return run
        sides = {"rulebooks": lambda: build_rulebooks(ops, coords, args.batch)}
        for k, n in nets.items():
            sides[f"{k} forward"] = fwd(n)
            sides[f"{k} forward+backward"] = fwd_bwd(n)
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
            row[f"composed_over_op {what}"] = row[f"composed {what}"]["median_ms"] / row[f"op {what}"]["median_ms"]
        print(json.dumps({k: ({"median_ms": v["median_ms"], "min_ms": v["min_ms"], "max_ms": v["max_ms"]}
                              if isinstance(v, dict) and "median_ms" in v else v) for k, v in row.items()}), flush=True)
        rows.append(row)
        del nets, books, res
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "windows": args.windows,
           "note": "milliseconds per pass over the twelve convolutions of VoxelBackBone8x (eval BatchNorm1d and ReLU between), "
                   "host clock around whole passes ending in a device synchronise; the op and the composition of stock "
                   "operators alternate window by window; 'rulebooks' builds the eight rulebooks of the sequence",
           "cases": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
