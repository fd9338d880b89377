#!/usr/bin/env python
"""Record tests/golden/pointnet2_batch.npz from the REFERENCE'S OWN KERNEL TEXT executed on the CPU.

The tool reads the four ``pcdet/ops/pointnet2/pointnet2_batch/src/*_gpu.cu`` files of a reference checkout at run
time, cuts their ``__global__`` / ``__device__`` functions out (the launchers stay behind: g++ cannot parse
``<<<>>>``), and compiles them in a temporary directory with ``g++ -std=c++20 -ffp-contract=off`` behind a small
stand-in header of our own (``dim3``, thread-local ``blockIdx`` / ``threadIdx``, ``__shared__`` -> ``static``, a
sequential ``atomicAdd``).  The barrier-free kernels run as plain loops over the grid; the furthest-point-sampling
kernel runs on one ``std::thread`` per CUDA thread with a ``std::barrier`` for ``__syncthreads()``.  That kernel
reads ``dists_i[0]`` and lets the next round overwrite it with no barrier in between; on CPU threads the race is
real, so ONE extra barrier is inserted after that read (nothing else of the text changes).  Neither the cut text nor
anything compiled from it is kept: the fixture holds inputs and recorded outputs only.

The inputs are built so that the contract bites, and the tool asserts that they do (tests/test_pointnet2_cpu.py
asserts the same again from the recorded data); it also checks tests/pointnet2_seq.py against what it recorded.

    python tools/make_golden_pointnet2.py [--ref /path/to/OpenPCDet] [--out tests/golden/pointnet2_batch.npz]
"""
import argparse
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pointnet2_seq as seq  # noqa: E402

SRC = "pcdet/ops/pointnet2/pointnet2_batch/src"
FILES = ("sampling_gpu.cu", "ball_query_gpu.cu", "group_points_gpu.cu", "interpolate_gpu.cu")

STANDIN = r"""
#include <algorithm>
#include <barrier>
#include <cmath>
#include <thread>
#include <vector>
struct dim3 { unsigned x = 1, y = 1, z = 1; };
static thread_local dim3 blockIdx, threadIdx, blockDim, gridDim;
#define __global__
#define __device__
#define __shared__ static
using std::max;
using std::min;
static inline float atomicAdd(float *p, float v) { float o = *p; *p = o + v; return o; }
static std::barrier<> *g_barrier = nullptr;
static inline void __syncthreads() { g_barrier->arrive_and_wait(); }
"""

# our own driver: what a launch does, as loops (a block of 256 threads, the grid of each launcher's DIVUP shape)
DRIVER = r"""
template <typename Fn> static void run_grid(unsigned gx, unsigned gy, unsigned gz, unsigned threads, Fn fn) {
    gridDim.x = gx; gridDim.y = gy; gridDim.z = gz; blockDim.x = threads;
    for (unsigned z = 0; z < gz; ++z) for (unsigned y = 0; y < gy; ++y) for (unsigned x = 0; x < gx; ++x)
        for (unsigned t = 0; t < threads; ++t) {
            blockIdx.x = x; blockIdx.y = y; blockIdx.z = z; threadIdx.x = t;
            fn();
        }
}
static unsigned divup(long a, long b) { return (unsigned)((a + b - 1) / b); }
template <unsigned BS> static void fps_block(int b, int n, int m, const float *xyz, float *temp, int *idx) {
    for (int cloud = 0; cloud < b; ++cloud) {
        std::barrier<> bar(BS);
        g_barrier = &bar;
        std::vector<std::thread> th;
        for (unsigned t = 0; t < BS; ++t)
            th.emplace_back([=] {
                blockIdx.x = cloud; threadIdx.x = t; blockDim.x = BS; gridDim.x = b;
                furthest_point_sampling_kernel<BS>(b, n, m, xyz, temp, idx);
            });
        for (auto &t : th) t.join();
    }
}
extern "C" {
int emu_fps(int bs, int b, int n, int m, const float *xyz, float *temp, int *idx) {
    switch (bs) {
        case 1024: fps_block<1024>(b, n, m, xyz, temp, idx); break;
        case 512: fps_block<512>(b, n, m, xyz, temp, idx); break;
        case 256: fps_block<256>(b, n, m, xyz, temp, idx); break;
        case 128: fps_block<128>(b, n, m, xyz, temp, idx); break;
        case 64: fps_block<64>(b, n, m, xyz, temp, idx); break;
        default: return -1;
    }
    return 0;
}
void emu_gather(int b, int c, int n, int m, const float *p, const int *idx, float *out) {
    run_grid(divup(m, 256), c, b, 256, [&] { gather_points_kernel_fast(b, c, n, m, p, idx, out); });
}
void emu_gather_grad(int b, int c, int n, int m, const float *g, const int *idx, float *gp) {
    run_grid(divup(m, 256), c, b, 256, [&] { gather_points_grad_kernel_fast(b, c, n, m, g, idx, gp); });
}
void emu_ball_query(int b, int n, int m, float radius, int nsample, const float *new_xyz, const float *xyz, int *idx) {
    run_grid(divup(m, 256), b, 1, 256, [&] { ball_query_kernel_fast(b, n, m, radius, nsample, new_xyz, xyz, idx); });
}
void emu_group(int b, int c, int n, int np, int ns, const float *p, const int *idx, float *out) {
    run_grid(divup((long)np * ns, 256), c, b, 256, [&] { group_points_kernel_fast(b, c, n, np, ns, p, idx, out); });
}
void emu_group_grad(int b, int c, int n, int np, int ns, const float *g, const int *idx, float *gp) {
    run_grid(divup((long)np * ns, 256), c, b, 256, [&] { group_points_grad_kernel_fast(b, c, n, np, ns, g, idx, gp); });
}
void emu_three_nn(int b, int n, int m, const float *u, const float *k, float *d2, int *idx) {
    run_grid(divup(n, 256), b, 1, 256, [&] { three_nn_kernel_fast(b, n, m, u, k, d2, idx); });
}
void emu_interp(int b, int c, int m, int n, const float *p, const int *idx, const float *w, float *out) {
    run_grid(divup(n, 256), c, b, 256, [&] { three_interpolate_kernel_fast(b, c, m, n, p, idx, w, out); });
}
void emu_interp_grad(int b, int c, int n, int m, const float *g, const int *idx, const float *w, float *gp) {
    run_grid(divup(n, 256), c, b, 256, [&] { three_interpolate_grad_kernel_fast(b, c, n, m, g, idx, w, gp); });
}
}
"""


def cut_device_functions(text):
    """the __global__ / __device__ functions of one .cu file, each from its first line to the closing brace in column 0"""
    lines, out, i = text.splitlines(), [], 0
    while i < len(lines):
        line = lines[i]
        start = line.startswith(("__global__", "__device__")) or (
            line.startswith("template") and i + 1 < len(lines) and lines[i + 1].startswith(("__global__", "__device__")))
        if not start:
            i += 1
            continue
        j = i
        while lines[j].rstrip() != "}":
            j += 1
        out.extend(lines[i:j + 1])
        i = j + 1
    return "\n".join(out) + "\n"


def build_emulator(ref, work):
    body = ""
    for f in FILES:
        body += cut_device_functions(open(os.path.join(ref, SRC, f)).read())
    read = "old = dists_i[0];"
    assert body.count(read) == 1, "the furthest-point-sampling kernel no longer reads its result where it did"
    body = body.replace(read, read + " __syncthreads();")   # the one barrier the emulation needs (see the docstring)
    src = os.path.join(work, "emu.cpp")
    with open(src, "w") as fh:
        fh.write(STANDIN + body + DRIVER)
    lib = os.path.join(work, "emu.so")
    subprocess.run(["g++", "-std=c++20", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-pthread", "-w", src, "-o", lib],
                   check=True)
    return C.CDLL(lib)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _i(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def ref_block_size(n):
    """opt_n_threads of the reference, in its own floating-point form"""
    return max(min(1 << int(np.log(float(n)) / np.log(2.0)), 1024), 1)


def lattice_cloud(rs, n, extent, step, dup):
    """points rounded to a coarse lattice (equal distances) with `dup` of them exact repeats of earlier ones"""
    p = rs.uniform(-1, 1, (n, 3)) * np.asarray(extent)
    p = np.round(p / step) * step
    src = rs.randint(0, n, dup)
    dst = rs.randint(0, n, dup)
    p[dst] = p[src]
    return p.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference/downstream/OpenPCDet")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "pointnet2_batch.npz"))
    args = ap.parse_args()
    rs = np.random.RandomState(20221)
    rec = {}
    with tempfile.TemporaryDirectory() as work:
        emu = build_emulator(args.ref, work)

        # ---- furthest point sampling: tie cases at bs = 64, 512, 1024; m = N; m = 1; one cloud without lattice
        fps_cases = [
            ("tie64", lattice_cloud(rs, 2 * 100, (2, 2, 1), 0.5, 30).reshape(2, 100, 3), 100, True),     # m = N
            ("tie512", lattice_cloud(rs, 2 * 700, (4, 4, 1), 0.5, 100).reshape(2, 700, 3), 160, True),
            ("tie1024", lattice_cloud(rs, 2 * 2500, (6, 6, 1.5), 0.5, 300).reshape(2, 2500, 3), 150, True),
            ("m1", rs.uniform(-5, 5, (2, 300, 3)).astype(np.float32), 1, False),
            ("plain", rs.uniform(-5, 5, (1, 1500, 3)).astype(np.float32), 120, False),
        ]
        for i, (name, xyz, m, tie) in enumerate(fps_cases):
            B, N, _ = xyz.shape
            bs = ref_block_size(N)
            assert bs == seq.fps_block_size(N)
            temp = np.full((B, N), 1e10, dtype=np.float32)
            if m == 1:
                temp[:] = rs.uniform(1, 2, temp.shape)     # m = 1 must leave temp alone
            temp0 = temp.copy()
            idx = np.full((B, m), -7, dtype=np.int32)
            assert emu.emu_fps(bs, B, N, m, _p(xyz), _p(temp), _p(idx)) == 0
            got, gtemp = seq.furthest_point_sample(xyz, m, temp0)
            assert np.array_equal(got, idx) and np.array_equal(gtemp.view(np.uint32), temp.view(np.uint32)), name
            if tie:
                low, _ = seq.furthest_point_sample(xyz, m, temp0, tie="lowest")
                steps = seq.fps_tie_steps(xyz, m)
                for b in range(B):
                    assert steps[b][0] > 0 and steps[b][1] > 0, (name, steps)
                    assert not np.array_equal(low[b], idx[b]), name
                print(name, "bs", bs, "tie steps (across residues, inside one)", steps)
            rec[f"fps{i}_xyz"], rec[f"fps{i}_temp0"], rec[f"fps{i}_idx"], rec[f"fps{i}_temp"] = xyz, temp0, idx, temp
        rec["fps_names"] = np.array([c[0] for c in fps_cases])

        # ---- ball query: lattice cloud, radius 0.5 (pairs at exactly d2 == radius^2), centres off the cloud; a plain case
        xyz = lattice_cloud(rs, 2 * 600, (1.5, 1.5, 0.5), 0.25, 40).reshape(2, 600, 3)
        cen = np.concatenate([xyz[:, rs.permutation(600)[:150]], rs.uniform(20, 30, (2, 50, 3)).astype(np.float32)], axis=1)
        cen2 = np.concatenate([rs.uniform(-3.7, 3.7, (2, 120, 3)), rs.uniform(10, 12, (2, 10, 3))], axis=1).astype(np.float32)
        bq_cases = [(xyz, _f(cen), 0.5, 8), (rs.uniform(-3, 3, (2, 500, 3)).astype(np.float32), cen2, 1.2, 8)]
        for i, (xyz, cen, radius, ns) in enumerate(bq_cases):
            B, N, _ = xyz.shape
            M = cen.shape[1]
            idx = np.zeros((B, M, ns), dtype=np.int32)
            emu.emu_ball_query(B, N, M, C.c_float(radius), ns, _p(cen), _p(xyz), _p(idx))
            assert np.array_equal(seq.ball_query(radius, ns, xyz, cen), idx), i
            d2 = seq._d2(cen[:, :, None, :], xyz[:, None, :, :])
            r2 = np.float32(radius) * np.float32(radius)
            cnt = (d2 < r2).sum(axis=2)
            assert (cnt == 0).any() and ((cnt > 0) & (cnt < ns)).any() and (cnt > ns).any(), i
            if i == 0:
                assert (d2 == r2).any()
            rec[f"bq{i}_xyz"], rec[f"bq{i}_new_xyz"], rec[f"bq{i}_idx"] = xyz, cen, idx
            rec[f"bq{i}_radius"], rec[f"bq{i}_nsample"] = np.float64(radius), np.int64(ns)

        # ---- three nearest neighbours: lattice (equal distances), m = 2, plain
        nn_cases = [(lattice_cloud(rs, 2 * 300, (1, 1, 0.5), 0.25, 0).reshape(2, 300, 3),
                     lattice_cloud(rs, 2 * 90, (1, 1, 0.5), 0.25, 10).reshape(2, 90, 3)),
                    (rs.uniform(-1, 1, (2, 70, 3)).astype(np.float32), rs.uniform(-1, 1, (2, 2, 3)).astype(np.float32)),
                    (rs.uniform(-4, 4, (1, 1100, 3)).astype(np.float32), rs.uniform(-4, 4, (1, 1300, 3)).astype(np.float32))]
        for i, (unk, kn) in enumerate(nn_cases):
            B, n, _ = unk.shape
            m = kn.shape[1]
            d2 = np.full((B, n, 3), -1, dtype=np.float32)
            idx = np.full((B, n, 3), -1, dtype=np.int32)
            emu.emu_three_nn(B, n, m, _p(unk), _p(kn), _p(d2), _p(idx))
            sd, si = seq.three_nn(unk, kn)
            assert np.array_equal(si, idx) and np.array_equal(sd.view(np.uint32), d2.view(np.uint32)), i
            if i == 0:
                assert (d2[:, :, 0] == d2[:, :, 1]).any() and (d2[:, :, 1] == d2[:, :, 2]).any()
            rec[f"nn{i}_unknown"], rec[f"nn{i}_known"], rec[f"nn{i}_dist2"], rec[f"nn{i}_idx"] = unk, kn, d2, idx

        # ---- gather / group / interpolate and the three gradients (one of each from a non-zero buffer)
        B, Cn, N, m = 2, 5, 400, 130
        pts = rs.randn(B, Cn, N).astype(np.float32)
        idx = rs.randint(0, N, (B, m)).astype(np.int32)
        idx[:, :20] = idx[:, 20:40]                        # repeated destinations
        out = np.zeros((B, Cn, m), dtype=np.float32)
        emu.emu_gather(B, Cn, N, m, _p(pts), _p(idx), _p(out))
        assert np.array_equal(seq.gather(pts, idx).view(np.uint32), out.view(np.uint32))
        go = rs.randn(B, Cn, m).astype(np.float32)
        given = (rs.randn(B, Cn, N) * (rs.rand(B, Cn, N) < 0.5)).astype(np.float32)
        grad = given.copy()
        emu.emu_gather_grad(B, Cn, N, m, _p(go), _p(idx), _p(grad))
        assert seq.check_grad(grad, given, seq.gather_grad(go, idx, N)) == 0
        rec.update(ga_points=pts, ga_idx=idx, ga_out=out, ga_grad_out=go, ga_given=given, ga_grad=grad)

        B, Cn, N, P, S = 2, 4, 350, 60, 9
        pts = rs.randn(B, Cn, N).astype(np.float32)
        idx = rs.randint(0, 120, (B, P, S)).astype(np.int32)   # two thirds of the rows are never reached
        out = np.zeros((B, Cn, P, S), dtype=np.float32)
        emu.emu_group(B, Cn, N, P, S, _p(pts), _p(idx), _p(out))
        assert np.array_equal(seq.group(pts, idx).view(np.uint32), out.view(np.uint32))
        go = rs.randn(B, Cn, P, S).astype(np.float32)
        grad = np.zeros((B, Cn, N), dtype=np.float32)
        emu.emu_group_grad(B, Cn, N, P, S, _p(go), _p(idx), _p(grad))
        assert seq.check_grad(grad, None, seq.group_grad(go, idx, N)) == 0
        rec.update(gr_points=pts, gr_idx=idx, gr_out=out, gr_grad_out=go, gr_grad=grad)

        B, Cn, mk, n = 2, 6, 90, 300
        pts = rs.randn(B, Cn, mk).astype(np.float32)
        unk, kn = rec["nn0_unknown"], rec["nn0_known"]
        idx = rec["nn0_idx"]
        w = 1.0 / (np.sqrt(rec["nn0_dist2"]) + np.float32(1e-8))
        w = (w / w.sum(axis=2, keepdims=True)).astype(np.float32)
        out = np.zeros((B, Cn, n), dtype=np.float32)
        emu.emu_interp(B, Cn, mk, n, _p(pts), _p(idx), _p(w), _p(out))
        assert np.array_equal(seq.three_interpolate(pts, idx, w).view(np.uint32), out.view(np.uint32))
        go = rs.randn(B, Cn, n).astype(np.float32)
        grad = np.zeros((B, Cn, mk), dtype=np.float32)
        emu.emu_interp_grad(B, Cn, n, mk, _p(go), _p(idx), _p(w), _p(grad))
        assert seq.check_grad(grad, None, seq.three_interpolate_grad(go, idx, w, mk)) == 0
        rec.update(ti_points=pts, ti_idx=idx, ti_weight=w, ti_out=out, ti_grad_out=go, ti_grad=grad)

    np.savez_compressed(args.out, **rec)
    print(args.out, os.path.getsize(args.out), "bytes,", len(rec), "arrays")


if __name__ == "__main__":
    main()
