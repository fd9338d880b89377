#!/usr/bin/env python
"""Record tests/golden/pointnet2_stack.npz from the REFERENCE'S OWN KERNEL TEXT executed on the CPU.

Built the way tools/make_golden_pointnet2.py is: the tool reads ``ball_query_gpu.cu``, ``voxel_query_gpu.cu``,
``group_points_gpu.cu`` and ``interpolate_gpu.cu`` of ``pcdet/ops/pointnet2/pointnet2_stack/src`` of a reference checkout
at run time, cuts their ``__global__`` functions out (the launchers stay behind), and compiles them in a temporary
directory with ``g++ -ffp-contract=off`` behind a small stand-in header of our own (``dim3``, ``blockIdx`` / ``threadIdx``,
a sequential ``atomicAdd``, an empty ``curandState`` and a no-op ``curand_init``: the voxel query's random state is dead
code).  The kernels have no barrier and run as plain loops over the grid.  Neither the cut text nor anything compiled
from it is kept: the fixture holds inputs and recorded outputs only.

Furthest point sampling is not recorded again: the tool asserts that the cut text of the stack extension's
``furthest_point_sampling_kernel`` and its ``__update`` helper equals the batch extension's (white space aside), which
tests/golden/pointnet2_batch.npz covers.

The inputs are built so that the contract bites, and the tool asserts that they do (tests/test_pointnet2_stack_cpu.py
asserts the same again from the recorded data); it also checks tests/pointnet2_stack_seq.py against what it recorded.
Every index the reference's kernels are given is in range: they check none.

    python tools/make_golden_pointnet2_stack.py [--ref /path/to/OpenPCDet] [--out tests/golden/pointnet2_stack.npz]
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pointnet2_stack_seq as seq  # noqa: E402
from make_golden_pointnet2 import cut_device_functions, lattice_cloud  # noqa: E402

SRC = "pcdet/ops/pointnet2/pointnet2_stack/src"
BATCH_SRC = "pcdet/ops/pointnet2/pointnet2_batch/src"
FILES = ("ball_query_gpu.cu", "voxel_query_gpu.cu", "group_points_gpu.cu", "interpolate_gpu.cu")

STANDIN = r"""
#include <algorithm>
#include <cmath>
struct dim3 { unsigned x = 1, y = 1, z = 1; };
static thread_local dim3 blockIdx, threadIdx, blockDim, gridDim;
#define __global__
#define __device__
using std::max;
using std::min;
static inline float atomicAdd(float *p, float v) { float o = *p; *p = o + v; return o; }
struct curandState {};
static inline void curand_init(unsigned long long, unsigned long long, unsigned long long, curandState *) {}
"""

# our own driver: what a launch does, as loops (a block of 256 threads, the grid of each launcher's DIVUP shape)
DRIVER = r"""
template <typename Fn> static void run_grid(unsigned gx, unsigned gy, unsigned threads, Fn fn) {
    gridDim.x = gx; gridDim.y = gy; blockDim.x = threads;
    for (unsigned y = 0; y < gy; ++y) for (unsigned x = 0; x < gx; ++x)
        for (unsigned t = 0; t < threads; ++t) {
            blockIdx.x = x; blockIdx.y = y; threadIdx.x = t;
            fn();
        }
}
static unsigned divup(long a, long b) { return (unsigned)((a + b - 1) / b); }
extern "C" {
void emu_ball_query(int B, int M, float radius, int nsample, const float *new_xyz, const int *new_cnt, const float *xyz,
                    const int *xyz_cnt, int *idx) {
    run_grid(divup(M, 256), 1, 256, [&] { ball_query_kernel_stack(B, M, radius, nsample, new_xyz, new_cnt, xyz, xyz_cnt, idx); });
}
void emu_voxel_query(int M, int R1, int R2, int R3, int nsample, float radius, int zr, int yr, int xr, const float *new_xyz,
                     const float *xyz, const int *new_coords, const int *point_indices, int *idx) {
    run_grid(divup(M, 256), 1, 256, [&] {
        voxel_query_kernel_stack(M, R1, R2, R3, nsample, radius, zr, yr, xr, new_xyz, xyz, new_coords, point_indices, idx);
    });
}
void emu_group(int B, int M, int Cn, int nsample, const float *f, const int *fcnt, const int *idx, const int *icnt, float *out) {
    run_grid(divup((long)M * Cn * nsample, 256), 1, 256, [&] { group_points_kernel_stack(B, M, Cn, nsample, f, fcnt, idx, icnt, out); });
}
void emu_group_grad(int B, int M, int Cn, int N, int nsample, const float *go, const int *idx, const int *icnt, const int *fcnt,
                    float *gf) {
    run_grid(divup((long)M * Cn * nsample, 256), 1, 256,
             [&] { group_points_grad_kernel_stack(B, M, Cn, N, nsample, go, idx, icnt, fcnt, gf); });
}
void emu_three_nn(int B, int N, int M, const float *u, const int *ucnt, const float *k, const int *kcnt, float *d2, int *idx) {
    run_grid(divup(N, 256), 1, 256, [&] { three_nn_kernel_stack(B, N, M, u, ucnt, k, kcnt, d2, idx); });
}
void emu_interp(int N, int Cn, const float *f, const int *idx, const float *w, float *out) {
    run_grid(divup(N, 256), Cn, 256, [&] { three_interpolate_kernel_stack(N, Cn, f, idx, w, out); });
}
void emu_interp_grad(int N, int Cn, const float *go, const int *idx, const float *w, float *gf) {
    run_grid(divup(N, 256), Cn, 256, [&] { three_interpolate_grad_kernel_stack(N, Cn, go, idx, w, gf); });
}
}
"""


def function_named(cut, name):
    """the one function of cut_device_functions' output whose head names `name`, white space collapsed"""
    found = []
    for part in ("\n" + cut).split("\n}\n"):
        head = part.split("{", 1)[0]
        if name + "(" in head.replace(" (", "("):
            found.append(" ".join((part + "\n}").split()))
    assert len(found) == 1, (name, len(found))
    return found[0]


def assert_sampling_is_the_batch_kernel(ref):
    cuts = [cut_device_functions(open(os.path.join(ref, d, "sampling_gpu.cu")).read()) for d in (SRC, BATCH_SRC)]
    for name in ("furthest_point_sampling_kernel", "__update"):
        a, b = (function_named(c, name) for c in cuts)
        assert a == b, f"{name}: the stack extension's text is no longer the batch extension's"


def build_emulator(ref, work):
    body = ""
    for f in FILES:
        body += cut_device_functions(open(os.path.join(ref, SRC, f)).read())
    src = os.path.join(work, "emu.cpp")
    with open(src, "w") as fh:
        fh.write(STANDIN + body + DRIVER)
    lib = os.path.join(work, "emu.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-w", src, "-o", lib], check=True)
    return C.CDLL(lib)


def _p(a):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


def _i(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def weights_of(dist2):
    """inverse-distance weights, normalised; an unused slot (inf) weighs 0, a row without any known point is all 0"""
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(np.isfinite(dist2), np.float32(1.0) / (np.sqrt(dist2) + np.float32(1e-8)), np.float32(0))
        s = w.sum(axis=1, keepdims=True)
        return (w / np.where(s > 0, s, np.float32(1))).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference/downstream/OpenPCDet")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "pointnet2_stack.npz"))
    args = ap.parse_args()
    assert_sampling_is_the_batch_kernel(args.ref)
    rs = np.random.RandomState(20231)
    rec = {}
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)   # noqa: E731
    with tempfile.TemporaryDirectory() as work:
        emu = build_emulator(args.ref, work)

        # ---- ball query: B = 3 with unequal counts and a scan without queries, lattice clouds and radius 0.5 (pairs at
        # exactly d2 == radius^2), centres on and far off the cloud; B = 1 on a plain cloud
        xcnt, qcnt = _i([300, 40, 260]), _i([90, 0, 70])
        xyz = lattice_cloud(rs, 600, (1.5, 1.5, 0.5), 0.25, 40)
        xs = np.cumsum(xcnt) - xcnt
        cen = np.concatenate([np.concatenate([xyz[xs[b] + rs.permutation(xcnt[b])[:qcnt[b] - 20]],
                                              rs.uniform(20, 30, (20, 3)).astype(np.float32)])[rs.permutation(qcnt[b])]
                              for b in (0, 2)]).astype(np.float32)
        xyz1 = rs.uniform(-3, 3, (500, 3)).astype(np.float32)
        cen1 = np.concatenate([rs.uniform(-3.7, 3.7, (120, 3)), rs.uniform(10, 12, (10, 3))]).astype(np.float32)
        bq_cases = [(xyz, xcnt, cen, qcnt, 0.5, 8), (xyz1, _i([500]), cen1, _i([130]), 1.2, 8)]
        for i, (xyz, xcnt, cen, qcnt, radius, ns) in enumerate(bq_cases):
            B, M = len(xcnt), len(cen)
            assert xcnt.sum() == len(xyz) and qcnt.sum() == M
            given = rs.randint(0, 5, (M, ns)).astype(np.int32) if i == 0 else np.zeros((M, ns), dtype=np.int32)
            idx = given.copy()
            emu.emu_ball_query(B, M, C.c_float(radius), ns, _p(cen), _p(qcnt), _p(xyz), _p(xcnt), _p(idx))
            assert np.array_equal(seq.ball_query(radius, ns, xyz, xcnt, cen, qcnt, given), idx), i
            scan = seq.scan_of_rows(M, qcnt)
            r2 = np.float32(radius) * np.float32(radius)
            d2 = seq._d2(cen[:, None, :], xyz[None, :, :])
            own = scan[:, None] == seq.scan_of_rows(len(xyz), xcnt)[None, :]
            cnt = ((d2 < r2) & own).sum(axis=1)
            assert (cnt == 0).any() and ((cnt > 0) & (cnt < ns)).any() and (cnt > ns).any(), i
            assert (idx[cnt == 0, 0] == -1).all() and np.array_equal(idx[cnt == 0, 1:], given[cnt == 0, 1:])
            if i == 0:
                assert ((d2 == r2) & own).any() and (qcnt == 0).any() and len(set(xcnt)) == 3
                assert ((d2 < r2) & ~own).any()                       # a hit in another scan: the counts decide
            rec.update({f"bq{i}_xyz": xyz, f"bq{i}_xyz_cnt": xcnt, f"bq{i}_new_xyz": cen, f"bq{i}_new_cnt": qcnt,
                        f"bq{i}_given": given, f"bq{i}_idx": idx, f"bq{i}_radius": np.float64(radius), f"bq{i}_nsample": np.int64(ns)})

        # ---- voxel query: a non-cubic grid, one point per occupied cell ON the lattice of cell centres (distances are
        # multiples of the cell size: pairs at exactly d2 == radius^2, which this query accepts), three different ranges,
        # queries on every corner and face of the grid and inside it, an empty region for rows without a hit
        B, R1, R2, R3, vs = 2, 5, 12, 9, np.float32(0.5)
        occ = rs.rand(B, R1, R2, R3) < 0.45
        occ[:, :, :3, :4] = False                                      # nothing near one corner
        bzyx = np.argwhere(occ)                                        # ascending (b, z, y, x): scan after scan
        xyz = np.ascontiguousarray(bzyx[:, [3, 2, 1]].astype(np.float32) * vs, dtype=np.float32)
        vcnt = _i(np.bincount(bzyx[:, 0], minlength=B))
        table = np.full((B, R1, R2, R3), -1, dtype=np.int32)
        table[tuple(bzyx.T)] = np.arange(len(bzyx), dtype=np.int32)
        corners = [(b, z, y, x) for b in range(B) for z in (0, R1 - 1) for y in (0, R2 - 1) for x in (0, R3 - 1)]
        faces = [(b, z, y, x) for b in range(B) for z, y, x in ((0, 6, 4), (R1 - 1, 6, 4), (2, 0, 4), (2, R2 - 1, 4), (2, 6, 0), (2, 6, R3 - 1))]
        inner = [(rs.randint(B), rs.randint(R1), rs.randint(R2), rs.randint(R3)) for _ in range(60)]
        coords = _i(sorted(corners + faces + inner))                  # scan after scan
        new_xyz = np.ascontiguousarray(coords[:, [3, 2, 1]].astype(np.float32) * vs, dtype=np.float32)
        off = rs.rand(len(coords)) < 0.5                               # half of the queries off the lattice
        new_xyz[off] += rs.uniform(-0.2, 0.2, (int(off.sum()), 3)).astype(np.float32)
        ranges, radius, ns = (1, 3, 2), 1.0, 6
        given = rs.randint(0, 5, (len(coords), ns)).astype(np.int32)
        idx = given.copy()
        emu.emu_voxel_query(len(coords), R1, R2, R3, ns, C.c_float(radius), *ranges, _p(new_xyz), _p(xyz), _p(coords), _p(table), _p(idx))
        assert np.array_equal(seq.voxel_query(ranges, radius, ns, xyz, new_xyz, coords, table, given), idx)
        strict = seq.voxel_query(ranges, np.nextafter(np.float32(radius), np.float32(0)), ns, xyz, new_xyz, coords, table, given)
        assert not np.array_equal(strict, idx)                         # equality is a hit, and it shows
        full = seq.voxel_query(ranges, radius, 10 ** 4, xyz, new_xyz, coords, table)
        cnt = np.where(full[:, 0] < 0, 0, [len(np.unique(r)) for r in full])
        assert (cnt == 0).any() and ((cnt > 0) & (cnt < ns)).any() and (cnt > ns).any()
        assert len(set(ranges)) == 3 and len({R1, R2, R3}) == 3
        rec.update(vq_xyz=xyz, vq_xyz_cnt=vcnt, vq_new_xyz=new_xyz, vq_new_coords=coords, vq_point_indices=table, vq_given=given,
                   vq_idx=idx, vq_ranges=np.asarray(ranges, dtype=np.int64), vq_radius=np.float64(radius), vq_nsample=np.int64(ns))

        # ---- three nearest neighbours: B = 4 on lattices (equal distances): a scan without known points (not the last:
        # its rows' indices point at the next scan's first row), a scan without queries, a scan with two known; B = 1
        ucnt, kcnt = _i([100, 30, 0, 40]), _i([60, 0, 25, 2])
        nn_cases = [(lattice_cloud(rs, int(ucnt.sum()), (1, 1, 0.5), 0.25, 0), ucnt, lattice_cloud(rs, int(kcnt.sum()), (1, 1, 0.5), 0.25, 8), kcnt),
                    (rs.uniform(-4, 4, (300, 3)).astype(np.float32), _i([300]), rs.uniform(-4, 4, (1100, 3)).astype(np.float32), _i([1100]))]
        for i, (unk, ucnt, kn, kcnt) in enumerate(nn_cases):
            d2 = np.full((len(unk), 3), -1, dtype=np.float32)
            idx = np.full((len(unk), 3), -1, dtype=np.int32)
            emu.emu_three_nn(len(ucnt), len(unk), len(kn), _p(unk), _p(ucnt), _p(kn), _p(kcnt), _p(d2), _p(idx))
            sd, si = seq.three_nn(unk, ucnt, kn, kcnt)
            assert np.array_equal(si, idx) and np.array_equal(bits(sd), bits(d2)), i
            assert idx.min() >= 0 and idx.max() < len(kn)
            if i == 0:
                fin = np.isfinite(d2)
                assert ((d2[:, 0] == d2[:, 1]) & fin[:, 1]).any() and ((d2[:, 1] == d2[:, 2]) & fin[:, 2]).any()
                assert (kcnt == 0).any() and (kcnt[ucnt > 0] == 0).any() and ((kcnt > 0) & (kcnt < 3) & (ucnt > 0)).any() and (ucnt == 0).any()
            rec.update({f"nn{i}_unknown": unk, f"nn{i}_unknown_cnt": ucnt, f"nn{i}_known": kn, f"nn{i}_known_cnt": kcnt,
                        f"nn{i}_dist2": d2, f"nn{i}_idx": idx})

        # ---- group and its gradient: the ball query's rows (B = 3, padded rows repeat a destination), and B = 1 with
        # random indices, its gradient from a non-zero buffer
        gidx0 = rec["bq0_idx"].copy()
        gidx0[gidx0[:, 0] < 0] = 0                                      # as the reference's Python side does
        gr_cases = [(rec["bq0_xyz_cnt"], gidx0, rec["bq0_new_cnt"], 5, False),
                    (_i([350]), rs.randint(0, 120, (60, 9)).astype(np.int32), _i([60]), 4, True)]
        for i, (fcnt, gidx, icnt, Cn, nonzero) in enumerate(gr_cases):
            N, (M, S), B = int(fcnt.sum()), gidx.shape, len(fcnt)
            feat = rs.randn(N, Cn).astype(np.float32)
            out = np.zeros((M, Cn, S), dtype=np.float32)
            emu.emu_group(B, M, Cn, S, _p(feat), _p(fcnt), _p(gidx), _p(icnt), _p(out))
            assert np.array_equal(bits(seq.group(feat, fcnt, gidx, icnt)), bits(out)), i
            go = rs.randn(M, Cn, S).astype(np.float32)
            given = (rs.randn(N, Cn) * (rs.rand(N, Cn) < 0.5)).astype(np.float32) if nonzero else np.zeros((N, Cn), dtype=np.float32)
            grad = given.copy()
            emu.emu_group_grad(B, M, Cn, N, S, _p(go), _p(gidx), _p(icnt), _p(fcnt), _p(grad))
            exact = seq.group_grad(go, gidx, icnt, fcnt, N)
            assert seq.check_grad(grad, given, exact) == 0 and exact[2].max() > 1 and (exact[2] == 0).any(), i
            rec.update({f"gr{i}_features": feat, f"gr{i}_features_cnt": fcnt, f"gr{i}_idx": gidx, f"gr{i}_idx_cnt": icnt,
                        f"gr{i}_out": out, f"gr{i}_grad_out": go, f"gr{i}_given": given, f"gr{i}_grad": grad})

        # ---- three-interpolate and its gradient on the first three-NN case, the gradient from a non-zero buffer
        tidx, Cn = rec["nn0_idx"], 6
        w = weights_of(rec["nn0_dist2"])
        Mk, N = len(rec["nn0_known"]), len(tidx)
        feat = rs.randn(Mk, Cn).astype(np.float32)
        out = np.zeros((N, Cn), dtype=np.float32)
        emu.emu_interp(N, Cn, _p(feat), _p(tidx), _p(w), _p(out))
        assert np.array_equal(bits(seq.three_interpolate(feat, tidx, w)), bits(out)) and np.isfinite(out).all()
        go = rs.randn(N, Cn).astype(np.float32)
        given = (rs.randn(Mk, Cn) * (rs.rand(Mk, Cn) < 0.5)).astype(np.float32)
        grad = given.copy()
        emu.emu_interp_grad(N, Cn, _p(go), _p(tidx), _p(w), _p(grad))
        exact = seq.three_interpolate_grad(go, tidx, w, Mk)
        assert seq.check_grad(grad, given, exact) == 0 and exact[2].max() > 1 and (given != 0).any()
        rec.update(ti_features=feat, ti_idx=tidx, ti_weight=w, ti_out=out, ti_grad_out=go, ti_given=given, ti_grad=grad)

    np.savez_compressed(args.out, **rec)
    print(args.out, os.path.getsize(args.out), "bytes,", len(rec), "arrays")


if __name__ == "__main__":
    main()
