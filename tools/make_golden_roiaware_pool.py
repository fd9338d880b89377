#!/usr/bin/env python
"""Record tests/golden/roiaware_pool.npz from the REFERENCE'S OWN KERNEL TEXT executed on the CPU.

The tool reads ``pcdet/ops/roiaware_pool3d/src/roiaware_pool3d_kernel.cu`` of a reference checkout at run time and cuts
out, by name, the predicate (``lidar_to_local_coords``, ``check_pt_in_box3d``), the four forward kernels
(``generate_pts_mask_for_box3d``, ``collect_inside_pts_for_box3d``, ``roiaware_maxpool3d``, ``roiaware_avgpool3d``) and
the two backward kernels.  They are compiled in a temporary directory with ``g++ -ffp-contract=off`` behind a small
stand-in header of our own and run as plain loops over the launchers' grids, the box index (``blockIdx.z``) outermost:
that is the order in which the backward's ``atomicAdd`` -- here a plain ``+=`` -- adds, and the order DESIGN.md section
7j fixes.  The voxel kernel's ``min(max(unsigned, int))`` has no meaning under g++; the stand-in header supplies those
two overloads with CUDA's meaning (the int is cast to unsigned).  Neither the cut text nor anything compiled from it is
kept: the fixture holds inputs and recorded outputs only.

As in tools/make_golden_roipool.py every heading is chosen by rejection so that the host C library's ``cosf`` / ``sinf``
and the contract's rounded double functions agree on it.  The host's float -> int conversion differs from the contract's
for NaN and out-of-range quotients, so the tool asserts that every recorded quotient is finite and inside int range;
those cases are covered against the restatement instead (tests/test_roiaware_pool_cpu.py, tests/test_gpu_roiaware_pool.py).
The inputs are built so that the contract bites, and the tool asserts that they do (tests/roiaware_seq.py
``fixture_cases``); it also checks the numpy restatement against what it recorded.

    python tools/make_golden_roiaware_pool.py [--ref /path/to/OpenPCDet] [--out tests/golden/roiaware_pool.npz]
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
sys.path.insert(0, ROOT)
import roiaware_seq as seq  # noqa: E402
from make_golden_roipool import cut_functions, heading_ok, headings, local_points  # noqa: E402

AWARE_SRC = "pcdet/ops/roiaware_pool3d/src/roiaware_pool3d_kernel.cu"
FUNCS = ("lidar_to_local_coords", "check_pt_in_box3d", "generate_pts_mask_for_box3d", "collect_inside_pts_for_box3d",
         "roiaware_maxpool3d", "roiaware_avgpool3d", "roiaware_maxpool3d_backward", "roiaware_avgpool3d_backward")
POOLED_SENTINEL = np.float32(-12345.5)
ARGMAX_SENTINEL = np.int32(-7)
LIST_SENTINEL = np.int32(-9)

STANDIN = r"""
#include <math.h>
#include <vector>
struct dim3 { unsigned x = 1, y = 1, z = 1; };
static thread_local dim3 blockIdx, threadIdx, blockDim, gridDim;
#define __global__
#define __device__
// CUDA's mixed overloads: the int is cast to unsigned
static inline unsigned max(unsigned a, int b) { return a > (unsigned)b ? a : (unsigned)b; }
static inline unsigned min(unsigned a, int b) { return a < (unsigned)b ? a : (unsigned)b; }
// one thread at a time: an atomic add is an add
static inline float atomicAdd(float *p, float v) { float old = *p; *p = old + v; return old; }
"""

# our own driver: what the two launchers do, as loops (blocks of 256 threads, the grids of the launchers' DIVUP shapes)
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
extern "C" {
void emu_forward(int n, int p, int c, int m, int ox, int oy, int oz, const float *rois, const float *pts,
                 const float *feat, int *argmax, int *lists, float *pooled, int method) {
    std::vector<int> mask((size_t)n * p + 1, -1);
    run_grid(divup(p, 256), n, 1, 256, [&] { generate_pts_mask_for_box3d(n, p, ox, oy, oz, rois, pts, mask.data()); });
    run_grid(divup(n, 256), 1, 1, 256, [&] { collect_inside_pts_for_box3d(n, p, m, ox, oy, oz, mask.data(), lists); });
    if (method == 0)
        run_grid(divup(ox * oy * oz, 256), c, n, 256,
                 [&] { roiaware_maxpool3d(n, p, c, m, ox, oy, oz, feat, lists, pooled, argmax); });
    else
        run_grid(divup(ox * oy * oz, 256), c, n, 256,
                 [&] { roiaware_avgpool3d(n, p, c, m, ox, oy, oz, feat, lists, pooled); });
}
void emu_backward(int n, int ox, int oy, int oz, int c, int m, const int *lists, const int *argmax,
                  const float *grad_out, float *grad_in, int method) {
    if (method == 0)
        run_grid(divup(ox * oy * oz, 256), c, n, 256,
                 [&] { roiaware_maxpool3d_backward(n, c, ox, oy, oz, argmax, grad_out, grad_in); });
    else
        run_grid(divup(ox * oy * oz, 256), c, n, 256,
                 [&] { roiaware_avgpool3d_backward(n, c, ox, oy, oz, m, lists, grad_out, grad_in); });
}
}
"""


def build_emulator(ref, work):
    body = "\n".join(cut_functions(open(os.path.join(ref, AWARE_SRC)).read(), FUNCS)) + "\n"
    src = os.path.join(work, "emu.cpp")
    with open(src, "w") as fh:
        fh.write(STANDIN + body + DRIVER)
    lib = os.path.join(work, "emu.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-w", src, "-o", lib], check=True)
    return C.CDLL(lib)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def voxel_point(box, out, ijk, frac=(0.5, 0.5, 0.5)):
    """a point of an UNROTATED box at `frac` of the way through voxel ijk, as float32"""
    b = box.astype(np.float64)
    loc = [(-0.5 + (ijk[a] + frac[a]) / out[a]) * b[3 + a] for a in range(3)]
    return np.array([b[0] + loc[0], b[1] + loc[1], b[2] + loc[2]], dtype=np.float32)


def crafted_scene(rs):
    """grid (3, 5, 2), max_pts 5, C = 4.  Box 0 is unrotated with extents (3, 5, 2) at the origin: its voxels are unit
    cubes and q = l + d / 2 exactly, so counts, faces and margins can be placed by hand.  Boxes 1-3 overlap at one site
    (rotated, headings by rejection): their points are shared by three boxes.  Box 4 is far from every point."""
    out, max_pts, c = (3, 5, 2), 5, 4
    hd = headings(rs, 12)
    n = 157
    pts = np.stack([rs.uniform(200, 260, n), rs.uniform(-30, 30, n), rs.uniform(-2, 1, n)], axis=1).astype(np.float32)
    feat = rs.randn(n, c).astype(np.float32)
    box0 = np.array([0, 0, 0, 3, 5, 2, 0], dtype=np.float32)
    k = iter(range(3, n))

    def put(ijk, count, frac=None):
        idx = []
        for _ in range(count):
            i = next(k)
            f = rs.uniform(0.2, 0.8, 3) if frac is None else frac
            pts[i] = voxel_point(box0, out, ijk, f)
            idx.append(i)
        return idx

    put((0, 0, 0), 1)                                   # count 1
    put((1, 0, 0), max_pts - 2)                         # count max_pts - 2
    put((2, 0, 0), max_pts - 1)                         # count max_pts - 1: full, nothing dropped
    over = put((0, 1, 1), max_pts + 2)                  # count > max_pts - 1: three dropped ...
    feat[over[-1]] = np.float32(50.0) + np.arange(c, dtype=np.float32)   # ... the largest values among them
    ties = put((1, 1, 0), 3)                            # equal maxima: slots 1 and 2 tie in channel 0, slot 0 is lower
    feat[ties[0], 0], feat[ties[1], 0], feat[ties[2], 0] = -1.0, 2.5, 2.5
    feat[ties[0], 1], feat[ties[1], 1], feat[ties[2], 1] = 0.0, -0.0, 0.0     # +0 and -0 are equal: the first wins
    dead = put((2, 1, 1), 2)                            # channel 0 only -inf / NaN: nobody wins; channel 1 NaN then a number
    feat[dead[0], 0], feat[dead[1], 0] = -np.inf, np.nan
    feat[dead[0], 1], feat[dead[1], 1] = np.nan, -3.0
    feat[dead[0], 2], feat[dead[1], 2] = np.nan, np.nan
    # q exactly an integer: lx = -0.5 -> q_x = 1.0, on the face between voxels 0 and 1 -> voxel 1
    pts[next(k)] = (-0.5, 2.25, 0.25)
    # on / beyond the high faces, inside the 1e-5 margin: q >= out is clamped to out - 1
    pts[next(k)] = (np.float32(1.5) + np.float32(5e-6), 2.25, 0.25)
    pts[next(k)] = (1.25, np.float32(2.5) + np.float32(7e-6), 0.25)
    pts[next(k)] = (1.25, 2.25, 1.0)                    # on the top face: q_z = 2.0 = out_z
    # in the low margin: -1 < q < 0 -> 0
    pts[next(k)] = (np.float32(-1.5) - np.float32(5e-6), -2.25, -0.25)
    pts[next(k)] = (-1.25, np.float32(-2.5) - np.float32(7e-6), -0.75)
    rois = [box0]
    site = np.array([40.0, -12.0, 0.3])
    for j, size in enumerate(((3.9, 1.6, 1.56), (4.4, 2.0, 1.8), (3.0, 3.0, 2.2))):
        rois.append(np.concatenate([site + 0.1 * j, size, [hd[4 + j]]]).astype(np.float32))
    shared = [next(k) for _ in range(40)]
    pts[shared] = local_points(rs, rois[1], len(shared), 0.95)
    rois.append(np.array([-300, 5, 0, 4, 2, 2, hd[8]], dtype=np.float32))
    pts[0] = voxel_point(box0, out, (0, 4, 1))          # first and last index of the cloud are inside points
    pts[n - 1] = voxel_point(box0, out, (2, 4, 0))
    return np.stack(rois), pts, feat, out, max_pts


def random_scene(rs, n_box, n_pts, c, out, max_pts, spread=4.0):
    hd = headings(rs, 12)
    pts = np.stack([rs.uniform(-spread, spread, n_pts), rs.uniform(-spread, spread, n_pts),
                    rs.uniform(-1.5, 1.5, n_pts)], axis=1).astype(np.float32)
    rois = np.zeros((n_box, 7), dtype=np.float32)
    rois[:, 0:2] = rs.uniform(-2, 2, (n_box, 2))
    rois[:, 2] = rs.uniform(-0.5, 0.5, n_box)
    rois[:, 3:6] = rs.uniform(2.0, 6.0, (n_box, 3))
    rois[:, 6] = hd[rs.randint(4, len(hd), n_box)]
    return rois, pts, rs.randn(n_pts, c).astype(np.float32), out, max_pts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference/downstream/OpenPCDet")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "roiaware_pool.npz"))
    args = ap.parse_args()
    rs = np.random.RandomState(20241)
    scenes = [("crafted",) + crafted_scene(rs),
              ("single", *random_scene(rs, 1, 203, 1, (1, 1, 1), 128, spread=2.0)),
              ("cubic", *random_scene(rs, 3, 131, 5, (4, 4, 4), 2)),
              ("nolist", *random_scene(rs, 2, 70, 1, (2, 2, 2), 1))]
    rec = {}
    with tempfile.TemporaryDirectory() as work:
        emu = build_emulator(args.ref, work)
        for name, rois, pts, feat, out, max_pts in scenes:
            n, p, c = len(rois), len(pts), feat.shape[1]
            for rz in rois[:, 6]:
                assert heading_ok(rz), (name, rz)
            mask, _ = seq.voxel_ids(pts, rois, out)
            for q in seq.local_q(pts, rois, out):
                assert np.isfinite(q[mask]).all() and (np.abs(q[mask]) < 2.0 ** 31).all(), name
            shape = (n,) + tuple(out)
            lists_given = np.full(shape + (max_pts,), LIST_SENTINEL, dtype=np.int32)
            lists_given[..., 0] = 0                      # the reference counts on from the given word
            pooled_given = np.full(shape + (c,), POOLED_SENTINEL, dtype=np.float32)
            argmax_given = np.full(shape + (c,), ARGMAX_SENTINEL, dtype=np.int32)
            grad_out = rs.randn(*(shape + (c,))).astype(np.float32)
            grad_in_given = rs.randn(p, c).astype(np.float32)
            got = {}
            for method, tag in ((0, "max"), (1, "avg")):
                lists, pooled, argmax = lists_given.copy(), pooled_given.copy(), argmax_given.copy()
                emu.emu_forward(n, p, c, max_pts, *out, _p(rois), _p(pts), _p(feat), _p(argmax), _p(lists), _p(pooled), method)
                grad_in = grad_in_given.copy()
                emu.emu_backward(n, *out, c, max_pts, _p(lists), _p(argmax), _p(grad_out), _p(grad_in), method)
                sl, sp, sa = seq.forward(rois, pts, feat, out, max_pts, method, lists_given, pooled_given, argmax_given)
                assert np.array_equal(sl, lists), (name, tag)
                assert np.array_equal(sp.view(np.uint32), pooled.view(np.uint32)), (name, tag)
                assert np.array_equal(sa, argmax), (name, tag)
                sg = seq.backward(lists, argmax, grad_out, grad_in_given, method)
                assert np.array_equal(sg.view(np.uint32), grad_in.view(np.uint32)), (name, tag)
                got[tag] = (lists, pooled, argmax, grad_in)
            assert np.array_equal(got["max"][0], got["avg"][0])
            counts = got["max"][0][..., 0]
            print(name, "N", n, "npoints", p, "C", c, "grid", out, "max_pts", max_pts, "inside", mask.sum(axis=1).tolist(),
                  "largest count", int(counts.max()))
            rec.update({f"{name}_rois": rois, f"{name}_pts": pts, f"{name}_feat": feat,
                        f"{name}_out": np.array(out, dtype=np.int64), f"{name}_lists_given": lists_given,
                        f"{name}_pooled_given": pooled_given, f"{name}_argmax_given": argmax_given,
                        f"{name}_grad_out": grad_out, f"{name}_grad_in_given": grad_in_given,
                        f"{name}_lists": got["max"][0]})
            for tag in ("max", "avg"):
                rec.update({f"{name}_pooled_{tag}": got[tag][1], f"{name}_argmax_{tag}": got[tag][2],
                            f"{name}_grad_in_{tag}": got[tag][3]})
    cases = seq.fixture_cases(rec)
    for k, v in cases.items():
        print("%-60s %s" % (k, v))
    assert all(cases.values()), [k for k, v in cases.items() if not v]
    np.savez_compressed(args.out, **rec)
    size = os.path.getsize(args.out)
    limit = os.path.getsize(os.path.join(ROOT, "tests", "golden", "pointnet2_batch.npz"))
    print(args.out, size, "bytes,", len(rec), "arrays")
    assert size <= limit, (size, limit)


if __name__ == "__main__":
    main()
