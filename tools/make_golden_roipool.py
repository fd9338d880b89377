#!/usr/bin/env python
"""Record tests/golden/roipool.npz from the REFERENCE'S OWN KERNEL TEXT executed on the CPU.

The tool reads ``pcdet/ops/roipoint_pool3d/src/roipoint_pool3d_kernel.cu`` and
``pcdet/ops/roiaware_pool3d/src/roiaware_pool3d_kernel.cu`` of a reference checkout at run time and cuts out, by name,
the three pooling kernels with ``lidar_to_local_coords`` and ``check_pt_in_box3d`` from the first file and
``points_in_boxes_kernel`` from the second (nothing else of that file: its voxel kernel does not compile under g++; the
two files' copies of the predicate are checked to be the same text).  They are compiled in a temporary directory with
``g++ -ffp-contract=off`` behind a small stand-in header of our own and run as plain loops over the grid (no kernel
here has a barrier).  Neither the cut text nor anything compiled from it is kept: the fixture holds inputs and recorded
outputs only.

The emulation's ``cos`` / ``sin`` on a float are the host C library's ``cosf`` / ``sinf``; the contract's are the double
functions rounded once.  Every heading of the fixture is therefore chosen by rejection so that
the two agree on it (asserted), and the recorded outputs are valid under both flavours.  The inputs are built so that
the contract bites, and the tool asserts that they do (tests/roipool_seq.py ``fixture_cases``;
tests/test_roipool_cpu.py asserts the same again from the recorded data); it also checks the numpy restatement against
what it recorded.

    python tools/make_golden_roipool.py [--ref /path/to/OpenPCDet] [--out tests/golden/roipool.npz]
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
sys.path.insert(0, ROOT)
import roipool_seq as seq  # noqa: E402
from modest_amd.kitti_infos import host_cos_sin_f32  # noqa: E402

POOL_SRC = "pcdet/ops/roipoint_pool3d/src/roipoint_pool3d_kernel.cu"
AWARE_SRC = "pcdet/ops/roiaware_pool3d/src/roiaware_pool3d_kernel.cu"
POOL_FUNCS = ("lidar_to_local_coords", "check_pt_in_box3d", "assign_pts_to_box3d", "get_pooled_idx", "roipool3d_forward")
AWARE_FUNCS = ("points_in_boxes_kernel",)
SENTINEL = np.float32(-12345.5)

STANDIN = r"""
#include <math.h>
#include <vector>
struct dim3 { unsigned x = 1, y = 1, z = 1; };
static thread_local dim3 blockIdx, threadIdx, blockDim, gridDim;
#define __global__
#define __device__
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
void emu_roipool(int b, int n, int m, int c, int s, const float *xyz, const float *boxes, const float *feat,
                 float *pooled, int *flag) {
    std::vector<int> assign((size_t)b * n * m + 1, -7), idx((size_t)b * m * s + 1, 0);
    run_grid(divup(n, 256), m, b, 256, [&] { assign_pts_to_box3d(b, n, m, xyz, boxes, assign.data()); });
    run_grid(divup(m, 256), b, 1, 256, [&] { get_pooled_idx(b, n, m, s, assign.data(), idx.data(), flag); });
    run_grid(divup(s, 256), m, b, 256, [&] { roipool3d_forward(b, n, m, c, s, xyz, idx.data(), feat, pooled, flag); });
}
void emu_points_in_boxes(int b, int m, int n, const float *boxes, const float *pts, int *box_idx) {
    run_grid(divup(n, 256), b, 1, 256, [&] { points_in_boxes_kernel(b, m, n, boxes, pts, box_idx); });
}
}
"""


def cut_functions(text, names):
    """the named __global__ / __device__ functions of one .cu file, each from its first line to the closing brace in
    column 0, in the file's order"""
    lines, out, i, found = text.splitlines(), [], 0, []
    while i < len(lines):
        line = lines[i]
        if not line.startswith(("__global__", "__device__")):
            i += 1
            continue
        j = i
        while lines[j].rstrip() != "}":
            j += 1
        name = line.split("(")[0].split()[-1]
        if name in names:
            out.append("\n".join(lines[i:j + 1]))
            found.append(name)
        i = j + 1
    assert sorted(found) == sorted(names), (found, names)
    return out


def build_emulator(ref, work):
    pool = cut_functions(open(os.path.join(ref, POOL_SRC)).read(), POOL_FUNCS)
    aware_text = open(os.path.join(ref, AWARE_SRC)).read()
    assert cut_functions(aware_text, POOL_FUNCS[:2]) == pool[:2], "the two files' predicates are no longer the same text"
    body = "\n".join(pool + cut_functions(aware_text, AWARE_FUNCS)) + "\n"
    src = os.path.join(work, "emu.cpp")
    with open(src, "w") as fh:
        fh.write(STANDIN + body + DRIVER)
    lib = os.path.join(work, "emu.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-w", src, "-o", lib], check=True)
    return C.CDLL(lib)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- headings ------------------------------------------------------------------------------------------------------
def heading_ok(rz):
    """glibc cosf / sinf of -rz equal the rounded double cos / sin"""
    rz = np.float32(rz)
    hc, hs = host_cos_sin_f32(np.array([rz], dtype=np.float32))
    dc, ds = seq.cos_sin_f32(np.array([rz], dtype=np.float32))
    return hc.view(np.uint32)[0] == dc.view(np.uint32)[0] and hs.view(np.uint32)[0] == ds.view(np.uint32)[0]


SPECIAL = [0.0, np.float32(np.pi / 2), -np.float32(np.pi / 2), np.float32(np.pi)]


def headings(rs, count):
    """the four special headings first (as floats; they must pass as they are), then negative ones, ones beyond +-2 pi
    and generic ones, each redrawn until the two trig flavours agree on it"""
    out = []
    for v in SPECIAL:
        assert heading_ok(v), f"the two trig flavours differ at the special heading {v!r}"
        out.append(np.float32(v))
    lo_hi = [(-3.0, -0.1), (6.5, 9.0), (-9.5, -6.5)]
    while len(out) < count:
        lo, hi = lo_hi[len(out) % 3] if len(out) < 10 else (-np.pi, np.pi)
        v = np.float32(rs.uniform(lo, hi))
        if heading_ok(v):
            out.append(v)
    return np.array(out, dtype=np.float32)


def local_points(rs, box, count, frac=0.8):
    """`count` points well inside `box` (within frac of every half extent), as float32"""
    b = box.astype(np.float64)
    loc = rs.uniform(-frac, frac, (count, 3)) * b[3:6] / 2.0
    c, s = np.cos(b[6]), np.sin(b[6])
    x = loc[:, 0] * c - loc[:, 1] * s + b[0]
    y = loc[:, 0] * s + loc[:, 1] * c + b[1]
    return np.stack([x, y, loc[:, 2] + b[2]], axis=1).astype(np.float32)


def find_wrong_dx(rs):
    """a box length whose float32 bound dx * 0.5f + 1e-5f rounds below the double bound"""
    while True:
        dx = np.float32(rs.uniform(1.0, 5.0))
        if seq.f32_bound_wrong(dx):
            return dx


def up_f32(d):
    f = np.float32(d)
    return f if np.float64(f) >= d else np.nextafter(f, np.float32(np.inf))


def crafted_cloud(rs, n, s, batch):
    """one cloud of the crafted scene: (xyz (n, 3), boxes (M, 7), flag_given (M,)).  Every box sits on its own site far
    from the others, its inside points at chosen indices; the rest of the cloud is background nobody contains."""
    assert n >= 400 and n % 64
    hd = list(headings(rs, 24))
    xyz = np.stack([rs.uniform(200, 260, n), rs.uniform(-30, 30, n), rs.uniform(-2, 1, n)], axis=1).astype(np.float32)
    boxes, flags = [], []

    def site(i):
        return np.array([12.0 * (i % 8) - 40.0, 15.0 * (i // 8) - 20.0, rs.uniform(-1, 1)])

    def add(idx, rz=None, size=(3.9, 1.6, 1.56), flag=0, frac=0.8):
        i = len(boxes)
        box = np.concatenate([site(i), size, [hd[i % len(hd)] if rz is None else rz]]).astype(np.float32)
        idx = np.asarray(idx, dtype=np.int64)
        xyz[idx] = local_points(rs, box, len(idx), frac)
        boxes.append(box)
        flags.append(flag)
        return i

    add([])                                                     # 0: empty
    add([0])                                                    # 1: cnt 1, at index 0
    add([63, 64])                                               # 2: cnt 2, first 63, last 64
    add(list(range(100, 100 + s - 2)) + [255])                  # 3: cnt S - 1, last 255
    add(range(256, 256 + s))                                    # 4: cnt S, first 256
    add(list(range(120, 120 + s)) + [n - 1])                    # 5: cnt S + 1, last N - 1 (beyond the S that are taken)
    big = add(range(140, 140 + 5 * s), size=(6.0, 3.0, 2.0))    # 6: cnt >> S
    add(range(n - 40, n - 30))                                  # 7: all inside points in the last 64
    # 8: overlaps box 6 (same site, shifted by a third of its length): they share points
    b8 = boxes[big].copy()
    b8[0] += np.float32(2.0)
    boxes.append(b8), flags.append(0)
    add(range(272, 272 + s), flag=1)                            # 9: pre-set flag on a non-empty box
    add([290, 291], flag=3)                                     # 10: another pre-set value
    # 11-13: boxes at heading 0 with cx = cy = 0, stacked in z: lx == x exactly
    zs = 20.0
    for j, kind in enumerate(("zface", "side", "wrong")):
        dx = find_wrong_dx(rs) if kind == "wrong" else np.float32(rs.uniform(2, 4))
        box = np.array([0, 0, zs, dx, 2.0, 1.5, 0], dtype=np.float32)
        zs += 10.0
        boxes.append(box), flags.append(0)
        k = list(range(300 + 8 * j, 300 + 8 * j + 6))
        D = np.float64(dx) / 2.0 + seq.MARGIN
        up = up_f32(D)
        dn = np.nextafter(up, np.float32(-np.inf))
        if kind == "zface":
            top, bot = np.float32(box[2] + np.float32(0.75)), np.float32(box[2] - np.float32(0.75))
            xyz[k[0]] = (0.3, 0.1, top)                                               # on the top face: inside
            xyz[k[1]] = (-0.2, 0.2, bot)                                              # on the bottom face: inside
            xyz[k[2]] = (0.3, 0.1, np.nextafter(top, np.float32(np.inf)))             # one float above: outside
            xyz[k[3]] = (0.3, 0.1, np.nextafter(bot, np.float32(-np.inf)))            # one float below: outside
            xyz[k[4]] = (0.1, 0.1, box[2])
            xyz[k[5]] = (0.1, -0.1, box[2])
        elif kind == "side":
            xyz[k[0]] = (dn, 0.1, box[2])                                             # one float inside the +x face
            xyz[k[1]] = (up, 0.1, box[2])                                             # the first float outside it
            xyz[k[2]] = (-dn, -0.1, box[2])
            xyz[k[3]] = (-up, -0.1, box[2])
            xyz[k[4]] = (0.1, np.nextafter(up_f32(1.0 + seq.MARGIN), np.float32(-np.inf)), box[2])   # same for +y
            xyz[k[5]] = (0.1, up_f32(1.0 + seq.MARGIN), box[2])
        else:
            f32sum = dx * np.float32(0.5) + np.float32(1e-5)
            assert np.float64(f32sum) < D
            xyz[k[0]] = (f32sum, 0.1, box[2])              # inside by the double rule, outside by a float32 rule
            xyz[k[1]] = (-f32sum, -0.1, box[2])
            xyz[k[2]] = (up, 0.1, box[2])
            xyz[k[3]] = (0.0, 0.0, box[2])
            xyz[k[4]] = (0.2, 0.0, box[2])
            xyz[k[5]] = (0.0, 0.3, box[2])
    # 14: (cloud 0 only) a box that holds the origin, ahead of the zero boxes
    if batch == 0:
        boxes.append(np.array([0.1, -0.1, 0.05, 1.0, 1.0, 0.5, hd[5]], dtype=np.float32)), flags.append(0)
    else:
        add([292, 293])
    xyz[330] = (0.0, 0.0, 0.0)                                   # the origin: in a zero box
    xyz[331] = (5e-6, -5e-6, 0.0)                                # within the margin of it
    xyz[332] = (2e-5, 0.0, 0.0)                                  # outside the margin
    xyz[333] = (0.0, 0.0, 1e-30)                                 # off its z face
    # 15, 16: NaN boxes -- a NaN centre holds nothing; a NaN dz does not reject (the z comparison is false)
    nb = np.array([np.nan, 0, 0, 2, 2, 2, 0], dtype=np.float32)
    boxes.append(nb), flags.append(0)
    add([294, 295, 296])
    boxes[-1][5] = np.nan
    # 17, 18: zero (padding) boxes
    boxes.append(np.zeros(7, dtype=np.float32)), flags.append(0)
    boxes.append(np.zeros(7, dtype=np.float32)), flags.append(0)
    # NaN points: a NaN x is in no box; a NaN z does not reject
    k = 297
    xyz[k] = local_points(rs, boxes[1], 1)[0]
    xyz[k, 0] = np.nan
    add([299, k + 1])                                            # 19: holds the point whose z is NaN
    xyz[k + 1, 2] = np.nan
    return xyz, np.stack(boxes), np.array(flags, dtype=np.int32)


def random_scene(rs, n, m):
    """boxes scattered through a dense cloud, headings from the accepted set; the last two boxes are zero padding"""
    hd = headings(rs, 16)
    xyz = np.stack([rs.uniform(-8, 8, (2, n)), rs.uniform(-8, 8, (2, n)), rs.uniform(-1.5, 1.5, (2, n))], axis=2)
    boxes = np.zeros((2, m, 7))
    boxes[:, :, 0:2] = rs.uniform(-8, 8, (2, m, 2))
    boxes[:, :, 2] = rs.uniform(-1, 1, (2, m))
    boxes[:, :, 3:6] = rs.uniform(0.5, 8.0, (2, m, 3))
    boxes[:, :, 6] = hd[rs.randint(0, len(hd), (2, m))]
    boxes[:, -2:] = 0
    boxes[0, 0, 0] = 100.0                                        # one box off the cloud
    return xyz.astype(np.float32), boxes.astype(np.float32), np.zeros((2, m), dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference/downstream/OpenPCDet")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "roipool.npz"))
    args = ap.parse_args()
    rs = np.random.RandomState(20231)
    rec = {}
    scenes = []
    n, s = 419, 16
    clouds = [crafted_cloud(rs, n, s, b) for b in range(2)]
    scenes.append(("crafted", np.stack([c[0] for c in clouds]), np.stack([c[1] for c in clouds]),
                   np.stack([c[2] for c in clouds]), 5, s))
    x, bx, fl = random_scene(rs, 333, 12)
    scenes.append(("rand37", x, bx, fl, 1, 37))
    x, bx, fl = random_scene(rs, 70, 9)
    fl[1, 3] = 1
    scenes.append(("rand1", x, bx, fl, 0, 1))
    with tempfile.TemporaryDirectory() as work:
        emu = build_emulator(args.ref, work)
        for name, xyz, boxes, flag_given, c, s in scenes:
            B, N, _ = xyz.shape
            M = boxes.shape[1]
            for rz in np.unique(boxes[:, :, 6][~np.isnan(boxes[:, :, 6])]):
                assert heading_ok(rz), (name, rz)
            feat = rs.randn(B, N, c).astype(np.float32)
            pooled_given = np.full((B, M, s, 3 + c), SENTINEL, dtype=np.float32)
            pooled, flag = pooled_given.copy(), flag_given.copy()
            emu.emu_roipool(B, N, M, c, s, _p(xyz), _p(boxes), _p(feat), _p(pooled), _p(flag))
            box_idx = np.full((B, N), -1, dtype=np.int32)
            emu.emu_points_in_boxes(B, M, N, _p(boxes), _p(xyz), _p(box_idx))
            sp, sf = seq.roipoint_pool3d(xyz, boxes, feat, s, pooled_given, flag_given)
            assert np.array_equal(sf, flag), name
            assert np.array_equal(sp.view(np.uint32), pooled.view(np.uint32)), name
            assert np.array_equal(seq.points_in_boxes(boxes, xyz), box_idx), name
            print(name, "N", N, "M", M, "C", c, "S", s, "counts", seq.inside_counts(xyz, boxes).tolist())
            rec.update({f"{name}_xyz": xyz, f"{name}_boxes": boxes, f"{name}_feat": feat, f"{name}_s": np.int64(s),
                        f"{name}_flag_given": flag_given, f"{name}_pooled_given": pooled_given,
                        f"{name}_pooled": pooled, f"{name}_flag": flag, f"{name}_box_idx": box_idx})
    cases = seq.fixture_cases(rec)
    for k, v in cases.items():
        print("%-50s %s" % (k, v))
    assert all(cases.values()), [k for k, v in cases.items() if not v]
    np.savez_compressed(args.out, **rec)
    size = os.path.getsize(args.out)
    limit = os.path.getsize(os.path.join(ROOT, "tests", "golden", "pointnet2_batch.npz"))
    print(args.out, size, "bytes,", len(rec), "arrays")
    assert size <= limit, (size, limit)


if __name__ == "__main__":
    main()
