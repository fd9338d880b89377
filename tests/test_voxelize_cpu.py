"""CPU: the host voxel generator (modest_amd/utils/spconv_utils.py over modest_voxelize_host) against the sequential
restatement of the contract (tests/voxel_seq.py) on every edge family, bit for bit with no element
excluded; a case worked by hand; the spconv.utils binding; and the host path staying off the GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxel_cases as vc  # noqa: E402
import voxel_seq as seq  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def assert_same(got, want, what):
    assert set(got) == set(seq.KEYS) | {"voxel_num"}, what
    assert got["voxel_num"] == want["voxel_num"], what
    for k in seq.KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        assert seq.same_bits(got[k], want[k]), (what, k)


# ---- a case worked by hand: range [0, 0, 0, 4, 2, 2], voxels of 1 x 1 x 1 -> grid [4, 2, 2]; P = 2, M = 3 --------------
HAND_RANGE, HAND_VOXEL = [0, 0, 0, 4, 2, 2], [1, 1, 1]
HAND_POINTS = np.asarray([
    [0.5, 0.5, 0.5, 10],    # 0: cell z0 y0 x0 -> voxel 0, slot 0
    [3.5, 1.5, 1.5, 11],    # 1: cell z1 y1 x3 -> voxel 1, slot 0
    [4.0, 0.5, 0.5, 12],    # 2: x == hi_x: floor 4 == grid_x, dropped
    [0.25, 0.75, 0.0, 13],  # 3: voxel 0, slot 1 (z == lo_z is inside)
    [0.9, 0.1, 0.9, 14],    # 4: voxel 0 is full (P = 2): dropped
    [2.5, 0.5, 1.0, 15],    # 5: cell z1 y0 x2 -> voxel 2, slot 0 (now M = 3 voxels are open)
    [1.5, 1.5, 0.5, 16],    # 6: a new cell after the cap: dropped, the walk goes on
    [3.0, 1.0, 1.0, 17],    # 7: back to voxel 1 (on its lower corner), slot 1
    [-0.5, 0.5, 0.5, 18],   # 8: x < lo_x: dropped
    [2.25, 0.5, 1.5, 19],   # 9: voxel 2, slot 1
], dtype=F)
HAND = {
    "voxels": np.asarray([[[0.5, 0.5, 0.5, 10], [0.25, 0.75, 0.0, 13]],
                          [[3.5, 1.5, 1.5, 11], [3.0, 1.0, 1.0, 17]],
                          [[2.5, 0.5, 1.0, 15], [2.25, 0.5, 1.5, 19]]], dtype=F),
    "coordinates": np.asarray([[0, 0, 0], [1, 1, 3], [1, 0, 2]], dtype=np.int32),
    "num_points_per_voxel": np.asarray([2, 2, 2], dtype=np.int32),
    "voxel_point_mask": np.asarray([[0, 3], [1, 7], [5, 9]], dtype=np.int32),
    "voxel_num": 3,
}


def test_hand_worked_case():
    from modest_amd.utils.spconv_utils import VoxelGenerator
    assert seq.grid_size(HAND_RANGE, HAND_VOXEL).tolist() == [4, 2, 2]
    assert_same(seq.voxelize(HAND_POINTS, HAND_VOXEL, HAND_RANGE, 2, 3), HAND, "voxel_seq")
    gen = VoxelGenerator(HAND_VOXEL, HAND_RANGE, 2, 3)
    assert gen.grid_size.tolist() == [4, 2, 2] and gen.grid_size.dtype == np.int64
    assert_same(gen.generate(HAND_POINTS), HAND, "host")
    # with room for a fourth voxel point 6 opens it; with P = 3 point 4 enters voxel 0
    got = gen.generate(HAND_POINTS, max_voxels=4)
    assert got["voxel_num"] == 4 and got["coordinates"][3].tolist() == [0, 1, 1] and got["voxel_point_mask"][3].tolist() == [6, -1]
    assert got["voxels"][3].tolist() == [[1.5, 1.5, 0.5, 16], [0, 0, 0, 0]] and not np.signbit(got["voxels"][3, 1]).any()
    assert_same(got, seq.voxelize(HAND_POINTS, HAND_VOXEL, HAND_RANGE, 2, 4), "M = 4")
    assert VoxelGenerator(HAND_VOXEL, HAND_RANGE, 3, 3).generate(HAND_POINTS)["voxel_point_mask"][0].tolist() == [0, 3, 4]
    # the table is left clean: the same generator gives the same answer again
    assert_same(gen.generate(HAND_POINTS), HAND, "host, second call")


def test_pointpillars_grid():
    from modest_amd.utils.spconv_utils import VoxelGeneratorV2
    gen = VoxelGeneratorV2(voxel_size=vc.PP_VOXEL, point_cloud_range=vc.PP_RANGE, max_num_points=32, max_voxels=16000)
    assert gen.grid_size.tolist() == vc.PP_GRID == seq.grid_size(vc.PP_RANGE, vc.PP_VOXEL).tolist()
    assert gen.voxel_size.dtype == F and gen.point_cloud_range.dtype == F and gen.max_num_points_per_voxel == 32
    assert seq.grid_size(vc.KITTI_RANGE, vc.FINE_VOXEL).tolist() == vc.FINE_GRID


@pytest.mark.parametrize("name", [c["name"] for c in vc.all_cases()])
def test_host_path_is_the_restatement(name):
    from modest_amd.utils.spconv_utils import VoxelGenerator
    c = next(x for x in vc.all_cases() if x["name"] == name)
    c["present"](c)
    gen = VoxelGenerator(c["voxel_size"], c["point_cloud_range"], c["P"], c["M"])
    # one generator for all clouds of the case: its cell table must come back clean every time
    for k, (cloud, want) in enumerate(zip(c["clouds"], vc.expected(name))):
        got = gen.generate(cloud)
        assert_same(got, want, (name, k))
        assert got["voxels"].shape[1:] == (c["P"], cloud.shape[1]) and got["coordinates"].shape[1:] == (3,)
    assert gen._table is None or (gen._table == -1).all()


def test_no_point_in_range_gives_empty_arrays_of_the_right_rank():
    from modest_amd.utils.spconv_utils import VoxelGenerator
    gen = VoxelGenerator(vc.PP_VOXEL, vc.PP_RANGE, 32, 100)
    for pts in (np.zeros((0, 4), dtype=F), np.full((5, 4), 1000.0, dtype=F)):
        got = gen.generate(pts)
        assert got["voxel_num"] == 0 and got["voxels"].shape == (0, 32, 4) and got["coordinates"].shape == (0, 3)
        assert got["num_points_per_voxel"].shape == (0,) and got["voxel_point_mask"].shape == (0, 32)
        assert_same(got, seq.voxelize(pts, vc.PP_VOXEL, vc.PP_RANGE, 32, 100), "empty")


def test_collate_restatement():
    outs = [seq.voxelize(HAND_POINTS, HAND_VOXEL, HAND_RANGE, 2, 3), seq.voxelize(HAND_POINTS[:0], HAND_VOXEL, HAND_RANGE, 2, 3),
            seq.voxelize(HAND_POINTS[5:], HAND_VOXEL, HAND_RANGE, 2, 3)]
    vox, coords, num, mask, counts = seq.collate(outs, [10, 0, 5])
    assert counts.tolist() == [3, 0, 3] and vox.shape == (6, 2, 4) and num.tolist() == [2, 2, 2, 2, 1, 1]
    assert coords.tolist() == [[0, 0, 0, 0], [0, 1, 1, 3], [0, 1, 0, 2], [2, 1, 0, 2], [2, 0, 1, 1], [2, 1, 1, 3]]
    assert mask.tolist() == [[0, 3], [1, 7], [5, 9], [10, 14], [11, -1], [12, -1]]
    stacked = seq.stack_points([HAND_POINTS, HAND_POINTS[:0], HAND_POINTS[5:]])
    assert stacked.shape == (15, 5) and stacked[:, 0].tolist() == [0] * 10 + [2] * 5
    assert np.array_equal(stacked[mask[3, 0], 1:], vox[3, 0])


def test_generator_arguments():
    from modest_amd.utils.spconv_utils import VoxelGenerator, VoxelGeneratorV2
    assert VoxelGenerator is VoxelGeneratorV2
    for kw in (dict(full_mean=True), dict(block_filtering=True), dict(block_factor=4), dict(height_threshold=0.2)):
        with pytest.raises(NotImplementedError):
            VoxelGeneratorV2(vc.PP_VOXEL, vc.PP_RANGE, 32, 100, **kw)
    with pytest.raises(ValueError):
        VoxelGenerator(vc.PP_VOXEL, vc.PP_RANGE, 0, 100)
    with pytest.raises(ValueError, match="2\\^31"):
        VoxelGenerator([0.001, 0.001, 0.001], vc.PP_RANGE, 32, 100)
    gen = VoxelGenerator(vc.PP_VOXEL, vc.PP_RANGE, 32, 100)
    with pytest.raises(ValueError):
        gen.generate(np.zeros((4, 2), dtype=F))
    # float64 rows are rounded to float32 first, a strided view is copied
    pts = vc.scatter_cloud(5, 40).astype(np.float64)
    assert_same(gen.generate(pts[::2]), seq.voxelize(pts[::2].astype(F), vc.PP_VOXEL, vc.PP_RANGE, 32, 100), "float64 view")


def test_spconv_utils_binding():
    from modest_amd.utils import pcdet_bind, spconv_utils
    names = list(pcdet_bind.SHIMS) + list(pcdet_bind.STAND_INS) + ["spconv.utils"]
    saved = {k: sys.modules.get(k) for k in names}
    try:
        for k in names:
            sys.modules.pop(k, None)
        before = sorted(pcdet_bind.SHIMS) + sorted(pcdet_bind.STAND_INS)
        bound = pcdet_bind.install()
        assert sorted(bound) == sorted(before)   # the returned dict keeps its keys
        from spconv.utils import VoxelGeneratorV2
        from spconv.utils import VoxelGenerator
        import spconv
        assert spconv.utils is spconv_utils and sys.modules["spconv.utils"] is spconv_utils
        assert VoxelGeneratorV2 is spconv_utils.VoxelGeneratorV2 and VoxelGenerator is spconv_utils.VoxelGenerator
        gen = VoxelGeneratorV2(voxel_size=HAND_VOXEL, point_cloud_range=np.asarray(HAND_RANGE, dtype=F), max_num_points=2,
                               max_voxels=3)
        assert_same(gen.generate(HAND_POINTS), HAND, "bound")
        with pytest.raises(NotImplementedError, match="not provided"):
            spconv.SparseModule()
        with pytest.raises(NotImplementedError, match="not provided"):
            spconv.SparseConvTensor(1, 2, 3, 4)
        again = pcdet_bind.install()
        assert all(again[k] is bound[k] for k in bound) and sys.modules["spconv.utils"] is spconv_utils
        # without stand-ins nothing of spconv is bound
        for k in list(pcdet_bind.STAND_INS) + ["spconv.utils"]:
            sys.modules.pop(k, None)
        assert sorted(pcdet_bind.install(stand_ins=False)) == sorted(pcdet_bind.SHIMS)
        assert "spconv" not in sys.modules and "spconv.utils" not in sys.modules
        # an spconv that is not a stand-in (an installed one) is left alone
        import types
        real = sys.modules["spconv"] = types.ModuleType("spconv")
        pcdet_bind.install()
        assert sys.modules["spconv"] is real and not hasattr(real, "utils") and "spconv.utils" not in sys.modules
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_host_path_stays_off_the_gpu():
    """DataLoader workers are forked: a fresh interpreter that voxelises must not have opened the GPU.  The child runs
    with the devices hidden, counts the calls of modest_device_count / modest_ctx_create and checks torch's own state."""
    code = ("import numpy as np, torch\n"
            "from modest_amd import _lib\n"
            "from modest_amd.utils.spconv_utils import VoxelGeneratorV2\n"
            "calls = []\n"
            "class Spy:\n"
            "    def __init__(self, lib): self._lib = lib\n"
            "    def __getattr__(self, name):\n"
            "        calls.append(name)\n"
            "        return getattr(self._lib, name)\n"
            "_lib._lib = Spy(_lib.load())\n"
            "g = VoxelGeneratorV2([0.16, 0.16, 4], [0, -39.68, -3, 89.6, 39.68, 1], 32, 16000)\n"
            "o = g.generate(np.asarray([[1, 1, 0, 0.5], [1.01, 1.01, 0, 0.25], [50, 0, 0, 1]], dtype=np.float32))\n"
            "assert o['voxel_num'] == 2 and o['num_points_per_voxel'].tolist() == [2, 1], o\n"
            "assert calls == ['modest_voxelize_host'], calls\n"
            "assert not torch.cuda.is_initialized()\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr


def test_entry_points_are_declared_and_mirrored():
    from modest_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "modest_hip.h")).read()
    for name, res, nargs in (("modest_voxelize_host", "int64_t", 13), ("modest_voxelize_workspace_bytes", "int64_t", 3),
                             ("modest_voxelize_plan", "int", 13), ("modest_voxelize_fill", "int", 16)):
        assert f"{res} {name}(" in hdr
        decl = hdr[hdr.index(f"{res} {name}("):]
        assert decl[:decl.index(";")].count(",") + 1 == nargs == len(_lib.SIGNATURES[name][1])
        assert hasattr(_lib.load(), name)


def test_workspace_does_not_depend_on_the_grid():
    from modest_amd import ops
    for n in (0, 1, 5003, 400_000):
        a = ops.voxelize_workspace_bytes(n, 4, vc.PP_GRID)
        assert a == ops.voxelize_workspace_bytes(n, 4, vc.FINE_GRID) == ops.voxelize_workspace_bytes(n, 4, [46340, 46340, 1])
        assert a <= 64 * n + (1 << 16)
    with pytest.raises(Exception, match="2\\^31"):
        ops.voxelize_workspace_bytes(1000, 4, [46341, 46341, 1])   # more than 2^31 - 1 cells


def test_kernels_use_no_scratch_memory():
    import json
    from modest_amd import build
    build.build(verbose=False)
    res = json.load(open(os.path.join(os.path.dirname(build.LIB), "kernel_resources.json")))
    mine = {k: v for k, v in res.items() if v.get("file") in ("voxelize.hip", "sort64.hip")}
    assert sum(v["file"] == "voxelize.hip" for v in mine.values()) == 7
    assert sum(v["file"] == "sort64.hip" for v in mine.values()) == 4   # count, scan, scatter with and without the payload
    assert all(v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 for v in mine.values()), mine
