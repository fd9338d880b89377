"""GPU: the device voxeliser (modest_amd/csrc/voxelize.hip through modest_amd.ops.voxelize) against `collate_batch` of
per-cloud runs of the sequential restatement (tests/voxel_seq.py): the edge families of
tests/voxel_cases.py as batches, bit for bit with no element excluded, into sentinel-filled outputs, twice."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxel_cases as vc  # noqa: E402
import voxel_seq as seq  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = 0x5A5A5A5A   # as int32 and as the float32 with these bits


@pytest.fixture(autouse=True)
def device(gpu):
    """every test here needs the device (tests/conftest.py: fails under -m gpu without one, skips on a GPU-less host)"""
    return gpu


def run(points, c_or_geom, P, M, batch_size):
    """plan + fill into sentinel-filled outputs -> numpy (voxels, coords, num, mask, counts)"""
    from modest_amd import ops
    pl = ops.voxelize_plan(points, c_or_geom["voxel_size"], c_or_geom["point_cloud_range"], P, M, batch_size=batch_size)
    width = points.shape[1] - 1
    outs = [torch.full(shape, SENTINEL, dtype=torch.int32, device=DEV)
            for shape in ((pl.total, P, width), (pl.total, 4), (pl.total,), (pl.total, P))]
    outs[0] = outs[0].view(torch.float32)
    vox, coords, num, mask = ops.voxelize_fill(pl, *outs)
    assert vox.data_ptr() == outs[0].data_ptr()
    return vox.cpu().numpy(), coords.cpu().numpy(), num.cpu().numpy(), mask.cpu().numpy(), pl.counts


def assert_same(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, g.shape, w.dtype, w.shape)
        assert seq.same_bits(g, w), (what, k)


@pytest.mark.parametrize("name", [c["name"] for c in vc.all_cases()])
def test_device_is_the_collated_restatement(name):
    c = next(x for x in vc.all_cases() if x["name"] == name)
    c["present"](c)
    want = seq.collate(vc.expected(name), [len(x) for x in c["clouds"]])
    points = torch.from_numpy(seq.stack_points(c["clouds"])).to(DEV)
    first = run(points, c, c["P"], c["M"], len(c["clouds"]))
    assert_same(first, want, name)
    # two calls give identical bytes (and the padding was written both times)
    assert_same(run(points, c, c["P"], c["M"], len(c["clouds"])), first, name + " again")
    # without a batch size the clouds seen are the last batch index + 1: a trailing empty cloud is not seen
    seen = max((b + 1 for b, x in enumerate(c["clouds"]) if len(x)), default=0)
    free = run(points, c, c["P"], c["M"], None)
    assert free[4].tolist() == want[4][:seen].tolist()
    assert_same(free[:4], want[:4], name + " without batch_size")


def test_workspace_is_the_query_and_does_not_depend_on_the_grid():
    from modest_amd import ops
    c = next(x for x in vc.all_cases() if x["name"] == "fine_grid")
    points = torch.from_numpy(seq.stack_points(c["clouds"])).to(DEV)
    n = len(points)
    nbytes = ops.voxelize_workspace_bytes(n, 2, vc.FINE_GRID)
    assert nbytes == ops.voxelize_workspace_bytes(n, 2, vc.PP_GRID)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
    pl = ops.voxelize_plan(points, c["voxel_size"], c["point_cloud_range"], c["P"], c["M"], batch_size=2, workspace=ws)
    assert pl.workspace is ws   # exactly the queried bytes are enough for 90 M cells
    got = [t.cpu().numpy() for t in ops.voxelize_fill(pl)] + [pl.counts]
    assert_same(got, seq.collate(vc.expected("fine_grid"), [len(x) for x in c["clouds"]]), "fine grid, exact workspace")
    with pytest.raises(Exception, match="2\\^31"):
        ops.voxelize(points, [0.001, 0.001, 0.001], c["point_cloud_range"], 5, 100, batch_size=2)


@pytest.fixture(scope="module")
def detector_batch():
    """B = 2 synthetic Lyft-shape clouds, reference computed once"""
    from modest_amd import synth
    world = synth.make_world(0)
    clouds = [synth.sample_frame(world, 1000 + k, n, synth._pose_matrix(5.0 * k, 0.0, 0.01), synth.default_l2e(),
                                 mobiles=synth.make_mobiles(k, 5.0 * k)) for k, n in ((0, 100_000), (1, 91_237))]
    return clouds, {m: tuple(seq.voxelize(cl, vc.PP_VOXEL, vc.PP_RANGE, 32, m) for cl in clouds) for m in (16000, 40000)}


@pytest.mark.parametrize("cap", [16000, 40000])
def test_detector_shape(detector_batch, cap):
    clouds, ref = detector_batch
    want = seq.collate(ref[cap], [len(x) for x in clouds])
    if cap == 16000:
        assert (want[4] == cap).all(), "the train cap binds on these clouds"
    else:
        assert (want[4] > 16000).all() and (want[4] < cap).all(), "the test cap does not"
    points = torch.from_numpy(seq.stack_points(clouds)).to(DEV)
    geom = dict(voxel_size=vc.PP_VOXEL, point_cloud_range=vc.PP_RANGE)
    assert_same(run(points, geom, 32, cap, 2), want, f"detector shape, cap {cap}")


def test_unsorted_batch_column_is_an_error_and_no_output():
    from modest_amd import ops
    c = next(x for x in vc.all_cases() if x["name"] == "batch3")
    stacked = seq.stack_points(c["clouds"])
    for bad, match in ((lambda s: s[::-1].copy(), "non-decreasing"),
                       (lambda s: np.concatenate([s[:5], s[-1:], s[5:-1]]), "non-decreasing"),
                       (lambda s: np.concatenate([s[:5], s[5:6] * np.asarray([[0.5] + [1] * 4], dtype=np.float32) + 0.5, s[6:]]),
                        "not an integer"),
                       (lambda s: np.concatenate([s, s[-1:] * np.asarray([[np.nan] + [1] * 4], dtype=np.float32)]), "not an integer"),
                       (lambda s: np.concatenate([s, s[-1:] + np.asarray([[1] + [0] * 4], dtype=np.float32)]), "not an integer")):
        pts = torch.from_numpy(np.ascontiguousarray(bad(stacked), dtype=np.float32)).to(DEV)
        with pytest.raises(Exception, match=match):
            ops.voxelize(pts, c["voxel_size"], c["point_cloud_range"], c["P"], c["M"], batch_size=3)
    # ... and the same workspace serves a good batch afterwards
    want = seq.collate(vc.expected("batch3"), [len(x) for x in c["clouds"]])
    got = ops.voxelize(torch.from_numpy(stacked).to(DEV), c["voxel_size"], c["point_cloud_range"], c["P"], c["M"], batch_size=3)
    assert_same([t.cpu().numpy() for t in got[:4]] + [got[4]], want, "after the errors")


def test_bad_tensors_raise():
    from modest_amd import ops
    geom = (vc.PP_VOXEL, vc.PP_RANGE, 32, 100)
    pts = torch.zeros((10, 5), dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError):
        ops.voxelize(pts.cpu(), *geom)
    with pytest.raises(TypeError):
        ops.voxelize(pts.double(), *geom)
    with pytest.raises(ValueError):
        ops.voxelize(pts[:, :3].contiguous(), *geom)
    with pytest.raises(ValueError):
        ops.voxelize(pts.t().contiguous().t(), *geom)
    with pytest.raises(Exception, match="positive"):
        ops.voxelize(pts, vc.PP_VOXEL, vc.PP_RANGE, 0, 100)


def test_module_fills_float_tensors_equal_to_the_int_ones():
    from modest_amd import ops
    from modest_amd.utils.voxelize import VoxelizeOnDevice
    c = next(x for x in vc.all_cases() if x["name"] == "batch_cap_per_cloud")
    points = torch.from_numpy(seq.stack_points(c["clouds"])).to(DEV)
    mod = VoxelizeOnDevice(c["voxel_size"], c["point_cloud_range"], c["P"], {"train": c["M"], "test": 16000})
    assert mod.grid_size.tolist() == vc.PP_GRID
    for training, m in ((True, c["M"]), (False, 16000), (True, c["M"])):   # the second round reuses the workspace
        mod.train(training)
        batch = mod({"points": points, "batch_size": 3})
        vox, coords, num, mask, counts = ops.voxelize(points, c["voxel_size"], c["point_cloud_range"], c["P"], m, batch_size=3)
        assert batch["voxel_coords"].dtype == torch.float32 and batch["voxel_num_points"].dtype == torch.float32
        assert torch.equal(batch["voxel_coords"], coords.float()) and torch.equal(batch["voxel_coords"].int(), coords)
        assert torch.equal(batch["voxel_num_points"], num.float()) and torch.equal(batch["voxel_num_points"].int(), num)
        assert torch.equal(batch["voxels"].view(torch.int32), vox.view(torch.int32)) and torch.equal(batch["voxel_point_mask"], mask)
        assert batch["points"] is points and len(coords) == int(counts.sum())
        if training:
            want = seq.collate(vc.expected(c["name"]), [len(x) for x in c["clouds"]])
            assert seq.same_bits(coords.cpu().numpy(), want[1]) and counts.tolist() == want[4].tolist()
    with pytest.raises(ValueError):
        mod({"points": points.cpu(), "batch_size": 3})
