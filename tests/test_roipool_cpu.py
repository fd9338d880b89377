"""CPU: the numpy restatement of the RoI point pooling and of points_in_boxes_gpu (tests/roipool_seq.py, the contract
of DESIGN.md section 7e) reproduces what the reference's own kernel text recorded (tests/golden/roipool.npz, written by
tools/make_golden_roipool.py), the fixture contains every case it promises, and the drop-in modules check their
arguments, stay on the host where they must and are bound under the names OpenPCDet imports."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import roipool_seq as seq  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "roipool.npz")


@pytest.fixture(scope="module")
def rec():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def scenes(rec):
    return sorted(k[:-4] for k in rec if k.endswith("_xyz"))


def test_restatement_reproduces_the_fixture_bit_for_bit(rec):
    assert len(scenes(rec)) == 3
    for sc in scenes(rec):
        xyz, boxes, feat, s = rec[sc + "_xyz"], rec[sc + "_boxes"], rec[sc + "_feat"], int(rec[sc + "_s"])
        pooled, flag = seq.roipoint_pool3d(xyz, boxes, feat, s, rec[sc + "_pooled_given"], rec[sc + "_flag_given"])
        assert np.array_equal(flag, rec[sc + "_flag"]), sc
        assert np.array_equal(pooled.view(np.uint32), rec[sc + "_pooled"].view(np.uint32)), sc
        assert np.array_equal(seq.points_in_boxes(boxes, xyz), rec[sc + "_box_idx"]), sc


def test_fixture_contains_every_promised_case(rec):
    cases = seq.fixture_cases(rec)
    assert len(cases) == 24
    assert all(cases.values()), [k for k, v in cases.items() if not v]


def test_fixture_headings_are_valid_under_both_trig_flavours(rec):
    """the recorded outputs used the host C library's cosf / sinf; the contract uses the rounded double functions"""
    from modest_amd.kitti_infos import host_cos_sin_f32
    seen = set()
    for sc in scenes(rec):
        rz = rec[sc + "_boxes"][:, :, 6].ravel()
        rz = rz[~np.isnan(rz)]
        hc, hs = host_cos_sin_f32(rz)
        dc, ds = seq.cos_sin_f32(rz)
        assert np.array_equal(hc.view(np.uint32), dc.view(np.uint32)) and np.array_equal(hs.view(np.uint32), ds.view(np.uint32))
        seen.update(float(v) for v in rz)
    for v in (0.0, np.float32(np.pi / 2), -np.float32(np.pi / 2), np.float32(np.pi)):
        assert float(v) in seen
    assert any(v < 0 for v in seen) and any(v > 2 * np.pi for v in seen) and any(v < -2 * np.pi for v in seen)


def test_fixture_is_small():
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(os.path.dirname(GOLDEN), "pointnet2_batch.npz"))


def test_float32_bound_differs_from_the_double_bound(rec):
    """the case a float32 comparison gets wrong: the point at dx * 0.5f + 1e-5f is inside by the double rule"""
    boxes, xyz = rec["crafted_boxes"], rec["crafted_xyz"]
    hits = 0
    for b in range(2):
        for i, bx in enumerate(boxes[b]):
            if bx[6] == 0 and bx[0] == 0 and bx[1] == 0 and bx[3] > 0 and seq.f32_bound_wrong(bx[3]):
                f32sum = bx[3] * np.float32(0.5) + np.float32(1e-5)
                k = np.flatnonzero((xyz[b, :, 0] == f32sum) & (xyz[b, :, 2] == bx[2]))
                assert len(k) == 1
                assert seq.inside_mask(xyz[b, k], bx[None])[0, 0]
                assert not (np.abs(xyz[b, k[0], 0]) < f32sum)
                assert rec["crafted_box_idx"][b, k[0]] == i
                hits += 1
    assert hits == 2


# ---- the drop-in modules ------------------------------------------------------------------------------------------------
def test_shims_reject_bad_tensors():
    from modest_amd.utils import roiaware_pool3d_cuda as aware
    from modest_amd.utils.roipoint_pool3d import roipoint_pool3d_cuda as pool
    xyz, boxes, feat = torch.zeros(2, 10, 3), torch.zeros(2, 4, 7), torch.zeros(2, 10, 5)
    pooled, flag = torch.zeros(2, 4, 8, 8), torch.zeros(2, 4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="CUDA"):
        pool.forward(xyz, boxes, feat, pooled, flag)
    with pytest.raises(RuntimeError, match="CUDA"):
        aware.points_in_boxes_gpu(boxes, xyz, torch.zeros(2, 10, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="shape"):
        pool.forward(xyz, torch.zeros(2, 4, 8), feat, pooled, flag)
    with pytest.raises(RuntimeError, match="shape"):
        aware.points_in_boxes_gpu(boxes, torch.zeros(2, 10, 4), torch.zeros(2, 10, dtype=torch.int32))
    with pytest.raises(RuntimeError):
        pool.forward(torch.zeros(2, 10, 3, device="meta"), boxes, feat, pooled, flag)
    if torch.cuda.is_available():
        d = torch.device("cuda")
        with pytest.raises(RuntimeError, match="int32"):
            pool.forward(xyz.to(d), boxes.to(d), feat.to(d), pooled.to(d), flag.to(d).long())
        with pytest.raises(RuntimeError, match="float32"):
            pool.forward(xyz.to(d).double(), boxes.to(d), feat.to(d), pooled.to(d), flag.to(d))
        with pytest.raises(RuntimeError, match="shape"):
            pool.forward(xyz.to(d), boxes.to(d), feat.to(d)[:, :9].contiguous(), pooled.to(d), flag.to(d))
        with pytest.raises(RuntimeError, match="shape"):
            aware.points_in_boxes_gpu(boxes.to(d), xyz.to(d), torch.zeros(2, 11, dtype=torch.int32, device=d))
        with pytest.raises(RuntimeError, match="contiguous"):
            pool.forward(xyz.to(d), boxes.to(d), feat.to(d), pooled.to(d).transpose(2, 3), flag.to(d))


def test_points_in_boxes_cpu_is_the_host_predicate(rec):
    from modest_amd.kitti_infos import points_in_boxes_host
    from modest_amd.utils import roiaware_pool3d_cuda as aware
    boxes, xyz = rec["rand37_boxes"][1], rec["rand37_xyz"][1]
    out = torch.full((len(boxes), len(xyz)), -5, dtype=torch.int32)
    assert aware.points_in_boxes_cpu(torch.from_numpy(boxes), torch.from_numpy(xyz), out) == 1
    want = points_in_boxes_host(xyz, boxes)
    assert want.any() and np.array_equal(out.numpy(), want)
    with pytest.raises(RuntimeError):
        aware.points_in_boxes_cpu(torch.from_numpy(boxes), torch.from_numpy(xyz), out[:, :-1].contiguous())
    with pytest.raises(RuntimeError):
        aware.points_in_boxes_cpu(torch.from_numpy(boxes).double(), torch.from_numpy(xyz), out)
    for fn in (aware.forward, aware.backward):
        with pytest.raises(NotImplementedError, match="not provided"):
            fn()


def test_points_in_boxes_cpu_stays_on_the_host():
    """DataLoader workers call it: a fresh interpreter that runs it must not have initialised the GPU"""
    import subprocess
    code = ("import torch\n"
            "from modest_amd.utils import roiaware_pool3d_cuda as a\n"
            "o = torch.zeros(1, 2, dtype=torch.int32)\n"
            "a.points_in_boxes_cpu(torch.tensor([[0., 0, 0, 2, 2, 2, 0.3]]), torch.tensor([[0., 0, 0], [5., 0, 0]]), o)\n"
            "assert o.tolist() == [[1, 0]] and not torch.cuda.is_initialized()\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_module_has_no_backward(monkeypatch):
    """autograd hands backward one gradient per output (rows and flags); the module answers NotImplementedError, as
    the reference means to.  The op is stubbed out: only the autograd plumbing is under test here."""
    from modest_amd.utils.roipoint_pool3d import roipoint_pool3d_utils as u
    monkeypatch.setattr(u.roipoint_pool3d_cuda, "forward", lambda *a: 1)
    x = torch.zeros(2, 10, 3, requires_grad=True)
    f = torch.zeros(2, 10, 4, requires_grad=True)
    pooled, flag = u.RoIPointPool3d(16, 0.5)(x, f, torch.zeros(2, 3, 7))
    assert pooled.shape == (2, 3, 16, 7) and flag.shape == (2, 3) and flag.dtype == torch.int32
    with pytest.raises(NotImplementedError):
        pooled.sum().backward()


def test_pcdet_bind_installs_every_name_once():
    from modest_amd.utils import pcdet_bind
    names = list(pcdet_bind.SHIMS) + list(pcdet_bind.STAND_INS)
    saved = {k: sys.modules.get(k) for k in names}
    try:
        for k in names:
            sys.modules.pop(k, None)
        first = pcdet_bind.install()
        assert sorted(first) == sorted(names)
        for k in names:
            assert sys.modules[k] is first[k]
        import modest_amd.kitti_eval
        import modest_amd.utils.iou3d_nms.iou3d_nms_cuda as iou
        import modest_amd.utils.pointnet2.pointnet2_batch.pointnet2_batch_cuda as pn2
        import modest_amd.utils.roiaware_pool3d_cuda as aware
        import modest_amd.utils.roipoint_pool3d.roipoint_pool3d_cuda as pool
        assert sys.modules["iou3d_nms_cuda"] is iou and sys.modules["pcdet.ops.iou3d_nms.iou3d_nms_cuda"] is iou
        assert sys.modules["pcdet.ops.pointnet2.pointnet2_batch.pointnet2_batch_cuda"] is pn2
        assert sys.modules["pcdet.ops.roipoint_pool3d.roipoint_pool3d_cuda"] is pool
        assert sys.modules["pcdet.ops.roiaware_pool3d.roiaware_pool3d_cuda"] is aware
        assert sys.modules["pcdet.datasets.kitti.kitti_object_eval_python.eval"] is modest_amd.kitti_eval
        assert hasattr(pool, "forward") and hasattr(aware, "points_in_boxes_gpu") and hasattr(aware, "points_in_boxes_cpu")
        second = pcdet_bind.install()
        assert sorted(second) == sorted(first) and all(second[k] is first[k] for k in first)
        # a stand-in imports, can be subclassed at import time, and fails when called
        for k in pcdet_bind.STAND_INS:
            mod = sys.modules[k]
            assert isinstance(mod, types.ModuleType)
            with pytest.raises(NotImplementedError, match="not provided"):
                mod.ball_query_wrapper(1, 2, 3)

            class Block(mod.SparseModule):
                pass
            with pytest.raises(NotImplementedError):
                Block()
        # without stand-ins only the shims are bound
        for k in pcdet_bind.STAND_INS:
            sys.modules.pop(k, None)
        assert sorted(pcdet_bind.install(stand_ins=False)) == sorted(pcdet_bind.SHIMS)
        assert not any(k in sys.modules for k in pcdet_bind.STAND_INS)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_entry_points_are_declared_and_mirrored():
    from modest_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "modest_hip.h")).read()
    for name, nargs in (("modest_roipoint_pool3d", 11), ("modest_points_in_boxes", 7)):
        assert f"int {name}(" in hdr
        assert len(_lib.SIGNATURES[name][1]) == nargs
        assert hasattr(_lib.load(), name)


def test_new_kernels_use_no_scratch_memory():
    import json
    from modest_amd import build
    build.build(verbose=False)
    res = json.load(open(os.path.join(os.path.dirname(build.LIB), "kernel_resources.json")))
    mine = {k: v for k, v in res.items() if v.get("file") == "roipool.hip"}
    assert len(mine) == 2
    assert all(v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 for v in mine.values()), mine
