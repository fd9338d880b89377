"""CPU: the numpy restatement of the RoI-aware voxel pooling (tests/roiaware_seq.py, the contract of DESIGN.md section
7j) reproduces what the reference's own kernel text recorded (tests/golden/roiaware_pool.npz, written by
tools/make_golden_roiaware_pool.py), the fixture contains every case it promises, the index rule holds where the host's
float -> int conversion could not record it, and the drop-in module, the layer and the binding check their arguments
without opening the GPU."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import roiaware_seq as seq  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "roiaware_pool.npz")
ENTRY_POINTS = (("modest_roiaware_pool3d_forward", "int", 15), ("modest_roiaware_pool3d_backward_workspace_bytes", "int64_t", 2),
                ("modest_roiaware_pool3d_backward", "int", 15))


@pytest.fixture(scope="module")
def rec():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_restatement_reproduces_the_fixture_bit_for_bit(rec):
    assert seq.scene_names(rec) == ["crafted", "cubic", "nolist", "single"]
    for sc in seq.scene_names(rec):
        out = tuple(int(v) for v in rec[sc + "_out"])
        max_pts = rec[sc + "_lists"].shape[-1]
        for method, tag in ((0, "max"), (1, "avg")):
            lists, pooled, argmax = seq.forward(rec[sc + "_rois"], rec[sc + "_pts"], rec[sc + "_feat"], out, max_pts, method,
                                                rec[sc + "_lists_given"], rec[sc + "_pooled_given"], rec[sc + "_argmax_given"])
            assert np.array_equal(lists, rec[sc + "_lists"]), (sc, tag)
            assert np.array_equal(bits(pooled), bits(rec[f"{sc}_pooled_{tag}"])), (sc, tag)
            assert np.array_equal(argmax, rec[f"{sc}_argmax_{tag}"]), (sc, tag)
            grad = seq.backward(lists, argmax, rec[sc + "_grad_out"], rec[sc + "_grad_in_given"], method)
            assert np.array_equal(bits(grad), bits(rec[f"{sc}_grad_in_{tag}"])), (sc, tag)
            # the count word is written, not counted on from: garbage there changes nothing
            dirty = rec[sc + "_lists_given"].copy()
            dirty[..., 0] = 99
            assert np.array_equal(seq.build_lists(rec[sc + "_pts"], rec[sc + "_rois"], out, max_pts, dirty)[0], lists)


def test_fixture_contains_every_promised_case(rec):
    cases = seq.fixture_cases(rec)
    assert len(cases) == 24
    assert all(cases.values()), [k for k, v in cases.items() if not v]


def test_fixture_quotients_are_finite_and_headings_valid_under_both_trig_flavours(rec):
    """the recording ran the host's float -> int conversion and cosf / sinf: both agree with the contract on what it holds"""
    from modest_amd.kitti_infos import host_cos_sin_f32
    from roipool_seq import cos_sin_f32
    for sc in seq.scene_names(rec):
        rois, pts = rec[sc + "_rois"], rec[sc + "_pts"]
        mask, _ = seq.voxel_ids(pts, rois, tuple(rec[sc + "_out"]))
        for q in seq.local_q(pts, rois, tuple(rec[sc + "_out"])):
            assert np.isfinite(q[mask]).all() and (np.abs(q[mask]) < 2.0 ** 31).all()
        hc, hs = host_cos_sin_f32(rois[:, 6])
        dc, ds = cos_sin_f32(rois[:, 6])
        assert np.array_equal(bits(hc), bits(dc)) and np.array_equal(bits(hs), bits(ds))


def test_fixture_is_small():
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(os.path.dirname(GOLDEN), "pointnet2_batch.npz"))


def test_index_rule_on_hand_made_quotients():
    f = np.float32
    q = np.array([np.nan, np.inf, -np.inf, -1.0, np.nextafter(f(-1), f(0)), -0.5, -0.0, 0.0, 0.999, 1.0, 6.999, 7.0,
                  7.5, 3e9, -3e9, 3.4e38], dtype=f)
    want = np.array([0, 6, 6, 6, 0, 0, 0, 0, 0, 1, 6, 6, 6, 6, 6, 6])
    assert seq.voxel_index(q, 7).tolist() == want.tolist()
    assert seq.voxel_index(q, 1).tolist() == [0] * len(q)
    assert seq.voxel_index(np.array([255.5, 256.0, -1.0], dtype=f), 256).tolist() == [255, 255, 255]
    # the rule IS min(max((unsigned)(int)q, 0), out - 1) with saturating conversions, NaN -> 0
    for out in (1, 7, 256):
        for v, got in zip(q, seq.voxel_index(q, out)):
            i = 0 if np.isnan(v) else int(np.clip(np.trunc(np.float64(v)), -2.0 ** 31, 2.0 ** 31 - 1))
            assert got == min(max(i % 2 ** 32, 0), out - 1), (v, out)


def test_zero_extent_boxes_follow_the_index_rule():
    """dx = 0: res = 0 and q = l / 0 is +-inf or NaN.  A point exactly on the plane gives NaN -> 0, one inside the margin
    on either side gives +-inf -> out - 1"""
    out, max_pts = (3, 2, 2), 4
    rois = np.array([[0, 0, 0, 0, 2, 2, 0], [0, 0, 0, 0, 0, 0, 0]], dtype=np.float32)
    pts = np.array([[0, 0.5, 0.5], [5e-6, 0.5, 0.5], [-5e-6, -0.5, -0.5], [0, 0, 0], [1, 0, 0]], dtype=np.float32)
    mask, vid = seq.voxel_ids(pts, rois, out)
    assert mask.tolist() == [[True, True, True, True, False], [False, False, False, True, False]]
    assert vid[0, :4].tolist() == [(0 * 2 + 1) * 2 + 1, (2 * 2 + 1) * 2 + 1, (2 * 2 + 0) * 2 + 0, (0 * 2 + 1) * 2 + 1]
    assert vid[1, 3] == 0                                 # the all-zero (padding) box: NaN on every axis
    lists, pooled, argmax = seq.forward(rois, pts, np.arange(5, dtype=np.float32)[:, None], out, max_pts, 0,
                                        np.full((2, 3, 2, 2, 4), -9, dtype=np.int32), np.zeros((2, 3, 2, 2, 1), dtype=np.float32),
                                        np.zeros((2, 3, 2, 2, 1), dtype=np.int32))
    assert lists[0, 0, 1, 1].tolist() == [2, 0, 3, -9] and argmax[0, 0, 1, 1, 0] == 3 and pooled[0, 0, 1, 1, 0] == 3.0
    assert lists[1, 0, 0, 0].tolist() == [1, 3, -9, -9]
    # NaN boxes: a NaN centre holds nothing; a NaN dz does not reject and sends z to voxel 0
    rois = np.array([[np.nan, 0, 0, 2, 2, 2, 0], [0, 0, 0, 2, 2, np.nan, 0]], dtype=np.float32)
    mask, vid = seq.voxel_ids(pts, rois, out)
    assert not mask[0].any() and mask[1].all()
    assert (vid[1] % 2 == 0).all()


def test_backward_ignores_an_argmax_outside_the_voxels_list():
    lists = np.array([[3, 0, 2, 4, -9], [0, -9, -9, -9, -9]], dtype=np.int32).reshape(1, 2, 1, 1, 5)
    argmax = np.array([[2, 1], [4, -1]], dtype=np.int32).reshape(1, 2, 1, 1, 2)   # 1 is not listed; 4 is, elsewhere
    grad = seq.backward(lists, argmax, np.ones((1, 2, 1, 1, 2), dtype=np.float32), np.zeros((5, 2), dtype=np.float32), 0)
    assert grad.tolist() == [[0, 0], [0, 0], [1, 0], [0, 0], [0, 0]]


# ---- the library -------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_mirrored():
    from modest_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "modest_hip.h")).read()
    for name, ret, nargs in ENTRY_POINTS:
        assert f"{ret} {name}(" in hdr
        decl = hdr.split(f"{ret} {name}(")[1].split(");")[0]
        assert decl.count(",") + 1 == nargs
        assert len(_lib.SIGNATURES[name][1]) == nargs
        assert hasattr(_lib.load(), name)


def test_new_kernels_use_no_scratch_memory_and_roipool_keeps_its_two():
    from modest_amd import build
    build.build(verbose=False)
    res = json.load(open(os.path.join(os.path.dirname(build.LIB), "kernel_resources.json")))
    mine = {k: v for k, v in res.items() if v.get("file") == "roiaware_pool.hip"}
    assert len(mine) == 6 and sum("roiaware_collect" in k for k in mine) == 1
    assert all(v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 for v in mine.values()), mine
    assert len([k for k, v in res.items() if v.get("file") == "roipool.hip"]) == 2


def test_workspace_bytes_and_argument_errors_need_no_gpu():
    """the size query and every refusal are host code: they return before anything is enqueued"""
    from modest_amd import _lib
    lib = _lib.load()
    assert lib.modest_roiaware_pool3d_backward_workspace_bytes(128, 16384) == 128 * 16384 * 4
    assert lib.modest_roiaware_pool3d_backward_workspace_bytes(0, 5) == 0
    assert lib.modest_roiaware_pool3d_backward_workspace_bytes(3, 0) == 0
    ok = dict(n=1, p=1, c=1, m=2, ox=2, oy=2, oz=2, method=0)
    for bad, word in ((dict(method=2), "pool_method"), (dict(method=-1), "pool_method"), (dict(m=0), "max_pts_each_voxel"),
                      (dict(ox=0), "1..256"), (dict(oz=257), "1..256"), (dict(ox=25, oy=24, oz=24), "13824"),
                      (dict(n=-1), "negative")):
        a = dict(ok, **bad)
        rc = lib.modest_roiaware_pool3d_forward(a["n"], a["p"], a["c"], a["m"], a["ox"], a["oy"], a["oz"], None, None, None,
                                                None, None, None, a["method"], None)
        assert rc != 0 and word in lib.modest_last_error().decode(), (bad, lib.modest_last_error())
        if "13824" in word:
            continue   # the backward has no LDS counters: its limit is 256 per axis
        rc = lib.modest_roiaware_pool3d_backward(a["n"], a["p"], a["ox"], a["oy"], a["oz"], a["c"], a["m"], None, None, None,
                                                 None, a["method"], None, 0, None)
        assert rc != 0 and word in lib.modest_last_error().decode(), (bad, lib.modest_last_error())
    # zero sizes are legal and touch nothing
    assert lib.modest_roiaware_pool3d_forward(0, 5, 3, 4, 2, 2, 2, None, None, None, None, None, None, 0, None) == 0
    assert lib.modest_roiaware_pool3d_backward(0, 5, 2, 2, 2, 3, 4, None, None, None, None, 1, None, 0, None) == 0
    assert lib.modest_roiaware_pool3d_backward(2, 0, 2, 2, 2, 3, 4, None, None, None, None, 1, None, 0, None) == 0
    assert lib.modest_roiaware_pool3d_backward(2, 5, 2, 2, 2, 0, 4, None, None, None, None, 0, None, 0, None) == 0


# ---- the drop-in module, the layer, the binding ----------------------------------------------------------------------------
def test_shim_rejects_bad_tensors_without_opening_the_gpu():
    import subprocess
    code = """
import pytest, torch
from modest_amd.utils import roiaware_voxel_pool_cuda as m
from modest_amd.utils import roiaware_pool3d_cuda as old
assert m.points_in_boxes_gpu is old.points_in_boxes_gpu and m.points_in_boxes_cpu is old.points_in_boxes_cpu
i = dict(dtype=torch.int32)
rois, pts, feat = torch.zeros(2, 7), torch.zeros(9, 3), torch.zeros(9, 4)
argmax, lists, pooled = torch.zeros(2, 3, 3, 3, 4, **i), torch.zeros(2, 3, 3, 3, 8, **i), torch.zeros(2, 3, 3, 3, 4)
grad_out, grad_in = torch.zeros(2, 3, 3, 3, 4), torch.zeros(9, 4)
with pytest.raises(RuntimeError, match="CUDA"):
    m.forward(rois, pts, feat, argmax, lists, pooled, 0)
with pytest.raises(RuntimeError, match="CUDA"):
    m.backward(lists, argmax, grad_out, grad_in, 1)
with pytest.raises(RuntimeError, match="shape"):
    m.forward(torch.zeros(2, 8), pts, feat, argmax, lists, pooled, 0)
with pytest.raises(RuntimeError, match="shape"):
    m.forward(rois, torch.zeros(9, 4), feat, argmax, lists, pooled, 0)
with pytest.raises(RuntimeError, match="shape"):
    m.forward(rois, pts, feat, argmax, torch.zeros(2, 3, 3, 8, **i), pooled, 0)
with pytest.raises(RuntimeError, match="shape"):
    m.backward(lists, argmax, torch.zeros(2, 3, 3, 4), grad_in, 0)
with pytest.raises(RuntimeError, match="pool_method"):
    m.forward(rois, pts, feat, argmax, lists, pooled, 2)
with pytest.raises(RuntimeError, match="pool_method"):
    m.backward(lists, argmax, grad_out, grad_in, "max")
with pytest.raises(RuntimeError):
    m.forward(torch.zeros(2, 7, device="meta"), pts, feat, argmax, lists, pooled, 0)
with pytest.raises(RuntimeError, match="tensor"):
    m.forward(None, pts, feat, argmax, lists, pooled, 0)
assert not torch.cuda.is_initialized()
"""
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_shim_checks_dtype_contiguity_and_shapes_on_the_device():
    if not torch.cuda.is_available():
        return   # the device-side half of the validation; the host-side half is the test above
    from modest_amd.utils import roiaware_voxel_pool_cuda as m
    d = torch.device("cuda")
    i = dict(dtype=torch.int32, device=d)
    rois, pts, feat = torch.zeros(2, 7, device=d), torch.zeros(9, 3, device=d), torch.zeros(9, 4, device=d)
    argmax, lists, pooled = torch.zeros(2, 3, 3, 3, 4, **i), torch.zeros(2, 3, 3, 3, 8, **i), torch.zeros(2, 3, 3, 3, 4, device=d)
    with pytest.raises(RuntimeError, match="int32"):
        m.forward(rois, pts, feat, argmax.long(), lists, pooled, 0)
    with pytest.raises(RuntimeError, match="float32"):
        m.forward(rois, pts, feat.double(), argmax, lists, pooled, 0)
    with pytest.raises(RuntimeError, match="shape"):
        m.forward(rois, pts, feat[:8].contiguous(), argmax, lists, pooled, 0)
    with pytest.raises(RuntimeError, match="shape"):
        m.forward(rois, pts, feat, argmax, lists, pooled[:, :2].contiguous(), 0)
    with pytest.raises(RuntimeError, match="contiguous"):
        m.forward(rois, pts, feat, argmax, lists, pooled.transpose(1, 2), 0)
    with pytest.raises(RuntimeError, match="shape"):
        m.backward(lists, argmax, pooled, torch.zeros(9, 5, device=d), 0)


def test_layer_argument_rules(monkeypatch):
    """the reference's out_size int-or-triple rule and assertions; the op is stubbed out: only the Python side is under test"""
    from modest_amd.utils import roiaware_pool3d_utils as u
    from modest_amd.utils import roiaware_voxel_pool_cuda as m
    seen = []
    monkeypatch.setattr(m, "forward", lambda *a: seen.append(("f", a)) or 1)
    monkeypatch.setattr(m, "backward", lambda *a: seen.append(("b", a)) or 1)
    rois, pts = torch.zeros(3, 7), torch.zeros(10, 3)
    feat = torch.zeros(10, 4, requires_grad=True)
    layer = u.RoIAwarePool3d(6)
    assert layer.out_size == 6 and layer.max_pts_each_voxel == 128
    out = layer(rois, pts, feat)                                    # pool_method defaults to 'max'
    assert out.shape == (3, 6, 6, 6, 4) and out.dtype == torch.float32 and (out == 0).all()
    _, a = seen[-1]
    assert a[6] == 0 and a[3].shape == (3, 6, 6, 6, 4) and a[3].dtype == torch.int32 and a[4].shape == (3, 6, 6, 6, 128)
    out.sum().backward()
    kind, a = seen[-1]
    assert kind == "b" and a[4] == 0 and a[3].shape == (10, 4) and (a[3] == 0).all() and feat.grad.shape == (10, 4)
    out = u.RoIAwarePool3d((3, 5, 2), max_pts_each_voxel=9)(rois, pts, feat, pool_method="avg")
    assert out.shape == (3, 3, 5, 2, 4) and seen[-1][1][6] == 1 and seen[-1][1][4].shape == (3, 3, 5, 2, 9)
    assert (seen[-1][1][3] == 0).all()                              # argmax of an avg call: zero-filled, never written
    assert u.RoIAwarePool3d([2, 2, 2])(rois, pts, feat).shape == (3, 2, 2, 2, 4)
    for bad in ((3, 5), (3, 5, 2, 1), (3.0, 5, 2)):
        with pytest.raises(AssertionError):
            u.RoIAwarePool3d(bad)(rois, pts, feat)
    with pytest.raises(AssertionError):
        layer(rois, pts, feat, pool_method="sum")
    with pytest.raises(AssertionError):
        layer(torch.zeros(3, 8), pts, feat)
    with pytest.raises(AssertionError):
        layer(rois, torch.zeros(10, 4), feat)


def test_install_binds_the_full_module_on_request():
    from modest_amd.utils import pcdet_bind
    import modest_amd.utils.roiaware_pool3d_cuda as old
    import modest_amd.utils.roiaware_voxel_pool_cuda as new
    name = "pcdet.ops.roiaware_pool3d.roiaware_pool3d_cuda"
    assert pcdet_bind.ROIAWARE_NAME == name and pcdet_bind.SHIMS[name] == "modest_amd.utils.roiaware_pool3d_cuda"
    names = list(pcdet_bind.SHIMS) + list(pcdet_bind.STAND_INS)
    saved = {k: sys.modules.get(k) for k in names + ["spconv.utils"]}
    try:
        for k in names:
            sys.modules.pop(k, None)
        default = pcdet_bind.install()
        assert sys.modules[name] is old and default[name] is old
        first = pcdet_bind.install(roiaware_pool=True)
        assert sys.modules[name] is new and first[name] is new and sorted(first) == sorted(default)
        assert all(first[k] is default[k] for k in default if k != name)
        second = pcdet_bind.install(roiaware_pool=True)             # idempotent
        assert sys.modules[name] is new and all(second[k] is first[k] for k in first)
        assert hasattr(new, "forward") and hasattr(new, "backward") and hasattr(new, "points_in_boxes_gpu")
        with pytest.raises(NotImplementedError, match="not provided"):
            old.forward()
        # the default call still binds the module without the pooling
        assert pcdet_bind.install()[name] is old and sys.modules[name] is old
        # a module that is neither of ours (the compiled extension) is left alone
        foreign = types.ModuleType(name)
        sys.modules[name] = foreign
        third = pcdet_bind.install(roiaware_pool=True)
        assert sys.modules[name] is foreign and third[name] is foreign
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
