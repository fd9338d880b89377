"""CPU: tests/anchor_targets_seq.py (the numpy restatement the GPU tests compare with) reproduces every output that
tools/make_golden_anchor_targets.py recorded from the reference's own AxisAlignedTargetAssigner -- labels, weights and
every target column bit for bit, the two sincos columns to the bound derived in DESIGN.md section 7i -- and the fixture
holds every case it promises.  Also: the header / ctypes mirror of the new entry points, no scratch in the kernels, the
options that are not provided, the output layout table and the opt-in binding."""
import json
import os
import sys
import types

import numpy as np
import pytest

import anchor_targets_seq as seq
from modest_amd.utils import target_assigner as ta

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "anchor_targets.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def test_fixture_is_small(gold):
    assert os.path.getsize(GOLD) <= os.path.getsize(os.path.join(os.path.dirname(GOLD), "pointnet2_batch.npz"))
    assert [n for n, _, _ in seq.scenes(gold)] == ["small", "big", "multi", "lyft", "crowd", "crowd_multi"]


def test_restatement_reproduces_the_reference(gold):
    for name, cfg, gt in seq.scenes(gold):
        anchors = seq.make_anchors(cfg)
        ours = seq.assign(cfg, anchors, gt)
        why = seq.report(ours, seq.recorded(gold, name), cfg, anchors, gt, sincos_cols_bounded=bool(cfg["sincos"]))
        assert not why, f"{name}\n{why}"
        ref = seq.recorded(gold, name)
        assert ref["box_cls_labels"].dtype == np.int32 and ref["box_reg_targets"].shape[-1] == seq.Coder(cfg).code_size
        assert (ref["box_cls_labels"] > 0).any()


def test_the_comparison_is_not_vacuous(gold):
    name, cfg, gt = seq.scenes(gold)[2]
    assert cfg["sincos"]
    ref = seq.recorded(gold, name)
    fg = np.argwhere(ref["box_cls_labels"] > 0)[0]
    for col, step in ((6, 8), (7, 8), (0, 1), (8, 1)):   # a sincos column past its bound, any other column by one float
        bad = {k: v.copy() for k, v in ref.items()}
        t = bad["box_reg_targets"]
        if step == 1:
            t[fg[0], fg[1], col] = np.nextafter(t[fg[0], fg[1], col], np.float32(9))
        else:
            t[fg[0], fg[1], col] += np.float32(step * 2.0 ** -24)
        assert seq.mismatches(bad, ref, cfg, sincos_cols_bounded=True), col
    ok = {k: v.copy() for k, v in ref.items()}
    ok["box_reg_targets"][fg[0], fg[1], 6] += np.float32(2.0 ** -24)
    assert not seq.mismatches(ok, ref, cfg, sincos_cols_bounded=True) and seq.mismatches(ok, ref, cfg)
    assert seq.SINCOS_BOUND == 5 * 2.0 ** -24
    bad = {k: v.copy() for k, v in ref.items()}
    bad["box_cls_labels"][fg[0], fg[1]] = -1
    assert seq.mismatches(bad, ref, cfg)


def test_fixture_cases(gold):
    cases = seq.fixture_cases(gold)
    assert len(cases) >= 40
    assert all(cases.values()), [k for k, v in cases.items() if not v]


def test_scalars_round_to_float32_as_the_contract_says():
    import torch
    q = torch.tensor([np.nextafter(seq.QUARTER, np.float32(0)), seq.QUARTER, np.nextafter(seq.QUARTER, np.float32(1))])
    assert (q < np.pi / 4).tolist() == [True, False, False]
    assert np.array_equal((q / np.pi).numpy(), q.numpy() / seq.PI32)
    m = np.float32(0.6)
    t = torch.tensor([np.nextafter(m, np.float32(0)), m, np.nextafter(m, np.float32(1))])
    assert (t >= 0.6).tolist() == [False, True, True] and (t < 0.6).tolist() == [True, False, False]
    assert torch.clamp_min(torch.tensor([0.0]), min=1e-5).numpy()[0] == seq.TINY


def test_output_layout_is_the_reference_concatenation():
    shapes = [(1, 5, 7, 1, 2, 7), (1, 5, 7, 2, 2, 7), (1, 5, 7, 1, 1, 7)]
    for multi in (False, True):
        rows, table, n_out = ta.output_layout(shapes, multi)
        assert rows == [70, 140, 35] and n_out == 245
        ids = [np.arange(first, first + n).reshape(s[:5]) for (first, n, *_), s in zip(table, shapes)]
        if multi:
            want = np.concatenate([i.reshape(-1) for i in ids])
        else:
            want = np.concatenate([i.reshape(1, 5, 7, -1) for i in ids], axis=-1).reshape(-1)
        got = np.full(n_out, -1)
        for first, n, k, stride, off in table:
            i = np.arange(n)
            got[(i // k) * stride + off + i % k] = first + i
        assert np.array_equal(got, want), multi
    with pytest.raises(ValueError, match="feature map"):
        ta.output_layout([(1, 5, 7, 1, 2, 7), (1, 4, 7, 1, 2, 7)], False)
    assert ta.output_layout([(1, 5, 7, 1, 2, 7), (1, 4, 7, 1, 2, 7)], True)[2] == 126


def test_options_that_are_not_provided_raise(gold):
    _, cfg, _ = seq.scenes(gold)[0]
    coder = seq.Coder(cfg)
    a = ta.AxisAlignedTargetAssigner(seq.model_cfg(cfg), cfg["class_names"], coder)
    assert a.anchor_class_names == ["Car", "Pedestrian", "Cyclist"] and a.matched_thresholds["Cyclist"] == 0.45
    with pytest.raises(NotImplementedError, match="POS_FRACTION"):
        ta.AxisAlignedTargetAssigner(seq.model_cfg(cfg, pos_fraction=0.5), cfg["class_names"], coder)
    with pytest.raises(NotImplementedError, match="MATCH_HEIGHT"):
        ta.AxisAlignedTargetAssigner(seq.model_cfg(cfg), cfg["class_names"], coder, match_height=True)
    with pytest.raises(NotImplementedError, match="NORM_BY_NUM_EXAMPLES"):
        ta.AxisAlignedTargetAssigner(seq.model_cfg(cfg, norm_by_num_examples=True), cfg["class_names"], coder)


def test_cpu_tensors_are_refused_without_loading_the_library(gold, monkeypatch):
    import torch
    from modest_amd import _lib, ops   # ops before the patch: it binds _lib.load at import

    def no_load(*a, **k):
        raise AssertionError("the library was opened")
    monkeypatch.setattr(_lib, "load", no_load)
    monkeypatch.setattr(ops, "load", no_load)
    _, cfg, gt = seq.scenes(gold)[0]
    a = ta.AxisAlignedTargetAssigner(seq.model_cfg(cfg), cfg["class_names"], seq.Coder(cfg))
    with pytest.raises(ValueError, match="device"):
        a.assign_targets([torch.from_numpy(x) for x in seq.make_anchors(cfg)], torch.from_numpy(gt))


# ------------------------------------------------------------------------------------------------ the binding
def test_binding_is_opt_in():
    import importlib
    from modest_amd.utils import pcdet_bind
    name = "pcdet.models.dense_heads.target_assigner.axis_aligned_target_assigner"
    names = list(pcdet_bind.SHIMS) + list(pcdet_bind.STAND_INS) + ["spconv.utils", name]
    saved = {k: sys.modules.get(k) for k in names}
    try:
        for k in names:
            sys.modules.pop(k, None)
        assert name == pcdet_bind.ANCHOR_TARGETS_NAME and name not in pcdet_bind.SHIMS and name not in pcdet_bind.STAND_INS
        keys = sorted(list(pcdet_bind.SHIMS) + list(pcdet_bind.STAND_INS))
        for kw in ({}, {"sparse_conv": True}, {"point_stack": True}):     # the default call binds nothing new
            bound = pcdet_bind.install(**kw)
            assert sorted(bound) == keys and name not in sys.modules, kw
        bound = pcdet_bind.install(anchor_targets=True)
        assert sorted(bound) == sorted(keys + [name]) and bound[name] is ta and sys.modules[name] is ta
        assert importlib.import_module(name).AxisAlignedTargetAssigner is ta.AxisAlignedTargetAssigner
        again = pcdet_bind.install(anchor_targets=True)                    # idempotent
        assert sorted(again) == sorted(bound) and all(again[k] is bound[k] for k in bound)
        assert sorted(pcdet_bind.install()) == keys and sys.modules[name] is ta   # a later default call leaves it bound
        bound = pcdet_bind.install(stand_ins=False, anchor_targets=True)
        assert sorted(bound) == sorted(list(pcdet_bind.SHIMS) + [name])
        # the reference's module already imported under that name: left alone
        real = sys.modules[name] = types.ModuleType(name)
        assert name not in pcdet_bind.install(anchor_targets=True) and sys.modules[name] is real
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    assert all(sys.modules.get(k) is v for k, v in saved.items())


# ------------------------------------------------------------------------------------------------ the build
def test_header_ctypes_mirror_and_no_scratch():
    import ctypes as C
    import re
    from modest_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "modest_hip.h")).read(), flags=re.S)
    ctype = {"int": C.c_int, "int64_t": C.c_int64}
    for fn in ("modest_anchor_targets", "modest_anchor_targets_workspace_bytes"):
        m = re.search(r"\b(int64_t|int)\s+%s\s*\(([^)]*)\)" % fn, src)
        assert m, fn
        args = [a.strip() for a in m.group(2).split(",")]
        want = [_lib.VP if "*" in a else ctype[a.split()[0]] for a in args]
        res, have = _lib.SIGNATURES[fn]
        assert res is ctype[m.group(1)] and have == want, fn
        assert hasattr(lib, fn)
    assert lib.modest_anchor_targets_workspace_bytes(4, 3, 25) == 4 * 3 * (8 + 7 * 25) * 4
    assert lib.modest_anchor_targets_workspace_bytes(-1, 3, 25) < 0
    res = json.load(open(os.path.join(os.path.dirname(build.LIB), "kernel_resources.json")))
    mine = {k: v for k, v in res.items() if v.get("file") == "anchor_targets.hip"}
    assert len(mine) == 3 and all(any(n in k for k in mine) for n in ("at_select", "at_colmax", "at_assign"))
    assert all(v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 for v in mine.values()), mine


# ------------------------------------------------------------------------------------------------ the benchmark's yardstick
def test_the_benchmark_yardstick_computes_the_reference_results(gold):
    """tools/anchor_targets_bench.py's PyTorch restatement of the reference path, on the CPU, against the recorded outputs"""
    import importlib.util
    import torch
    spec = importlib.util.spec_from_file_location("anchor_targets_bench", os.path.join(os.path.dirname(GOLD), "..", "..", "tools",
                                                                                      "anchor_targets_bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    for name, cfg, gt in seq.scenes(gold):
        anchors = [torch.from_numpy(a) for a in seq.make_anchors(cfg)]
        out = {k: v.numpy() for k, v in bench.yard_assign(cfg, anchors, torch.from_numpy(gt.copy())).items()}
        assert not seq.mismatches(out, seq.recorded(gold, name), cfg, sincos_cols_bounded=bool(cfg["sincos"])), name
