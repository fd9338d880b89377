"""CPU: tests/anchor_loss_seq.py (the numpy restatement the GPU tests compare with bit for bit) against every scene that
tools/make_golden_anchor_loss.py recorded from the reference's own AnchorHeadTemplate.get_loss and its autograd: the direction
bins and the zero pattern of the three gradients exactly, every gradient element and the four scalars -- ours and the recorded
ones -- within the bound exact() derives, no element left out.  Also: the edge cases through the
restatement, the scalar-rounding rules against torch on the CPU, the header / ctypes mirror of the new entry points, no scratch
in the kernels, and CPU tensors refused before the library is opened."""
import json
import os

import numpy as np
import pytest

import anchor_loss_seq as seq
from anchor_loss_cases import CASES

F = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "anchor_loss.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def evaluated(gold):
    """per scene (cfg, inputs, restatement, decisions, exact, recorded): computed once, left unchanged"""
    out = {}
    for name, cfg in seq.scenes(gold):
        inp = seq.make_inputs(cfg)
        ours, dec = seq._evaluate(inp, cfg, None)
        out[name] = (cfg, inp, ours, dec, seq.exact(inp, cfg, dec), seq.recorded(gold, name))
    return out


def test_fixture_is_small_and_holds_its_scenes(gold):
    assert os.path.getsize(GOLD) <= 64 * 1024
    names = [n for n, _ in seq.scenes(gold)]
    assert names == ["kitti", "lyft", "wide", "edge", "l1", "nan6"]
    cfgs = dict(seq.scenes(gold))
    assert all(c["N"] <= 1100 and c["B"] <= 3 for c in cfgs.values())
    assert cfgs["lyft"]["num_class"] == 1 and cfgs["lyft"]["label_max"] == 3 and cfgs["lyft"]["samples"] == ["mixed", "none", "all"]
    assert cfgs["wide"]["code"] == 9 and cfgs["wide"]["bins"] == 4 and cfgs["wide"]["int64"] and cfgs["edge"]["bins"] == 0
    assert cfgs["l1"]["beta"] == 0.0 and "ignore" in cfgs["edge"]["samples"]
    for name, cfg in cfgs.items():
        rec = seq.recorded(gold, name)
        assert rec["losses"].dtype == F and rec["losses"].shape == (4,)
        assert rec["grad_cls"].shape == (cfg["B"], cfg["N"], cfg["num_class"]) and rec["grad_box"].shape[-1] == cfg["code"]
        assert ("grad_dir" in rec) == bool(cfg["bins"])


def test_restatement_and_reference_lie_within_the_derived_bound(evaluated):
    worst = {}
    for name, (cfg, inp, ours, dec, ex, rec) in evaluated.items():
        assert set(ours) == set(rec) == set(ex), name
        for who, got in (("ours", ours), ("reference", rec)):
            why, ratios = seq.bound_report(got, ex, who)
            assert not why, f"{name}\n{why}"
            for k, v in ratios.items():
                worst[(who, k)] = max(worst.get((who, k), 0.0), v)
    print({f"{w} {k}": round(v, 3) for (w, k), v in sorted(worst.items())})
    assert all(v <= 1.0 for v in worst.values())
    # the bound is a float32 bound, not a loose one: the scalars are held to a few 1e-6 of their size
    cfg, inp, ours, dec, ex, rec = evaluated["kitti"]
    v, e = ex["losses"]
    assert (e[[0, 1, 3]] < 2e-5 * np.abs(v[[0, 1, 3]])).all() and (v[[0, 1, 3]] > 0).all()


def test_zero_patterns_and_direction_bins_are_the_reference_ones(evaluated):
    for name, (cfg, inp, ours, dec, ex, rec) in evaluated.items():
        assert not seq.zero_report(ours, rec), name
        pos = inp["labels"] > 0
        assert (ours["grad_box"][~pos] == 0).all() and np.array_equal(dec["count"], pos.sum(axis=1))
        if cfg["bins"]:
            # softmax - onehot is negative in the target's bin alone
            assert (ours["grad_dir"][~pos] == 0).all()
            ref_bin = np.argmin(rec["grad_dir"], axis=-1)
            assert ((rec["grad_dir"] < 0).sum(axis=-1)[pos] == 1).all(), name
            assert np.array_equal(ref_bin[pos], dec["bin"][pos]), name
            assert len(np.unique(dec["bin"][pos])) == cfg["bins"], name     # every bin occurs


def test_nan_scene_and_kink_scene_say_what_the_contract_says(evaluated):
    cfg, inp, ours, dec, ex, rec = evaluated["nan6"]
    # a NaN in a target's column 6: the encoded input is a NaN as well, so the replacement keeps it -- as the reference
    for got in (ours, rec):
        assert np.isnan(got["losses"][[1, 3]]).all() and not np.isnan(got["losses"][[0, 2]]).any()
        assert np.isnan(got["grad_box"]).sum() == 1 and not np.isnan(got["grad_cls"]).any()
    cfg, inp, ours, dec, ex, rec = evaluated["edge"]
    # a NaN in column 2 is replaced: no NaN anywhere, gradient 0 there; d == 0: gradient 0; |d| == beta: the second branch
    rows = np.flatnonzero(inp["labels"][0] > 0)
    for got in (ours, rec):
        assert not any(np.isnan(v).any() for v in got.values())
        assert got["grad_box"][0, rows[7], 2] == 0 and got["grad_box"][0, rows[6], 1] == 0
    assert np.isnan(inp["tg"][0, rows[7], 2]) and dec["replaced"][0, rows[7], 2] and not dec["quad"][0, rows[6], 0]
    g = F(cfg["loc_weight"]) / F(cfg["B"]) * (F(1) / F(dec["count"][0]))
    assert ours["grad_box"][0, rows[6], 0] == g and abs(rec["grad_box"][0, rows[6], 0] - g) <= 2 * seq.U * g
    # the kink: at a logit of exactly +-0 the bce derivative is 1 - t, not s - t
    x = inp["cls"][0]
    zero = np.argwhere(x == 0)
    assert len(zero) >= 4 and np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
    assert {30.0, -30.0, 100.0, -100.0} <= set(np.unique(x).tolist())


def test_the_comparison_is_not_vacuous(evaluated):
    cfg, inp, ours, dec, ex, rec = evaluated["kitti"]
    pos = np.argwhere(inp["labels"] > 0)[0]
    for name, idx in (("grad_cls", (pos[0], pos[1], 0)), ("grad_box", (pos[0], pos[1], 6)), ("grad_dir", (pos[0], pos[1], 1)),
                      ("losses", (3,))):
        bad = {k: v.copy() for k, v in ours.items()}
        bad[name][idx] = bad[name][idx] * F(1 + 2e-5)
        assert name in seq.bound_report(bad, ex)[0], name
        assert name in seq.report(bad, ours), name
        step = {k: v.copy() for k, v in ours.items()}
        step[name][idx] = np.nextafter(step[name][idx], F(9))
        assert name in seq.report(step, ours) and not seq.report(ours, ours)
    bad = {k: v.copy() for k, v in ours.items()}
    bad["grad_box"][0, np.flatnonzero(inp["labels"][0] <= 0)[0], 3] = F(1e-30)
    assert "grad_box" in seq.zero_report(bad, rec)
    bad = {k: v.copy() for k, v in ours.items()}
    bad["grad_cls"][0, 0, 0] = F(np.nan)
    assert "grad_cls" in seq.bound_report(bad, ex)[0]


@pytest.mark.parametrize("name", sorted(CASES))
def test_edge_cases_through_the_restatement(name):
    cfg = CASES[name]
    inp = seq.make_inputs(cfg)
    ours, dec = seq._evaluate(inp, cfg, None)
    why, ratios = seq.bound_report(ours, seq.exact(inp, cfg, dec))
    assert not why, why
    pos = inp["labels"] > 0
    assert (ours["grad_box"][~pos] == 0).all() and (ours["grad_cls"][inp["labels"] < 0] == 0).all()
    for b, mode in enumerate(cfg["samples"]):
        assert dec["count"][b] == {"none": 0, "ignore": 0, "all": cfg["N"]}.get(mode, dec["count"][b])
    if "label_above" in name:
        above = inp["labels"] > cfg["num_class"]
        assert above.any() and (ours["grad_box"][above] != 0).any()
        t_grad = ours["grad_cls"][above]                 # no class column is the target: every column pushes down
        assert (t_grad >= 0).all()
    if name == "nan6":
        assert np.isnan(ours["losses"][3])
    else:
        assert not any(np.isnan(v).any() for v in ours.values())


def test_tree_sum_is_the_written_tree():
    rs = np.random.RandomState(5)
    lanes = rs.uniform(0, 1, size=(3, 1040)).astype(F)
    got = seq.tree_sum(lanes)
    # by hand: butterflies of 64, (w0 + w1) + (w2 + w3), strided partials, the same tree again
    pad = np.zeros((3, 5 * 256), dtype=F)
    pad[:, :1040] = lanes
    part = []
    for b in range(3):
        for blk in range(5):
            w = []
            for q in range(4):
                v = pad[b, blk * 256 + q * 64: blk * 256 + (q + 1) * 64].copy()
                for off in (32, 16, 8, 4, 2, 1):
                    v = v + v[np.arange(64) ^ off]
                w.append(v[0])
            part.append((w[0] + w[1]) + (w[2] + w[3]))
    acc = np.zeros(256, dtype=F)
    acc[:15] = np.array(part, dtype=F)
    w = []
    for q in range(4):
        v = acc[q * 64:(q + 1) * 64].copy()
        for off in (32, 16, 8, 4, 2, 1):
            v = v + v[np.arange(64) ^ off]
        w.append(v[0])
    assert got == (w[0] + w[1]) + (w[2] + w[3])
    assert abs(float(got) - lanes.astype(np.float64).sum()) <= seq.tree_depth(3, 1040, 0) * seq.U * lanes.sum()
    assert seq.tree_depth(4, 321408, 3) == 3 + 8 + 20 + 8


def test_scalars_round_to_float32_as_the_contract_says():
    import torch
    # n < beta at n = float32(1 / 9): the second branch, as with beta rounded to float32
    n = F(1.0 / 9.0)
    t = torch.tensor([np.nextafter(n, F(0)), n, np.nextafter(n, F(1))])
    assert (t < 1.0 / 9.0).tolist() == [True, False, False] == (t.numpy() < F(1.0 / 9.0)).tolist()
    assert np.array_equal((0.5 * t ** 2 / (1.0 / 9.0)).numpy(), (F(0.5) * (t.numpy() * t.numpy())) / F(1.0 / 9.0))
    assert np.array_equal((t - 0.5 * (1.0 / 9.0)).numpy(), t.numpy() - seq.scalars32(dict(beta=1.0 / 9.0, bins=2, dir_offset=0, cls_weight=1,
                                                                                      loc_weight=1, dir_weight=1, B=1))["half_beta"])
    # 2 pi / bins and the period: the Python double, rounded once
    x = torch.from_numpy(np.random.RandomState(1).uniform(-20, 20, 4000).astype(F))
    for bins in (2, 3, 4, 6, 8):
        assert np.array_equal((x / (2 * np.pi / bins)).numpy(), x.numpy() / F(2 * np.pi / bins))
    lim = x - torch.floor(x / (2 * np.pi) + 0) * (2 * np.pi)
    assert np.array_equal(lim.numpy(), x.numpy() - np.floor(x.numpy() / F(2 * np.pi) + F(0)) * F(2 * np.pi))
    assert np.array_equal((x - 0.78539).numpy(), x.numpy() - F(0.78539))
    # 1.0 / cnt
    cnt = torch.arange(1, 3000).float()
    w = torch.ones(2999)
    w /= torch.clamp(cnt, min=1.0)
    assert np.array_equal(w.numpy(), F(1.0) / np.arange(1, 3000).astype(F))
    # the kink: torch's clamp passes its gradient at 0 and -0, its abs passes none
    for t_ in (0.0, 1.0):
        xz = torch.tensor([0.0, -0.0], requires_grad=True)
        bce = torch.clamp(xz, min=0) - xz * t_ + torch.log1p(torch.exp(-torch.abs(xz)))
        bce.sum().backward()
        assert xz.grad.tolist() == [1.0 - t_, 1.0 - t_]
    # the focal power and the loss weights
    p = torch.tensor([0.3, 0.7])
    assert np.array_equal(torch.pow(p, 2.0).numpy(), p.numpy() * p.numpy())


def test_restatement_takes_the_kink_as_torch_does():
    import torch
    cfg = seq.base_cfg(B=1, N=70, num_class=2, bins=0, seed=3, pos=0.3)
    inp = seq.make_inputs(cfg)
    inp["cls"][0, :10, 0] = F(0.0)
    inp["cls"][0, 10:20, 1] = F(-0.0)
    ours = seq.restate(inp, cfg)
    head, preds = seq.bare_head(cfg, inp)
    x = preds["cls"]
    labels = torch.from_numpy(inp["labels"].astype(np.int64))
    t = torch.nn.functional.one_hot(labels.clamp(min=0), 3)[..., 1:].float()
    w = ((labels >= 0).float() / (labels > 0).sum(1, keepdim=True).clamp(min=1).float()).unsqueeze(-1)
    s = torch.sigmoid(x)
    pt = t * (1.0 - s) + (1.0 - t) * s
    loss = (t * 0.25 + (1 - t) * 0.75) * torch.pow(pt, 2.0) * (torch.clamp(x, min=0) - x * t + torch.log1p(torch.exp(-torch.abs(x)))) * w
    (loss.sum() / 1 * cfg["cls_weight"]).backward()
    got, ref = ours["grad_cls"][0, :20], x.grad.numpy()[0, :20]
    assert np.allclose(got, ref, rtol=1e-5, atol=1e-9) and (np.abs(ref[:10, 0]) > 0).any()


def test_cpu_tensors_are_refused_without_loading_the_library(monkeypatch):
    import torch
    from modest_amd import _lib, ops   # ops before the patch: it binds _lib.load at import

    def no_load(*a, **k):
        raise AssertionError("the library was opened")
    monkeypatch.setattr(_lib, "load", no_load)
    monkeypatch.setattr(ops, "load", no_load)
    cfg = CASES["n70"]
    inp = seq.make_inputs(cfg)
    t = {k: torch.from_numpy(v) for k, v in inp.items() if v is not None}
    with pytest.raises(ValueError, match="device"):
        ops.anchor_loss(t["cls"], t["box"], t["dir"], t["labels"], t["tg"], t["anchors"], t["cw"])
    with pytest.raises(ValueError, match="device"):
        ops.anchor_loss_backward((t["cls"], t["box"], None), torch.ones(1))
    from modest_amd.utils import anchor_head_loss
    head, _ = seq.bare_head(cfg, inp)
    with pytest.raises(ValueError, match="cls_preds must be a device tensor"):
        anchor_head_loss.get_loss(head)


# ------------------------------------------------------------------------------------------------ the build
def test_header_ctypes_mirror_and_no_scratch():
    import ctypes as C
    import re
    from modest_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "modest_hip.h")).read(), flags=re.S)
    ctype = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float}
    for fn in ("modest_anchor_loss", "modest_anchor_loss_backward", "modest_anchor_loss_workspace_bytes"):
        m = re.search(r"\b(int64_t|int)\s+%s\s*\(([^)]*)\)" % fn, src)
        assert m, fn
        args = [a.strip() for a in m.group(2).split(",")]
        want = [_lib.VP if "*" in a else ctype[a.split()[0]] for a in args]
        res, have = _lib.SIGNATURES[fn]
        assert res is ctype[m.group(1)] and have == want, fn
        assert hasattr(lib, fn)
    blocks = lambda n: (n + 255) // 256        # noqa: E731
    up = lambda v: (v + 255) // 256 * 256      # noqa: E731
    assert lib.modest_anchor_loss_workspace_bytes(4, 321408) == up(4 * 4) + up(4 * 3 * 4 * blocks(321408))
    assert lib.modest_anchor_loss_workspace_bytes(65536, 10) < 0 and lib.modest_anchor_loss_workspace_bytes(1, -1) < 0
    assert b"65535" in lib.modest_last_error()
    res = json.load(open(os.path.join(os.path.dirname(build.LIB), "kernel_resources.json")))
    mine = {k: v for k, v in res.items() if v.get("file") == "anchor_loss.hip"}
    assert len(mine) == 4 and all(any(n in k for k in mine) for n in ("al_count", "al_loss", "al_finish", "al_scale"))
    assert all(v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 for v in mine.values()), mine


# ------------------------------------------------------------------------------------------------ the benchmark's yardstick
def test_the_benchmark_yardstick_computes_the_reference_results(evaluated):
    """tools/anchor_loss_bench.py's restatement of the reference path in stock PyTorch operators, on the CPU, against the
    recorded outputs: the same operators in the same order give the same bits"""
    import importlib.util
    import torch
    spec = importlib.util.spec_from_file_location("anchor_loss_bench", os.path.join(os.path.dirname(GOLD), "..", "..", "tools",
                                                                                   "anchor_loss_bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    for name, (cfg, inp, ours, dec, ex, rec) in evaluated.items():
        head, preds = seq.bare_head(cfg, inp)
        loss, tb = bench.yard_get_loss(head)
        loss.backward()
        got = dict(losses=np.array([tb["rpn_loss_cls"], tb["rpn_loss_loc"], tb.get("rpn_loss_dir", 0.0), tb["rpn_loss"]], dtype=F),
                   grad_cls=preds["cls"].grad.numpy(), grad_box=preds["box"].grad.numpy())
        if "dir" in preds:
            got["grad_dir"] = preds["dir"].grad.numpy()
        assert not seq.report(got, rec, "the yardstick"), name
