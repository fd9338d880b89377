"""CPU: tests/roi_loss_seq.py (the numpy restatement the GPU tests compare with bit for bit) against every scene that
tools/make_golden_roi_loss.py recorded from the reference's own RoIHeadTemplate.get_loss and its autograd: fg_sum and the zero
pattern of the two gradients exactly, every gradient element and the scalars -- ours and the recorded ones -- within the bound
exact() derives, no element left out, the ratios recomputed.  Also: the edge cases through the
restatement, every rule of the contract against torch's operators on the CPU, deliberate mis-statements of the contract that
each must change a named case, the tree reused from section 7p, the header / ctypes mirror of the new entry points, no scratch
in the kernels, CPU tensors refused before the library is opened, and the benchmark's yardstick against the fixture."""
import json
import os

import numpy as np
import pytest

import anchor_loss_seq
import roi_loss_seq as seq
from roi_loss_cases import CASES, MAY_HOLD_NAN

F = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "roi_loss.npz")
EDGES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "roi_loss_edges.npz")
SCENES = ["pointrcnn", "pvrcnn", "nofg", "nocorner", "wide", "edge"]


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


_cases = {}


def case(name):
    """(cfg, inputs, restatement, decisions) of a case: computed once, left unchanged"""
    if name not in _cases:
        cfg = CASES[name]
        inp = seq.make_inputs(cfg)
        _cases[name] = (cfg, inp) + seq._evaluate(inp, cfg, None)
    return _cases[name]


def test_fixture_is_small_and_holds_its_scenes(gold):
    assert os.path.getsize(GOLD) <= 64 * 1024
    assert [n for n, _ in seq.scenes(gold)] == SCENES
    cfgs = dict(seq.scenes(gold))
    assert (cfgs["pointrcnn"]["B"], cfgs["pointrcnn"]["M"], cfgs["pointrcnn"]["labels"]) == (2, 128, "cls")
    assert (cfgs["pvrcnn"]["B"], cfgs["pvrcnn"]["M"], cfgs["pvrcnn"]["labels"]) == (3, 64, "iou")
    assert cfgs["pvrcnn"]["samples"] == ["mixed", "nofg", "allfg"] and cfgs["nofg"]["samples"] == ["nofg", "nofg"]
    assert not cfgs["nocorner"]["corner"] and all(c["corner"] for n, c in cfgs.items() if n != "nocorner")
    assert cfgs["wide"]["code"] == 9 and len(set(cfgs["wide"]["code_weights"])) > 1
    assert len({cfgs["wide"][k] for k in ("cls_weight", "reg_weight", "corner_weight")}) == 3
    assert cfgs["edge"]["specials"] == seq.EDGE_RECORDED
    for name, cfg in cfgs.items():
        rec, R = seq.recorded(gold, name), cfg["B"] * cfg["M"]
        assert rec["table"].dtype == F and rec["table"].shape == (6,)
        assert rec["grad_cls"].shape == (R,) and rec["grad_reg"].shape == (R, cfg["code"])
    # ignored rows in the hard-label scene, none of them counted
    inp = seq.make_inputs(cfgs["pointrcnn"])
    assert (inp["labels"] < 0).sum() > 10 and seq.recorded(gold, "pointrcnn")["table"][5] == (inp["labels"] >= 0).sum()


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
    cfg, inp, ours, dec, ex, rec = evaluated["pointrcnn"]
    v, e = ex["table"]
    assert (e[:4] < 2e-5 * np.abs(v[:4])).all() and (v[:4] > 0).all() and (e[4:] == 0).all()


def test_zero_patterns_and_counts_are_the_reference_ones(evaluated):
    for name, (cfg, inp, ours, dec, ex, rec) in evaluated.items():
        assert not seq.zero_report(ours, rec), name
        fg, valid = inp["mask"] > 0, inp["labels"] >= 0
        assert ours["table"][4] == rec["table"][4] == fg.sum() and ours["table"][5] == rec["table"][5] == valid.sum(), name
        assert (ours["grad_reg"][~fg] == 0).all() and (ours["grad_cls"][~valid] == 0).all()
        assert (ours["table"][2] != 0) == (bool(cfg["corner"]) and fg.any()) == (rec["table"][2] != 0), name
    cfg, inp, ours, dec, ex, rec = evaluated["pvrcnn"]
    per_sample = (inp["mask"] > 0).reshape(3, 64).sum(axis=1)
    assert per_sample[1] == 0 and per_sample[2] == 64 and 0 < per_sample[0] < 64
    cfg, inp, ours, dec, ex, rec = evaluated["wide"]
    assert (ours["grad_reg"][inp["mask"] > 0][:, 7:] != 0).all()          # the extra columns take part in the smooth L1


def test_the_edge_scene_says_what_the_contract_says(evaluated):
    cfg, inp, ours, dec, ex, rec = evaluated["edge"]
    rows = np.arange(0, 120, 3)
    x = inp["cls"]
    assert {0.0, 30.0, -30.0, 100.0, -100.0, -80.0} <= set(np.unique(x).tolist())
    assert np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
    assert {0.0, 0.5, 1.0} <= set(np.unique(inp["labels"]).tolist())
    for got in (ours, rec):
        assert not any(np.isnan(v).any() for v in got.values())
        a, b = rows[0], rows[1]
        assert got["grad_reg"][b, 6] != 0          # d == 0 in the smooth L1: what is left is the corner term's share
    # |d| == beta: the linear side, gradient w_reg / fg on top of the corner term's share
    assert not dec["quad"][rows[0], 6] and dec["quad"][rows[1], 6] and dec["sign_d"][rows[1], 6] == 0
    # the prediction that equals its gt: every corner at distance 0 from it, gradient of the corner term 0
    r = rows[2]
    assert all(dec[f"zero_a{k}"][r] and not dec[f"second{k}"][r] for k in range(8))
    noc = seq.restate(inp, dict(cfg, corner=False))
    assert np.array_equal(ours["grad_reg"][r], noc["grad_reg"][r]) and (ours["grad_reg"][rows[3]] != noc["grad_reg"][rows[3]]).all()
    # sizes: the gt's clamped in the encoding, the roi's there and not in the decode
    assert dec["gt_size3"][rows[3]] and dec["gt_size5"][rows[3]] and dec["roi_size4"][rows[4]] and dec["roi_size4"].sum() == 1
    # the NaN target is replaced: gradient of the smooth L1 zero there
    assert np.isnan(inp["gt"][rows[5], 1]) and dec["replaced"][rows[5], 1] and dec["replaced"].sum() == 1
    assert abs(inp["rois"][rows[6], 6]) > np.pi and abs(inp["src"][rows[6], 6]) > np.pi
    # no corner pair ties in a recorded scene; the s that rounds to 1 is floored at -100 and its gradient is exactly 0
    for name, (cfg_, inp_, ours_, dec_, ex_, rec_) in evaluated.items():
        assert not any(dec_[f"tie{k}"][inp_["mask"] > 0].any() for k in range(8) if f"tie{k}" in dec_), name
    big = x >= 30
    assert dec["floor_a"][big].all() and (ours["grad_cls"][big] == 0).all() and (rec["grad_cls"][big] == 0).all()


def test_the_comparison_is_not_vacuous(evaluated):
    cfg, inp, ours, dec, ex, rec = evaluated["pointrcnn"]
    row = np.flatnonzero(inp["mask"] > 0)[0]
    for name, idx in (("grad_cls", (row,)), ("grad_reg", (row, 6)), ("grad_reg", (row, 0)), ("table", (3,)), ("table", (2,))):
        bad = {k: v.copy() for k, v in ours.items()}
        bad[name][idx] = bad[name][idx] * F(1 + 1e-4)
        assert name in seq.bound_report(bad, ex)[0], name
        assert name in seq.report(bad, ours), name
        step = {k: v.copy() for k, v in ours.items()}
        step[name][idx] = np.nextafter(step[name][idx], F(9))
        assert name in seq.report(step, ours) and not seq.report(ours, ours)
    bad = {k: v.copy() for k, v in ours.items()}
    bad["grad_reg"][np.flatnonzero(inp["mask"] <= 0)[0], 3] = F(1e-30)
    assert "grad_reg" in seq.zero_report(bad, rec)
    bad = {k: v.copy() for k, v in ours.items()}
    bad["grad_cls"][0] = F(np.nan)
    assert "grad_cls" in seq.bound_report(bad, ex)[0]
    bad = {k: v.copy() for k, v in ours.items()}
    bad["table"][4] += 1
    assert "fg_sum" in seq.bound_report(bad, ex)[0]


@pytest.mark.parametrize("name", sorted(CASES))
def test_edge_cases_through_the_restatement(name):
    cfg, inp, ours, dec = case(name)
    why, ratios = seq.bound_report(ours, seq.exact(inp, cfg, dec))
    assert not why, why
    fg, valid = inp["mask"] > 0, inp["labels"] >= 0
    assert (ours["grad_reg"][~fg] == 0).all() and (ours["grad_cls"][~valid] == 0).all()
    assert ours["table"][4] == fg.sum() and ours["table"][5] == valid.sum()
    for k, v in ours.items():      # a NaN only in the named outputs of the named cases
        assert np.isnan(v).any() == (k in MAY_HOLD_NAN.get(name, ())), (name, k)
    assert ours["grad_reg"].shape == (cfg["B"] * cfg["M"], cfg["code"]) and inp["gt"].shape[1] == cfg["gt_cols"]
    if not fg.any():
        assert ours["table"][1] == 0 and ours["table"][2] == 0 and ours["table"][3] == ours["table"][0]
    elif name not in MAY_HOLD_NAN:
        assert (ours["grad_reg"][fg] != 0).any() and ours["table"][1] > 0 and (ours["table"][2] > 0) == bool(cfg["corner"])


def test_cases_cover_what_they_name():
    per = lambda name: (case(name)[1]["mask"] > 0).reshape(CASES[name]["B"], -1).sum(axis=1)      # noqa: E731
    assert per("b3").tolist() == [0, 100, 0] and (case("b3")[1]["labels"].reshape(3, 100)[2] < 0).all()
    assert case("all_ignored")[2]["table"].tolist() == [0, 0, 0, 0, 0, 0]
    assert sorted(CASES[n]["B"] * CASES[n]["M"] for n in CASES if n.startswith("r") and n[1].isdigit() and "_" not in n) == [
        1, 63, 64, 65, 255, 256, 257, 1040]
    assert {CASES[n]["code"] for n in CASES} == {7, 8, 9, 16}
    assert {str(case(n)[1]["labels"].dtype) for n in CASES} == {"int32", "int64", "float32"}
    assert {str(case(n)[1]["mask"].dtype) for n in CASES} == {"int32", "int64"}
    # the tie: four corners as far from the gt as from the flipped gt, in different directions; half the gradient to each side
    cfg, inp, ours, dec = case("tie")
    r = 21
    assert all(dec[f"tie{k}"][r] == (k % 2 == 0) and not dec[f"zero_a{k}"][r] for k in range(8))
    whole = seq.restate(inp, cfg, faults=("tie_to_first",))
    assert whole["grad_reg"][r, 0] != ours["grad_reg"][r, 0] and whole["grad_reg"][r, 1] != ours["grad_reg"][r, 1]
    assert not any(dec[f"tie{k}"][np.arange(len(dec["tie0"])) != r].any() for k in range(8))
    # mask values 2 and -1; a logit of -100 against a label above 0 (the contract's sigmoid is not 0 there)
    cfg, inp, ours, dec = case("tie_zero")
    assert inp["mask"][24] == 2 and (ours["grad_reg"][24] != 0).any() and inp["mask"][27] == -1 and (ours["grad_reg"][27] == 0).all()
    cfg, inp, ours, dec = case("edge")
    at = (inp["cls"] == F(-100)) & (inp["labels"] > 0)
    assert at.sum() == 2 and (ours["grad_cls"][at] < 0).all() and (np.abs(ours["grad_cls"][at]) < 1e-30).all()
    # the class column behind the code is not read: another value there, the same results
    cfg, inp, ours, dec = case("strided")
    other = dict(inp, gt=inp["gt"].copy(), src=inp["src"].copy())
    other["gt"][:, 7:], other["src"][:, 7:] = F(np.nan), F(np.inf)
    assert not seq.report(seq.restate(other, cfg), ours)


# ------------------------------------------------------------------------------------------------ the recorded edge scenes
@pytest.fixture(scope="module")
def edges():
    return dict(np.load(EDGES))


def scene_mismatch(cfg, inp, ours, dec, rec):
    """the comparison of a recorded scene -> text, "" when everything agrees: the recorded values and ours within the bound of
    exact() along ours' decisions with NaNs at the same places, and the zero patterns"""
    ex = seq.exact(inp, cfg, dec)
    return "\n".join(line for line in (seq.bound_report(ours, ex, "ours")[0], seq.bound_report(rec, ex, "the reference")[0],
                                       seq.zero_report(ours, rec)) if line)


def test_edges_fixture_is_small_and_holds_the_case_configs(edges):
    assert os.path.getsize(EDGES) <= 64 * 1024
    cfgs = seq.edge_scene_cfgs()
    assert [n for n, _ in seq.scenes(edges)] == list(cfgs)
    for name, cfg in seq.scenes(edges):
        assert cfg == json.loads(json.dumps(cfgs[name])) == json.loads(json.dumps(CASES[name])), name
    assert cfgs["nonfinite_corner"]["corner"] and cfgs["extreme_corner"]["corner"] and cfgs["nonfinite_l1"]["beta"] == 0.0


def test_edge_scenes_lie_within_the_derived_bound(edges):
    worst = {}
    for name, cfg in seq.scenes(edges):
        cfg, inp, ours, dec = case(name)
        rec, ex = seq.recorded(edges, name), seq.exact(inp, cfg, dec)
        why = scene_mismatch(cfg, inp, ours, dec, rec)
        assert not why, f"{name}\n{why}"
        for who, got in (("ours", ours), ("reference", rec)):
            for k, v in seq.bound_report(got, ex, who)[1].items():
                worst[(who, k)] = max(worst.get((who, k), 0.0), v)
        for k, v in rec.items():
            assert np.isnan(v).any() == (k in MAY_HOLD_NAN.get(name, ())), (name, k)
        # the special values sit on foreground rows (the logits on rows that are valid and not foreground)
        fg = inp["mask"] > 0
        assert np.isfinite(inp["reg"][~fg]).all() and np.isfinite(inp["gt"][~fg]).all() and (np.abs(inp["reg"][~fg]) < 10).all()
        assert not np.isfinite(inp["reg"][fg]).all() or (np.abs(inp["reg"][fg]) >= 1e20).any()
    print({f"{w} {k}": round(v, 3) for (w, k), v in sorted(worst.items())})
    assert all(v <= 1.0 for v in worst.values())
    cfg, inp, ours, dec = case("nonfinite_inf")
    assert np.isposinf(ours["table"][[1, 3]]).all() and np.isposinf(seq.recorded(edges, "nonfinite_inf")["table"][[1, 3]]).all()
    cfg, inp, ours, dec = case("extreme_corner")      # squared corner distances past float32: an infinite corner term
    assert np.isposinf(ours["table"][2]) and np.isposinf(seq.recorded(edges, "extreme_corner")["table"][2])
    assert any(dec[f"na_inf{k}"].any() for k in range(8))


def test_the_smooth_l1_gradient_without_the_dead_share_fails_the_recorded_scenes(edges):
    rows = np.arange(0, 120, 3)
    for name, turned in (("nonfinite", [[rows[10], 1], [rows[11], 1], [rows[12], 1], [rows[13], 6], [rows[14], 6], [rows[15], 6], [rows[16], 1],
                                       [rows[17], 6]]),
                         ("nonfinite_corner", [[rows[11], 2], [rows[11], 5], [rows[12], 2], [rows[12], 5], [rows[16], 1], [rows[17], 6]])):
        cfg, inp, ours, dec = case(name)
        rec = seq.recorded(edges, name)
        assert not scene_mismatch(cfg, inp, ours, dec, rec)
        bad, bad_dec = seq._evaluate(inp, cfg, None, (seq.NO_DEAD_SHARE,))
        why = scene_mismatch(cfg, inp, bad, bad_dec, rec)
        assert "grad_reg" in why and seq.report(bad, ours), name
        # the elements the share turns from finite to NaN (with the corner term: its z and dz paths, whose unit vector is
        # z / inf = 0, on top of the smooth L1's own)
        assert np.argwhere(np.isnan(ours["grad_reg"]) & ~np.isnan(bad["grad_reg"])).tolist() == turned, name
        assert np.array_equal(np.isnan(ours["grad_reg"]), np.isnan(rec["grad_reg"]))
    cfg, inp, ours, dec = case("nonfinite_l1")          # WeightedL1Loss has no where(): nothing changes
    assert not seq.report(seq.restate(inp, cfg, (seq.NO_DEAD_SHARE,)), ours)


def test_what_is_not_recorded_is_pinned():
    """outside the contract: a NaN logit, where the reference raises, and -88.9 against a label of 1,
    where a float32 sigmoid is exactly 0"""
    cfg, inp, ours, dec = case("nan_cls")
    at = np.isnan(inp["cls"])
    assert at.sum() == 2 and np.array_equal(np.isnan(ours["grad_cls"]), at) and np.isnan(ours["table"][[0, 3]]).all()
    assert not np.isnan(ours["table"][[1, 2]]).any() and not np.isnan(ours["grad_reg"]).any()
    cfg, inp, ours, dec = case("extreme_sigmoid")
    at = (inp["cls"] == F(-88.9)) & (inp["labels"] > 0)
    assert at.sum() == 1 and (ours["grad_cls"][at] < 0).all() and (np.abs(ours["grad_cls"][at]) < 1e-25).all()


# which case each mis-statement of the contract must change, and in which output
FAULTS = {"decode_clamps_roi": ("edge", "grad_reg"), "flip_by_2pi": ("r63", "table"), "tie_to_first": ("tie", "grad_reg"),
          "reg_reports_corner": ("r63", "table"), "zero_norm_divides": ("tie_zero", "grad_reg"), "corner_on_extra": ("code8", "grad_reg")}


@pytest.mark.parametrize("fault", seq.FAULTS)
def test_a_misstated_contract_changes_its_case(fault):
    name, output = FAULTS[fault]
    cfg, inp, ours, dec = case(name)
    bad = seq.restate(inp, cfg, faults=(fault,))
    with np.errstate(invalid="ignore"):
        changed = bad[output].view(np.uint32) != ours[output].view(np.uint32)
    assert changed.any(), fault
    if fault == "reg_reports_corner":
        assert changed.tolist() == [False, True, False, False, False, False] and bad["table"][1] == ours["table"][1] + ours["table"][2]
    if fault == "decode_clamps_roi":
        assert changed[12].any() and not changed[np.arange(len(changed)) != 12].any()      # the row with a roi size of 0
    if fault == "zero_norm_divides":
        assert np.isnan(bad["grad_reg"][6]).any()                                           # 0 / 0 at the zero distance
    if fault == "corner_on_extra":
        assert changed[:, 7].any() and not changed[:, :7].any()
    # the cases that do not hold the fault's branch stay as they are
    if fault in ("tie_to_first", "zero_norm_divides", "decode_clamps_roi"):
        cfg, inp, ours, dec = case("r63")
        assert not seq.report(seq.restate(inp, cfg, faults=(fault,)), ours)


def test_tree_sum_is_the_one_of_the_anchor_loss():
    assert seq.tree_sum is anchor_loss_seq.tree_sum and seq.Bounded is anchor_loss_seq.Bounded and seq.FUNC_U == anchor_loss_seq.FUNC_U
    cfg, inp, ours, dec = case("r1040")
    # the classification scalar by hand: one lane per row, the tree of section 7p over ONE sample of R lanes (5 workgroups)
    x, t, valid = inp["cls"].astype(np.float64), inp["labels"].astype(F), inp["labels"] >= 0
    s = (1.0 / (1.0 + np.exp(-x))).astype(F)
    lanes = (t - F(1)) * np.log1p(-s.astype(np.float64)).astype(F) - t * np.log(s.astype(np.float64)).astype(F)
    lanes = np.where(valid, lanes, F(0)).astype(F)
    total = anchor_loss_seq.tree_sum(lanes.reshape(1, 1040))
    assert ours["table"][0] == (total / F(valid.sum())) * F(cfg["cls_weight"])
    assert total != lanes.sum(dtype=F) or total != np.cumsum(lanes, dtype=F)[-1]      # not just any order
    assert abs(float(total) - lanes.astype(np.float64).sum()) <= anchor_loss_seq.tree_depth(1, 1040, 0) * seq.U * np.abs(lanes).sum()


def test_every_rule_of_the_contract_against_torch_on_the_cpu():
    import torch
    # ---- the classification term: the form of binary_cross_entropy, its -100 floor, the 1e-12 floor of its gradient
    xs = np.array([0.0, -0.0, 30.0, -30.0, 100.0, -100.0, 1.5, -2.25, 12.0], dtype=F)
    for tv in (0.0, 1.0, 0.5):
        x = torch.from_numpy(xs.copy()).requires_grad_(True)
        s = torch.sigmoid(x)
        s.retain_grad()
        t = torch.full_like(x, tv)
        loss = torch.nn.functional.binary_cross_entropy(s, t, reduction='none')
        (loss * 0.75).sum().backward()
        s32 = s.detach().numpy()
        with np.errstate(divide="ignore"):
            la = np.maximum(np.log1p(-s32.astype(np.float64)).astype(F), F(-100))
            lb = np.maximum(np.log(s32.astype(np.float64)).astype(F), F(-100))
        want = (F(tv) - F(1)) * la - F(tv) * lb
        assert np.allclose(loss.detach().numpy(), want, rtol=3e-7, atol=0), tv          # the form, on torch's own s
        assert (loss.detach().numpy()[2] == 100 * (1 - tv)) and s32[2] == 1 and s32[4] == 1      # s rounds to 1: log1p(-1) floored
        g_s = (F(0.75) * (s32 - F(tv))) / np.maximum((F(1) - s32) * s32, F(1e-12))
        assert np.allclose(s.grad.numpy(), g_s, rtol=3e-7, atol=0), tv                  # (g (s - t)) / max((1 - s) s, 1e-12)
        g_x = (g_s * (F(1) - s32)) * s32
        assert np.allclose(x.grad.numpy(), g_x, rtol=3e-7, atol=1e-45), tv              # the sigmoid's (g (1 - s)) s
        assert x.grad.numpy()[2] == 0 and x.grad.numpy()[4] == 0                        # ... exactly 0 where s is 1
        # what 7q reports: torch's float32 sigmoid is exactly 0 at -100 (exp(100) overflows float32), the contract's is not
        assert s32[5] == 0 and F(1.0 / (1.0 + np.exp(100.0))) > 0
    # torch's CPU kernel refuses a target of -1; with the target clamped the row is finite and masked by 0
    with pytest.raises(RuntimeError, match="between 0 and 1"):
        torch.nn.functional.binary_cross_entropy(torch.tensor([0.5]), torch.tensor([-1.0]))
    # ---- Python's scalars meet float32 tensors as float32
    v = torch.from_numpy(np.random.RandomState(2).uniform(-3, 5, 4000).astype(F))
    assert np.array_equal(torch.clamp_min(v, min=1e-5).numpy(), np.maximum(v.numpy(), F(1e-5)))
    assert np.array_equal((v + np.pi).numpy(), v.numpy() + F(np.pi))
    n = F(1.0 / 9.0)
    t3 = torch.tensor([np.nextafter(n, F(0)), n, np.nextafter(n, F(1))])
    assert (t3 < 1.0 / 9.0).tolist() == [True, False, False]                              # |d| == beta: the linear side
    assert np.array_equal((0.5 * t3 ** 2 / (1.0 / 9.0)).numpy(), (F(0.5) * (t3.numpy() * t3.numpy())) / F(1.0 / 9.0))
    assert np.array_equal((t3 - 0.5 * (1.0 / 9.0)).numpy(), t3.numpy() - seq.scalars32(seq.base_cfg())["half_beta"])
    assert np.array_equal((v.abs() / max(37, 1)).numpy(), np.abs(v.numpy()) / F(37))
    assert np.array_equal((v ** 2).numpy(), v.numpy() * v.numpy())
    # ---- / is correctly rounded in torch as in numpy; torch's vectorised CPU sqrt is not always (it is within one ulp of
    # the correctly rounded root the contract asks for, which is why the bound budgets a whole ulp for a square root)
    a, b = v.abs() + 0.1, torch.flip(v, [0]).abs() + 0.1
    assert np.array_equal((a / b).numpy(), a.numpy() / b.numpy())
    root = np.sqrt(a.numpy())
    assert (np.abs(torch.sqrt(a).numpy().astype(np.float64) - root) <= np.spacing(root)).all()
    assert np.array_equal(root, np.sqrt(a.numpy().astype(np.float64)).astype(F))      # numpy's float32 root: correctly rounded
    # ---- min of two equal values hands half the gradient to each side; the smaller side takes all of it
    p = torch.tensor([1.0, 2.0, 3.0], requires_grad=True)
    q = torch.tensor([1.0, 5.0, 0.5], requires_grad=True)
    (torch.min(p, q) * torch.tensor([3.0, 3.0, 3.0])).sum().backward()
    assert p.grad.tolist() == [1.5, 3.0, 0.0] and q.grad.tolist() == [1.5, 0.0, 3.0]
    # ---- the norm of a zero vector hands on 0; elsewhere g (d / n)
    d = torch.tensor([[0.0, 0.0, 0.0], [3.0, 0.0, 4.0]], requires_grad=True)
    torch.norm(d, dim=1).sum().backward()
    assert d.grad.tolist() == [[0.0, 0.0, 0.0], [F(3) / F(5), 0.0, F(4) / F(5)]]
    # ---- smooth L1 through where: |d| passes sign(d), 0 at d == 0; the quadratic side ((g / beta) 0.5) (2 n)
    d = torch.tensor([0.0, 0.05, -0.05, 0.5, -0.5], requires_grad=True)
    nn_ = torch.abs(d)
    torch.where(nn_ < 1.0 / 9.0, 0.5 * nn_ ** 2 / (1.0 / 9.0), nn_ - 0.5 * (1.0 / 9.0)).sum().backward()
    g = F(1)
    quad = ((g / F(1.0 / 9.0)) * F(0.5)) * (F(2) * F(0.05))
    assert d.grad.tolist() == [0.0, quad, -quad, 1.0, -1.0]
    # ---- a NaN target replaced by the input: no gradient to the input from that column
    i = torch.tensor([0.3, 0.4], requires_grad=True)
    tg = torch.tensor([float("nan"), 0.1])
    tg2 = torch.where(torch.isnan(tg), i, tg)
    torch.abs(i - tg2).sum().backward()
    assert i.grad.tolist() == [0.0, 1.0]


def test_restatement_equals_autograd_on_the_tie_and_zero_distance_rows():
    """the half-and-half tie and the zero norm, through torch's own operators on the CPU (the benchmark's yardstick), against
    the restatement: the rows that no recorded scene holds"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("roi_loss_bench", os.path.join(os.path.dirname(GOLD), "..", "..", "tools", "roi_loss_bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    cfg, inp, ours, dec = case("tie_zero")
    head, preds = seq.bare_head(cfg, inp)
    loss, tb = bench.yard_get_loss(head)
    loss.backward()
    got = preds["reg"].grad.numpy()
    for r in (21, 6):      # the tie row, the zero-distance row
        assert np.allclose(got[r], ours["grad_reg"][r], rtol=2e-5, atol=1e-9), (r, got[r], ours["grad_reg"][r])
    whole = seq.restate(inp, cfg, faults=("tie_to_first",))["grad_reg"]
    assert not np.allclose(got[21], whole[21], rtol=2e-5, atol=1e-9)      # torch does not hand the tie whole to one side
    ex = seq.exact(inp, cfg, dec)
    why, _ = seq.bound_report({"table": ours["table"], "grad_cls": preds["cls"].grad.numpy().reshape(-1), "grad_reg": got}, ex, "autograd")
    assert not why, why


def test_cpu_tensors_are_refused_without_loading_the_library(monkeypatch):
    import torch
    from modest_amd import _lib, ops   # ops before the patch: it binds _lib.load at import

    def no_load(*a, **k):
        raise AssertionError("the library was opened")
    monkeypatch.setattr(_lib, "load", no_load)
    monkeypatch.setattr(ops, "load", no_load)
    cfg, inp, _, _ = case("r63")
    t = {k: torch.from_numpy(v) for k, v in inp.items()}
    with pytest.raises(ValueError, match="rcnn_cls must be a device tensor"):
        ops.roi_loss(t["cls"], t["reg"], t["labels"], t["mask"], t["gt"], t["src"], t["rois"], t["cw"])
    with pytest.raises(ValueError, match="device"):
        ops.roi_loss_backward((t["cls"], t["reg"]), torch.ones(1))
    from modest_amd.utils import roi_head_loss
    head, _ = seq.bare_head(cfg, inp)
    with pytest.raises(ValueError, match="rcnn_cls must be a device tensor"):
        roi_head_loss.get_loss(head)


# ------------------------------------------------------------------------------------------------ the build
def test_header_ctypes_mirror_and_no_scratch():
    import ctypes as C
    import re
    from modest_amd import _lib, build, ops
    build.build(verbose=False)
    lib = _lib.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "modest_hip.h")).read(), flags=re.S)
    ctype = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float}
    for fn in ("modest_roi_loss", "modest_roi_loss_backward", "modest_roi_loss_workspace_bytes", "modest_roi_loss_max_rows"):
        m = re.search(r"\b(int64_t|int)\s+%s\s*\(([^)]*)\)" % fn, src)
        assert m, fn
        args = [a.strip() for a in m.group(2).split(",") if a.strip() != "void"]
        want = [_lib.VP if "*" in a else ctype[a.split()[0]] for a in args]
        res, have = _lib.SIGNATURES[fn]
        assert res is ctype[m.group(1)] and have == want, fn
        assert hasattr(lib, fn)
    up = lambda v: (v + 255) // 256 * 256      # noqa: E731
    assert lib.modest_roi_loss_workspace_bytes(512) == up(4 * 3 * 2) and lib.modest_roi_loss_workspace_bytes(0) == 256
    assert lib.modest_roi_loss_max_rows() == ops.ROI_LOSS_MAX_ROWS == 1 << 20
    assert lib.modest_roi_loss_workspace_bytes(ops.ROI_LOSS_MAX_ROWS + 1) < 0 and lib.modest_roi_loss_workspace_bytes(-1) < 0
    assert b"2^20" in lib.modest_last_error()
    res = json.load(open(os.path.join(os.path.dirname(build.LIB), "kernel_resources.json")))
    mine = {k: v for k, v in res.items() if v.get("file") == "roi_loss.hip"}
    assert len(mine) == 3 and all(any(n in k for k in mine) for n in ("rl_loss", "rl_finish", "rl_scale"))
    assert all(v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 for v in mine.values()), mine


# ------------------------------------------------------------------------------------------------ the benchmark's yardstick
def test_the_benchmark_yardstick_computes_the_reference_results(evaluated):
    """tools/roi_loss_bench.py's restatement of the reference path in stock PyTorch operators, on the CPU, against the
    recorded outputs: the same operators in the same order give the same bits; like the reference it leaves the sizes of the
    dict's gt_of_rois clamped"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("roi_loss_bench", os.path.join(os.path.dirname(GOLD), "..", "..", "tools", "roi_loss_bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    for name, (cfg, inp, ours, dec, ex, rec) in evaluated.items():
        head, preds = seq.bare_head(cfg, inp)
        loss, tb = bench.yard_get_loss(head)
        loss.backward()
        assert ("rcnn_loss_corner" in tb) == (rec["table"][2] != 0), name
        got = dict(table=np.array([tb["rcnn_loss_cls"], tb["rcnn_loss_reg"], tb.get("rcnn_loss_corner", 0.0), tb["rcnn_loss"],
                                   rec["table"][4], rec["table"][5]], dtype=F),
                   grad_cls=preds["cls"].grad.numpy().reshape(-1), grad_reg=preds["reg"].grad.numpy())
        assert not seq.report(got, rec, "the yardstick"), name
        after = head.forward_ret_dict["gt_of_rois"].numpy().reshape(inp["gt"].shape)
        assert (after[:, 3:6] >= F(1e-5)).all() or np.isnan(after[:, 3:6]).any()
    assert (evaluated["edge"][1]["gt"][:, 3:6] <= 0).any()
