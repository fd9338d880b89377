"""CPU: tests/point_loss_seq.py (the numpy restatement the GPU tests compare with bit for bit) against every scene that
tools/make_golden_point_loss.py recorded from the reference's own three get_loss methods and their autograd: point_pos_num and
the zero pattern of the gradients exactly, every gradient element and the scalars -- ours and the recorded ones -- strictly
within the bound exact() derives, no element left out, the ratios recomputed.  Also: the edge cases
through the restatement, every rule of the contract against torch's operators on the CPU, deliberate mis-statements of the
contract that each must change a named case and leave the others, the tree reused from section 7p, the header / ctypes mirror
of the new entry points, no scratch and no spill in the kernels, CPU tensors refused before the library is opened, and the
benchmark's yardstick against the fixture."""
import importlib.util
import json
import os

import numpy as np
import pytest

import anchor_loss_seq
import point_loss_seq as seq
from point_loss_cases import CASES, MAY_HOLD_NAN

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "point_loss.npz")
EDGES = os.path.join(HERE, "golden", "point_loss_edges.npz")
SCENES = ["pointrcnn", "pointrcnn3", "parta2", "parta2_nobox", "pvrcnn", "nopos", "edge"]


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


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("point_loss_bench", os.path.join(HERE, "..", "tools", "point_loss_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_cases = {}


def case(name):
    """(cfg, inputs, restatement, decisions) of a case: computed once, left unchanged"""
    if name not in _cases:
        cfg = CASES[name]
        inp = seq.make_inputs(cfg)
        _cases[name] = (cfg, inp) + seq._evaluate(inp, cfg, None)
    return _cases[name]


def same_bits(a, b):
    return not seq.report(a, b)


def test_fixture_is_small_and_holds_its_scenes(gold):
    assert os.path.getsize(GOLD) <= 64 * 1024
    assert [n for n, _ in seq.scenes(gold)] == SCENES
    cfgs = dict(seq.scenes(gold))
    heads = {n: (c["head"], seq.terms_of(c)) for n, c in cfgs.items()}
    assert heads["pointrcnn"] == heads["pointrcnn3"] == ("PointHeadBox", ("cls", "box"))
    assert heads["parta2"] == ("PointIntraPartOffsetHead", ("cls", "part", "box"))
    assert heads["parta2_nobox"] == ("PointIntraPartOffsetHead", ("cls", "part")) and heads["pvrcnn"] == ("PointHeadSimple", ("cls",))
    c = cfgs["pointrcnn"]
    assert (c["B"], c["N"], c["num_class"], c["code"]) == (2, 128, 1, 8) and cfgs["pointrcnn3"]["num_class"] == 3
    assert cfgs["nopos"]["samples"] == ["none", "none"] and cfgs["edge"]["specials"] == seq.EDGE_RECORDED
    assert {c["int64"] for c in cfgs.values()} == {True, False}
    for name, cfg in cfgs.items():
        rec, R, terms = seq.recorded(gold, name), cfg["B"] * cfg["N"], seq.terms_of(cfg)
        assert 100 <= R <= 400 and rec["table"].dtype == F and rec["table"].shape == (5,)
        assert rec["grad_cls"].shape == (R, cfg["num_class"])
        assert ("grad_part" in rec) == ("part" in terms) and ("grad_box" in rec) == ("box" in terms)
        if "part" in terms:
            inp = seq.make_inputs(cfg)
            assert rec["grad_part"].shape == (R, 3) and inp["part_t"].min() >= 0 and inp["part_t"].max() <= 1
        if "box" in terms:
            assert rec["grad_box"].shape == (R, cfg["code"])
    inp = seq.make_inputs(cfgs["pointrcnn"])
    assert (inp["labels"] < 0).sum() > 10 and (inp["labels"] > 0).sum() > 10       # ignored rows and positives


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
    print("largest error over bound: ours %.3f, reference %.3f" % tuple(
        max(v for (w, _), v in worst.items() if w == who) for who in ("ours", "reference")))
    assert all(v < 1.0 for v in worst.values())                                   # strictly below 1, for both
    # the bound is a float32 bound, not a loose one: the scalars are held to a few 1e-6 of their size
    cfg, inp, ours, dec, ex, rec = evaluated["parta2"]
    v, e = ex["table"]
    assert (e[:4] < 2e-5 * np.abs(v[:4])).all() and (v[:4] > 0).all() and e[4] == 0


def test_zero_patterns_and_point_pos_num_are_the_reference_ones(evaluated):
    for name, (cfg, inp, ours, dec, ex, rec) in evaluated.items():
        assert not seq.zero_report(ours, rec), name
        pos, cared = inp["labels"] > 0, inp["labels"] >= 0
        assert ours["table"][4] == rec["table"][4] == pos.sum(), name
        assert (ours["grad_cls"][~cared] == 0).all() and (ours["grad_cls"][cared] != 0).any()
        for k in ("grad_part", "grad_box"):
            if k in ours:
                assert (ours[k][~pos] == 0).all() and (rec[k][~pos] == 0).all(), (name, k)
        terms = seq.terms_of(cfg)
        assert (ours["table"][1] != 0) == ("part" in terms and pos.any()) == (rec["table"][1] != 0), name
        assert (ours["table"][2] != 0) == ("box" in terms and pos.any()) == (rec["table"][2] != 0), name
    assert evaluated["nopos"][2]["table"][4] == 0 and evaluated["nopos"][2]["table"][0] > 0


def test_the_edge_scene_says_what_the_contract_says(evaluated):
    cfg, inp, ours, dec, ex, rec = evaluated["edge"]
    rows = seq.SPECIAL_ROWS
    x = inp["cls"]
    assert {0.0, 30.0, -30.0, 100.0, -100.0} <= set(np.unique(x).tolist())
    assert np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
    xp = inp["part"]
    assert {0.0, 30.0, -30.0, 100.0, -80.0} <= set(np.unique(xp).tolist()) and not (xp == -100).any()
    assert np.signbit(xp[xp == 0]).any() and not np.signbit(xp[xp == 0]).all()
    assert all(inp["part_t"][rows[8 + j]].tolist() == [0.0, 1.0, 0.5] and inp["labels"][rows[8 + j]] > 0 for j in range(6))
    for got in (ours, rec):
        assert not any(np.isnan(v).any() for v in got.values())
    # the kink of the focal term at a logit of +-0: the derivative of max(x, 0) - x t is 1 - t, on both signs of zero
    for j in (0, 1):
        r = rows[j]
        c = inp["labels"][r] - 1
        for got in (ours, rec):
            assert got["grad_cls"][r, c] < 0 and (np.delete(got["grad_cls"][r], c) > 0).all()
    assert np.array_equal(np.sort(ours["grad_cls"][rows[0]]), np.sort(ours["grad_cls"][rows[1]]))      # +0 and -0: the same values
    # |d| == beta: the linear side; d == 0: gradient 0; the NaN label: replaced, gradient 0
    a, b, n = rows[16], rows[17], rows[18]
    assert not dec["quad"][a, 0] and np.abs(inp["box"][a, 0] * inp["cw"][0]) == F(cfg["beta"])
    assert dec["sign_d"][b, 1] == 0 and ours["grad_box"][b, 1] == 0 and rec["grad_box"][b, 1] == 0
    assert np.isnan(inp["box_t"][n, 2]) and dec["replaced"][n, 2] and dec["replaced"].sum() == 1
    assert ours["grad_box"][n, 2] == 0 and rec["grad_box"][n, 2] == 0 and (ours["grad_box"][n, :2] != 0).all()
    # the part sigmoid that rounds to 1 is floored at -100 and its gradient is exactly 0
    big = (xp >= 30) & (inp["labels"] > 0)[:, None]
    assert big.sum() == 6 and dec["part_floor_a"][big].all() and (ours["grad_part"][big] == 0).all() and (rec["grad_part"][big] == 0).all()


def test_the_comparison_is_not_vacuous(evaluated):
    cfg, inp, ours, dec, ex, rec = evaluated["parta2"]
    row = np.flatnonzero(inp["labels"] > 0)[0]
    for name, idx in (("grad_cls", (row, 0)), ("grad_part", (row, 2)), ("grad_box", (row, 0)), ("table", (3,)), ("table", (1,))):
        bad = {k: v.copy() for k, v in ours.items()}
        bad[name][idx] = bad[name][idx] * F(1 + 1e-4)
        assert name in seq.bound_report(bad, ex)[0], name
        assert name in seq.report(bad, ours), name
        step = {k: v.copy() for k, v in ours.items()}
        step[name][idx] = np.nextafter(step[name][idx], F(9))
        assert name in seq.report(step, ours) and not seq.report(ours, ours)
    bad = {k: v.copy() for k, v in ours.items()}
    bad["grad_box"][np.flatnonzero(inp["labels"] <= 0)[0], 3] = F(1e-30)
    assert "grad_box" in seq.zero_report(bad, rec)
    bad = {k: v.copy() for k, v in ours.items()}
    bad["grad_cls"][0, 0] = F(np.nan)
    assert "grad_cls" in seq.bound_report(bad, ex)[0]
    bad = {k: v.copy() for k, v in ours.items()}
    bad["table"][4] += 1
    assert "point_pos_num" in seq.bound_report(bad, ex)[0]
    less = {k: v for k, v in ours.items() if k != "grad_part"}
    assert "grad_part" in seq.report(less, ours) and "grad_part" in seq.bound_report(less, ex)[0]


@pytest.mark.parametrize("name", sorted(CASES))
def test_edge_cases_through_the_restatement(name):
    cfg, inp, ours, dec = case(name)
    why, ratios = seq.bound_report(ours, seq.exact(inp, cfg, dec))
    assert not why, why
    terms = seq.terms_of(cfg)
    pos, cared = inp["labels"] > 0, inp["labels"] >= 0
    R = cfg["B"] * cfg["N"]
    assert sorted(ours) == sorted(["table", "grad_cls"] + [f"grad_{t}" for t in terms[1:]])
    assert ours["table"][4] == pos.sum() and (ours["grad_cls"][~cared] == 0).all()
    for k, v in ours.items():      # a NaN only in the named outputs of the named cases
        assert np.isnan(v).any() == (k in MAY_HOLD_NAN.get(name, ())), (name, k)
    assert ours["grad_cls"].shape == (R, cfg["num_class"])
    for k, cols in (("grad_part", 3), ("grad_box", cfg["code"])):
        if k in ours:
            assert ours[k].shape == (R, cols) and (ours[k][~pos] == 0).all()
            assert (ours[k][pos] != 0).any() == bool(pos.any())
    if not pos.any():
        assert ours["table"][1] == 0 and ours["table"][2] == 0 and ours["table"][3] == ours["table"][0]


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
        assert set(seq.recorded(edges, name)) == set(case(name)[2]), name
    assert cfgs["nonfinite_l1"]["beta"] == 0.0 and {seq.terms_of(c) for c in cfgs.values()} == {("cls", "box"), ("cls", "part", "box")}


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
        # the special part and box values sit on positive rows
        pos = inp["labels"] > 0
        for k in ("part", "part_t", "box", "box_t"):
            if k in inp:
                assert np.isfinite(inp[k][~pos]).all() and (np.abs(inp[k][~pos]) < 20).all(), (name, k)
    print({f"{w} {k}": round(v, 3) for (w, k), v in sorted(worst.items())})
    assert all(v <= 1.0 for v in worst.values())
    cfg, inp, ours, dec = case("nonfinite_inf")
    assert np.isposinf(ours["table"][[2, 3]]).all() and np.isposinf(seq.recorded(edges, "nonfinite_inf")["table"][[2, 3]]).all()


def test_the_smooth_l1_gradient_without_the_dead_share_fails_the_recorded_scene(edges):
    rows = seq.SPECIAL_ROWS
    cfg, inp, ours, dec = case("nonfinite")
    rec = seq.recorded(edges, "nonfinite")
    assert not scene_mismatch(cfg, inp, ours, dec, rec)
    bad, bad_dec = seq._evaluate(inp, cfg, None, (seq.NO_DEAD_SHARE,))
    why = scene_mismatch(cfg, inp, bad, bad_dec, rec)
    assert "grad_box" in why and seq.report(bad, ours)
    # the elements the share turns from finite to NaN: a NaN or infinite box value, an infinite box label
    assert np.argwhere(np.isnan(ours["grad_box"]) & ~np.isnan(bad["grad_box"])).tolist() == [[rows[26 + j], 1] for j in range(4)]
    assert np.array_equal(np.isnan(ours["grad_box"]), np.isnan(rec["grad_box"]))
    cfg, inp, ours, dec = case("nonfinite_l1")          # WeightedL1Loss has no where(): nothing changes
    assert same_bits(seq.restate(inp, cfg, (seq.NO_DEAD_SHARE,)), ours)


def test_what_is_not_recorded_is_pinned():
    """outside the contract: a NaN part logit, where the reference raises, and -88.9 against a part
    label above 0, where a float32 sigmoid is exactly 0"""
    cfg, inp, ours, dec = case("nan_part")
    at = np.isnan(inp["part"])
    assert at.sum() == 1 and np.array_equal(np.isnan(ours["grad_part"]), at) and np.isnan(ours["table"][[1, 3]]).all()
    assert not np.isnan(ours["table"][[0, 2]]).any()
    cfg, inp, ours, dec = case("extreme_sigmoid")
    at = (inp["part"] == F(-88.9)) & (inp["part_t"] > 0)
    assert at.sum() == 2 and (ours["grad_part"][at] < 0).all() and (np.abs(ours["grad_part"][at]) < 1e-25).all()


def test_cases_cover_what_they_name():
    sizes = sorted(CASES[n]["B"] * CASES[n]["N"] for n in CASES if n.startswith("n") and n[1].isdigit() and "_" not in n)
    assert sizes == [1, 63, 64, 65, 255, 256, 257, 65537]
    assert (65537 + 255) // 256 > 256                                      # pl_finish: a second partial for lane 0
    assert {CASES[n]["num_class"] for n in CASES} == {1, 3, 32} and {CASES[n]["code"] for n in CASES} == {7, 8, 16}
    assert {seq.terms_of(CASES[n]) for n in CASES} == {("cls",), ("cls", "box"), ("cls", "part"), ("cls", "part", "box")}
    assert {CASES[n]["int64"] for n in CASES} == {True, False}
    per = lambda name: (case(name)[1]["labels"] > 0).reshape(CASES[name]["B"], -1).sum(axis=1)      # noqa: E731
    assert per("one_sample").tolist() == [0, 100, 0] and (case("one_sample")[1]["labels"].reshape(3, 100)[2] < 0).all()
    assert per("nopos").tolist() == [0, 0] and per("allpos").tolist() == [70, 70]
    assert case("all_ignored")[2]["table"].tolist() == [0, 0, 0, 0, 0]
    assert per("b2_uneven")[1] == 0 < per("b2_uneven")[0]
    assert CASES["l1"]["beta"] == 0 and len(set(CASES["weights"]["code_weights"])) > 1
    assert len({CASES["weights"][k] for k in ("cls_weight", "part_weight", "box_weight")}) == 3
    # +-100 against part labels above 0: the contract's sigmoid is not 0 at -100, the gradient tiny and not 0
    cfg, inp, ours, dec = case("edge")
    at = (inp["part"] == F(-100)) & (inp["part_t"] > 0)
    assert at.sum() == 2 and (ours["grad_part"][at] < 0).all() and (np.abs(ours["grad_part"][at]) < 1e-30).all()
    assert ((inp["part"] == F(100)) & (inp["part_t"] > 0)).sum() == 2
    # part labels just outside [0, 1]: simply evaluated; a label above num_class: no class column, a positive
    cfg, inp, ours, dec = case("outside")
    r = seq.SPECIAL_ROWS[20]
    assert inp["part_t"][r, 0] > 1 and inp["part_t"][r, 1] < 0 and np.isfinite(ours["grad_part"][r]).all() and (ours["grad_part"][r] != 0).all()
    r = seq.SPECIAL_ROWS[22]
    assert inp["labels"][r] == cfg["num_class"] + 5 and (ours["grad_cls"][r] > 0).all() and (ours["grad_box"][r] != 0).any()
    assert ours["table"][4] == (inp["labels"] > 0).sum()
    # non-finite part and box values in rows that are not positive are not read: other values there, the same results
    a, b = seq.SPECIAL_ROWS[24] + 1, seq.SPECIAL_ROWS[25] + 1
    assert inp["labels"][a] == 0 and inp["labels"][b] == -1
    assert all(np.isnan(inp[k][a]).all() and np.isinf(inp[k][b, :2]).all() for k in ("part", "part_t", "box", "box_t"))
    other = {k: v.copy() for k, v in inp.items()}
    for k in ("part", "part_t", "box", "box_t"):
        other[k][inp["labels"] <= 0] = F(7.5)
    assert same_bits(seq.restate(other, cfg), ours) and np.isfinite(ours["table"]).all()


# which case each mis-statement of the contract must change, in which output, and a case it must leave as it is
FAULTS = {"count_per_sample": ("cls_box", "table", "n257"), "part_divisor_without_3": ("cls_part", "table", "cls_box"),
          "ignored_rows_weighted": ("cls", "grad_cls", "allpos"), "target_at_label": ("cls", "grad_cls", "all_ignored"),
          "box_for_background": ("cls_box", "grad_box", "allpos"), "part_grad_off_positives": ("cls_part", "grad_part", "allpos")}


@pytest.mark.parametrize("fault", seq.FAULTS)
def test_a_misstated_contract_changes_its_case(fault):
    name, output, untouched = FAULTS[fault]
    cfg, inp, ours, dec = case(name)
    bad = seq.restate(inp, cfg, faults=(fault,))
    with np.errstate(invalid="ignore"):
        changed = {k: bad[k].view(np.uint32) != ours[k].view(np.uint32) for k in ours}
    assert changed[output].any(), fault
    pos, cared = inp["labels"] > 0, inp["labels"] >= 0
    if fault == "count_per_sample":
        assert changed["table"].tolist() == [True, False, True, True, False]        # no part term; the count itself is the batch's
    if fault == "part_divisor_without_3":
        assert changed["table"].tolist() == [False, True, False, True, False] and not changed["grad_cls"].any()
        assert abs(bad["table"][1] / ours["table"][1] - 3) < 1e-5
    if fault == "ignored_rows_weighted":
        assert changed["grad_cls"][~cared].any() and not changed["grad_cls"][cared].any() and changed["table"][0]
    if fault == "target_at_label":
        assert changed["grad_cls"][inp["labels"] == 0].any() and changed["grad_cls"][pos].any()
    if fault == "box_for_background":
        assert changed["grad_box"][inp["labels"] == 0].any() and not changed["grad_box"][pos].any() and changed["table"][2]
        assert not changed["grad_box"][~cared].any() and not changed["grad_cls"].any()
    if fault == "part_grad_off_positives":
        assert changed["grad_part"][~pos].any() and not changed["grad_part"][pos].any() and not changed["table"].any()
    # a case that does not hold the fault's branch stays as it is
    cfg, inp, ours, dec = case(untouched)
    assert same_bits(seq.restate(inp, cfg, faults=(fault,)), ours), (fault, untouched)


def test_tree_sum_is_the_one_of_the_anchor_loss():
    assert seq.tree_sum is anchor_loss_seq.tree_sum and seq.Bounded is anchor_loss_seq.Bounded and seq.FUNC_U == anchor_loss_seq.FUNC_U
    cfg, inp, ours, dec = case("cls_part")
    # the part scalar by hand: one lane per point, the tree of section 7p over ONE sample of all B * N lanes (2 workgroups)
    pos = inp["labels"] > 0
    x, t = inp["part"].astype(np.float64), inp["part_t"]
    s = (1.0 / (1.0 + np.exp(-x))).astype(F)
    v = (t - F(1)) * np.log1p(-s.astype(np.float64)).astype(F) - t * np.log(s.astype(np.float64)).astype(F)
    lanes = np.where(pos, (v[:, 0] + v[:, 1]) + v[:, 2], F(0)).astype(F)
    total = anchor_loss_seq.tree_sum(lanes.reshape(1, 260))
    assert ours["table"][1] == (total / F(3 * pos.sum())) * F(cfg["part_weight"])
    assert abs(float(total) - lanes.astype(np.float64).sum()) <= anchor_loss_seq.tree_depth(1, 260, 3) * seq.U * np.abs(lanes).sum()


def test_every_rule_of_the_contract_against_torch_on_the_cpu():
    import torch
    rs = np.random.RandomState(4)
    # ---- the weights: 1.0 / max(P, 1) in float32 for the rows with label >= 0, P over the whole stacked batch
    labels = torch.from_numpy(rs.randint(-1, 4, size=300))
    pos = labels > 0
    w = ((labels == 0) * 1.0 + 1.0 * pos).float()
    w /= torch.clamp(pos.sum(dim=0).float(), min=1.0)
    P = int(pos.sum())
    assert np.array_equal(w.numpy(), np.where(labels.numpy() >= 0, F(1) / F(P), F(0)))
    # ---- the class target: scatter_ of label (ignored rows as 0), the background column dropped: strictly label == c + 1
    onehot = torch.zeros(300, 4)
    onehot.scatter_(-1, (labels * (labels >= 0).long()).unsqueeze(-1), 1.0)
    assert np.array_equal(onehot[:, 1:].numpy(), (labels.numpy()[:, None] == np.arange(3)[None, :] + 1).astype(F))
    with pytest.raises(RuntimeError):
        torch.zeros(2, 4).scatter_(-1, torch.tensor([[4], [1]]), 1.0)                  # a label above num_class
    # ---- the focal term and its four gradient paths, the kink at +-0 included
    xs = np.array([0.0, -0.0, 30.0, -30.0, 100.0, -100.0, 1.5, -2.25], dtype=F)
    for tv in (0.0, 1.0):
        x = torch.from_numpy(xs.copy()).requires_grad_(True)
        t = torch.full_like(x, tv)
        s = torch.sigmoid(x)
        aw = t * 0.25 + (1 - t) * (1 - 0.25)
        pt = t * (1.0 - s) + (1.0 - t) * s
        bce = torch.clamp(x, min=0) - x * t + torch.log1p(torch.exp(-torch.abs(x)))
        wgt = F(1) / F(7)
        ((aw * torch.pow(pt, 2.0) * bce * float(wgt)).sum() * 1.5).backward()
        s32 = s.detach().numpy()
        e = np.exp(-np.abs(xs).astype(np.float64)).astype(F)
        bce32 = (np.maximum(xs, F(0)) - xs * F(tv)) + np.log1p(e.astype(np.float64)).astype(F)
        assert np.allclose(bce.detach().numpy(), bce32, rtol=3e-7, atol=1e-45)
        aw32, oms = F(0.25) if tv else F(0.75), F(1) - s32
        pt32 = oms if tv else s32
        fw = aw32 * (pt32 * pt32)
        gw = F(1.5) * wgt
        g_fw, g_bce = gw * bce32, gw * fw
        c1 = np.where(xs >= 0, g_bce, F(0))
        c2 = -(g_bce * F(tv))
        c3 = (-((g_bce / (e + F(1))) * e)) * np.sign(xs)
        g_pt = (g_fw * aw32) * (F(2) * pt32)
        want = ((c1 + c2) + c3) + ((-g_pt if tv else g_pt) * oms) * s32
        assert np.allclose(x.grad.numpy(), want, rtol=2e-6, atol=1e-30), (tv, x.grad.numpy(), want)
        assert x.grad.numpy()[0] == x.grad.numpy()[1] and (x.grad.numpy()[0] < 0) == bool(tv)      # the kink: 1 - t on both zeros
    # ---- the part term: the form of binary_cross_entropy, its -100 floor, the 1e-12 floor of its gradient, the divisor
    xs = np.array([0.0, -0.0, 30.0, -30.0, 100.0, -80.0, 1.5, -2.25, 12.0], dtype=F)
    for tv in (0.0, 1.0, 0.5):
        x = torch.from_numpy(xs.copy()).requires_grad_(True)
        s = torch.sigmoid(x)
        s.retain_grad()
        t = torch.full_like(x, tv)
        loss = torch.nn.functional.binary_cross_entropy(s, t, reduction='none')
        (loss.sum() / (3 * 7) * 0.75).backward()
        s32 = s.detach().numpy()
        with np.errstate(divide="ignore"):
            la = np.maximum(np.log1p(-s32.astype(np.float64)).astype(F), F(-100))
            lb = np.maximum(np.log(s32.astype(np.float64)).astype(F), F(-100))
        assert np.allclose(loss.detach().numpy(), (F(tv) - F(1)) * la - F(tv) * lb, rtol=3e-7, atol=0), tv
        g = F(0.75) / F(21)
        g_s = (g * (s32 - F(tv))) / np.maximum((F(1) - s32) * s32, F(1e-12))
        assert np.allclose(s.grad.numpy(), g_s, rtol=3e-7, atol=0), tv
        assert np.allclose(x.grad.numpy(), (g_s * (F(1) - s32)) * s32, rtol=3e-7, atol=1e-45), tv
        assert x.grad.numpy()[2] == 0 and x.grad.numpy()[4] == 0                        # exactly 0 where s is 1
    assert torch.sigmoid(torch.tensor([-100.0]))[0] == 0 and F(1.0 / (1.0 + np.exp(100.0))) > 0      # why -100 is not recorded
    v = torch.from_numpy(rs.uniform(0, 5, 4000).astype(F))
    assert np.array_equal((v / (3 * 5592407)).numpy(), v.numpy() / F(3 * 5592407))       # the Python integer, rounded once
    with pytest.raises(RuntimeError, match="between 0 and 1"):
        torch.nn.functional.binary_cross_entropy(torch.tensor([0.5]), torch.tensor([1.0 + 2.0 ** -23]))
    # ---- smooth L1: Python's scalars as float32, |d| == beta on the linear side, sign(0) = 0, the NaN target replaced
    n = F(1.0 / 9.0)
    t3 = torch.tensor([np.nextafter(n, F(0)), n, np.nextafter(n, F(1))])
    assert (t3 < 1.0 / 9.0).tolist() == [True, False, False]
    assert np.array_equal((0.5 * t3 ** 2 / (1.0 / 9.0)).numpy(), (F(0.5) * (t3.numpy() * t3.numpy())) / F(1.0 / 9.0))
    assert np.array_equal((t3 - 0.5 * (1.0 / 9.0)).numpy(), t3.numpy() - seq.scalars32(seq.base_cfg())["half_beta"])
    d = torch.tensor([0.0, 0.05, -0.05, 0.5, -0.5], requires_grad=True)
    nn_ = torch.abs(d)
    torch.where(nn_ < 1.0 / 9.0, 0.5 * nn_ ** 2 / (1.0 / 9.0), nn_ - 0.5 * (1.0 / 9.0)).sum().backward()
    quad = ((F(1) / F(1.0 / 9.0)) * F(0.5)) * (F(2) * F(0.05))
    assert d.grad.tolist() == [0.0, quad, -quad, 1.0, -1.0]
    i = torch.tensor([0.3, 0.4], requires_grad=True)
    tg = torch.tensor([float("nan"), 0.1])
    torch.abs(i - torch.where(torch.isnan(tg), i, tg)).sum().backward()
    assert i.grad.tolist() == [0.0, 1.0]
    # ---- a non-finite value in a row that is not positive poisons the reference's sum through NaN * 0
    assert torch.isnan((torch.tensor([float("nan"), 1.0]) * torch.tensor([0.0, 1.0])).sum())


def test_cpu_tensors_are_refused_without_loading_the_library(monkeypatch):
    import torch
    from modest_amd import _lib, ops   # ops before the patch: it binds _lib.load at import

    def no_load(*a, **k):
        raise AssertionError("the library was opened")
    monkeypatch.setattr(_lib, "load", no_load)
    monkeypatch.setattr(ops, "load", no_load)
    cfg, inp, _, _ = case("cls_part_box")
    t = {k: torch.from_numpy(v) for k, v in inp.items()}
    with pytest.raises(ValueError, match="cls_preds must be a device tensor"):
        ops.point_loss(t["cls"], t["labels"], t["part"], t["part_t"], t["box"], t["box_t"], t["cw"])
    with pytest.raises(ValueError, match="device"):
        ops.point_loss_backward((t["cls"], None, None), torch.ones(1))
    with pytest.raises(ValueError, match="part_preds and part_labels come together"):
        ops.point_loss(t["cls"], t["labels"], t["part"], None)
    with pytest.raises(ValueError, match="box_preds, box_labels and code_weights come together"):
        ops.point_loss(t["cls"], t["labels"], None, None, t["box"], t["box_t"], None)
    head, _ = seq.bare_head(cfg, inp)
    with pytest.raises(ValueError, match="point_cls_preds must be a device tensor"):
        head.get_loss()


# ------------------------------------------------------------------------------------------------ the build
def test_header_ctypes_mirror_workspace_limits_and_no_scratch():
    import ctypes as C
    import re
    from modest_amd import _lib, build, ops
    build.build(verbose=False)
    lib = _lib.load()
    root = os.path.dirname(HERE)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "modest_hip.h")).read(), flags=re.S)
    ctype = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float}
    for fn in ("modest_point_loss", "modest_point_loss_backward", "modest_point_loss_workspace_bytes", "modest_point_loss_max_rows"):
        m = re.search(r"\b(int64_t|int)\s+%s\s*\(([^)]*)\)" % fn, src)
        assert m, fn
        args = [a.strip() for a in m.group(2).split(",") if a.strip() != "void"]
        want = [_lib.VP if "*" in a else ctype[a.split()[0]] for a in args]
        res, have = _lib.SIGNATURES[fn]
        assert res is ctype[m.group(1)] and have == want, fn
        assert hasattr(lib, fn)
    up = lambda v: (v + 255) // 256 * 256      # noqa: E731
    # the counter, then three partials per workgroup of 256 points
    assert lib.modest_point_loss_workspace_bytes(0) == 256 + 256 and lib.modest_point_loss_workspace_bytes(512) == 256 + up(4 * 3 * 2)
    assert lib.modest_point_loss_workspace_bytes(65537) == 256 + up(4 * 3 * 257)
    assert lib.modest_point_loss_workspace_bytes(1 << 24) == 256 + 4 * 3 * (1 << 16)
    assert lib.modest_point_loss_max_rows() == ops.POINT_LOSS_MAX_ROWS == 1 << 24
    assert (ops.POINT_LOSS_MAX_CLASS, ops.POINT_LOSS_MAX_CODE, ops.POINT_LOSS_PART) == (32, 16, 3)
    assert float(F(1 << 24)) == (1 << 24) and float(F((1 << 24) + 1)) != (1 << 24) + 1                 # why 2^24: the count stays exact in float32
    assert lib.modest_point_loss_workspace_bytes(ops.POINT_LOSS_MAX_ROWS + 1) < 0 and lib.modest_point_loss_workspace_bytes(-1) < 0
    assert b"2^24" in lib.modest_last_error()
    # the argument refusals launch nothing and need no device: every limit one step past it
    args = lambda N, Cn, code, box=1: (N, Cn, code, None, None, 0, None, None, box or None, box or None, box or None, 0.1, 1.0, 1.0,      # noqa: E731
                                       1.0, None, None, None, None, None, 0, None)
    for a, text in (((4, 0, 8), b"num_class between 1 and 32"), ((4, 33, 8), b"num_class between 1 and 32"),
                    ((4, 1, 0), b"code size between 1 and 16"), ((4, 1, 17), b"code size between 1 and 16"),
                    ((-1, 1, 8), b"n_rows between 0 and 2^24"), (((1 << 24) + 1, 1, 8), b"n_rows between 0 and 2^24"),
                    ((4, 1, 8), b"NULL or unaligned buffer")):
        assert lib.modest_point_loss(*args(*a)) != 0
        assert text in lib.modest_last_error(), (a, lib.modest_last_error())
    assert lib.modest_point_loss_backward(-1, 0, 0, None, None, None, None, None) != 0
    assert lib.modest_point_loss_backward(4, 0, 0, None, None, None, None, None) != 0 and b"NULL buffer" in lib.modest_last_error()
    assert lib.modest_point_loss_backward(0, 0, 0, None, None, None, None, None) == 0
    res = json.load(open(os.path.join(os.path.dirname(build.LIB), "kernel_resources.json")))
    mine = {k: v for k, v in res.items() if v.get("file") == "point_loss.hip"}
    assert len(mine) == 4 and all(any(n in k for k in mine) for n in ("pl_count", "pl_loss", "pl_finish", "pl_scale"))
    assert all(v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 for v in mine.values()), mine
    print({k: (v["VGPRs"], v["TotalSGPRs"], v["LDS Size [bytes/block]"], v["Occupancy [waves/SIMD]"]) for k, v in mine.items()})


# ------------------------------------------------------------------------------------------------ the benchmark's yardstick
def test_the_benchmark_yardstick_computes_the_reference_results(evaluated, bench):
    """tools/point_loss_bench.py's restatement of the reference path in stock PyTorch operators, on the CPU, against the
    recorded outputs: the same operators in the same order give the same bits, and the same keys in the same order"""
    for name, (cfg, inp, ours, dec, ex, rec) in evaluated.items():
        head, preds = seq.bare_head(cfg, inp)
        loss, tb = bench.yard_get_loss(head)
        loss.backward()
        terms = seq.terms_of(cfg)
        assert list(tb) == ["point_loss_cls", "point_pos_num"] + (["point_loss_part"] if "part" in terms else []) + (
            ["point_loss_box"] if "box" in terms else []), name
        got = seq.outputs_of(loss.item(), tb, preds)
        assert not seq.report(got, rec, "the yardstick"), name
        assert got["table"][3] == rec["table"][3]


def test_the_yardstick_is_poisoned_where_ours_is_not(bench):
    """a NaN in a box row that is not positive: NaN * 0 reaches the yardstick's sum (and the reference's), not ours"""
    cfg, inp, ours, dec = case("cls_box")
    bad = {k: v.copy() for k, v in inp.items()}
    bad["box"][np.flatnonzero(inp["labels"] == 0)[0], 1] = F(np.nan)
    head, preds = seq.bare_head(cfg, bad)
    loss, tb = bench.yard_get_loss(head)
    assert np.isnan(tb["point_loss_box"]) and same_bits(seq.restate(bad, cfg), ours)
