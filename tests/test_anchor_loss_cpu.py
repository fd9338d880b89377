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
from anchor_loss_cases import CASES, MAY_HOLD_NAN

F = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "anchor_loss.npz")
EDGES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "anchor_loss_edges.npz")


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
def test_edge_cases_through_the_restatement(name, edge_evaluated):
    cfg = CASES[name]
    if name in edge_evaluated:      # a recorded config: evaluated once
        cfg, inp, ours, dec, ex, _ = edge_evaluated[name]
        assert cfg == CASES[name]
    else:
        inp = seq.make_inputs(cfg)
        ours, dec = seq._evaluate(inp, cfg, None)
        ex = seq.exact(inp, cfg, dec)
    why, ratios = seq.bound_report(ours, ex)
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
    # a NaN only in the named outputs of the named cases
    for k, v in ours.items():
        assert np.isnan(v).any() == (k in MAY_HOLD_NAN.get(name, ())), (name, k)
    if name == "nan6":
        assert np.isnan(ours["losses"][3])
    if name == "nonfinite_inf":      # infinities alone: +inf in the scalars, as exact() has it; a NaN in three gradient elements
        assert np.isposinf(ours["losses"][[1, 3]]).all() and np.isnan(ours["grad_box"]).sum() == 3
    if name.startswith("labels_wide"):
        rows = np.arange(0, 40, 3)                       # the fixed positives of a config with specials
        lab = inp["labels"][0, rows[:4]].astype(np.int64)
        if cfg["int64"]:
            assert lab.tolist() == [2 ** 32 + 1, 2 ** 31, -2 ** 40, -2 ** 63]
            # 2^32 + 1 and 2^31 are labels above num_class (positives without a target column), the negative ones are ignored
            assert (ours["grad_box"][0, rows[:2]] != 0).any(axis=-1).all() and (ours["grad_cls"][0, rows[:2]] > 0).all()
            assert (ours["grad_cls"][0, rows[2:4]] == 0).all() and (ours["grad_box"][0, rows[2:4]] == 0).all()
        else:
            assert lab[0] == -7 and (ours["grad_cls"][0, rows[0]] == 0).all() and (ours["grad_box"][0, rows[0]] == 0).all()
    if name == "parts_b2049":
        assert set(np.unique(dec["count"]).tolist()) == {0, 1}


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
    # 2061 partials (9 samples of 229 workgroups): al_finish's lane t adds partials t, t + 256, .. in ascending order, nine rows
    # of them, the last of 13; written with Python loops over the partials of a cheap sum (one value a workgroup)
    B, blocks = 9, 229
    lanes = np.zeros((B, blocks * 256 - 255), dtype=F)                      # N = 58369: the last workgroup holds one anchor
    lanes[:, ::256] = rs.uniform(0, 1, size=(B, blocks)).astype(F)          # one non-zero lane a workgroup: its partial
    part = lanes[:, ::256].reshape(-1)
    assert part.size == 2061
    acc = [F(0)] * 256
    for j in range(part.size):
        acc[j % 256] = acc[j % 256] + part[j]
    w = []
    for q in range(4):
        v = np.array(acc[q * 64:(q + 1) * 64], dtype=F)
        for off in (32, 16, 8, 4, 2, 1):
            v = v + v[np.arange(64) ^ off]
        w.append(v[0])
    want = (w[0] + w[1]) + (w[2] + w[3])
    assert seq.tree_sum(lanes) == want
    # ... and a reader of only the first row, or only the first 8 rows, gives another sum
    assert seq.tree_sum(lanes, rows_read=1) != want and seq.tree_sum(lanes, rows_read=8) != want
    assert seq.tree_sum(lanes, rows_read=9) == want and seq.tree_depth(9, 58369, 0) == 8 + 9 + 8


# ------------------------------------------------------------------------------------------------ the recorded edge scenes
@pytest.fixture(scope="module")
def edges():
    return dict(np.load(EDGES))


@pytest.fixture(scope="module")
def edge_evaluated(edges):
    """per edge scene (cfg, inputs, restatement, decisions, exact, recorded): computed once, left unchanged"""
    out = {}
    for name, cfg in seq.scenes(edges):
        inp = seq.make_inputs(cfg)
        ours, dec = seq._evaluate(inp, cfg, None)
        out[name] = (cfg, inp, ours, dec, seq.exact(inp, cfg, dec), seq.recorded(edges, name))
    return out


def scene_mismatch(cfg, inp, ours, dec, rec, ex=None):
    """the comparison of a recorded scene -> text, "" when everything agrees: the recorded values and ours within the bound
    of exact() along ours' decisions with NaNs at the same places, the zero patterns, and the direction bin read off the
    one negative element of each recorded grad_dir row"""
    ex = seq.exact(inp, cfg, dec) if ex is None else ex
    lines = [seq.bound_report(seq.only(ours, rec), seq.only(ex, rec), "ours")[0],
             seq.bound_report(rec, seq.only(ex, rec), "the reference")[0], seq.zero_report(seq.only(ours, rec), rec)]
    pos = inp["labels"] > 0
    if "grad_dir" in rec and cfg["bins"] > 1:
        rows = pos & ((rec["grad_dir"] < 0).sum(axis=-1) == 1)
        if not rows[pos].all() and "dir_logits" not in cfg["specials"]:      # a saturated softmax leaves 0 in the target's bin
            lines.append("a recorded grad_dir row without exactly one negative element")
        differ = rows & (np.argmin(rec["grad_dir"], axis=-1) != dec["bin"])
        if differ.any():
            b, i = np.argwhere(differ)[0]
            lines.append(f"{int(differ.sum())} direction bins differ, the first at (sample {b}, anchor {i}): heading {inp['tg'][b, i, 6]!r}")
    return "\n".join(line for line in lines if line)


def test_edges_fixture_is_small_and_holds_the_case_configs(edges):
    assert os.path.getsize(EDGES) <= 64 * 1024
    cfgs = seq.edge_scene_cfgs()
    assert [n for n, _ in seq.scenes(edges)] == list(cfgs)
    for name, cfg in seq.scenes(edges):
        assert cfg == json.loads(json.dumps(cfgs[name])) == json.loads(json.dumps(CASES[name])), name
        rec = seq.recorded(edges, name)
        assert set(rec) == set(cfg.get("record", seq.OUTPUTS)), name
        assert cfg["N"] <= 600 or cfg["record"] == ["losses"]
        assert rec["losses"].dtype == F and rec["losses"].shape == (4,)
    assert {(c["bins"], c["dir_offset"]) for n, c in cfgs.items() if n.startswith("dir_edges")} == {
        (2, 0.78539), (3, 0.3), (4, 0.0), (8, 0.78539), (1, 0.0)}
    assert cfgs["nonfinite_l1"]["beta"] == 0.0 and cfgs["layout"]["layout"] == [2, 3]


def test_edge_scenes_lie_within_the_derived_bound(edge_evaluated):
    worst = {}
    for name, (cfg, inp, ours, dec, ex, rec) in edge_evaluated.items():
        why = scene_mismatch(cfg, inp, ours, dec, rec, ex)
        assert not why, f"{name}\n{why}"
        for v, e in ex.values():
            assert not (np.isnan(e) & ~np.isnan(v)).any() and not (np.isinf(e) & np.isfinite(v)).any(), name      # a finite value, a finite bound
        for who, got in (("ours", seq.only(ours, rec)), ("reference", rec)):
            for k, v in seq.bound_report(got, seq.only(ex, rec), who)[1].items():
                worst[(who, k)] = max(worst.get((who, k), 0.0), v)
        for k, v in rec.items():
            assert np.isnan(v).any() == (k in MAY_HOLD_NAN.get(name, ())), (name, k)
    print({f"{w} {k}": round(v, 3) for (w, k), v in sorted(worst.items())})
    assert all(v <= 1.0 for v in worst.values())


def test_direction_bins_at_their_edges(edge_evaluated):
    for name, (cfg, inp, ours, dec, ex, rec) in edge_evaluated.items():
        if not name.startswith("dir_edges"):
            continue
        bins, S = cfg["bins"], seq.scalars32(cfg)
        assert (inp["labels"] > 0).all()
        h = seq.edge_headings(bins, cfg["dir_offset"])
        flat = inp["tg"][..., 6].reshape(-1)
        assert np.array_equal(flat[:2 * h.size:2].view(np.uint32), h.view(np.uint32)) and np.array_equal(flat[:2 * h.size:2], flat[1:2 * h.size:2])
        assert F(-1e-7) in h and F(3e38) in h and F(-50) in h and F(1e4) in h and np.signbit(h[h == 0]).any()
        for j in (-2 * bins, -1, 1, 3 * bins):
            e = F(j * (2 * np.pi / bins) + cfg["dir_offset"])
            assert {e, np.nextafter(e, F(9e9)), np.nextafter(e, F(-9e9))} <= set(h.tolist())
        bin_ = dec["bin"]
        assert len(np.unique(bin_)) == bins                                  # every bin occurs
        if bins == 1:
            assert (rec["grad_dir"] == 0).all() and (ours["grad_dir"] == 0).all()      # softmax of one logit is 1
            continue
        assert ((rec["grad_dir"] < 0).sum(axis=-1) == 1).all() and np.array_equal(np.argmin(rec["grad_dir"], axis=-1), bin_), name
        # a value just below 0 after the offset: lim rounds to 2 pi, the quotient to `bins`, and only the upper clamp keeps
        # the index in range
        val = (inp["tg"][..., 6] + inp["anchors"][None, :, 6]) - S["dir_offset"]
        lim = val - np.floor(val / S["two_pi"] + F(0)) * S["two_pi"]
        top = np.floor(lim / S["bin_width"]) >= bins
        assert top.any() and (val[top] < 0).all() and (val[top] > -1e-6).all() and (bin_[top] == bins - 1).all(), name
        if cfg["dir_offset"] == 0.0:
            assert flat[2 * (h.size - 6)] == F(-1e-7) and top.reshape(-1)[2 * (h.size - 6)]
        # negative and multi-period headings: truncation instead of floor would take another bin
        assert (val < -S["two_pi"]).any() and (val > 2 * S["two_pi"]).any()


def test_layout_scene_is_the_heads_real_layout(edge_evaluated):
    import torch
    cfg, inp, ours, dec, ex, rec = edge_evaluated["layout"]
    tensors = seq.anchor_tensors(cfg, inp["anchors"])
    assert len(tensors) == 3 and all(t.shape == (1, 2, 3, 1, 2, 7) for t in tensors)
    assert len({tuple(t[0, 0, 0, 0, :, 3:].reshape(-1).tolist()) for t in tensors}) == 3      # distinct sizes and rotations
    flat = torch.cat([torch.from_numpy(t) for t in tensors], dim=-3).reshape(-1, 7).numpy()    # as the reference flattens them
    assert np.array_equal(flat, inp["anchors"])
    head, preds = seq.bare_head(cfg, inp)
    assert head.num_anchors_per_location == 6 and [tuple(p.shape) for p in preds.values()] == [(2, 2, 3, 18), (2, 2, 3, 42), (2, 2, 3, 12)]
    # the wrapper's own flattening (the branch for several anchor tensors), without a device
    from modest_amd.utils import anchor_head_loss
    assert np.array_equal(anchor_head_loss._flat_anchors(head).numpy(), inp["anchors"])
    assert anchor_head_loss._flat_anchors(head) is anchor_head_loss._flat_anchors(head)       # built once
    # another order of concatenation changes at least one direction bin of a positive
    pos = inp["labels"] > 0
    for order in ((1, 0, 2), (2, 1, 0), (1, 2, 0)):
        other = np.concatenate(seq.anchor_tensors(cfg, inp["anchors"], order), axis=-3).reshape(-1, 7)
        assert (seq.decisions(dict(inp, anchors=other), cfg)["bin"] != dec["bin"])[pos].any(), order


MUTATIONS = {"trunc_period": "dir_edges_b4", "no_upper_clamp": "dir_edges_b4", "no_dead_share": "nonfinite", "finish_256": "parts2061",
             "finish_2048": "parts2061", "anchor order": "layout"}


@pytest.mark.parametrize("fault", sorted(MUTATIONS))
def test_each_mutation_fails_its_recorded_scene(edge_evaluated, fault):
    cfg, inp, ours, dec, ex, rec = edge_evaluated[MUTATIONS[fault]]
    assert not scene_mismatch(cfg, inp, ours, dec, rec, ex)
    if fault == "anchor order":
        inp = dict(inp, anchors=np.concatenate(seq.anchor_tensors(cfg, inp["anchors"], (1, 0, 2)), axis=-3).reshape(-1, 7))
        bad, bad_dec = seq._evaluate(inp, cfg, None)
    else:
        assert fault in seq.FAULTS
        bad, bad_dec = seq._evaluate(inp, cfg, None, (fault,))
    why = scene_mismatch(cfg, inp, bad, bad_dec, rec, ex if fault.startswith("finish") else None)      # the sum decides no branch
    assert why, fault
    expected = {"trunc_period": "direction bins differ", "no_upper_clamp": "direction bins differ", "no_dead_share": "grad_box",
                "finish_256": "losses", "finish_2048": "losses", "anchor order": "direction bins differ"}[fault]
    assert expected in why, why
    assert seq.report(bad, ours)                    # and the bit-for-bit comparison of the device tests sees it as well
    if fault == "no_dead_share":
        # the elements the share turns from finite to NaN: an infinite or NaN box value, or an infinite target, outside the
        # heading column (there the sine is a NaN already), on a smooth-L1 head
        rows = np.flatnonzero(inp["labels"][0] > 0)
        turned = np.argwhere(np.isnan(ours["grad_box"]) & ~np.isnan(bad["grad_box"])).tolist()
        assert turned == [[0, rows[0], 1], [0, rows[1], 1], [0, rows[2], 1], [0, rows[6], 1]]
        assert np.array_equal(np.isnan(ours["grad_box"]), np.isnan(rec["grad_box"]))
        assert bad["grad_box"][0, rows[0], 1] == 0 and abs(bad["grad_box"][0, rows[1], 1]) > 0
        # with WeightedL1Loss there is no where(): nothing changes
        cfg1, inp1, ours1, *_ = edge_evaluated["nonfinite_l1"]
        assert not seq.report(seq.restate(inp1, cfg1, (fault,)), ours1)


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
