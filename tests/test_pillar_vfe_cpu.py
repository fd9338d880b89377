"""CPU: the arithmetic contract of the PillarVFE / BEV scatter kernels (tests/pillar_vfe_seq.py) against
the reference's own PillarVFE, PointPillarScatter and autograd, recorded in tests/golden/pillar_vfe.npz by
tools/make_golden_pillar_vfe.py.  On every scene the restatement and the recording each lie within the DERIVED float32 bound of
the exact float64 value in every element (out, the running buffers, dW, dgamma, dbeta); the canvas and the features' gradient
equal the recording bit for bit; NaN and inf patterns are equal.  The bound is not vacuous: each deliberately wrong variant of
the restatement leaves it on a recorded scene.  Plus the restatement's own properties on the named cases: the tree's seams, ties,
rows out of range, what a second step does to the buffers."""
import os

import numpy as np
import pytest

import pillar_vfe_seq as seq
from pillar_vfe_cases import CASES, out_of_range_coords

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pillar_vfe.npz")
F, D = np.float32, np.float64
SCENES = ["abs_c64", "rel_c32", "dist_c64", "eval_c32", "two_steps", "eval_dist"]


@pytest.fixture(scope="module")
def gold():
    return {name: (case, rec) for name, case, rec in seq.scenes(dict(np.load(GOLD)))}


@pytest.fixture(scope="module")
def worked(gold):
    """per scene: the exact values with their bounds, the restatement's and the recording's results; computed once"""
    res = {}
    for name, (case, rec) in gold.items():
        train = case["training"]
        ex = seq.exact(case, case["grad"] if train else None)
        ours = seq.restate_steps(case)
        got, theirs = {"out": ours["out"]}, {"out": rec["pillar_features"]}
        if train:
            dW, dg, db = seq.restate_backward(case, ours, case["grad"])
            got.update(running_mean=ours["running_mean"], running_var=ours["running_var"], dW=dW, dgamma=dg, dbeta=db)
            theirs.update({k: rec[k] for k in got if k != "out"})
        res[name] = (ex, got, theirs, ours)
    return res


def test_the_fixture_holds_the_scenes_the_issue_names(gold):
    assert list(gold) == SCENES and os.path.getsize(GOLD) < 100 * 1024
    shapes = {n: c["voxels"].shape + c["W"].shape for n, (c, _) in gold.items()}
    assert all(5 <= s[0] <= 12 and s[1] in (20, 32) and s[2] in (4, 5) and s[3] in (32, 64) for s in shapes.values())
    assert {s[3] for s in shapes.values()} == {32, 64} and {s[1] for s in shapes.values()} == {20, 32}
    assert {bool(c["parts"] & seq.XYZ) for c, _ in gold.values()} == {True, False}
    assert any(c["parts"] & seq.DIST for c, _ in gold.values())
    assert {c["training"] for c, _ in gold.values()} == {True, False} and gold["two_steps"][0]["steps"] == 2
    for case, _ in gold.values():
        num, S = case["num"], case["voxels"].shape[1]
        assert num.dtype == F and case["coords"].dtype == F                      # as load_data_to_gpu hands them over
        assert (num == 1).any() and (num == S).any() and ((num > 1) & (num < S)).any()


@pytest.mark.parametrize("name", SCENES)
def test_restatement_and_recording_within_the_derived_bound(worked, name):
    ex, got, theirs, _ = worked[name]
    assert not ex["margin"], ex["margin"]                  # the winners are decided beyond the error: the gradients' bound holds
    for who, res in (("the restatement", got), ("the recording", theirs)):
        for k, a in res.items():
            why, ratio = seq.bound_report(a, ex[k][0], ex[k][1], f"{name}: {who}: {k}")
            print(f"{name}: {who}: {k}: error / bound = {ratio:.4f}")
            assert not why, why
    for k in got:
        why = seq.pattern_report(got[k], theirs[k], f"{name}: {k}")
        assert not why, why


@pytest.mark.parametrize("name", SCENES)
def test_canvas_gradient_and_buffers_equal_the_recording_bit_for_bit(gold, worked, name):
    case, rec = gold[name]
    B, ny, nx = case["batch_size"], case["ny"], case["nx"]
    why = seq.report(seq.scatter(rec["pillar_features"], case["coords"], B, ny, nx), rec["canvas"], "canvas:")
    assert not why, why
    ours = worked[name][3]
    if case["training"]:
        why = seq.report(seq.scatter_backward(seq.grad_canvas_of(case), case["coords"]), rec["grad_feat"], "grad_feat:")
        assert not why, why
        assert seq.same_bits(seq.grad_feat_of(case), rec["grad_feat"])
        assert int(rec["tracked"]) == ours["tracked"] == case["steps"]
    else:                                                  # eval mode changes no buffer, in the reference as here
        for k in ("running_mean", "running_var"):
            assert seq.same_bits(rec[k], case[k]) and seq.same_bits(ours[k], case[k])
        assert int(rec["tracked"]) == ours["tracked"] == 0 and ours["winner"] is None and ours["sums"] is None


@pytest.mark.parametrize("wrong", seq.WRONG)
def test_the_bound_is_not_vacuous(gold, worked, wrong):
    """a deliberately wrong variant of the restatement leaves the bound on at least one recorded scene"""
    caught = []
    for name, (case, _) in gold.items():
        ex = worked[name][0]
        bad = seq.restate_steps(case, wrong)
        res = {"out": bad["out"]}
        if case["training"]:
            res.update(running_mean=bad["running_mean"], running_var=bad["running_var"])
        if any(seq.bound_report(a, ex[k][0], ex[k][1])[0] for k, a in res.items()):
            caught.append(name)
    assert caught, wrong


def test_padded_slots_win_maxima_and_ties_change_nothing(gold, worked):
    case, _ = gold["abs_c64"]
    ours = worked["abs_c64"][3]
    num = seq.to_int(case["num"])
    padded = ours["winner"] >= num[:, None]
    assert padded.any()                                                          # relu(BN(0)) of a padded slot wins some maxima
    # name the LAST slot of every tie instead of the first: out, dW, dgamma, dbeta keep their bits
    f, W = ours["features"], case["W"]
    mean32, invstd32 = ours["stat"]
    x = seq.linear(f, W)
    y = (x - mean32) * invstd32 * case["gamma"] + case["beta"]
    y = np.where(y > 0, y, F(0))
    S = y.shape[1]
    last = (S - 1 - np.argmax(y[:, ::-1, :], axis=1)).astype(np.uint8)
    assert (last != ours["winner"]).any()
    other = dict(ours, winner=last)
    a, b = seq.restate_backward(case, ours, case["grad"]), seq.restate_backward(case, other, case["grad"])
    assert all(seq.same_bits(u, v) for u, v in zip(a, b))
    assert seq.same_bits(np.take_along_axis(y, last[:, None, :].astype(np.int64), 1)[:, 0], ours["out"])


def test_the_tree_depends_on_the_shape_only():
    """a sum over the tree differs from numpy's pairwise sum, equals a plain loop in the stated order, and its seams are where the
    constants say"""
    rng = np.random.default_rng(7)
    runs = seq.GROUP + 3
    part = rng.standard_normal((runs, 2)) * 10.0 ** rng.integers(-8, 8, (runs, 2))
    total = seq.tree_total(part)
    want = np.zeros(2)
    for g in range(0, runs, seq.GROUP):
        acc = np.zeros(2)
        for r in range(g, min(g + seq.GROUP, runs)):
            acc = acc + part[r]
        want = want + acc
    assert seq.same_bits(total, want)
    flat = np.zeros(2)
    for r in range(runs):
        flat = flat + part[r]
    assert not seq.same_bits(total, flat)                                        # the second seam is felt
    for name in ("run_below", "run_at", "run_above", "group_below", "group_at", "group_above"):
        case = CASES[name]
        P = case["voxels"].shape[0]
        sums = seq.restate(case)["sums"]
        assert np.isfinite(sums).all() and sums.shape == (2 * case["W"].shape[0] + case["W"].size + case["W"].shape[1],), (name, P)


def test_num_0_gives_nan_as_the_reference_and_non_finite_points_spread_as_the_arithmetic_says():
    res = seq.restate(CASES["num_0_train"])
    assert np.isnan(res["out"]).all() and np.isnan(res["running_mean"]).all()   # the statistics take the NaN rows in
    res = seq.restate(CASES["num_0_eval"])
    assert np.isnan(res["out"][1]).all() and np.isfinite(np.delete(res["out"], 1, axis=0)).all()
    res = seq.restate(CASES["nan_point_eval"])
    assert np.isnan(res["out"][1]).all() and np.isfinite(np.delete(res["out"], 1, axis=0)).all()
    fwd = seq.restate(CASES["relu_zeroes_channel"])
    dW, dg, db = seq.restate_backward(CASES["relu_zeroes_channel"], fwd, CASES["relu_zeroes_channel"]["grad"])
    assert not fwd["out"][:, 2].any() and not dW[2].any() and dg[2] == 0 and db[2] == 0
    fwd = seq.restate(CASES["zero_weight_row"])
    assert fwd["stat"][0][3] == 0 and fwd["stat"][1][3] == F(1.0 / np.sqrt(1e-3))   # var = 0: invstd = 1 / sqrt(eps)


def test_scatter_skips_rows_out_of_range_and_its_backward_gives_them_zeros():
    case = CASES["run_at"]
    B, ny, nx = case["batch_size"], case["ny"], case["nx"]
    feat = seq.restate(case)["out"]
    whole = seq.scatter(feat, case["coords"], B, ny, nx)
    for dtype in (np.float32, np.int32, np.int64):
        coords, pushed = out_of_range_coords(case, dtype)
        canvas = seq.scatter(feat, coords, B, ny, nx)
        kept = np.ones(len(feat), bool)
        kept[pushed] = False
        assert seq.same_bits(canvas, seq.scatter(feat[kept], case["coords"][kept], B, ny, nx)) and not seq.same_bits(canvas, whole)
        grad = seq.scatter_backward(seq.grad_canvas_of(case), coords)
        assert not grad[pushed].any() and seq.same_bits(grad[kept], case["grad"][kept])


def test_steps_carry_the_buffers_and_the_cumulative_average():
    case = CASES["momentum_none"]
    res = seq.restate_steps(case)
    assert res["tracked"] == 3
    one = seq.restate(case)
    # the cumulative average of three equal batches is the batch's own statistics (up to the roundings of each step)
    mean = one["sums"][:case["W"].shape[0]] / float(case["voxels"].shape[0] * case["voxels"].shape[1])
    assert np.allclose(res["running_mean"], mean, rtol=1e-6, atol=1e-7)
    two = seq.restate_steps(dict(CASES["eps_momentum"], steps=2))
    assert not seq.same_bits(two["running_var"], seq.restate(CASES["eps_momentum"])["running_var"])
