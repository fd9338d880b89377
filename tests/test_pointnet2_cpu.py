"""CPU: tests/pointnet2_seq.py (the numpy restatement the GPU tests compare with) reproduces every output that
tools/make_golden_pointnet2.py recorded from the reference's own kernel text -- indices, temp, float32
distances and interpolations bit for bit, gradients to the derived bound -- and the fixture's inputs make
the contract bite (the conditions the tool asserted, asserted again from the recorded data)."""
import os

import numpy as np
import pytest

import pointnet2_seq as seq

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pointnet2_batch.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def fps_cases(g):
    return [(i, str(n)) for i, n in enumerate(g["fps_names"])]


def test_fixture_is_small_and_complete(gold):
    assert os.path.getsize(GOLD) < 1 << 20
    assert [n for _, n in fps_cases(gold)] == ["tie64", "tie512", "tie1024", "m1", "plain"]
    assert all(f"bq{i}_idx" in gold for i in range(2)) and all(f"nn{i}_idx" in gold for i in range(3))


def test_fps_reproduces_the_reference_kernel(gold):
    for i, name in fps_cases(gold):
        xyz, idx = gold[f"fps{i}_xyz"], gold[f"fps{i}_idx"]
        got, temp = seq.furthest_point_sample(xyz, idx.shape[1], gold[f"fps{i}_temp0"])
        assert np.array_equal(got, idx), name
        assert np.array_equal(bits(temp), bits(gold[f"fps{i}_temp"])), name
        assert (idx[:, 0] == 0).all()


def test_fps_fixture_makes_the_tie_rule_bite(gold):
    sizes = {}
    for i, name in fps_cases(gold):
        xyz, idx = gold[f"fps{i}_xyz"], gold[f"fps{i}_idx"]
        B, N, _ = xyz.shape
        m = idx.shape[1]
        sizes[name] = (seq.fps_block_size(N), N, m)
        if not name.startswith("tie"):
            continue
        low, _ = seq.furthest_point_sample(xyz, m, gold[f"fps{i}_temp0"], tie="lowest")
        for b, (across, inside) in enumerate(seq.fps_tie_steps(xyz, m)):
            assert across > 0 and inside > 0, (name, b)
            assert not np.array_equal(low[b], idx[b]), (name, b)      # "lowest index" is NOT the reference's rule
    assert sizes["tie64"][0] in (64, 128) and sizes["tie512"][0] == 512 and sizes["tie1024"][0] == 1024
    assert sizes["tie64"][1] == sizes["tie64"][2]                     # one case has m = N
    assert sizes["m1"][2] == 1
    i = [n for _, n in fps_cases(gold)].index("m1")
    assert np.array_equal(bits(gold[f"fps{i}_temp"]), bits(gold[f"fps{i}_temp0"]))   # m = 1 touches nothing but idx[0]


def test_fps_block_size_is_the_reference_quotient():
    # opt_n_threads: 1 << int(log(n) / log(2)), at most 1024; the integer form equals it for every n < 70 000
    n = np.arange(1, 70000)
    ref = np.minimum(1 << (np.log(n.astype(np.float64)) / np.log(2.0)).astype(np.int64), 1024)
    assert all(seq.fps_block_size(int(k)) == r for k, r in zip(n[:5000], ref[:5000]))
    assert all(seq.fps_block_size(int(k)) == 1024 for k in (5000, 12288, 40000, 69999)) and (ref[4999:] == 1024).all()


def test_ball_query(gold):
    for i in range(2):
        xyz, cen, idx = gold[f"bq{i}_xyz"], gold[f"bq{i}_new_xyz"], gold[f"bq{i}_idx"]
        radius, ns = float(gold[f"bq{i}_radius"]), int(gold[f"bq{i}_nsample"])
        assert np.array_equal(seq.ball_query(radius, ns, xyz, cen), idx), i
        d2 = seq._d2(cen[:, :, None, :], xyz[:, None, :, :])
        r2 = np.float32(radius) * np.float32(radius)
        cnt = (d2 < r2).sum(axis=2)
        assert (cnt == 0).any() and ((cnt > 0) & (cnt < ns)).any() and (cnt > ns).any()
        assert (idx[cnt == 0] == 0).all()                             # untouched rows
        if i == 0:
            assert radius == 0.5 and (d2 == r2).any()                 # pairs at exactly the radius: strict <


def test_three_nn(gold):
    for i in range(3):
        d2, idx = seq.three_nn(gold[f"nn{i}_unknown"], gold[f"nn{i}_known"])
        assert np.array_equal(idx, gold[f"nn{i}_idx"]), i
        assert np.array_equal(bits(d2), bits(gold[f"nn{i}_dist2"])), i
    d = gold["nn0_dist2"]
    assert (d[:, :, 0] == d[:, :, 1]).any() and (d[:, :, 1] == d[:, :, 2]).any()     # equal distances
    assert gold["nn1_known"].shape[1] == 2
    assert np.isinf(gold["nn1_dist2"][:, :, 2]).all() and (gold["nn1_idx"][:, :, 2] == 0).all()


def test_gather_group_interpolate_forward(gold):
    assert np.array_equal(bits(seq.gather(gold["ga_points"], gold["ga_idx"])), bits(gold["ga_out"]))
    assert np.array_equal(bits(seq.group(gold["gr_points"], gold["gr_idx"])), bits(gold["gr_out"]))
    assert np.array_equal(bits(seq.three_interpolate(gold["ti_points"], gold["ti_idx"], gold["ti_weight"])), bits(gold["ti_out"]))


def test_gradients_to_the_bound(gold):
    g = gold
    assert (g["ga_given"] != 0).any()                                 # one case starts from a non-zero buffer
    assert seq.check_grad(g["ga_grad"], g["ga_given"], seq.gather_grad(g["ga_grad_out"], g["ga_idx"], g["ga_points"].shape[2])) == 0
    assert seq.check_grad(g["gr_grad"], None, seq.group_grad(g["gr_grad_out"], g["gr_idx"], g["gr_points"].shape[2])) == 0
    assert seq.check_grad(g["ti_grad"], None, seq.three_interpolate_grad(g["ti_grad_out"], g["ti_idx"], g["ti_weight"],
                                                                         g["ti_points"].shape[2])) == 0
    # the check itself is not vacuous: a 1e-3 relative error on one element misses it
    bad = g["gr_grad"].copy()
    j = np.unravel_index(np.argmax(np.abs(bad)), bad.shape)
    bad[j] *= np.float32(1 + 1e-3)
    assert seq.check_grad(bad, None, seq.group_grad(g["gr_grad_out"], g["gr_idx"], g["gr_points"].shape[2])) == 1
