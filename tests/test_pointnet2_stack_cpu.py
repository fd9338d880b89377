"""CPU: tests/pointnet2_stack_seq.py (the numpy restatement the GPU tests compare with) reproduces every output that
tools/make_golden_pointnet2_stack.py recorded from the reference's own kernel text -- indices, float32 distances,
grouped rows and interpolations bit for bit, gradients to the derived bound -- and the fixture's inputs make the
contract bite (the conditions the tool asserted, asserted again from the recorded data).  Also: the binding of the
shim is opt-in, and the shim refuses CPU tensors and wrong shapes before it opens the library."""
import os
import sys
import types

import numpy as np
import pytest
import torch

import pointnet2_stack_seq as seq
from modest_amd.utils.pointnet2.pointnet2_stack import pointnet2_stack_cuda as ops

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pointnet2_stack.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_fixture_is_small_and_complete(gold):
    assert os.path.getsize(GOLD) < 300 * 1000
    for k in ("bq0_idx", "bq1_idx", "vq_idx", "nn0_idx", "nn1_idx", "gr0_out", "gr1_grad", "ti_out", "ti_grad"):
        assert k in gold, k


def test_scan_of_rows_is_the_reference_loop():
    def loop(p, cnt):   # ball_query_kernel_stack's own search
        b, total = 0, cnt[0]
        for k in range(1, len(cnt)):
            if p < total:
                break
            total += cnt[k]
            b = k
        return b
    for cnt in ([65, 0, 63], [5], [0, 0, 4], [3, 2, 0], [1] * 70, [0, 7, 0, 0, 2, 0]):
        m = sum(cnt) + 3   # rows past the total: the last scan
        assert list(seq.scan_of_rows(m, cnt)) == [loop(p, cnt) for p in range(m)], cnt
    assert list(seq.scan_of_rows(4, [2, -5, 2])) == [0, 0, 2, 2]   # a negative count counts as 0


def test_ball_query(gold):
    g = gold
    for i in range(2):
        xyz, xcnt, cen, qcnt = g[f"bq{i}_xyz"], g[f"bq{i}_xyz_cnt"], g[f"bq{i}_new_xyz"], g[f"bq{i}_new_cnt"]
        radius, ns, given, idx = float(g[f"bq{i}_radius"]), int(g[f"bq{i}_nsample"]), g[f"bq{i}_given"], g[f"bq{i}_idx"]
        assert np.array_equal(seq.ball_query(radius, ns, xyz, xcnt, cen, qcnt, given), idx), i
        r2 = np.float32(radius) * np.float32(radius)
        d2 = seq._d2(cen[:, None, :], xyz[None, :, :])
        own = seq.scan_of_rows(len(cen), qcnt)[:, None] == seq.scan_of_rows(len(xyz), xcnt)[None, :]
        cnt = ((d2 < r2) & own).sum(axis=1)
        assert (cnt == 0).any() and ((cnt > 0) & (cnt < ns)).any() and (cnt > ns).any()
        assert (idx[cnt == 0, 0] == -1).all() and np.array_equal(idx[cnt == 0, 1:], given[cnt == 0, 1:])   # left as given
        assert (idx[cnt > 0] >= 0).all() and (idx[cnt > 0] < xcnt[seq.scan_of_rows(len(cen), qcnt)][cnt > 0, None]).all()   # scan-local
        if i == 0:
            assert len(xcnt) == 3 and len(set(xcnt)) == 3 and (qcnt == 0).any() and (given != 0).any()
            assert radius == 0.5 and ((d2 == r2) & own).any()         # pairs at exactly the radius: strict <
            assert ((d2 < r2) & ~own).any()                           # ... and hits in another scan: the counts decide
        else:
            assert len(xcnt) == 1


def test_voxel_query(gold):
    g = gold
    xyz, new_xyz, coords, table = g["vq_xyz"], g["vq_new_xyz"], g["vq_new_coords"], g["vq_point_indices"]
    ranges, radius, ns, given, idx = tuple(g["vq_ranges"]), float(g["vq_radius"]), int(g["vq_nsample"]), g["vq_given"], g["vq_idx"]
    assert np.array_equal(seq.voxel_query(ranges, radius, ns, xyz, new_xyz, coords, table, given), idx)
    B, R1, R2, R3 = table.shape
    assert len({R1, R2, R3}) == 3 and len(set(ranges)) == 3          # a non-cubic grid, three different ranges
    have = {tuple(c) for c in coords}
    assert all((b, z, y, x) in have for b in range(B) for z in (0, R1 - 1) for y in (0, R2 - 1) for x in (0, R3 - 1))   # every corner
    full = seq.voxel_query(ranges, radius, 10 ** 4, xyz, new_xyz, coords, table)
    cnt = np.where(full[:, 0] < 0, 0, [len(np.unique(r)) for r in full])
    assert (cnt == 0).any() and ((cnt > 0) & (cnt < ns)).any() and (cnt > ns).any()
    assert (idx[cnt == 0, 0] == -1).all() and np.array_equal(idx[cnt == 0, 1:], given[cnt == 0, 1:])
    # equality is a hit: a kept neighbour lies at exactly d2 == radius^2, and a strict test gives other rows
    r2 = np.float32(radius) * np.float32(radius)
    kept = cnt > 0
    assert (seq._d2(xyz[idx[kept]], new_xyz[kept][:, None, :]) == r2).any()
    strict = seq.voxel_query(ranges, np.nextafter(np.float32(radius), np.float32(0)), ns, xyz, new_xyz, coords, table, given)
    assert not np.array_equal(strict, idx)
    # global rows: the second scan's queries get rows past the first scan's count
    second = coords[:, 0] == 1
    assert (idx[second & kept] >= g["vq_xyz_cnt"][0]).all() and (idx[~second & kept] < g["vq_xyz_cnt"][0]).all()


def test_voxel_query_skips_what_the_reference_reads_out_of_bounds():
    xyz = np.zeros((2, 3), dtype=np.float32)
    table = np.array([[[[0, 1, 2, -1]]]], dtype=np.int32)            # entry 2 >= the row count of xyz
    coords = np.array([[0, 0, 0, 1], [1, 0, 0, 1], [-1, 0, 0, 1]], dtype=np.int32)   # two batch indices outside [0, B)
    got = seq.voxel_query((0, 0, 3), 1.0, 4, xyz, np.zeros((3, 3), dtype=np.float32), coords, table)
    assert got.tolist() == [[0, 1, 0, 0], [-1, 0, 0, 0], [-1, 0, 0, 0]]


def test_three_nn(gold):
    g = gold
    for i in range(2):
        d2, idx = seq.three_nn(g[f"nn{i}_unknown"], g[f"nn{i}_unknown_cnt"], g[f"nn{i}_known"], g[f"nn{i}_known_cnt"])
        assert np.array_equal(idx, g[f"nn{i}_idx"]), i
        assert np.array_equal(bits(d2), bits(g[f"nn{i}_dist2"])), i
    d, idx, ucnt, kcnt = g["nn0_dist2"], g["nn0_idx"], g["nn0_unknown_cnt"], g["nn0_known_cnt"]
    fin = np.isfinite(d)
    assert ((d[:, 0] == d[:, 1]) & fin[:, 1]).any() and ((d[:, 1] == d[:, 2]) & fin[:, 2]).any()     # equal distances
    scan = seq.scan_of_rows(len(d), ucnt)
    start = np.cumsum(kcnt) - kcnt
    none, few = np.flatnonzero((kcnt == 0) & (ucnt > 0)), np.flatnonzero((kcnt > 0) & (kcnt < 3) & (ucnt > 0))
    assert len(none) and len(few) and (ucnt == 0).any() and len(g["nn1_unknown_cnt"]) == 1
    rows = scan == none[0]
    assert np.isinf(d[rows]).all() and (idx[rows] == start[none[0]]).all()          # unused slots: inf and start_b
    rows = scan == few[0]
    assert np.isinf(d[rows, 2]).all() and (idx[rows, 2] == start[few[0]]).all() and np.isfinite(d[rows, :2]).all()
    assert ((idx >= start[scan][:, None]) & (idx < np.maximum(start + kcnt, start + 1)[scan][:, None])).all()   # global, own scan


def test_group_and_interpolate_forward(gold):
    g = gold
    for i in range(2):
        out = seq.group(g[f"gr{i}_features"], g[f"gr{i}_features_cnt"], g[f"gr{i}_idx"], g[f"gr{i}_idx_cnt"])
        assert np.array_equal(bits(out), bits(g[f"gr{i}_out"])), i
    assert len(g["gr0_idx_cnt"]) == 3 and len(g["gr1_idx_cnt"]) == 1
    assert np.array_equal(bits(seq.three_interpolate(g["ti_features"], g["ti_idx"], g["ti_weight"])), bits(g["ti_out"]))


def test_out_of_range_indices_read_as_zero_and_are_skipped():
    rs = np.random.RandomState(0)
    feat = rs.randn(7, 2).astype(np.float32)
    idx = np.array([[0, 3, -1], [0, 4, 2]], dtype=np.int32)           # scan 0 has 3 rows, scan 1 has 4
    out = seq.group(feat, [3, 4], idx, [1, 1])
    assert np.array_equal(out[0], np.stack([feat[0], 0 * feat[0], 0 * feat[0]], axis=1))
    assert np.array_equal(out[1], np.stack([feat[3], 0 * feat[0], feat[5]], axis=1))
    s, a, k = seq.group_grad(np.ones((2, 2, 3), dtype=np.float32), idx, [1, 1], [3, 4], 7)
    assert k[:, 0].tolist() == [1, 0, 0, 1, 0, 1, 0] and np.array_equal(s, k)
    ti = np.array([[0, 7, -2]], dtype=np.int32)
    w = np.array([[0.5, 0.25, 0.25]], dtype=np.float32)
    assert np.array_equal(seq.three_interpolate(feat, ti, w), 0.5 * feat[:1])
    s, a, k = seq.three_interpolate_grad(np.ones((1, 2), dtype=np.float32), ti, w, 7)
    assert k.sum() == 2 and s[0].tolist() == [0.5, 0.5]


def test_gradients_to_the_bound(gold):
    g = gold
    for i in range(2):
        exact = seq.group_grad(g[f"gr{i}_grad_out"], g[f"gr{i}_idx"], g[f"gr{i}_idx_cnt"], g[f"gr{i}_features_cnt"], len(g[f"gr{i}_features"]))
        assert seq.check_grad(g[f"gr{i}_grad"], g[f"gr{i}_given"], exact) == 0, i
        assert exact[2].max() > 1 and (exact[2] == 0).any()           # repeated destinations, and rows no term reaches
    assert (g["gr1_given"] != 0).any() and (g["ti_given"] != 0).any()  # from non-zero buffers
    exact = seq.three_interpolate_grad(g["ti_grad_out"], g["ti_idx"], g["ti_weight"], len(g["ti_features"]))
    assert seq.check_grad(g["ti_grad"], g["ti_given"], exact) == 0 and exact[2].max() > 1
    # the check itself is not vacuous: a 1e-3 relative error on one element misses it
    bad = g["ti_grad"].copy()
    j = np.unravel_index(np.argmax(np.abs(bad)), bad.shape)
    bad[j] *= np.float32(1 + 1e-3)
    assert seq.check_grad(bad, g["ti_given"], exact) == 1


# ------------------------------------------------------------------------------------------------ the binding
def test_binding_is_opt_in():
    from modest_amd.utils import pcdet_bind
    name = "pcdet.ops.pointnet2.pointnet2_stack.pointnet2_stack_cuda"
    names = list(pcdet_bind.SHIMS) + list(pcdet_bind.STAND_INS) + ["spconv.utils"]
    saved = {k: sys.modules.get(k) for k in names}

    def clear():
        for k in list(pcdet_bind.STAND_INS) + ["spconv.utils"]:
            sys.modules.pop(k, None)
    try:
        for k in names:
            sys.modules.pop(k, None)
        assert name in pcdet_bind.STAND_INS and name not in pcdet_bind.SHIMS      # both tables keep their contents
        keys = sorted(list(pcdet_bind.SHIMS) + list(pcdet_bind.STAND_INS))
        # the default call and sparse_conv=True: a stand-in, as before
        for kw in ({}, {"sparse_conv": True}):
            clear()
            bound = pcdet_bind.install(**kw)
            assert sorted(bound) == keys and isinstance(sys.modules[name], pcdet_bind.StandIn), kw
            with pytest.raises(NotImplementedError, match="not provided"):
                sys.modules[name].ball_query_wrapper(1, 2, 3)
        # opt in: the shim replaces the stand-in, the keys stay, spconv stays what it was
        spconv = sys.modules["spconv"]
        bound = pcdet_bind.install(point_stack=True)
        assert sorted(bound) == keys and bound[name] is ops and sys.modules[name] is ops and sys.modules["spconv"] is spconv
        import importlib
        assert importlib.import_module(name).voxel_query_wrapper is ops.voxel_query_wrapper
        # idempotent, and a later default call leaves the shim bound
        again = pcdet_bind.install(point_stack=True)
        assert all(again[k] is bound[k] for k in bound)
        assert pcdet_bind.install()[name] is ops and sys.modules[name] is ops
        # from nothing, without the stand-ins: bound and returned
        clear()
        bound = pcdet_bind.install(stand_ins=False, point_stack=True)
        assert sorted(bound) == sorted(list(pcdet_bind.SHIMS) + [name]) and sys.modules[name] is ops and "spconv" not in sys.modules
        # together with the sparse convolutions
        clear()
        bound = pcdet_bind.install(sparse_conv=True, point_stack=True)
        assert sorted(bound) == keys and bound[name] is ops and not isinstance(bound["spconv"], pcdet_bind.StandIn)
        # a module bound there that is neither ours nor a stand-in (the compiled extension) is left alone
        clear()
        real = sys.modules[name] = types.ModuleType(name)
        assert pcdet_bind.install(point_stack=True)[name] is real and sys.modules[name] is real
        assert name not in pcdet_bind.install(stand_ins=False, point_stack=True)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


# ------------------------------------------------------------------------------------------------ the shim's checks
def test_shim_raises_on_cpu_tensors_and_wrong_shapes_without_loading_the_library(monkeypatch):
    from modest_amd import _lib
    from modest_amd.utils import _ext

    def no_load(*a, **k):
        raise AssertionError("the library was opened")
    monkeypatch.setattr(_lib, "load", no_load)
    monkeypatch.setattr(_ext, "_fns", {})   # the binders' shared cache of entry points
    f, i = torch.float32, torch.int32
    xyz, new, cnt = torch.zeros((10, 3), dtype=f), torch.zeros((4, 3), dtype=f), torch.tensor([4], dtype=i)
    idx = torch.zeros((4, 8), dtype=i)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.ball_query_wrapper(1, 4, 0.5, 8, new, cnt, xyz, cnt, idx)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.voxel_query_wrapper(4, 2, 3, 4, 8, 0.5, 1, 1, 1, new, xyz, torch.zeros((4, 4), dtype=i), torch.zeros((1, 2, 3, 4), dtype=i), idx)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.furthest_point_sampling_wrapper(1, 10, 4, xyz[None], torch.zeros((1, 10)), torch.zeros((1, 4), dtype=i))
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.group_points_wrapper(1, 4, 3, 8, xyz, cnt, idx, cnt, torch.zeros((4, 3, 8)))
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.group_points_grad_wrapper(1, 4, 3, 10, 8, torch.zeros((4, 3, 8)), idx, cnt, cnt, torch.zeros((10, 3)))
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.three_nn_wrapper(new, cnt, xyz, cnt, torch.zeros((4, 3)), torch.zeros((4, 3), dtype=i))
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.three_interpolate_wrapper(xyz, torch.zeros((4, 3), dtype=i), torch.zeros((4, 3)), torch.zeros((4, 3)))
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.three_interpolate_grad_wrapper(torch.zeros((4, 3)), torch.zeros((4, 3), dtype=i), torch.zeros((4, 3)), xyz)
    with pytest.raises(RuntimeError, match="tensor"):
        ops.three_nn_wrapper(new, cnt, "known", cnt, new, idx)
    with pytest.raises(RuntimeError, match="int"):
        ops.ball_query_wrapper(1, 4.0, 0.5, 8, new, cnt, xyz, cnt, idx)
    with pytest.raises(RuntimeError, match="out of range"):
        ops.voxel_query_wrapper(4, 2, 3, 4, 8, 0.5, -1, 1, 1, new, xyz, torch.zeros((4, 4), dtype=i), torch.zeros((1, 2, 3, 4), dtype=i), idx)
    # the order of the checks is device, layout, dtype, shape: a meta-free way to reach the shape check is a tensor that
    # passes the first three, which needs a device; the shape rules themselves are plain Python
    class Fake(torch.Tensor):
        is_cuda = True
    fake = lambda t: t.as_subclass(Fake)   # noqa: E731
    with pytest.raises(RuntimeError, match="shape"):
        ops.ball_query_wrapper(1, 4, 0.5, 8, fake(new), fake(cnt), fake(xyz), fake(cnt), fake(torch.zeros((4, 9), dtype=i)))
    with pytest.raises(RuntimeError, match="shape"):
        ops.ball_query_wrapper(2, 4, 0.5, 8, fake(new), fake(cnt), fake(xyz), fake(cnt), fake(idx))     # B says two counts
    with pytest.raises(RuntimeError, match="shape"):
        ops.group_points_wrapper(1, 4, 3, 8, fake(xyz), fake(cnt), fake(idx), fake(cnt), fake(torch.zeros((4, 8, 3))))
    with pytest.raises(RuntimeError, match="shape"):
        ops.three_nn_wrapper(fake(new), fake(cnt), fake(xyz), fake(torch.tensor([5, 5], dtype=i)), fake(torch.zeros((4, 3))),
                             fake(torch.zeros((4, 3), dtype=i)))
    with pytest.raises(RuntimeError, match="shape"):
        ops.three_interpolate_wrapper(fake(xyz), fake(torch.zeros((4, 3), dtype=i)), fake(torch.zeros((5, 3))), fake(torch.zeros((4, 3))))
    with pytest.raises(RuntimeError, match="int32"):
        ops.ball_query_wrapper(1, 4, 0.5, 8, fake(new), fake(cnt.long()), fake(xyz), fake(cnt), fake(idx))
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.ball_query_wrapper(1, 4, 0.5, 8, fake(torch.zeros((3, 4)).t()), fake(cnt), fake(xyz), fake(cnt), fake(idx))


# ------------------------------------------------------------------------------------------------ the benchmark's yardstick
def test_the_benchmark_yardstick_computes_the_same_results():
    """tools/pointnet2_stack_bench.py's composition of stock operators, on the CPU, against the restatement (inputs on a
    lattice with an off-lattice radius: cdist's rounding decides nothing)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("pointnet2_stack_bench", os.path.join(os.path.dirname(GOLD), "..", "..", "tools",
                                                                                        "pointnet2_stack_bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    rs = np.random.RandomState(1)
    xcnt, qcnt, ns = (90, 60), (25, 31), 5
    xyz = (np.round(rs.uniform(-2, 2, (sum(xcnt), 3)) * 2) / 2).astype(np.float32)
    new = np.concatenate([(np.round(rs.uniform(-2, 2, (sum(qcnt) - 3, 3)) * 2) / 2), rs.uniform(9, 10, (3, 3))]).astype(np.float32)
    t = torch.from_numpy
    got = bench.yard_ball(0.8, ns, t(xyz), xcnt, t(new), qcnt)()
    ref = seq.ball_query(0.8, ns, xyz, xcnt, new, qcnt)
    assert np.array_equal(got.numpy(), ref) and (ref[:, 0] == -1).any() and (ref[:, 0] >= 0).any()
    d2, i3 = bench.yard_nn(t(new), qcnt, t(xyz), xcnt)()
    rd2, ri3 = seq.three_nn(new, qcnt, xyz, xcnt)
    assert np.allclose(d2.numpy(), rd2, rtol=1e-4, atol=1e-5) and (np.sort(i3.numpy(), axis=1) == np.sort(ri3, axis=1)).mean() > 0.7   # ties: any order
    idx = ref.copy()
    idx[idx[:, 0] < 0] = 0
    feat = rs.randn(sum(xcnt), 4).astype(np.float32)
    rows = bench.global_rows(t(idx), qcnt, xcnt)
    assert np.array_equal(bench.yard_group(t(feat), rows)().numpy(), seq.group(feat, xcnt, idx, qcnt))
    go = rs.randn(len(idx), 4, ns).astype(np.float32)
    assert seq.check_grad(bench.yard_group_grad(t(go), rows, sum(xcnt))().numpy(), None, seq.group_grad(go, idx, qcnt, xcnt, sum(xcnt))) == 0
    w = rs.rand(len(new), 3).astype(np.float32)
    out = bench.yard_interp(t(feat), t(ri3), t(w))().numpy()
    assert np.allclose(out, seq.three_interpolate(feat, ri3, w), rtol=1e-5, atol=1e-6)
    go = rs.randn(len(new), 4).astype(np.float32)
    s, a, k = seq.three_interpolate_grad(go, ri3, w, sum(xcnt))
    assert np.allclose(bench.yard_interp_grad(t(go), t(ri3), t(w), sum(xcnt))().numpy(), s, rtol=1e-4, atol=1e-5)
    # the voxel query: one point per occupied cell, rows ascending in (b, z, y, x)
    B, R1, R2, R3 = 2, 4, 7, 6
    occ = np.argwhere(rs.rand(B, R1, R2, R3) < 0.5)
    pts = ((occ[:, [3, 2, 1]] + rs.uniform(0.2, 0.8, (len(occ), 3))) * 0.5).astype(np.float32)
    table = np.full((B, R1, R2, R3), -1, dtype=np.int32)
    table[tuple(occ.T)] = np.arange(len(occ), dtype=np.int32)
    vcnt = tuple(np.bincount(occ[:, 0], minlength=B))
    coords = np.array(sorted((rs.randint(B), rs.randint(R1), rs.randint(R2), rs.randint(R3)) for _ in range(40)), dtype=np.int32)
    qn = tuple(np.bincount(coords[:, 0], minlength=B))
    q = ((coords[:, [3, 2, 1]] + rs.uniform(0.2, 0.8, (len(coords), 3))) * 0.5).astype(np.float32)
    got = bench.yard_voxel((1, 2, 1), 0.7, 4, t(pts), vcnt, t(q), t(coords), qn, t(occ[:, 1:].astype(np.int64)))()
    ref = seq.voxel_query((1, 2, 1), 0.7, 4, pts, q, coords, table)
    assert np.array_equal(got.numpy(), ref) and (ref[:, 0] >= 0).any()


# ------------------------------------------------------------------------------------------------ the build
def test_library_exports_the_entry_points_and_the_kernels_use_no_scratch():
    import json
    from modest_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    names = ("ball_query", "voxel_query", "three_nn", "group", "group_grad", "three_interpolate", "three_interpolate_grad")
    assert all(hasattr(lib, "modest_pn2s_" + n) and "modest_pn2s_" + n in _lib.SIGNATURES for n in names)
    res = json.load(open(os.path.join(os.path.dirname(build.LIB), "kernel_resources.json")))
    mine = {k: v for k, v in res.items() if v.get("file") == "pointnet2_stack.hip"}
    assert len(mine) == 7 and sum("pn2s_group" in k for k in mine) == 2 and sum("pn2s_three_interpolate" in k for k in mine) == 2
    assert all(v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 for v in mine.values()), mine
