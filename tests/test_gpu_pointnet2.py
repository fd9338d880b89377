"""GPU: the nine PointNet++ ops through the pointnet2_batch_cuda shim.

* against the outputs recorded from the reference's own kernel text (tests/golden/pointnet2_batch.npz): integers and
  forward floats bit for bit;
* at the shapes PointRCNN runs at under pointrcnn_dynamic_obj.yaml with B = 2, against the numpy restatement
  (tests/pointnet2_seq.py, itself checked against the fixture on the CPU), bit for bit; clouds built like real input: a
  synthetic Lyft-shape scan sampled to 12 288 points WITH repetition, so exact duplicates (FPS ties) occur;
* gradients against float64 scatter-adds of the same terms, per output element
  |got - exact| <= k * 2^-23 * sum|term|, k = terms added into the element, a non-zero initial value counted as one
  (with u = 2^-24: k - 1 float32 additions in any order give (k - 1) u sum|term| to first order, the rounding of the
  products u sum|term|; the bound is twice their sum -- derived, not measured); an element no term reaches stays
  exactly as given.
"""
import os
import sys

import numpy as np
import pytest
import torch

import pointnet2_seq as seq

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pointnet2_batch.npz")
SA_NPOINTS = (4096, 1024, 256, 64)
SA_RADIUS = ((0.1, 0.5), (0.5, 1.0), (1.0, 2.0), (2.0, 4.0))
SA_NSAMPLE = ((16, 32), (16, 32), (16, 32), (16, 32))


@pytest.fixture(scope="module")
def ops(gpu):
    from modest_amd.utils.pointnet2.pointnet2_batch import pointnet2_batch_cuda
    return pointnet2_batch_cuda


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(t, ref):
    return np.array_equal(bits(t.cpu().numpy()), bits(ref))


# ---- thin callers (allocate like the reference's Python side does) -----------------------------------------------
def run_fps(ops, gpu, xyz, m, temp0=None):
    B, N, _ = xyz.shape
    x = dev(xyz, gpu)
    temp = torch.full((B, N), 1e10, dtype=torch.float32, device=gpu) if temp0 is None else dev(temp0, gpu)
    idx = torch.full((B, m), -7, dtype=torch.int32, device=gpu)
    assert ops.furthest_point_sampling_wrapper(B, N, m, x, temp, idx) == 1
    return idx.cpu().numpy(), temp.cpu().numpy()


def run_ball(ops, gpu, radius, ns, xyz, cen):
    B, N, _ = xyz.shape
    M = cen.shape[1]
    idx = torch.zeros((B, M, ns), dtype=torch.int32, device=gpu)
    assert ops.ball_query_wrapper(B, N, M, radius, ns, dev(cen, gpu), dev(xyz, gpu), idx) == 1
    return idx.cpu().numpy()


def run_nn(ops, gpu, unk, kn):
    B, n, _ = unk.shape
    d2 = torch.full((B, n, 3), -1.0, dtype=torch.float32, device=gpu)
    idx = torch.full((B, n, 3), -1, dtype=torch.int32, device=gpu)
    assert ops.three_nn_wrapper(B, n, kn.shape[1], dev(unk, gpu), dev(kn, gpu), d2, idx) == 1
    return d2.cpu().numpy(), idx.cpu().numpy()


def run_gather(ops, gpu, pts, idx):
    B, C, N = pts.shape
    out = torch.full((B, C, idx.shape[1]), -1.0, dtype=torch.float32, device=gpu)
    assert ops.gather_points_wrapper(B, C, N, idx.shape[1], dev(pts, gpu), dev(idx, gpu), out) == 1
    return out


def run_group(ops, gpu, pts, idx):
    B, C, N = pts.shape
    _, P, S = idx.shape
    out = torch.full((B, C, P, S), -1.0, dtype=torch.float32, device=gpu)
    assert ops.group_points_wrapper(B, C, N, P, S, dev(pts, gpu), dev(idx, gpu), out) == 1
    return out


def run_interp(ops, gpu, pts, idx, w):
    B, C, m = pts.shape
    n = idx.shape[1]
    out = torch.full((B, C, n), -1.0, dtype=torch.float32, device=gpu)
    assert ops.three_interpolate_wrapper(B, C, m, n, dev(pts, gpu), dev(idx, gpu), dev(w, gpu), out) == 1
    return out


def run_gather_grad(ops, gpu, go, idx, n, given=None):
    B, C, m = go.shape
    grad = torch.zeros((B, C, n), dtype=torch.float32, device=gpu) if given is None else dev(given, gpu)
    assert ops.gather_points_grad_wrapper(B, C, n, m, dev(go, gpu), dev(idx, gpu), grad) == 1
    return grad.cpu().numpy()


def run_group_grad(ops, gpu, go, idx, n, given=None):
    B, C, P, S = go.shape
    grad = torch.zeros((B, C, n), dtype=torch.float32, device=gpu) if given is None else dev(given, gpu)
    assert ops.group_points_grad_wrapper(B, C, n, P, S, dev(go, gpu), dev(idx, gpu), grad) == 1
    return grad.cpu().numpy()


def run_interp_grad(ops, gpu, go, idx, w, m, given=None):
    B, C, n = go.shape
    grad = torch.zeros((B, C, m), dtype=torch.float32, device=gpu) if given is None else dev(given, gpu)
    assert ops.three_interpolate_grad_wrapper(B, C, n, m, dev(go, gpu), dev(idx, gpu), dev(w, gpu), grad) == 1
    return grad.cpu().numpy()


def weights_of(dist2):
    """the feature-propagation weights the detector forms from three_nn's distances (inverse distance, normalised)"""
    w = np.float32(1.0) / (np.sqrt(dist2) + np.float32(1e-8))
    return (w / w.sum(axis=2, keepdims=True)).astype(np.float32)


# ---- the fixture: recorded from the reference's own kernel text ---------------------------------------------------
def test_fixture_fps(ops, gpu, gold):
    for i, name in enumerate(gold["fps_names"]):
        want = gold[f"fps{i}_idx"]
        idx, temp = run_fps(ops, gpu, gold[f"fps{i}_xyz"], want.shape[1], gold[f"fps{i}_temp0"])
        assert np.array_equal(idx, want), str(name)
        assert np.array_equal(bits(temp), bits(gold[f"fps{i}_temp"])), str(name)


def test_fixture_ball_query_and_three_nn(ops, gpu, gold):
    for i in range(2):
        got = run_ball(ops, gpu, float(gold[f"bq{i}_radius"]), int(gold[f"bq{i}_nsample"]), gold[f"bq{i}_xyz"], gold[f"bq{i}_new_xyz"])
        assert np.array_equal(got, gold[f"bq{i}_idx"]), i
    for i in range(3):
        d2, idx = run_nn(ops, gpu, gold[f"nn{i}_unknown"], gold[f"nn{i}_known"])
        assert np.array_equal(idx, gold[f"nn{i}_idx"]), i
        assert np.array_equal(bits(d2), bits(gold[f"nn{i}_dist2"])), i


def test_fixture_gathers_and_gradients(ops, gpu, gold):
    g = gold
    assert same_bits(run_gather(ops, gpu, g["ga_points"], g["ga_idx"]), g["ga_out"])
    assert same_bits(run_group(ops, gpu, g["gr_points"], g["gr_idx"]), g["gr_out"])
    assert same_bits(run_interp(ops, gpu, g["ti_points"], g["ti_idx"], g["ti_weight"]), g["ti_out"])
    n = g["ga_points"].shape[2]
    got = run_gather_grad(ops, gpu, g["ga_grad_out"], g["ga_idx"], n, g["ga_given"])          # from a non-zero buffer
    assert seq.check_grad(got, g["ga_given"], seq.gather_grad(g["ga_grad_out"], g["ga_idx"], n)) == 0
    n = g["gr_points"].shape[2]
    got = run_group_grad(ops, gpu, g["gr_grad_out"], g["gr_idx"], n)
    assert seq.check_grad(got, None, seq.group_grad(g["gr_grad_out"], g["gr_idx"], n)) == 0
    m = g["ti_points"].shape[2]
    got = run_interp_grad(ops, gpu, g["ti_grad_out"], g["ti_idx"], g["ti_weight"], m)
    assert seq.check_grad(got, None, seq.three_interpolate_grad(g["ti_grad_out"], g["ti_idx"], g["ti_weight"], m)) == 0


# ---- PointRCNN's shapes ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def levels(ops, gpu):
    """B = 2 clouds of 12 288 points sampled with repetition from synthetic Lyft-shape scans, and the backbone's four
    sampling levels below them, each checked against the restatement as it is made."""
    from modest_amd import synth
    rs = np.random.RandomState(7)
    clouds = []
    for s in (11, 12):
        xyz = synth.make_scan(s, n_live=9000 if s == 11 else 30000, n_trav=1, n_frames=1, n_per_frame=2000).live_xyz
        clouds.append(xyz[rs.choice(len(xyz), 12288, replace=True)])    # the first scan is short: every point repeats
    xyz = [np.ascontiguousarray(np.stack(clouds), dtype=np.float32)]
    for m in SA_NPOINTS:
        idx, temp = run_fps(ops, gpu, xyz[-1], m)
        ref_idx, ref_temp = seq.furthest_point_sample(xyz[-1], m)
        assert np.array_equal(idx, ref_idx), m
        assert np.array_equal(bits(temp), bits(ref_temp)), m
        xyz.append(np.take_along_axis(xyz[-1], idx.astype(np.int64)[:, :, None], axis=1))
    return xyz


def test_backbone_fps_has_ties(levels):
    # sampled with repetition: the clouds hold exact duplicates, so the tie rule decided some of the rounds above
    for b in range(2):
        assert len(np.unique(levels[0][b], axis=0)) < 12288
    assert all(a + i > 0 for a, i in seq.fps_tie_steps(levels[0], 1024))


@pytest.fixture(scope="module")
def rois(levels):
    """256 clouds of 512 points like the RoI head's pooled points: the neighbourhood of a random point, padded by repetition"""
    rs = np.random.RandomState(3)
    out = []
    for r in range(256):
        cloud = levels[0][r % 2]
        c = cloud[rs.randint(len(cloud))]
        near = cloud[np.abs(cloud - c).max(axis=1) < 2.5]
        out.append(near[rs.choice(len(near), 512, replace=True)] - c)
    return np.ascontiguousarray(np.stack(out), dtype=np.float32)


def test_roi_head_fps_and_ball_query(ops, gpu, rois):
    xyz = rois
    for m, radius in ((128, 0.2), (32, 0.4)):
        idx, temp = run_fps(ops, gpu, xyz, m)
        ref_idx, ref_temp = seq.furthest_point_sample(xyz, m)
        assert np.array_equal(idx, ref_idx) and np.array_equal(bits(temp), bits(ref_temp)), m
        new = np.take_along_axis(xyz, idx.astype(np.int64)[:, :, None], axis=1)
        assert np.array_equal(run_ball(ops, gpu, radius, 16, xyz, new), seq.ball_query(radius, 16, xyz, new)), m
        xyz = new


@pytest.mark.parametrize("level", range(4))
def test_backbone_ball_query_and_grouping(ops, gpu, levels, level):
    xyz, new = levels[level], levels[level + 1]
    rs = np.random.RandomState(level)
    for radius, ns in zip(SA_RADIUS[level], SA_NSAMPLE[level]):
        got = run_ball(ops, gpu, radius, ns, xyz, new)
        assert np.array_equal(got, seq.ball_query(radius, ns, xyz, new)), (radius, ns)
    # grouping at the last (radius, nsample) of the level, a few channels more than a multiple of the kernel's chunk
    C = 3 + 8
    pts = rs.randn(2, C, xyz.shape[1]).astype(np.float32)
    assert same_bits(run_group(ops, gpu, pts, got), seq.group(pts, got))
    go = rs.randn(2, C, *got.shape[1:]).astype(np.float32)
    grad = run_group_grad(ops, gpu, go, got, xyz.shape[1])
    assert seq.check_grad(grad, None, seq.group_grad(go, got, xyz.shape[1])) == 0


@pytest.mark.parametrize("level", range(4))
def test_backbone_three_nn_and_interpolation(ops, gpu, levels, level):
    unk, kn = levels[level], levels[level + 1]        # (12288, 4096), (4096, 1024), (1024, 256), (256, 64)
    d2, idx = run_nn(ops, gpu, unk, kn)
    rd2, ridx = seq.three_nn(unk, kn)
    assert np.array_equal(idx, ridx) and np.array_equal(bits(d2), bits(rd2))
    rs = np.random.RandomState(10 + level)
    C = (19, 32, 64, 128)[level]
    w = weights_of(d2)
    pts = rs.randn(2, C, kn.shape[1]).astype(np.float32)
    assert same_bits(run_interp(ops, gpu, pts, idx, w), seq.three_interpolate(pts, idx, w))
    go = rs.randn(2, C, unk.shape[1]).astype(np.float32)
    given = (rs.randn(2, C, kn.shape[1]) * (rs.rand(2, C, kn.shape[1]) < 0.3)).astype(np.float32) if level == 1 else None
    grad = run_interp_grad(ops, gpu, go, idx, w, kn.shape[1], given)
    assert seq.check_grad(grad, given, seq.three_interpolate_grad(go, idx, w, kn.shape[1])) == 0
    # the backbone's gather of the sampled coordinates (gather_operation on (B, 3, N))
    fidx, _ = seq.furthest_point_sample(unk[:, :300], 40)
    cols = np.ascontiguousarray(unk.transpose(0, 2, 1))
    assert same_bits(run_gather(ops, gpu, cols, fidx), seq.gather(cols, fidx))


# ---- past the register path, odd sizes, channel counts -------------------------------------------------------------
def test_fps_any_n(ops, gpu):
    rs = np.random.RandomState(5)
    big = np.round(rs.uniform(-40, 40, (2, 40000, 3)) * 4) / 4          # lattice: ties at the global-memory path too
    for xyz, m in ((big, 512), (rs.uniform(-9, 9, (3, 1000, 3)), 200), (rs.uniform(-9, 9, (2, 777, 3)), 777),
                   (rs.uniform(-9, 9, (2, 5000, 3)), 300), (np.round(rs.uniform(-2, 2, (4, 63, 3)) * 2) / 2, 80),
                   (rs.uniform(-1, 1, (2, 1, 3)), 3), (rs.uniform(-1, 1, (2, 2, 3)), 1)):
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        idx, temp = run_fps(ops, gpu, xyz, m)                            # one case has m > N: the same rule keeps picking
        ref_idx, ref_temp = seq.furthest_point_sample(xyz, m)
        assert np.array_equal(idx, ref_idx), (xyz.shape, m)
        assert np.array_equal(bits(temp), bits(ref_temp)), (xyz.shape, m)


@pytest.mark.parametrize("C", (1, 515))
def test_channel_counts_and_odd_sizes(ops, gpu, C):
    rs = np.random.RandomState(C)
    B, N, P, S, n = 2, 1003, 77, 5, 333
    pts = rs.randn(B, C, N).astype(np.float32)
    idx = rs.randint(0, N, (B, P, S)).astype(np.int32)
    assert same_bits(run_group(ops, gpu, pts, idx), seq.group(pts, idx))
    assert same_bits(run_gather(ops, gpu, pts, idx[:, :, 0].copy()), seq.gather(pts, idx[:, :, 0]))
    go = rs.randn(B, C, P, S).astype(np.float32)
    assert seq.check_grad(run_group_grad(ops, gpu, go, idx, N), None, seq.group_grad(go, idx, N)) == 0
    go1 = np.ascontiguousarray(go[:, :, :, 0])
    assert seq.check_grad(run_gather_grad(ops, gpu, go1, idx[:, :, 0].copy(), N), None, seq.gather_grad(go1, idx[:, :, 0], N)) == 0
    unk, kn = rs.uniform(-3, 3, (B, n, 3)).astype(np.float32), rs.uniform(-3, 3, (B, N, 3)).astype(np.float32)
    d2, i3 = run_nn(ops, gpu, unk, kn)
    rd2, ri3 = seq.three_nn(unk, kn)
    assert np.array_equal(i3, ri3) and np.array_equal(bits(d2), bits(rd2))
    w = weights_of(d2)
    assert same_bits(run_interp(ops, gpu, pts, i3, w), seq.three_interpolate(pts, i3, w))
    go = rs.randn(B, C, n).astype(np.float32)
    assert seq.check_grad(run_interp_grad(ops, gpu, go, i3, w, N), None, seq.three_interpolate_grad(go, i3, w, N)) == 0


@pytest.mark.parametrize("N", (8192, 8193, 36864, 40000))
def test_gradient_rows_at_every_capacity(ops, gpu, N):
    """rows of the small LDS tile, of the large one, its last size, and rows no LDS holds (global atomics)"""
    rs = np.random.RandomState(N)
    B, C, m = 2, 5, 6000
    idx = rs.randint(0, N, (B, m)).astype(np.int32)
    idx[:, :3000] = rs.randint(0, 50, (B, 3000))                         # hot destinations: many terms per element
    go = rs.randn(B, C, m).astype(np.float32)
    given = (rs.randn(B, C, N) * (rs.rand(B, C, N) < 0.5)).astype(np.float32)
    got = run_gather_grad(ops, gpu, go, idx, N, given)
    assert seq.check_grad(got, given, seq.gather_grad(go, idx, N)) == 0
    pts = rs.uniform(-4, 4, (B, N, 3)).astype(np.float32)
    cen = pts[:, :500].copy()
    assert np.array_equal(run_ball(ops, gpu, 0.7, 9, pts, cen), seq.ball_query(0.7, 9, pts, cen))


# ---- autograd functions ----------------------------------------------------------------------------------------------
def test_autograd_functions(gpu, ops):
    from modest_amd.utils.pointnet2.pointnet2_batch import pointnet2_utils as pu
    rs = np.random.RandomState(9)
    B, C, N, P, S = 2, 7, 900, 120, 6
    xyz = torch.from_numpy(rs.uniform(-3, 3, (B, N, 3)).astype(np.float32)).to(gpu).requires_grad_(True)
    feat = torch.from_numpy(rs.randn(B, C, N).astype(np.float32)).to(gpu)

    fidx = pu.furthest_point_sample(xyz, P)
    assert fidx.dtype == torch.int32 and not fidx.requires_grad
    new_xyz = pu.gather_operation(xyz.detach().transpose(1, 2).contiguous(), fidx).transpose(1, 2).contiguous()
    bidx = pu.ball_query(0.9, S, xyz, new_xyz)
    assert not bidx.requires_grad and bidx.shape == (B, P, S)
    dist, nidx = pu.three_nn(xyz, new_xyz.requires_grad_(True))
    assert not dist.requires_grad and not nidx.requires_grad
    assert np.array_equal(bidx.cpu().numpy(), seq.ball_query(0.9, S, xyz.detach().cpu().numpy(), new_xyz.detach().cpu().numpy()))

    def exact(fn, f, go):
        f64 = f.detach().double().requires_grad_(True)
        (fn(f64) * go.double()).sum().backward()
        return f64.grad.cpu().numpy()

    # grouping_operation
    f = feat.clone().requires_grad_(True)
    out = pu.grouping_operation(f, bidx)
    go = torch.from_numpy(rs.randn(*out.shape).astype(np.float32)).to(gpu)
    out.backward(go)
    li = bidx.long()
    ref = exact(lambda x: torch.gather(x.unsqueeze(2).expand(-1, -1, P, -1), 3, li.unsqueeze(1).expand(-1, C, -1, -1)), feat, go)
    ex = seq.group_grad(go.cpu().numpy(), bidx.cpu().numpy(), N)
    assert np.allclose(ref, ex[0], rtol=1e-12, atol=1e-12)
    assert seq.check_grad(f.grad.cpu().numpy(), None, (ref, ex[1], ex[2])) == 0

    # gather_operation
    f = feat.clone().requires_grad_(True)
    out = pu.gather_operation(f, fidx)
    go = torch.from_numpy(rs.randn(*out.shape).astype(np.float32)).to(gpu)
    out.backward(go)
    ref = exact(lambda x: torch.gather(x, 2, fidx.long().unsqueeze(1).expand(-1, C, -1)), feat, go)
    ex = seq.gather_grad(go.cpu().numpy(), fidx.cpu().numpy(), N)
    assert np.allclose(ref, ex[0], rtol=1e-12, atol=1e-12)
    assert seq.check_grad(f.grad.cpu().numpy(), None, (ref, ex[1], ex[2])) == 0

    # three_interpolate: features on the P sampled points interpolated back to all N
    known = torch.from_numpy(rs.randn(B, C, P).astype(np.float32)).to(gpu)
    w = 1.0 / (dist + 1e-8)
    w = (w / w.sum(dim=2, keepdim=True)).contiguous()
    f = known.clone().requires_grad_(True)
    out = pu.three_interpolate(f, nidx, w)
    go = torch.from_numpy(rs.randn(*out.shape).astype(np.float32)).to(gpu)
    out.backward(go)
    ni = nidx.long()

    def interp(x):
        g = torch.gather(x.unsqueeze(2).expand(-1, -1, N, -1), 3, ni.unsqueeze(1).expand(-1, C, -1, -1))
        return (g * w.double().unsqueeze(1)).sum(dim=3)

    ref = exact(interp, known, go)
    ex = seq.three_interpolate_grad(go.cpu().numpy(), nidx.cpu().numpy(), w.cpu().numpy(), P)
    assert np.allclose(ref, ex[0], rtol=1e-12, atol=1e-12)
    assert seq.check_grad(f.grad.cpu().numpy(), None, (ref, ex[1], ex[2])) == 0

    # QueryAndGroup / GroupAll on top of them
    qg = pu.QueryAndGroup(0.9, S)(xyz.detach(), new_xyz.detach(), feat)
    assert qg.shape == (B, 3 + C, P, S)
    rel = seq.group(xyz.detach().cpu().numpy().transpose(0, 2, 1), bidx.cpu().numpy()) - new_xyz.detach().cpu().numpy().transpose(0, 2, 1)[:, :, :, None]
    assert np.array_equal(qg[:, :3].cpu().numpy(), rel)
    assert pu.GroupAll()(xyz.detach(), None, feat).shape == (B, 3 + C, 1, N)


# ---- streams, errors, the sys.modules binding -----------------------------------------------------------------------
def test_non_default_stream(ops, gpu, gold):
    xyz, want = gold["fps2_xyz"], gold["fps2_idx"]
    s = torch.cuda.Stream(device=gpu)
    x = dev(xyz, gpu)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        temp = torch.full(xyz.shape[:2], 1e10, dtype=torch.float32, device=gpu)
        idx = torch.empty(want.shape, dtype=torch.int32, device=gpu)
        ops.furthest_point_sampling_wrapper(xyz.shape[0], xyz.shape[1], want.shape[1], x, temp, idx)
        new = torch.gather(x, 1, idx.long().unsqueeze(-1).expand(-1, -1, 3)).contiguous()
        ball = torch.zeros((xyz.shape[0], want.shape[1], 8), dtype=torch.int32, device=gpu)
        ops.ball_query_wrapper(xyz.shape[0], xyz.shape[1], want.shape[1], 0.5, 8, new, x, ball)
    s.synchronize()
    assert np.array_equal(idx.cpu().numpy(), want)
    assert np.array_equal(ball.cpu().numpy(), seq.ball_query(0.5, 8, xyz, new.cpu().numpy()))


def test_argument_errors_raise_and_leave_the_process_usable(ops, gpu, gold):
    B, N, m = 2, 100, 10
    xyz = torch.zeros((B, N, 3), dtype=torch.float32, device=gpu)
    temp = torch.full((B, N), 1e10, dtype=torch.float32, device=gpu)
    idx = torch.zeros((B, m), dtype=torch.int32, device=gpu)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.furthest_point_sampling_wrapper(B, N, m, xyz.cpu(), temp, idx)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.furthest_point_sampling_wrapper(B, N, m, torch.zeros((B, 3, N), device=gpu).transpose(1, 2), temp, idx)
    with pytest.raises(RuntimeError, match="int32"):
        ops.furthest_point_sampling_wrapper(B, N, m, xyz, temp, idx.long())
    with pytest.raises(RuntimeError, match="shape"):
        ops.furthest_point_sampling_wrapper(B, N + 1, m, xyz, temp, idx)
    with pytest.raises(RuntimeError, match="shape"):
        ops.ball_query_wrapper(B, N, m, 0.5, 4, xyz[:, :m].contiguous(), xyz, torch.zeros((B, m, 5), dtype=torch.int32, device=gpu))
    with pytest.raises(RuntimeError, match="float32"):
        ops.gather_points_wrapper(B, 3, N, m, torch.zeros((B, 3, N), dtype=torch.float64, device=gpu), idx,
                                  torch.zeros((B, 3, m), device=gpu))
    with pytest.raises(RuntimeError):
        ops.three_nn_wrapper(B, N, m, xyz, "known", temp, idx)
    with pytest.raises(RuntimeError, match="n >= 1"):
        ops.furthest_point_sampling_wrapper(B, 0, m, xyz[:, :0].contiguous(), temp[:, :0].contiguous(), idx)
    # ... and the next call works
    i = 0
    got, _ = run_fps(ops, gpu, gold[f"fps{i}_xyz"], gold[f"fps{i}_idx"].shape[1])
    assert np.array_equal(got, gold[f"fps{i}_idx"])


def test_sys_modules_binding_serves_the_reference_import_path(ops, gpu, gold):
    """OpenPCDet's `from . import pointnet2_batch_cuda` resolves to the shim once it is bound"""
    key = "pcdet.ops.pointnet2.pointnet2_batch.pointnet2_batch_cuda"
    had = sys.modules.get(key)
    sys.modules[key] = ops
    try:
        import importlib
        mod = importlib.import_module(key)
        names = ("ball_query_wrapper", "group_points_wrapper", "group_points_grad_wrapper", "gather_points_wrapper",
                 "gather_points_grad_wrapper", "furthest_point_sampling_wrapper", "three_nn_wrapper",
                 "three_interpolate_wrapper", "three_interpolate_grad_wrapper")
        assert all(callable(getattr(mod, n)) for n in names)
    finally:
        if had is None:
            del sys.modules[key]
        else:
            sys.modules[key] = had
