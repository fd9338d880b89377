"""GPU: the stacked-batch PointNet++ ops through the pointnet2_stack_cuda shim.

* against the outputs recorded from the reference's own kernel text (tests/golden/pointnet2_stack.npz): integers and
  forward floats bit for bit;
* scan boundaries at the smallest sizes where the device-side resolution of a row's scan can go wrong, nsample and channel
  counts on both sides of every tile size, PV-RCNN's shapes with B = 2 and Voxel R-CNN's voxel query, all against the numpy
  restatement (tests/pointnet2_stack_seq.py, itself checked against the fixture on the CPU), bit for bit;
* gradients against float64 scatter-adds of the same terms, per output element
  |got - exact| <= k * 2^-23 * sum|term|, k = terms added into the element, a non-zero initial value counted as one
  (the bound of tests/test_gpu_pointnet2.py, derived there); an element no term reaches stays exactly as given.

An out-of-range index in these tests is one the contract defines (read as 0, skipped), never a wild pointer.
"""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

import pointnet2_stack_seq as seq

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pointnet2_stack.npz")
I32 = np.int32


@pytest.fixture(scope="module")
def ops(gpu):
    from modest_amd.utils.pointnet2.pointnet2_stack import pointnet2_stack_cuda
    return pointnet2_stack_cuda


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def cnt_of(c):
    return np.ascontiguousarray(c, dtype=I32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, ref):
    return got.shape == ref.shape and np.array_equal(bits(got), bits(ref))


# ---- thin callers (allocate like the reference's Python side does) -----------------------------------------------
def run_ball(ops, gpu, radius, ns, xyz, xcnt, cen, qcnt, given=None):
    idx = torch.zeros((len(cen), ns), dtype=torch.int32, device=gpu) if given is None else dev(given, gpu)
    assert ops.ball_query_wrapper(len(xcnt), len(cen), radius, ns, dev(cen, gpu), dev(cnt_of(qcnt), gpu), dev(xyz, gpu),
                                  dev(cnt_of(xcnt), gpu), idx) == 1
    return idx.cpu().numpy()


def run_voxel(ops, gpu, ranges, radius, ns, xyz, new_xyz, coords, table, given=None):
    idx = torch.zeros((len(new_xyz), ns), dtype=torch.int32, device=gpu) if given is None else dev(given, gpu)
    _, R1, R2, R3 = table.shape
    assert ops.voxel_query_wrapper(len(new_xyz), R1, R2, R3, ns, radius, int(ranges[0]), int(ranges[1]), int(ranges[2]),
                                   dev(new_xyz, gpu), dev(xyz, gpu), dev(coords, gpu), dev(table, gpu), idx) == 1
    return idx.cpu().numpy()


def run_nn(ops, gpu, unk, ucnt, kn, kcnt):
    d2 = torch.full((len(unk), 3), -1.0, dtype=torch.float32, device=gpu)
    idx = torch.full((len(unk), 3), -1, dtype=torch.int32, device=gpu)
    assert ops.three_nn_wrapper(dev(unk, gpu), dev(cnt_of(ucnt), gpu), dev(kn, gpu), dev(cnt_of(kcnt), gpu), d2, idx) == 1
    return d2.cpu().numpy(), idx.cpu().numpy()


def run_group(ops, gpu, feat, fcnt, idx, icnt):
    (M, S), C = idx.shape, feat.shape[1]
    out = torch.full((M, C, S), -1.0, dtype=torch.float32, device=gpu)
    assert ops.group_points_wrapper(len(fcnt), M, C, S, dev(feat, gpu), dev(cnt_of(fcnt), gpu), dev(idx, gpu),
                                    dev(cnt_of(icnt), gpu), out) == 1
    return out.cpu().numpy()


def run_group_grad(ops, gpu, go, idx, icnt, fcnt, n, given=None):
    M, C, S = go.shape
    grad = torch.zeros((n, C), dtype=torch.float32, device=gpu) if given is None else dev(given, gpu)
    assert ops.group_points_grad_wrapper(len(fcnt), M, C, n, S, dev(go, gpu), dev(idx, gpu), dev(cnt_of(icnt), gpu),
                                         dev(cnt_of(fcnt), gpu), grad) == 1
    return grad.cpu().numpy()


def run_interp(ops, gpu, feat, idx, w):
    out = torch.full((len(idx), feat.shape[1]), -1.0, dtype=torch.float32, device=gpu)
    assert ops.three_interpolate_wrapper(dev(feat, gpu), dev(idx, gpu), dev(w, gpu), out) == 1
    return out.cpu().numpy()


def run_interp_grad(ops, gpu, go, idx, w, m, given=None):
    grad = torch.zeros((m, go.shape[1]), dtype=torch.float32, device=gpu) if given is None else dev(given, gpu)
    assert ops.three_interpolate_grad_wrapper(dev(go, gpu), dev(idx, gpu), dev(w, gpu), grad) == 1
    return grad.cpu().numpy()


def weights_of(dist2):
    """inverse-distance weights, normalised; an unused slot (inf) weighs 0, a row without any known point is all 0"""
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(np.isfinite(dist2), np.float32(1.0) / (np.sqrt(dist2) + np.float32(1e-8)), np.float32(0))
        s = w.sum(axis=1, keepdims=True)
        return (w / np.where(s > 0, s, np.float32(1))).astype(np.float32)


def zero_empty(idx):
    idx = idx.copy()
    idx[idx[:, 0] < 0] = 0
    return idx


# ---- the fixture: recorded from the reference's own kernel text ---------------------------------------------------
def test_fixture_queries_and_three_nn(ops, gpu, gold):
    g = gold
    for i in range(2):
        got = run_ball(ops, gpu, float(g[f"bq{i}_radius"]), int(g[f"bq{i}_nsample"]), g[f"bq{i}_xyz"], g[f"bq{i}_xyz_cnt"],
                       g[f"bq{i}_new_xyz"], g[f"bq{i}_new_cnt"], g[f"bq{i}_given"])
        assert np.array_equal(got, g[f"bq{i}_idx"]), i
    got = run_voxel(ops, gpu, g["vq_ranges"], float(g["vq_radius"]), int(g["vq_nsample"]), g["vq_xyz"], g["vq_new_xyz"],
                    g["vq_new_coords"], g["vq_point_indices"], g["vq_given"])
    assert np.array_equal(got, g["vq_idx"])
    for i in range(2):
        d2, idx = run_nn(ops, gpu, g[f"nn{i}_unknown"], g[f"nn{i}_unknown_cnt"], g[f"nn{i}_known"], g[f"nn{i}_known_cnt"])
        assert np.array_equal(idx, g[f"nn{i}_idx"]), i
        assert same_bits(d2, g[f"nn{i}_dist2"]), i


def test_fixture_group_interpolate_and_gradients(ops, gpu, gold):
    g = gold
    for i in range(2):
        feat, fcnt, idx, icnt = g[f"gr{i}_features"], g[f"gr{i}_features_cnt"], g[f"gr{i}_idx"], g[f"gr{i}_idx_cnt"]
        assert same_bits(run_group(ops, gpu, feat, fcnt, idx, icnt), g[f"gr{i}_out"]), i
        got = run_group_grad(ops, gpu, g[f"gr{i}_grad_out"], idx, icnt, fcnt, len(feat), g[f"gr{i}_given"])
        assert seq.check_grad(got, g[f"gr{i}_given"], seq.group_grad(g[f"gr{i}_grad_out"], idx, icnt, fcnt, len(feat))) == 0, i
    assert same_bits(run_interp(ops, gpu, g["ti_features"], g["ti_idx"], g["ti_weight"]), g["ti_out"])
    m = len(g["ti_features"])
    got = run_interp_grad(ops, gpu, g["ti_grad_out"], g["ti_idx"], g["ti_weight"], m, g["ti_given"])       # from a non-zero buffer
    assert seq.check_grad(got, g["ti_given"], seq.three_interpolate_grad(g["ti_grad_out"], g["ti_idx"], g["ti_weight"], m)) == 0


# ---- scan boundaries -----------------------------------------------------------------------------------------------
# (queries per scan, points per scan): a workgroup's rows straddling two scans, an empty scan, a tile plus one, fewer than
# three known; one scan; more scans than lanes (70, every one of them short, two of them empty on either side)
B70_Q = [3, 0, 1, 5] + [2] * 60 + [0, 4, 1, 0, 2, 9]
B70_X = [4, 2, 0, 7] + [3] * 59 + [130, 0, 2, 1, 5, 0, 66]
SCAN_CASES = {"b3": ((65, 0, 63), (1025, 1, 64)), "b1": ((130,), (300,)), "b70": (B70_Q, B70_X)}


@pytest.mark.parametrize("case", sorted(SCAN_CASES))
def test_scan_boundaries(ops, gpu, case):
    qcnt, xcnt = SCAN_CASES[case]
    assert len(qcnt) == len(xcnt) and (case != "b70" or len(qcnt) == 70)
    rs = np.random.RandomState(len(qcnt))
    M, N = int(np.sum(qcnt)), int(np.sum(xcnt))
    xyz = (np.round(rs.uniform(-2, 2, (N, 3)) * 4) / 4).astype(np.float32)      # one small lattice for every scan: a hit
    cen = (np.round(rs.uniform(-2, 2, (M, 3)) * 4) / 4).astype(np.float32)      # in a neighbouring scan is always near
    ns = 6
    given = rs.randint(0, 4, (M, ns)).astype(I32)
    got = run_ball(ops, gpu, 0.75, ns, xyz, xcnt, cen, qcnt, given)
    ref = seq.ball_query(0.75, ns, xyz, xcnt, cen, qcnt, given)
    assert np.array_equal(got, ref)
    assert (ref[:, 0] == -1).any() and (ref[:, 0] >= 0).any()
    d2, i3 = run_nn(ops, gpu, cen, qcnt, xyz, xcnt)
    rd2, ri3 = seq.three_nn(cen, qcnt, xyz, xcnt)
    assert np.array_equal(i3, ri3) and same_bits(d2, rd2)
    # grouping with the query's rows; the rows of an empty ball hold 0, which is out of range where the scan has no point
    idx = zero_empty(ref)
    C = 5
    feat = rs.randn(N, C).astype(np.float32)
    assert same_bits(run_group(ops, gpu, feat, xcnt, idx, qcnt), seq.group(feat, xcnt, idx, qcnt))
    go = rs.randn(M, C, ns).astype(np.float32)
    given = (rs.randn(N, C) * (rs.rand(N, C) < 0.5)).astype(np.float32)
    got = run_group_grad(ops, gpu, go, idx, qcnt, xcnt, N, given)
    assert seq.check_grad(got, given, seq.group_grad(go, idx, qcnt, xcnt, N)) == 0
    # interpolation back with the three neighbours
    w = weights_of(d2)
    known = rs.randn(N, C).astype(np.float32)
    assert same_bits(run_interp(ops, gpu, known, i3, w), seq.three_interpolate(known, i3, w))
    go = rs.randn(M, C).astype(np.float32)
    assert seq.check_grad(run_interp_grad(ops, gpu, go, i3, w, N), None, seq.three_interpolate_grad(go, i3, w, N)) == 0


def test_counts_that_disagree_with_the_tensors(ops, gpu):
    """rows past the counts' total belong to the last scan, a scan's rows are clipped to the tensor, negative counts are 0"""
    rs = np.random.RandomState(4)
    xyz = rs.uniform(-1, 1, (50, 3)).astype(np.float32)
    cen = rs.uniform(-1, 1, (40, 3)).astype(np.float32)
    for qcnt, xcnt in (((10, 5), (30, 40)), ((10, -3, 5), (20, 7, 100)), ((0, 0), (60, 5))):
        got = run_ball(ops, gpu, 0.6, 4, xyz, xcnt, cen, qcnt)
        assert np.array_equal(got, seq.ball_query(0.6, 4, xyz, xcnt, cen, qcnt)), (qcnt, xcnt)
        d2, i3 = run_nn(ops, gpu, cen, qcnt, xyz, xcnt)
        rd2, ri3 = seq.three_nn(cen, qcnt, xyz, xcnt)
        assert np.array_equal(i3, ri3) and same_bits(d2, rd2), (qcnt, xcnt)
        idx = rs.randint(-1, 45, (40, 3)).astype(I32)
        feat = rs.randn(50, 2).astype(np.float32)
        assert same_bits(run_group(ops, gpu, feat, xcnt, idx, qcnt), seq.group(feat, xcnt, idx, qcnt)), (qcnt, xcnt)
        go = rs.randn(40, 2, 3).astype(np.float32)
        got = run_group_grad(ops, gpu, go, idx, qcnt, xcnt, 50)
        assert seq.check_grad(got, None, seq.group_grad(go, idx, qcnt, xcnt, 50)) == 0, (qcnt, xcnt)


# ---- nsample and channel counts on both sides of the tiles (32 samples x 64 channels) ---------------------------------
@pytest.mark.parametrize("nsample", (1, 5, 32, 33, 70))
@pytest.mark.parametrize("C", (1, 3, 33, 64, 65, 130))
def test_group_and_interpolate_sizes(ops, gpu, nsample, C):
    rs = np.random.RandomState(nsample * 1000 + C)
    fcnt, icnt = (37, 90), (21, 12)
    N, M = sum(fcnt), sum(icnt)
    feat = rs.randn(N, C).astype(np.float32)
    idx = np.concatenate([rs.randint(0, fcnt[b], (icnt[b], nsample)) for b in range(2)]).astype(I32)
    idx[::7, 0] = -1                                                   # reads as 0, skipped by the gradient
    idx[3::7, -1] = 37                                                 # past the first scan's count there, fine in the second
    assert same_bits(run_group(ops, gpu, feat, fcnt, idx, icnt), seq.group(feat, fcnt, idx, icnt))
    go = rs.randn(M, C, nsample).astype(np.float32)
    given = (rs.randn(N, C) * (rs.rand(N, C) < 0.5)).astype(np.float32)
    got = run_group_grad(ops, gpu, go, idx, icnt, fcnt, N, given)
    assert seq.check_grad(got, given, seq.group_grad(go, idx, icnt, fcnt, N)) == 0
    if nsample == 1:
        n = 301
        i3 = rs.randint(0, N, (n, 3)).astype(I32)
        i3[::11, 1] = N                                                # reads as 0, skipped by the gradient
        i3[5::11, 2] = -1
        w = rs.rand(n, 3).astype(np.float32)
        assert same_bits(run_interp(ops, gpu, feat, i3, w), seq.three_interpolate(feat, i3, w))
        go = rs.randn(n, C).astype(np.float32)
        got = run_interp_grad(ops, gpu, go, i3, w, N, given)
        assert seq.check_grad(got, given, seq.three_interpolate_grad(go, i3, w, N)) == 0


@pytest.mark.parametrize("nsample", (1, 5, 32, 70, 300))
def test_query_nsample(ops, gpu, nsample):
    """rows shorter and longer than a wavefront's step, and more hits than a step of 256 candidates holds"""
    rs = np.random.RandomState(nsample)
    xcnt, qcnt = (700, 333), (40, 27)
    xyz = rs.uniform(-1.5, 1.5, (sum(xcnt), 3)).astype(np.float32)
    cen = np.concatenate([rs.uniform(-1.5, 1.5, (sum(qcnt) - 5, 3)), rs.uniform(8, 9, (5, 3))]).astype(np.float32)
    for radius in (0.5, 4.0):
        got = run_ball(ops, gpu, radius, nsample, xyz, xcnt, cen, qcnt)
        assert np.array_equal(got, seq.ball_query(radius, nsample, xyz, xcnt, cen, qcnt)), radius


# ---- the batch layout and the stacked one run one walk and one three-NN core (csrc/pn2_search.h) -------------------------
def layouts_case():
    """B = 3 clouds of equal size on the seams of the shared code: 300 points (one whole 256-point step of the ball walk and
    a partial one), 1100 known points (one whole tile of 1024 and 76 more, all in the first wavefront's quarter).  Centres
    lie along rays out of the cloud, so their balls hold from many points down to none; some known points are repeated,
    on both sides of the tile seam, and some unknown points sit right next to them: equal distances."""
    rs = np.random.RandomState(5)
    B, n, M, m, nu = 3, 300, 40, 1100, 70
    xyz = rs.uniform(-1.5, 1.5, (B, n, 3)).astype(np.float32)
    ray = rs.randn(B, M, 3)
    ray /= np.linalg.norm(ray, axis=2, keepdims=True)
    cen = (ray * np.linspace(0.0, 4.5, M)[None, :, None]).astype(np.float32)
    known = rs.uniform(-1.5, 1.5, (B, m, 3)).astype(np.float32)
    twins = ((3, 700), (1023, 1024), (5, 1090), (1030, 1099), (200, 201))
    for a, b in twins:
        known[:, b] = known[:, a]
    unknown = rs.uniform(-1.5, 1.5, (B, nu, 3)).astype(np.float32)
    for j, (a, _) in enumerate(twins):
        unknown[:, j] = known[:, a] + np.float32(0.01) * rs.randn(B, 3).astype(np.float32)
    return B, n, M, m, nu, xyz, cen, known, unknown


def row_classes(idx):
    """(no hit, short, full) of stacked ball-query rows over a prefill that no index equals: a row that was padded ends
    in its first hit, a full one in a later point"""
    hit = idx[:, 0] >= 0
    return ~hit, hit & (idx[:, -1] == idx[:, 0]), hit & (idx[:, -1] != idx[:, 0])


def test_the_two_layouts_agree(ops, gpu):
    import pointnet2_seq as bseq
    from modest_amd.utils.pointnet2.pointnet2_batch import pointnet2_batch_cuda as bops
    B, n, M, m, nu, xyz, cen, known, unknown = layouts_case()
    radius = 1.3                                        # about 100 of a cloud's 300 points around its middle
    for ns in (5, 70):
        given = (9000 + np.arange(B * M * ns)).reshape(B, M, ns).astype(I32)          # no index of a cloud
        ref_b = bseq.ball_query(radius, ns, xyz, cen, given)
        ref_s = seq.ball_query(radius, ns, xyz.reshape(-1, 3), (n,) * B, cen.reshape(-1, 3), (M,) * B, given.reshape(-1, ns))
        none, short, full = row_classes(ref_s)
        assert none.any() and short.any() and full.any(), (ns, none.sum(), short.sum(), full.sum())
        got_b = dev(given, gpu)
        assert bops.ball_query_wrapper(B, n, M, radius, ns, dev(cen, gpu), dev(xyz, gpu), got_b) == 1
        got_b = got_b.cpu().numpy().reshape(-1, ns)
        got_s = run_ball(ops, gpu, radius, ns, xyz.reshape(-1, 3), (n,) * B, cen.reshape(-1, 3), (M,) * B, given.reshape(-1, ns))
        assert np.array_equal(got_b, ref_b.reshape(-1, ns)) and np.array_equal(got_s, ref_s), ns
        assert np.array_equal(got_s[~none], got_b[~none]), ns                          # scan-local = the cloud's own
        left = given.reshape(-1, ns)[none]
        assert np.array_equal(got_b[none], left), ns
        assert (got_s[none, 0] == -1).all() and np.array_equal(got_s[none, 1:], left[:, 1:]), ns
    rd2_b, ri_b = bseq.three_nn(unknown, known)
    rd2_s, ri_s = seq.three_nn(unknown.reshape(-1, 3), (nu,) * B, known.reshape(-1, 3), (m,) * B)
    assert ((rd2_s[:, 0] == rd2_s[:, 1]) | (rd2_s[:, 1] == rd2_s[:, 2])).any()        # a tie the index order decides
    d2_b = torch.full((B, nu, 3), -1.0, dtype=torch.float32, device=gpu)
    i_b = torch.full((B, nu, 3), -1, dtype=torch.int32, device=gpu)
    assert bops.three_nn_wrapper(B, nu, m, dev(unknown, gpu), dev(known, gpu), d2_b, i_b) == 1
    d2_b, i_b = d2_b.cpu().numpy(), i_b.cpu().numpy()
    d2_s, i_s = run_nn(ops, gpu, unknown.reshape(-1, 3), (nu,) * B, known.reshape(-1, 3), (m,) * B)
    assert same_bits(d2_b, rd2_b) and np.array_equal(i_b, ri_b)
    assert same_bits(d2_s, rd2_s) and np.array_equal(i_s, ri_s)
    assert same_bits(d2_s, d2_b.reshape(-1, 3))
    assert np.array_equal(i_s.reshape(B, nu, 3), i_b + (np.arange(B, dtype=I32) * m)[:, None, None])


# ---- PV-RCNN's shapes, B = 2 -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(ops, gpu):
    """B = 2 clouds of 16 384 raw points sampled with repetition from synthetic Lyft-shape scans (test_gpu_pointnet2.py's
    clouds), 2 048 keypoints of each by furthest point sampling, ~20 000 voxel centres of each"""
    from modest_amd import synth
    rs = np.random.RandomState(7)
    raw, centres = [], []
    for s, n_centres in ((11, 20000), (12, 18517)):
        xyz = synth.make_scan(s, n_live=9000 if s == 11 else 60000, n_trav=1, n_frames=1, n_per_frame=2000).live_xyz
        raw.append(xyz[rs.choice(len(xyz), 16384, replace=True)])
        dense = synth.make_scan(s, n_live=120000, n_trav=1, n_frames=1, n_per_frame=2000).live_xyz
        vs = np.array([0.2, 0.2, 0.4], dtype=np.float32)
        cells = np.unique(np.floor(dense / vs).astype(np.int64), axis=0)
        cells = cells[np.sort(rs.choice(len(cells), n_centres, replace=False))]
        centres.append(((cells.astype(np.float32) + np.float32(0.5)) * vs).astype(np.float32))
    raw = np.ascontiguousarray(np.stack(raw), dtype=np.float32)
    B, N, _ = raw.shape
    temp = torch.full((B, N), 1e10, dtype=torch.float32, device=gpu)
    fidx = torch.empty((B, 2048), dtype=torch.int32, device=gpu)
    assert ops.furthest_point_sampling_wrapper(B, N, 2048, dev(raw, gpu), temp, fidx) == 1
    fidx = fidx.cpu().numpy().astype(np.int64)
    keys = np.take_along_axis(raw, fidx[:, :, None], axis=1)
    return dict(raw=raw.reshape(-1, 3), raw_cnt=(N, N), keys=np.ascontiguousarray(keys.reshape(-1, 3)), key_cnt=(2048, 2048),
                centres=np.concatenate(centres), centre_cnt=tuple(len(c) for c in centres), fidx=fidx, raw3=raw)


def test_keypoint_sampling_is_the_batch_kernel(scene):
    import pointnet2_seq
    ref, _ = pointnet2_seq.furthest_point_sample(scene["raw3"], 2048)
    assert np.array_equal(scene["fidx"], ref)


@pytest.mark.parametrize("radius", (0.4, 0.8))
def test_pvrcnn_keypoints_against_raw_points(ops, gpu, scene, radius):
    s = scene
    got = run_ball(ops, gpu, radius, 16, s["raw"], s["raw_cnt"], s["keys"], s["key_cnt"])
    assert np.array_equal(got, seq.ball_query(radius, 16, s["raw"], s["raw_cnt"], s["keys"], s["key_cnt"]))
    if radius == 0.8:   # the set abstraction's grouping of the raw points' (x, y, z, intensity-like) rows
        rs = np.random.RandomState(1)
        feat = rs.randn(len(s["raw"]), 4).astype(np.float32)
        assert same_bits(run_group(ops, gpu, feat, s["raw_cnt"], got, s["key_cnt"]), seq.group(feat, s["raw_cnt"], got, s["key_cnt"]))


@pytest.mark.parametrize("radius", (1.2, 2.4))
def test_pvrcnn_keypoints_against_voxel_centres(ops, gpu, scene, radius):
    s = scene
    assert s["centre_cnt"] == (20000, 18517)
    got = run_ball(ops, gpu, radius, 32, s["centres"], s["centre_cnt"], s["keys"], s["key_cnt"])
    assert np.array_equal(got, seq.ball_query(radius, 32, s["centres"], s["centre_cnt"], s["keys"], s["key_cnt"]))
    if radius == 1.2:   # grouping of the voxel features and its gradient at the backbone's 32 channels
        rs = np.random.RandomState(2)
        idx, n = zero_empty(got), len(s["centres"])
        feat = rs.randn(n, 32).astype(np.float32)
        assert same_bits(run_group(ops, gpu, feat, s["centre_cnt"], idx, s["key_cnt"]), seq.group(feat, s["centre_cnt"], idx, s["key_cnt"]))
        go = rs.randn(len(idx), 32, 32).astype(np.float32)
        grad = run_group_grad(ops, gpu, go, idx, s["key_cnt"], s["centre_cnt"], n)
        assert seq.check_grad(grad, None, seq.group_grad(go, idx, s["key_cnt"], s["centre_cnt"], n)) == 0


@pytest.mark.parametrize("radius", (0.8, 1.6))
def test_pvrcnn_roi_grid_against_keypoints(ops, gpu, scene, radius):
    s = scene
    rs = np.random.RandomState(3)
    keys = s["keys"].reshape(2, 2048, 3)
    t = (np.arange(6, dtype=np.float32) + np.float32(0.5)) / np.float32(6) - np.float32(0.5)
    cube = np.stack(np.meshgrid(t, t, t, indexing="ij"), axis=-1).reshape(-1, 3)          # 216 grid points of a unit box
    grid = []
    for b in range(2):
        for r in range(16):
            c, size = keys[b, rs.randint(2048)], rs.uniform((3.5, 1.5, 1.4), (5.0, 2.2, 2.0)).astype(np.float32)
            a = np.float32(rs.uniform(-np.pi, np.pi))
            rot = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], dtype=np.float32)
            grid.append(((cube * size) @ rot.T + c).astype(np.float32))
    grid = np.ascontiguousarray(np.concatenate(grid), dtype=np.float32)
    qcnt = (16 * 216, 16 * 216)
    got = run_ball(ops, gpu, radius, 16, s["keys"], s["key_cnt"], grid, qcnt)
    ref = seq.ball_query(radius, 16, s["keys"], s["key_cnt"], grid, qcnt)
    assert np.array_equal(got, ref) and (ref[:, 0] >= 0).sum() > 1000


def test_pvrcnn_three_nn_and_interpolation(ops, gpu, scene):
    s = scene
    d2, idx = run_nn(ops, gpu, s["raw"], s["raw_cnt"], s["keys"], s["key_cnt"])
    rd2, ridx = seq.three_nn(s["raw"], s["raw_cnt"], s["keys"], s["key_cnt"])
    assert np.array_equal(idx, ridx) and same_bits(d2, rd2)
    assert (d2[:, 0] == 0).sum() >= 4096                               # the keypoints are raw points
    rs = np.random.RandomState(4)
    w = weights_of(d2)
    feat = rs.randn(len(s["keys"]), 128).astype(np.float32)
    assert same_bits(run_interp(ops, gpu, feat, idx, w), seq.three_interpolate(feat, idx, w))
    go = rs.randn(len(s["raw"]), 128).astype(np.float32)
    grad = run_interp_grad(ops, gpu, go, idx, w, len(feat))
    assert seq.check_grad(grad, None, seq.three_interpolate_grad(go, idx, w, len(feat))) == 0


# ---- Voxel R-CNN's voxel query ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def voxel_scene(scene):
    """a (2, 11, 50, 44) table filled from the voxelised raw clouds (the first point of a cell stands for it), RoI-grid-like
    queries inside the grid and on every face and corner of it"""
    rs = np.random.RandomState(5)
    B, R1, R2, R3 = 2, 11, 50, 44
    lo, vs = np.array([-17.6, -20, -2], dtype=np.float32), np.array([0.8, 0.8, 0.4], dtype=np.float32)
    table = np.full((B, R1, R2, R3), -1, dtype=I32)
    xyz = []
    for b in range(B):
        pts = scene["raw3"][b]
        c = np.floor((pts - lo) / vs).astype(np.int64)
        ok = ((c >= 0) & (c < np.array([R3, R2, R1]))).all(axis=1)
        _, first = np.unique(c[ok] @ np.array([1, R3, R3 * R2]), return_index=True)
        first = np.sort(first)
        cells = c[ok][first]
        table[b, cells[:, 2], cells[:, 1], cells[:, 0]] = sum(len(x) for x in xyz) + np.arange(len(cells), dtype=I32)
        xyz.append(pts[ok][first])
    xyz = np.ascontiguousarray(np.concatenate(xyz), dtype=np.float32)
    coords = []
    for b in range(B):
        border = [(b, z, y, x) for z in (0, R1 // 2, R1 - 1) for y in (0, R2 // 2, R2 - 1) for x in (0, R3 // 2, R3 - 1)]   # 8 corners, 12 edges, 6 faces, 1 inside
        occ = np.argwhere(table[b] >= 0)
        near = occ[rs.choice(len(occ), 900)] + rs.randint(-2, 3, (900, 3))                 # around occupied cells, some outside
        coords += border + [(b, *v) for v in near]
    coords = np.ascontiguousarray(coords, dtype=I32)
    new_xyz = ((coords[:, [3, 2, 1]].astype(np.float32) + rs.uniform(0, 1, (len(coords), 3)).astype(np.float32)) * vs + lo)
    return dict(xyz=xyz, table=table, coords=coords, new_xyz=np.ascontiguousarray(new_xyz, dtype=np.float32))


def test_voxel_rcnn_voxel_query(ops, gpu, voxel_scene):
    v = voxel_scene
    assert v["table"].shape == (2, 11, 50, 44) and (v["table"] >= 0).sum() == len(v["xyz"]) > 2000
    got = run_voxel(ops, gpu, (1, 4, 4), 0.8, 16, v["xyz"], v["new_xyz"], v["coords"], v["table"])
    ref = seq.voxel_query((1, 4, 4), 0.8, 16, v["xyz"], v["new_xyz"], v["coords"], v["table"])
    assert np.array_equal(got, ref)
    hits = (ref[:, 0] >= 0)
    assert hits.sum() > 500 and (~hits).sum() > 10
    # other ranges: none at all, one axis only, a box larger than the grid (more than 256 cells, clipped on every side)
    for ranges, radius, ns in (((0, 0, 0), 0.8, 3), ((0, 0, 7), 2.0, 5), ((11, 50, 44), 1.5, 40)):
        got = run_voxel(ops, gpu, ranges, radius, ns, v["xyz"], v["new_xyz"][:300], v["coords"][:300], v["table"])
        assert np.array_equal(got, seq.voxel_query(ranges, radius, ns, v["xyz"], v["new_xyz"][:300], v["coords"][:300], v["table"])), ranges


def test_voxel_query_skips_bad_batch_indices_and_table_entries(ops, gpu, voxel_scene):
    v = voxel_scene
    coords, table = v["coords"][:200].copy(), v["table"].copy()
    coords[::5, 0] = 2                                                 # a batch index outside [0, B)
    coords[1::5, 0] = -1
    occ = np.argwhere(table >= 0)
    table[tuple(occ[::3].T)] = len(v["xyz"]) + 5                       # entries past the rows of xyz
    got = run_voxel(ops, gpu, (1, 4, 4), 0.8, 16, v["xyz"], v["new_xyz"][:200], coords, table)
    ref = seq.voxel_query((1, 4, 4), 0.8, 16, v["xyz"], v["new_xyz"][:200], coords, table)
    assert np.array_equal(got, ref) and (ref[::5, 0] == -1).all() and (ref[:, 0] >= 0).any()


# ---- autograd functions and modules ----------------------------------------------------------------------------------
def _exact(fn, f, go):
    f64 = f.detach().double().requires_grad_(True)
    (fn(f64) * go.double()).sum().backward()
    return f64.grad.cpu().numpy()


def test_autograd_functions_and_query_and_group(gpu, ops):
    from modest_amd.utils.pointnet2.pointnet2_stack import pointnet2_utils as pu
    rs = np.random.RandomState(9)
    xcnt, qcnt, C, S = (500, 400), (70, 50), 7, 6
    N, M = sum(xcnt), sum(qcnt)
    xyz_np = rs.uniform(-3, 3, (N, 3)).astype(np.float32)
    new_np = np.concatenate([xyz_np[:65], rs.uniform(30, 40, (5, 3)).astype(np.float32), xyz_np[500:550]])   # five empty balls
    xyz, new_xyz = dev(xyz_np, gpu), dev(new_np, gpu)
    xc, qc = dev(cnt_of(xcnt), gpu), dev(cnt_of(qcnt), gpu)
    feat = dev(rs.randn(N, C).astype(np.float32), gpu)
    start = torch.repeat_interleave(torch.tensor([0, xcnt[0]], device=gpu), torch.tensor(qcnt, device=gpu))

    idx, empty = pu.ball_query(0.9, S, xyz, xc, new_xyz, qc)
    assert idx.dtype == torch.int32 and not idx.requires_grad and empty.dtype == torch.bool and int(empty.sum()) == 5
    ref = seq.ball_query(0.9, S, xyz_np, xcnt, new_np, qcnt)
    assert np.array_equal(empty.cpu().numpy(), ref[:, 0] == -1) and np.array_equal(idx.cpu().numpy(), zero_empty(ref))
    rows = (idx.long() + start[:, None])                               # global rows of the grouped points

    # grouping_operation: forward against indexing, exactly; backward against autograd of the indexing, to the bound
    f = feat.clone().requires_grad_(True)
    out = pu.grouping_operation(f, xc, idx, qc)
    assert torch.equal(out, feat[rows].permute(0, 2, 1))
    go = dev(rs.randn(*out.shape).astype(np.float32), gpu)
    out.backward(go)
    ref = _exact(lambda x: x[rows].permute(0, 2, 1), feat, go)
    ex = seq.group_grad(go.cpu().numpy(), idx.cpu().numpy(), qcnt, xcnt, N)
    assert np.allclose(ref, ex[0], rtol=1e-12, atol=1e-12)
    assert seq.check_grad(f.grad.cpu().numpy(), None, (ref, ex[1], ex[2])) == 0

    # three_nn and three_interpolate: features of the M centres interpolated back to all N points
    dist, nidx = pu.three_nn(xyz, xc, new_xyz, qc)
    assert not dist.requires_grad and not nidx.requires_grad and nidx.dtype == torch.int32
    rd2, ridx = seq.three_nn(xyz_np, xcnt, new_np, qcnt)
    assert np.array_equal(nidx.cpu().numpy(), ridx) and torch.equal(dist, torch.sqrt(dev(rd2, gpu)))
    w = 1.0 / (dist + 1e-8)
    w = (w / w.sum(dim=1, keepdim=True)).contiguous()
    known = dev(rs.randn(M, C).astype(np.float32), gpu)
    f = known.clone().requires_grad_(True)
    out = pu.three_interpolate(f, nidx, w)
    ni = nidx.long()
    assert torch.equal(out, (w[:, 0, None] * known[ni[:, 0]] + w[:, 1, None] * known[ni[:, 1]]) + w[:, 2, None] * known[ni[:, 2]])
    go = dev(rs.randn(*out.shape).astype(np.float32), gpu)
    out.backward(go)
    ref = _exact(lambda x: (x[ni] * w.double().unsqueeze(-1)).sum(dim=1), known, go)
    ex = seq.three_interpolate_grad(go.cpu().numpy(), nidx.cpu().numpy(), w.cpu().numpy(), M)
    assert np.allclose(ref, ex[0], rtol=1e-12, atol=1e-12)
    assert seq.check_grad(f.grad.cpu().numpy(), None, (ref, ex[1], ex[2])) == 0

    # furthest_point_sample: the batch kernel behind the stack extension's name
    import pointnet2_seq
    fidx = pu.furthest_point_sample(xyz[:500].unsqueeze(0), 40)
    assert fidx.dtype == torch.int32 and np.array_equal(fidx.cpu().numpy(), pointnet2_seq.furthest_point_sample(xyz_np[None, :500], 40)[0])

    # QueryAndGroup: relative coordinates, then features; the rows of empty balls zeroed; gradient through the features
    f = feat.clone().requires_grad_(True)
    new_features, qidx = pu.QueryAndGroup(0.9, S)(xyz, xc, new_xyz, qc, f)
    assert torch.equal(qidx, idx) and new_features.shape == (M, 3 + C, S)
    keep = (~empty)[:, None, None]
    want = torch.cat([(xyz[rows].permute(0, 2, 1) - new_xyz.unsqueeze(-1)) * keep, feat[rows].permute(0, 2, 1) * keep], dim=1)
    assert torch.equal(new_features, want) and (new_features[empty] == 0).all()
    go = dev(rs.randn(*new_features.shape).astype(np.float32), gpu)
    new_features.backward(go)
    gf = (go[:, 3:] * keep).contiguous()
    ref = _exact(lambda x: x[rows].permute(0, 2, 1) * keep, feat, go[:, 3:])
    ex = seq.group_grad(gf.cpu().numpy(), idx.cpu().numpy(), qcnt, xcnt, N)
    assert np.allclose(ref, ex[0], rtol=1e-12, atol=1e-12)
    assert seq.check_grad(f.grad.cpu().numpy(), None, (ref, ex[1], ex[2])) == 0
    only_xyz, _ = pu.QueryAndGroup(0.9, S)(xyz, xc, new_xyz, qc)
    assert torch.equal(only_xyz, want[:, :3])
    no_xyz, _ = pu.QueryAndGroup(0.9, S, use_xyz=False)(xyz, xc, new_xyz, qc, feat)
    assert torch.equal(no_xyz, want[:, 3:])


def test_voxel_query_and_grouping(gpu, ops, voxel_scene):
    from modest_amd.utils.pointnet2.pointnet2_stack import voxel_query_utils as vu
    v = voxel_scene
    rs = np.random.RandomState(6)
    per = len(v["coords"]) // 2                                        # the same number of queries in both scans
    xcnt = [int(((v["table"][b] >= 0)).sum()) for b in range(2)]
    xyz, new_xyz, coords, table = (dev(v[k], gpu) for k in ("xyz", "new_xyz", "coords", "table"))
    xc, qc = dev(cnt_of(xcnt), gpu), dev(cnt_of([per, per]), gpu)
    C, S, ranges = 9, 16, (1, 4, 4)
    feat = dev(rs.randn(len(v["xyz"]), C).astype(np.float32), gpu)

    idx, empty = vu.voxel_query(ranges, 0.8, S, xyz, new_xyz, coords, table)
    ref = seq.voxel_query(ranges, 0.8, S, v["xyz"], v["new_xyz"], v["coords"], v["table"])
    assert np.array_equal(empty.cpu().numpy(), ref[:, 0] == -1) and np.array_equal(idx.cpu().numpy(), zero_empty(ref))
    assert 0 < int(empty.sum()) < len(ref)

    f = feat.clone().requires_grad_(True)
    gfeat, gxyz, mask = vu.VoxelQueryAndGrouping(ranges, 0.8, S)(coords, xyz, xc, new_xyz, qc, f, table)
    rows = idx.long().masked_fill(empty[:, None], 0)
    rows[per:][empty[per:]] = xcnt[0]                                  # an empty row reads the first row of ITS scan
    assert torch.equal(mask, empty)
    assert torch.equal(gfeat, feat[rows].permute(0, 2, 1)) and torch.equal(gxyz, xyz[rows].permute(0, 2, 1))
    go = dev(rs.randn(*gfeat.shape).astype(np.float32), gpu)
    gfeat.backward(go)
    ref = _exact(lambda x: x[rows].permute(0, 2, 1), feat, go)
    local = (rows - torch.tensor([0, xcnt[0]], device=gpu).repeat_interleave(per)[:, None]).int().cpu().numpy()
    ex = seq.group_grad(go.cpu().numpy(), local, [per, per], xcnt, len(v["xyz"]))
    assert np.allclose(ref, ex[0], rtol=1e-12, atol=1e-12)
    assert seq.check_grad(f.grad.cpu().numpy(), None, (ref, ex[1], ex[2])) == 0


# ---- streams, errors, the sys.modules binding -----------------------------------------------------------------------
def test_non_default_stream(ops, gpu, gold):
    g = gold
    s = torch.cuda.Stream(device=gpu)
    xyz, xcnt, cen, qcnt = (dev(g[k], gpu) for k in ("bq0_xyz", "bq0_xyz_cnt", "bq0_new_xyz", "bq0_new_cnt"))
    given = dev(g["bq0_given"], gpu)
    feat = dev(g["gr0_features"], gpu)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        idx = given.clone()
        ops.ball_query_wrapper(3, len(cen), 0.5, 8, cen, qcnt, xyz, xcnt, idx)
        idx[idx[:, 0] < 0] = 0
        out = torch.empty((len(cen), feat.shape[1], 8), dtype=torch.float32, device=gpu)
        ops.group_points_wrapper(3, len(cen), feat.shape[1], 8, feat, xcnt, idx, qcnt, out)
    s.synchronize()
    assert np.array_equal(idx.cpu().numpy(), g["gr0_idx"]) and same_bits(out.cpu().numpy(), g["gr0_out"])


def test_argument_errors_raise_and_leave_the_process_usable(ops, gpu, gold):
    f, i = torch.float32, torch.int32
    xyz, new = torch.zeros((10, 3), dtype=f, device=gpu), torch.zeros((4, 3), dtype=f, device=gpu)
    cnt, cnt2 = torch.tensor([4], dtype=i, device=gpu), torch.tensor([10], dtype=i, device=gpu)
    idx = torch.zeros((4, 8), dtype=i, device=gpu)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.ball_query_wrapper(1, 4, 0.5, 8, new.cpu(), cnt, xyz, cnt2, idx)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.ball_query_wrapper(1, 4, 0.5, 8, new, cnt.cpu(), xyz, cnt2, idx)          # the counts live on the device
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.ball_query_wrapper(1, 4, 0.5, 8, torch.zeros((3, 4), device=gpu).t(), cnt, xyz, cnt2, idx)
    with pytest.raises(RuntimeError, match="int32"):
        ops.ball_query_wrapper(1, 4, 0.5, 8, new, cnt.long(), xyz, cnt2, idx)
    with pytest.raises(RuntimeError, match="shape"):
        ops.ball_query_wrapper(1, 4, 0.5, 9, new, cnt, xyz, cnt2, idx)
    with pytest.raises(RuntimeError, match="shape"):
        ops.ball_query_wrapper(2, 4, 0.5, 8, new, cnt, xyz, cnt2, idx)
    with pytest.raises(RuntimeError, match="shape"):
        ops.voxel_query_wrapper(4, 2, 3, 4, 8, 0.5, 1, 1, 1, new, xyz, torch.zeros((4, 3), dtype=i, device=gpu),
                                torch.zeros((1, 2, 3, 4), dtype=i, device=gpu), idx)
    with pytest.raises(RuntimeError, match="shape"):
        ops.voxel_query_wrapper(4, 2, 3, 4, 8, 0.5, 1, 1, 1, new, xyz, torch.zeros((4, 4), dtype=i, device=gpu),
                                torch.zeros((1, 2, 3, 5), dtype=i, device=gpu), idx)
    with pytest.raises(RuntimeError, match="out of range"):
        ops.voxel_query_wrapper(4, 2, 3, 4, 8, 0.5, 1, -1, 1, new, xyz, torch.zeros((4, 4), dtype=i, device=gpu),
                                torch.zeros((1, 2, 3, 4), dtype=i, device=gpu), idx)
    with pytest.raises(RuntimeError, match="float32"):
        ops.group_points_wrapper(1, 4, 3, 8, xyz.double(), cnt2, idx, cnt, torch.zeros((4, 3, 8), device=gpu))
    with pytest.raises(RuntimeError, match="shape"):
        ops.group_points_grad_wrapper(1, 4, 3, 11, 8, torch.zeros((4, 3, 8), device=gpu), idx, cnt, cnt2, torch.zeros((10, 3), device=gpu))
    with pytest.raises(RuntimeError, match="shape"):
        ops.three_nn_wrapper(new, cnt, xyz, torch.tensor([5, 5], dtype=i, device=gpu), torch.zeros((4, 3), device=gpu),
                             torch.zeros((4, 3), dtype=i, device=gpu))
    with pytest.raises(RuntimeError):
        ops.three_nn_wrapper(new, cnt, "known", cnt2, torch.zeros((4, 3), device=gpu), torch.zeros((4, 3), dtype=i, device=gpu))
    with pytest.raises(RuntimeError, match="shape"):
        ops.three_interpolate_wrapper(xyz, torch.zeros((4, 3), dtype=i, device=gpu), torch.zeros((4, 3), device=gpu),
                                      torch.zeros((4, 4), device=gpu))
    with pytest.raises(RuntimeError, match="shape"):
        ops.three_interpolate_grad_wrapper(torch.zeros((4, 3), device=gpu), torch.zeros((4, 3), dtype=i, device=gpu),
                                           torch.zeros((4, 3), device=gpu), torch.zeros((10, 4), device=gpu))
    with pytest.raises(RuntimeError, match="n >= 1"):
        ops.furthest_point_sampling_wrapper(1, 0, 2, xyz[None, :0].contiguous(), torch.zeros((1, 0), device=gpu),
                                            torch.zeros((1, 2), dtype=i, device=gpu))
    # ... and the next call works; empty tensors are no error either
    g = gold
    got = run_ball(ops, gpu, float(g["bq1_radius"]), int(g["bq1_nsample"]), g["bq1_xyz"], g["bq1_xyz_cnt"], g["bq1_new_xyz"], g["bq1_new_cnt"])
    assert np.array_equal(got, g["bq1_idx"])
    none = run_ball(ops, gpu, 0.5, 4, np.zeros((0, 3), np.float32), [0], g["bq1_new_xyz"][:3], [3])
    assert none.tolist() == [[-1, 0, 0, 0]] * 3
    assert run_group(ops, gpu, np.zeros((0, 2), np.float32), [0], np.zeros((3, 4), I32), [3]).tolist() == np.zeros((3, 2, 4)).tolist()
    assert run_interp(ops, gpu, np.zeros((0, 2), np.float32), np.zeros((3, 3), I32), np.ones((3, 3), np.float32)).tolist() == [[0, 0]] * 3


def test_install_serves_the_reference_import_path(ops, gpu):
    """OpenPCDet's `from . import pointnet2_stack_cuda` resolves to the shim once install(point_stack=True) ran"""
    from modest_amd.utils import pcdet_bind
    key = "pcdet.ops.pointnet2.pointnet2_stack.pointnet2_stack_cuda"
    names = list(pcdet_bind.SHIMS) + list(pcdet_bind.STAND_INS) + ["spconv.utils"]
    saved = {k: sys.modules.get(k) for k in names}
    try:
        sys.modules.pop(key, None)
        assert pcdet_bind.install(point_stack=True)[key] is ops
        mod = importlib.import_module(key)
        fns = ("ball_query_wrapper", "voxel_query_wrapper", "furthest_point_sampling_wrapper", "group_points_wrapper",
               "group_points_grad_wrapper", "three_nn_wrapper", "three_interpolate_wrapper", "three_interpolate_grad_wrapper")
        assert mod is ops and all(callable(getattr(mod, n)) for n in fns)
        xyz = torch.tensor([[0, 0, 0], [1, 0, 0], [5, 5, 5]], dtype=torch.float32, device=gpu)
        cnt = torch.tensor([3], dtype=torch.int32, device=gpu)
        idx = torch.zeros((3, 2), dtype=torch.int32, device=gpu)
        assert mod.ball_query_wrapper(1, 3, 1.5, 2, xyz, cnt, xyz, cnt, idx) == 1
        assert idx.cpu().tolist() == [[0, 1], [0, 1], [2, 2]]
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
