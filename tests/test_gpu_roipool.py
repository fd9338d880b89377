"""GPU: the RoI point pooling (roipoint_pool3d_cuda.forward) and points_in_boxes_gpu of csrc/roipool.hip, bit for bit
against

* the recorded outputs of the reference's own kernel text (tests/golden/roipool.npz), flags, rows, the sentinel rows of
  empty and pre-flagged boxes and box_idx;
* the numpy restatement of the contract (tests/roipool_seq.py) at the detector's shapes: B = 2
  clouds of 12 288 points sampled WITH repetition from synthetic Lyft-shape scans, 128 / 100 RoIs, 512 samples, 130
  feature channels; 40 gt boxes padded with zero rows and their 0.2-enlarged twins; and at small edge shapes.

No element is excluded from any comparison.  The one known source of a mismatch is a last-bit difference between the
device's and the host's float64 cos / sin that changes the float32 rounding (about one angle in 2^29, derived not
measured); a failing comparison reports the headings of the boxes involved.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import roipool_seq as seq  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "roipool.npz")
SENTINEL = np.float32(-777.25)


@pytest.fixture(scope="module")
def pool(gpu):
    from modest_amd.utils.roipoint_pool3d import roipoint_pool3d_cuda
    return roipoint_pool3d_cuda


@pytest.fixture(scope="module")
def aware(gpu):
    from modest_amd.utils import roiaware_pool3d_cuda
    return roiaware_pool3d_cuda


@pytest.fixture(scope="module")
def rec():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run_pool(pool, gpu, xyz, boxes, feat, s, pooled_given=None, flag_given=None):
    B, M = boxes.shape[:2]
    c = feat.shape[2]
    pooled = (torch.full((B, M, s, 3 + c), float(SENTINEL), dtype=torch.float32, device=gpu) if pooled_given is None
              else dev(pooled_given, gpu))
    flag = torch.zeros((B, M), dtype=torch.int32, device=gpu) if flag_given is None else dev(flag_given, gpu)
    assert pool.forward(dev(xyz, gpu), dev(boxes, gpu), dev(feat, gpu), pooled, flag) == 1
    return pooled.cpu().numpy(), flag.cpu().numpy()


def run_pib(aware, gpu, boxes, pts, given=None):
    B, N = pts.shape[:2]
    out = torch.full((B, N), -1, dtype=torch.int32, device=gpu) if given is None else dev(given, gpu)
    assert aware.points_in_boxes_gpu(dev(boxes, gpu), dev(pts, gpu), out) == 1
    return out.cpu().numpy()


def check_pool(got, want, boxes):
    (gp, gf), (wp, wf) = got, want
    bad = np.argwhere(gf != wf)
    assert len(bad) == 0, ("flags differ at (cloud, box), headings:", bad[:8].tolist(), [float(boxes[b, i, 6]) for b, i in bad[:8]])
    diff = (bits(gp) != bits(wp)).any(axis=(2, 3))
    bad = np.argwhere(diff)
    assert len(bad) == 0, ("rows differ at (cloud, box), headings:", bad[:8].tolist(), [float(boxes[b, i, 6]) for b, i in bad[:8]])


def check_pib(got, want, boxes):
    bad = np.argwhere(got != want)
    heads = [(float(boxes[b, got[b, k], 6]) if got[b, k] >= 0 else None, float(boxes[b, want[b, k], 6]) if want[b, k] >= 0 else None)
             for b, k in bad[:8]]
    assert len(bad) == 0, ("box_idx differs at (cloud, point), headings (got, want):", bad[:8].tolist(), heads)


# ---- the fixture -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["crafted", "rand37", "rand1"])
def test_fixture_bit_for_bit(pool, aware, gpu, rec, scene):
    xyz, boxes, feat, s = rec[scene + "_xyz"], rec[scene + "_boxes"], rec[scene + "_feat"], int(rec[scene + "_s"])
    got = run_pool(pool, gpu, xyz, boxes, feat, s, rec[scene + "_pooled_given"], rec[scene + "_flag_given"])
    check_pool(got, (rec[scene + "_pooled"], rec[scene + "_flag"]), boxes)
    # the sentinel rows of empty and of pre-flagged boxes are part of the comparison above; say so once more, by name
    untouched = (rec[scene + "_flag"] != 0)
    assert untouched.any()
    assert np.array_equal(bits(got[0][untouched]), bits(rec[scene + "_pooled_given"][untouched]))
    check_pib(run_pib(aware, gpu, boxes, xyz), rec[scene + "_box_idx"], boxes)


# ---- the detector's shapes ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scans():
    """B = 2 clouds of 12 288 points sampled with repetition from synthetic Lyft-shape scans, 130 feature channels, and
    the scans' objects as boxes [cx, cy, cz, dx, dy, dz, rz] in the clouds' frame"""
    return seq.synthetic_scans()


rois = seq.synthetic_rois


@pytest.mark.parametrize("m", [128, 100])
def test_full_pooling_shape(pool, gpu, scans, m):
    xyz, feat, objs = scans
    boxes = seq.enlarge(rois(np.random.RandomState(m), objs, m), (1.0, 1.0, 1.0))
    s = 512
    cnt = seq.inside_counts(xyz, boxes)
    assert (cnt == 0).any() and ((cnt > 0) & (cnt < s)).any() and (cnt >= 4 * s).any(), np.sort(cnt.ravel())
    flag0 = np.zeros((2, m), dtype=np.int32)
    flag0[:, 5] = 1
    given = np.full((2, m, s, 133), SENTINEL, dtype=np.float32)
    want = seq.roipoint_pool3d(xyz, boxes, feat, s, given, flag0)
    got = run_pool(pool, gpu, xyz, boxes, feat, s, given, flag0)
    assert got[0].nbytes == 2 * m * s * 133 * 4              # 70 MB at m = 128, 54 MB at m = 100
    check_pool(got, want, boxes)


def test_full_target_assignment_shape(aware, gpu, scans):
    xyz, _, objs = scans
    rs = np.random.RandomState(40)
    m = 40
    boxes = seq.gt_boxes(rs, objs, m, (23, 31))                   # the rest are OpenPCDet's zero rows
    pts = xyz.copy()
    pts[0, 100] = 0.0                                            # a point at the origin: the first zero row takes it
    for bx in (boxes, seq.enlarge(boxes.reshape(-1, 7), (0.2, 0.2, 0.2)).reshape(2, m, 7)):
        want = seq.points_in_boxes(bx, pts)
        assert (want >= 0).sum() > 200 and (want == -1).any()
        check_pib(run_pib(aware, gpu, bx, pts), want, bx)
    assert 0 <= seq.points_in_boxes(boxes, pts)[0, 100] <= 23    # the first zero row, unless a gt box holds the origin
    # more boxes than one LDS tile, the decisive box last
    many = np.concatenate([np.repeat(boxes[:, 36:37], 300, axis=1), boxes], axis=1)
    want = seq.points_in_boxes(many, pts)
    assert want.max() >= 300
    check_pib(run_pib(aware, gpu, many, pts), want, many)


# ---- small edge shapes -----------------------------------------------------------------------------------------------
def small_case(rs, n, m, c):
    xyz = rs.uniform(-3, 3, (2, n, 3)).astype(np.float32)
    boxes = np.zeros((2, m, 7), dtype=np.float32)
    boxes[:, :, :3] = rs.uniform(-2, 2, (2, m, 3))
    boxes[:, :, 3:6] = rs.uniform(1.0, 5.0, (2, m, 3))
    boxes[:, :, 6] = rs.uniform(-7, 7, (2, m))
    if m > 1:
        boxes[0, 1, :2] += 50.0
    return xyz, boxes, rs.randn(2, n, c).astype(np.float32)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_small_edge_shapes(pool, aware, gpu, n):
    rs = np.random.RandomState(n)
    for m in (1, 5):
        for s in (1, 37, 512):
            for c in (0, 1):
                xyz, boxes, feat = small_case(rs, n, m, c)
                given = np.full((2, m, s, 3 + c), SENTINEL, dtype=np.float32)
                flag0 = np.zeros((2, m), dtype=np.int32)
                want = seq.roipoint_pool3d(xyz, boxes, feat, s, given, flag0)
                check_pool(run_pool(pool, gpu, xyz, boxes, feat, s, given, flag0), want, boxes)
        check_pib(run_pib(aware, gpu, boxes, xyz), seq.points_in_boxes(boxes, xyz), boxes)


def test_walk_longer_than_one_chunk_keeps_index_order(pool, gpu):
    """hits spread thinly over 5 000 points: the list is filled over several chunks by all four wavefronts"""
    rs = np.random.RandomState(5)
    n, s = 5003, 64
    xyz = rs.uniform(-20, 20, (2, n, 3)).astype(np.float32)
    boxes = np.array([[[0, 0, 0, 9, 7, 50, 0.4], [3, 2, 0, 14, 9, 50, -1.1], [0, 0, 0, 100, 100, 100, 2.0]]] * 2, dtype=np.float32)
    feat = rs.randn(2, n, 3).astype(np.float32)
    cnt = seq.inside_counts(xyz, boxes)
    assert (cnt[:, 0] > s).all() and (cnt[:, 2] == n).all()
    given = np.zeros((2, 3, s, 6), dtype=np.float32)
    flag0 = np.zeros((2, 3), dtype=np.int32)
    check_pool(run_pool(pool, gpu, xyz, boxes, feat, s, given, flag0), seq.roipoint_pool3d(xyz, boxes, feat, s, given, flag0), boxes)
    s = 3000                                                      # most of the cloud is walked, the fill repeats
    given = np.zeros((2, 3, s, 6), dtype=np.float32)
    check_pool(run_pool(pool, gpu, xyz, boxes, feat, s, given, flag0), seq.roipoint_pool3d(xyz, boxes, feat, s, given, flag0), boxes)


def test_zero_size_calls(pool, aware, gpu):
    f = dict(dtype=torch.float32, device=gpu)
    i = dict(dtype=torch.int32, device=gpu)
    # no boxes, no clouds: nothing is written
    assert pool.forward(torch.zeros(2, 10, 3, **f), torch.zeros(2, 0, 7, **f), torch.zeros(2, 10, 4, **f),
                        torch.zeros(2, 0, 8, 7, **f), torch.zeros(2, 0, **i)) == 1
    assert pool.forward(torch.zeros(0, 10, 3, **f), torch.zeros(0, 3, 7, **f), torch.zeros(0, 10, 4, **f),
                        torch.zeros(0, 3, 8, 7, **f), torch.zeros(0, 3, **i)) == 1
    # no points: every flag is set, the rows stay
    pooled, flag = torch.full((2, 3, 8, 7), 5.0, **f), torch.zeros(2, 3, **i)
    assert pool.forward(torch.zeros(2, 0, 3, **f), torch.ones(2, 3, 7, **f), torch.zeros(2, 0, 4, **f), pooled, flag) == 1
    assert (flag == 1).all() and (pooled == 5.0).all()
    # no samples: every flag is set (the reference's count never leaves 0)
    flag = torch.zeros(2, 3, **i)
    assert pool.forward(torch.zeros(2, 4, 3, **f), torch.ones(2, 3, 7, **f), torch.zeros(2, 4, 4, **f),
                        torch.zeros(2, 3, 0, 7, **f), flag) == 1
    assert (flag == 1).all()
    for b, m, n in ((0, 3, 5), (2, 0, 5), (2, 3, 0)):
        out = torch.full((b, n), -3, **i)
        assert aware.points_in_boxes_gpu(torch.zeros(b, m, 7, **f), torch.zeros(b, n, 3, **f), out) == 1
        assert (out == -3).all()
    with pytest.raises(RuntimeError, match="15360"):
        pool.forward(torch.zeros(1, 4, 3, **f), torch.ones(1, 1, 7, **f), torch.zeros(1, 4, 0, **f),
                     torch.zeros(1, 1, 15361, 3, **f), torch.zeros(1, 1, **i))
    torch.cuda.synchronize()


# ---- module level ----------------------------------------------------------------------------------------------------
def test_modules_match_the_raw_ops(pool, aware, gpu, scans):
    from modest_amd.utils import roiaware_pool3d_utils
    from modest_amd.utils.roipoint_pool3d.roipoint_pool3d_utils import RoIPointPool3d
    xyz, feat, objs = scans
    boxes = rois(np.random.RandomState(3), objs, 64)
    x, f, bx = dev(xyz, gpu), dev(feat[:, :, :16], gpu), dev(boxes, gpu)
    raw_pooled, raw_flag = run_pool(pool, gpu, xyz, boxes, feat[:, :, :16], 512,
                                    np.zeros((2, 64, 512, 19), dtype=np.float32))
    raw_idx = run_pib(aware, gpu, boxes, xyz)
    layer = RoIPointPool3d(512, (0, 0, 0))
    stream = torch.cuda.Stream(device=gpu)
    # a non-contiguous view of the features and of the points: the wrappers make them contiguous
    f_nc = dev(np.ascontiguousarray(feat[:, :, :16].transpose(0, 2, 1)), gpu).transpose(1, 2)
    x_nc = dev(np.ascontiguousarray(xyz.transpose(0, 2, 1)), gpu).transpose(1, 2)
    assert not f_nc.is_contiguous() and not x_nc.is_contiguous()
    stream.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(stream):
        pooled, flag = layer(x_nc, f_nc, bx)
        idx = roiaware_pool3d_utils.points_in_boxes_gpu(x_nc, bx)
    stream.synchronize()
    assert pooled.shape == (2, 64, 512, 19) and flag.dtype == torch.int32 and idx.dtype == torch.int32
    assert np.array_equal(flag.cpu().numpy(), raw_flag) and np.array_equal(bits(pooled.cpu().numpy()), bits(raw_pooled))
    assert np.array_equal(idx.cpu().numpy(), raw_idx)
    # the module enlarges the boxes itself
    wide = RoIPointPool3d(512, (1.0, 1.0, 1.0))(x, f, bx)
    want = seq.roipoint_pool3d(xyz, seq.enlarge(boxes, (1.0, 1.0, 1.0)), feat[:, :, :16], 512,
                               np.zeros((2, 64, 512, 19), dtype=np.float32), np.zeros((2, 64), dtype=np.int32))
    check_pool((wide[0].cpu().numpy(), wide[1].cpu().numpy()), want, boxes)
    with pytest.raises(NotImplementedError):
        p, _ = RoIPointPool3d(16, 0.5)(x.requires_grad_(True), f.clone().requires_grad_(True), bx)
        p.sum().backward()
