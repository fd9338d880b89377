"""GPU: the RoI-aware voxel pooling of csrc/roiaware_pool.hip (roiaware_pool3d_cuda.forward / backward), bit for bit
against

* the recorded outputs of the reference's own kernel text (tests/golden/roiaware_pool.npz): lists, pooled features,
  argmax and input gradients for both pool methods, sentinels included, with the lists' count words left non-zero on
  input to show that they are overwritten;
* the numpy restatement of the contract (tests/roiaware_seq.py) at edge shapes, on zero-extent and
  NaN boxes, with one voxel filled from many chunks by all four wavefronts, and at a detector-shaped case.

No element is excluded from any comparison.  The one known source of a mismatch is the one section 7e names, a last-bit
difference between the device's and the host's float64 cos / sin that changes the float32 rounding (about one angle in
2^29, derived not measured); a failing comparison reports the headings of the boxes involved.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import roiaware_seq as seq  # noqa: E402
import roipool_seq  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "roiaware_pool.npz")
POOLED_SENTINEL = np.float32(-777.25)
ARGMAX_SENTINEL, LIST_SENTINEL, COUNT_GARBAGE = -7, -9, 77
METHODS = ((0, "max"), (1, "avg"))


@pytest.fixture(scope="module")
def op(gpu):
    from modest_amd.utils import roiaware_voxel_pool_cuda
    return roiaware_voxel_pool_cuda


@pytest.fixture(scope="module")
def rec():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def givens(n, out, max_pts, c):
    """sentinel-filled outputs; the count words hold garbage: the forward writes them"""
    shape = (n,) + tuple(out)
    lists = np.full(shape + (max_pts,), LIST_SENTINEL, dtype=np.int32)
    lists[..., 0] = COUNT_GARBAGE
    return (lists, np.full(shape + (c,), POOLED_SENTINEL, dtype=np.float32),
            np.full(shape + (c,), ARGMAX_SENTINEL, dtype=np.int32))


def run_forward(op, gpu, rois, pts, feat, method, lists_given, pooled_given, argmax_given):
    lists, pooled, argmax = dev(lists_given, gpu), dev(pooled_given, gpu), dev(argmax_given, gpu)
    assert op.forward(dev(rois, gpu), dev(pts, gpu), dev(feat, gpu), argmax, lists, pooled, method) == 1
    return lists.cpu().numpy(), pooled.cpu().numpy(), argmax.cpu().numpy()


def run_backward(op, gpu, lists, argmax, grad_out, grad_in_given, method):
    grad_in = dev(grad_in_given, gpu)
    assert op.backward(dev(lists, gpu), dev(argmax, gpu), dev(grad_out, gpu), grad_in, method) == 1
    return grad_in.cpu().numpy()


def check(what, got, want, rois, as_bits=False):
    """every element; the boxes that differ are reported with their headings"""
    g, w = (bits(got), bits(want)) if as_bits else (np.asarray(got), np.asarray(want))
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if g.size == 0:
        return
    diff = g != w
    if what.startswith("grad_in"):
        assert not diff.any(), (what, "differs at (point, channel):", np.argwhere(diff)[:8].tolist(),
                                "headings of all boxes:", [float(v) for v in rois[:16, 6]])
        return
    bad = np.flatnonzero(diff.reshape(len(rois), -1).any(axis=1))
    assert len(bad) == 0, (what, "differs in boxes", bad[:8].tolist(), "headings", [float(rois[b, 6]) for b in bad[:8]])


def check_both_ways(op, gpu, rois, pts, feat, out, max_pts, rs, methods=METHODS):
    """forward and backward of the given methods against the restatement -> the lists"""
    n, c = len(rois), feat.shape[1]
    lists_given, pooled_given, argmax_given = givens(n, out, max_pts, c)
    grad_out = rs.randn(*((n,) + tuple(out) + (c,))).astype(np.float32)
    grad_in_given = rs.randn(len(pts), c).astype(np.float32)
    want_lists, _ = seq.build_lists(pts, rois, out, max_pts, lists_given)
    for method, tag in methods:
        want_pooled, want_argmax = seq.pool(want_lists, feat, method, pooled_given, argmax_given)
        lists, pooled, argmax = run_forward(op, gpu, rois, pts, feat, method, lists_given, pooled_given, argmax_given)
        check("lists " + tag, lists, want_lists, rois)
        check("pooled " + tag, pooled, want_pooled, rois, as_bits=True)
        check("argmax " + tag, argmax, want_argmax, rois)
        want_grad = seq.backward(want_lists, want_argmax, grad_out, grad_in_given, method)
        check("grad_in " + tag, run_backward(op, gpu, lists, argmax, grad_out, grad_in_given, method), want_grad, rois,
              as_bits=True)
    return want_lists


# ---- the fixture -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["crafted", "single", "cubic", "nolist"])
def test_fixture_bit_for_bit(op, gpu, rec, scene):
    rois, pts, feat = rec[scene + "_rois"], rec[scene + "_pts"], rec[scene + "_feat"]
    lists_given = rec[scene + "_lists_given"].copy()
    assert (lists_given[..., 0] == 0).all()
    lists_given[..., 0] = COUNT_GARBAGE                 # the reference needs zeros there; here the word is written
    for method, tag in METHODS:
        lists, pooled, argmax = run_forward(op, gpu, rois, pts, feat, method, lists_given, rec[scene + "_pooled_given"],
                                            rec[scene + "_argmax_given"])
        check("lists " + tag, lists, rec[scene + "_lists"], rois)
        check("pooled " + tag, pooled, rec[f"{scene}_pooled_{tag}"], rois, as_bits=True)
        check("argmax " + tag, argmax, rec[f"{scene}_argmax_{tag}"], rois)
        grad = run_backward(op, gpu, rec[scene + "_lists"], rec[f"{scene}_argmax_{tag}"], rec[scene + "_grad_out"],
                            rec[scene + "_grad_in_given"], method)
        check("grad_in " + tag, grad, rec[f"{scene}_grad_in_{tag}"], rois, as_bits=True)
    # the sentinels are part of the comparisons above; say so once more, by name
    empty = rec[scene + "_lists"][..., 0] == 0
    assert empty.any() or scene == "single"             # (one box, one voxel, 45 points: no empty voxel there)
    assert (pooled[empty] == rec[scene + "_pooled_given"][empty]).all()
    assert np.array_equal(argmax, rec[scene + "_argmax_given"])          # the last method was avg: argmax untouched


# ---- edge shapes -----------------------------------------------------------------------------------------------------
def small_case(rs, n_pts, n_box, c):
    pts = rs.uniform(-3, 3, (n_pts, 3)).astype(np.float32)
    rois = np.zeros((n_box, 7), dtype=np.float32)
    rois[:, :3] = rs.uniform(-2, 2, (n_box, 3))
    rois[:, 3:6] = rs.uniform(1.0, 5.0, (n_box, 3))
    rois[:, 6] = rs.uniform(-7, 7, n_box)
    if n_box > 1:
        rois[1, :2] += 50.0                              # one box off the cloud
    feat = rs.randn(n_pts, c).astype(np.float32)
    if c and n_pts > 4:
        feat[rs.randint(0, n_pts, n_pts // 4)] = np.float32(1.5)   # equal values: ties in many voxels
    return rois, pts, feat


# every npoints with every box count, grid, channel count and list length of the issue (not the full product)
EDGE_CONFIGS = ((1, (1, 1, 1), 0, 1), (5, (3, 5, 2), 1, 2), (130, (3, 5, 2), 4, 5), (5, (12, 12, 12), 65, 128),
                (1, (12, 12, 12), 128, 5))


@pytest.mark.parametrize("n_pts", [1, 63, 64, 65, 1000, 5003])
def test_edge_shapes(op, gpu, n_pts):
    rs = np.random.RandomState(n_pts)
    for n_box, out, c, max_pts in EDGE_CONFIGS:
        rois, pts, feat = small_case(rs, n_pts, n_box, c)
        check_both_ways(op, gpu, rois, pts, feat, out, max_pts, rs)


def test_one_voxel_filled_from_many_chunks_by_all_wavefronts(op, gpu):
    """one big box, one voxel, 5 003 points: every chunk and every wavefront's sub-blocks add to the same list, whose
    order must be the points' -- capped at 127 and, with max_pts 5004, not capped at all"""
    rs = np.random.RandomState(5)
    n = 5003
    pts = rs.uniform(-20, 20, (n, 3)).astype(np.float32)
    rois = np.array([[0, 0, 0, 100, 100, 100, 2.0]], dtype=np.float32)
    feat = rs.randn(n, 3).astype(np.float32)
    for max_pts in (128, 5004):
        lists = check_both_ways(op, gpu, rois, pts, feat, (1, 1, 1), max_pts, rs)
        kept = min(n, max_pts - 1)
        assert lists[0, 0, 0, 0, 0] == kept and lists[0, 0, 0, 0, 1:1 + kept].tolist() == list(range(kept))
    # the same cloud through a grid whose voxel ids meet every wavefront (id mod 4) in every chunk
    check_both_ways(op, gpu, rois, pts, feat, (3, 5, 2), 128, rs)


def test_zero_extent_and_nan_boxes(op, gpu):
    rs = np.random.RandomState(9)
    pts = rs.uniform(-1, 1, (300, 3)).astype(np.float32)
    pts[:40, 0] = rs.choice(np.array([0.0, -0.0, 5e-6, -5e-6, 9e-6], dtype=np.float32), 40)   # on / beside the plane x = 0
    pts[40:60] = 0.0
    pts[50:60, :2] = rs.uniform(-9e-6, 9e-6, (10, 2))                                        # within the margin of the origin
    pts[60, 2] = np.nan
    pts[61, 0] = np.nan
    rois = np.array([[0, 0, 0, 0, 2, 2, 0],            # no extent in x: q_x is +-inf or NaN
                     [0, 0, 0, 2, 0, 2, 0.0],          # ... in y
                     [0, 0, 0, 2, 2, 0, 0],            # ... in z: only z == 0 is inside
                     [0, 0, 0, 0, 0, 0, 0],            # the padding box
                     [np.nan, 0, 0, 2, 2, 2, 0],       # holds nothing
                     [0, 0, 0, 2, 2, np.nan, 0],       # a NaN dz does not reject; q_z is NaN -> 0
                     [0, 0, 0, np.inf, 2, 2, 0],       # res = inf, q = NaN
                     [0, 0, 0, 2, 2, 2, np.nan]], dtype=np.float32)
    feat = rs.randn(300, 4).astype(np.float32)
    mask, _ = seq.voxel_ids(pts, rois, (3, 5, 2))
    assert mask[:4].any(axis=1).all() and not mask[4].any() and mask[5].sum() > 100
    check_both_ways(op, gpu, rois, pts, feat, (3, 5, 2), 128, rs)
    check_both_ways(op, gpu, rois, pts, feat, (4, 4, 4), 3, rs)


def test_grid_above_the_lds_limit_is_an_error_and_writes_nothing(op, gpu):
    rs = np.random.RandomState(2)
    rois, pts, feat = small_case(rs, 100, 1, 1)
    out, max_pts = (25, 24, 24), 2                       # 14 400 voxels > 13 824
    given = givens(1, out, max_pts, 1)
    t = [dev(a, gpu) for a in given]
    with pytest.raises(RuntimeError, match="13824"):
        op.forward(dev(rois, gpu), dev(pts, gpu), dev(feat, gpu), t[2], t[0], t[1], 0)
    torch.cuda.synchronize()
    for a, b in zip(t, given):
        assert np.array_equal(a.cpu().numpy(), b)
    # the largest grid that fits does run
    check_both_ways(op, gpu, rois, pts, feat, (24, 24, 24), 2, rs, methods=METHODS[:1])


# ---- the detector's shape, kept small -------------------------------------------------------------------------------------
def test_detector_shape(op, gpu):
    """2 clouds of 12 288 points x 16 RoIs, 12^3 voxels, 128 words per list: C = 4 avg and C = 128 max, forward and backward"""
    xyz, feat, objs = roipool_seq.synthetic_scans()
    rois = roipool_seq.synthetic_rois(np.random.RandomState(16), objs, 16)
    rs = np.random.RandomState(1)
    counts = []
    for b in range(2):
        lists = check_both_ways(op, gpu, rois[b], xyz[b], feat[b, :, :4], (12, 12, 12), 128, rs, methods=METHODS[1:])
        check_both_ways(op, gpu, rois[b], xyz[b], np.ascontiguousarray(feat[b, :, :128]), (12, 12, 12), 128, rs,
                        methods=METHODS[:1])
        _, full = seq.build_lists(xyz[b], rois[b], (12, 12, 12), 128, lists)
        counts += [len(k) for groups in full for k in groups.values()]
        assert (lists[..., 0] == 0).any()
    counts = np.array(counts)
    assert ((counts > 0) & (counts < 127)).any() and (counts > 127).any(), np.sort(counts)[-8:]


def test_backward_has_one_set_of_bits(op, gpu):
    """overlapping boxes: many (point, channel) sums have several terms; two runs of the same backward agree bit for bit"""
    rs = np.random.RandomState(31)
    rois, pts, feat = small_case(rs, 5003, 40, 16)
    rois[:, :3] *= 0.2                                   # all boxes around one site
    out, max_pts = (3, 5, 2), 128
    mask, _ = seq.voxel_ids(pts, rois, out)
    assert (mask.sum(axis=0) >= 8).sum() > 500
    grad_out = rs.randn(40, 3, 5, 2, 16).astype(np.float32)
    zero = np.zeros((5003, 16), dtype=np.float32)
    for method, tag in METHODS:
        lists, _, argmax = run_forward(op, gpu, rois, pts, feat, method, *givens(40, out, max_pts, 16))
        a = run_backward(op, gpu, lists, argmax, grad_out, zero, method)
        b = run_backward(op, gpu, lists, argmax, grad_out, zero, method)
        assert np.array_equal(bits(a), bits(b)), tag
        check("grad_in " + tag, a, seq.backward(lists, argmax, grad_out, zero, method), rois, as_bits=True)


def test_zero_size_calls(op, gpu):
    f = dict(dtype=torch.float32, device=gpu)
    i = dict(dtype=torch.int32, device=gpu)
    for method in (0, 1):
        # no boxes: nothing to write
        assert op.forward(torch.zeros(0, 7, **f), torch.zeros(5, 3, **f), torch.zeros(5, 4, **f), torch.zeros(0, 2, 2, 2, 4, **i),
                          torch.zeros(0, 2, 2, 2, 8, **i), torch.zeros(0, 2, 2, 2, 4, **f), method) == 1
        assert op.backward(torch.zeros(0, 2, 2, 2, 8, **i), torch.zeros(0, 2, 2, 2, 4, **i), torch.zeros(0, 2, 2, 2, 4, **f),
                           torch.full((5, 4), 3.0, **f), method) == 1
        # no points: every count is written as 0, argmax (max) is -1, pooled stays
        lists, pooled = torch.full((3, 2, 2, 2, 8), 5, **i), torch.full((3, 2, 2, 2, 4), 2.5, **f)
        argmax = torch.full((3, 2, 2, 2, 4), 9, **i)
        assert op.forward(torch.ones(3, 7, **f), torch.zeros(0, 3, **f), torch.zeros(0, 4, **f), argmax, lists, pooled, method) == 1
        assert (lists[..., 0] == 0).all() and (lists[..., 1:] == 5).all() and (pooled == 2.5).all()
        assert (argmax == (-1 if method == 0 else 9)).all()
        assert op.backward(lists, argmax, torch.ones(3, 2, 2, 2, 4, **f), torch.zeros(0, 4, **f), method) == 1
        # no channels: the lists are still built
        lists = torch.full((3, 2, 2, 2, 8), 5, **i)
        assert op.forward(torch.tensor([[0, 0, 0, 4, 4, 4, 0.0]] * 3, **f), torch.zeros(6, 3, **f), torch.zeros(6, 0, **f),
                          torch.zeros(3, 2, 2, 2, 0, **i), lists, torch.zeros(3, 2, 2, 2, 0, **f), method) == 1
        assert lists[..., 0].sum().item() == 18 and lists[0, 1, 1, 1].tolist() == [6, 0, 1, 2, 3, 4, 5, 5]
        assert op.backward(lists, torch.zeros(3, 2, 2, 2, 0, **i), torch.zeros(3, 2, 2, 2, 0, **f), torch.zeros(6, 0, **f), method) == 1
    torch.cuda.synchronize()


# ---- module level ----------------------------------------------------------------------------------------------------
def test_layer_matches_the_raw_ops_and_autograd_the_raw_backward(op, gpu):
    from modest_amd.utils.roiaware_pool3d_utils import RoIAwarePool3d
    rs = np.random.RandomState(77)
    rois, pts, feat = small_case(rs, 1000, 5, 16)
    out, max_pts = (3, 5, 2), 16
    stream = torch.cuda.Stream(device=gpu)
    layer = RoIAwarePool3d(out, max_pts_each_voxel=max_pts)
    grad_out = rs.randn(5, 3, 5, 2, 16).astype(np.float32)
    for method, tag in METHODS:
        lists_given, _, argmax_given = givens(5, out, max_pts, 16)
        zeros = np.zeros((5, 3, 5, 2, 16), dtype=np.float32)
        lists, raw_pooled, argmax = run_forward(op, gpu, rois, pts, feat, method, lists_given, zeros, argmax_given)
        raw_grad = run_backward(op, gpu, lists, argmax, grad_out, np.zeros((1000, 16), dtype=np.float32), method)
        # non-contiguous views of every input, on a side stream
        r_nc = dev(np.ascontiguousarray(rois.T), gpu).t()
        p_nc = dev(np.ascontiguousarray(pts.T), gpu).t()
        f_nc = dev(np.ascontiguousarray(feat.T), gpu).t().requires_grad_(True)
        assert not (r_nc.is_contiguous() or p_nc.is_contiguous() or f_nc.is_contiguous())
        g_nc = dev(np.ascontiguousarray(np.moveaxis(grad_out, 4, 0)), gpu).permute(1, 2, 3, 4, 0)
        stream.wait_stream(torch.cuda.current_stream(gpu))
        with torch.cuda.stream(stream):
            pooled = layer(r_nc, p_nc, f_nc, pool_method=tag)
            pooled.backward(g_nc)
        stream.synchronize()
        assert pooled.shape == (5, 3, 5, 2, 16) and f_nc.grad.shape == (1000, 16)
        assert np.array_equal(bits(pooled.detach().cpu().numpy()), bits(raw_pooled)), tag
        assert (raw_pooled != 0).any() and (raw_pooled[lists[..., 0] == 0] == 0).all()
        assert np.array_equal(bits(f_nc.grad.cpu().numpy()), bits(raw_grad)), tag
        assert (raw_grad != 0).any()
