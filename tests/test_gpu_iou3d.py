"""GPU: csrc/iou3d.hip (rotated BEV overlap / IoU, 3-D IoU, rotated and axis-aligned NMS) at detector shapes and on
degenerate geometry.  Inputs, exact geometry and the derived bounds come from tests/iou3d_cases.py;
tests/test_iou3d_oracle_cpu.py proves on the CPU that the reference's own arithmetic meets every cap asserted here.

Three yardsticks, none of them tuned:
  * the f64 twin of the oracle (oracle/iou3d_oracle.c with the double trig of trig_f32.h) for the kernels that evaluate
    their trig on the device -- pair kernels and NMS keep lists, BIT FOR BIT, no tolerance;
  * the glibc build of the oracle for the paths that are handed the host's cosf / sinf, bit for bit;
  * tests/rect_exact.py (exact clipping) within (P_a + P_b) * ulp32(R) on well-conditioned pairs.
The only tolerances in this file are that derived bound and the 2 ulp of boxes_iou3d_gpu (same IEEE operations as its
NumPy statement; the allowance is for the order of the three-factor volume product).

One-line mutants of iou3d.hip this module was run against on an MI355X (not committed):
  * in_box2d `<` -> `<=`: fails test_pair_kernels_equal_the_twin_bit_for_bit at both offsets (the negative-extent family,
    whose half extent + margin is exactly 0, and a few pairs of "shifted by 0.01" / "turned by 0.1");
  * the diagonal tile starting at `lane + 2`: fails 17 NMS tests (detector-like proposals, n >= 127, pre_maxsize, equal
    scores, the reused context, the side stream);
  * the tile's column decoded one short (the last column block of a row never computed): fails 20 NMS tests, from n = 65 on;
  * the diagonal tile starting at `lane` instead of `lane + 1`: passes, and no test through the API can fail it -- it only
    sets a box's own bit in its own row, which the host walk ORs in after it has kept that box and never reads again.
"""
import math

import numpy as np
import pytest

import iou3d_cases as ic
from oracle import labels as ol

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (1, 65), (65, 1), (63, 3), (128, 50), (ic.K, ic.K))
MAX_DROPPED = 0.001      # share of input rows that may be dropped because device and host libm round a heading differently


def _dev(x, gpu):
    import torch
    return torch.from_numpy(np.array(x)).to(gpu)      # a copy: the shared inputs are read-only


def _same(got, want):
    return np.array_equal(got, want, equal_nan=True)


def _describe(got, want, A, B):
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    i, j = np.nonzero(bad)
    k = int(np.argmax(np.abs(got.astype(np.float64) - want)[i, j])) if len(i) else 0
    return (f"{bad.sum()} of {bad.size} values differ, largest |d| {np.abs(got.astype(np.float64) - want)[bad].max():.3g} at "
            f"a={A[i[k]].tolist()} b={B[j[k]].tolist()}: got {got[i[k], j[k]]!r}, want {want[i[k], j[k]]!r}")


def _trig_differs(h, gpu):
    """rows whose heading the device's double cos / sin, rounded to float32, evaluates differently from the host's double
    libm (math.cos / math.sin: the functions the twin calls): there kernel and twin start from different numbers and a
    bit-for-bit comparison says nothing about the kernel"""
    import torch
    hd = _dev(h, gpu).double()
    dev = torch.stack([torch.cos(hd).float(), torch.sin(hd).float(), torch.cos(-hd).float(), torch.sin(-hd).float()], 1).cpu().numpy()
    host = np.array([[math.cos(v), math.sin(v), math.cos(-v), math.sin(-v)] for v in h.astype(np.float64)]).astype(np.float32)
    return (dev != host).any(1)


# --------------------------------------------------------------------------------------- a. pair kernels, bit for bit
@pytest.mark.parametrize("offset", ic.OFFSETS)
def test_pair_kernels_equal_the_twin_bit_for_bit(gpu, offset):
    """ops.boxes_iou_bev (IoU and overlap_only) on every family of tests/iou3d_cases.py, 500 x 500 and the slices (1, 1),
    (1, 65), (65, 1), (63, 3), (128, 50): np.array_equal with the f64 twin.  Rows whose heading the device's double libm
    rounds differently from the host's are dropped first and counted (at most 0.1 % of the rows); no tolerance anywhere.
    The disjoint family must be exactly 0 and nothing may be NaN (the twin holds none on these inputs)."""
    from modest_amd import ops
    n_rows = n_dropped = 0
    for name, (A, B) in ic.families(offset).items():
        drop = _trig_differs(A[:, 6], gpu) | _trig_differs(B[:, 6], gpu)
        n_rows += 2 * len(A)
        n_dropped += 2 * int(drop.sum())
        A, B = A[~drop], B[~drop]
        want_iou, want_ov = ic.bev(A, B, False, "f64"), ic.bev(A, B, True, "f64")
        assert not np.isnan(want_iou).any()
        if name == "disjoint":
            assert ic.family_disjoint_is_disjoint(A, B) and not want_iou.any() and not want_ov.any()
        a, b = _dev(A, gpu), _dev(B, gpu)
        for na, nb in SHAPES:
            na, nb = min(na, len(A)), min(nb, len(B))
            got_iou = ops.boxes_iou_bev(a[:na], b[:nb]).cpu().numpy()
            got_ov = ops.boxes_iou_bev(a[:na], b[:nb], overlap_only=True).cpu().numpy()
            assert got_iou.shape == got_ov.shape == (na, nb)
            assert _same(got_iou, want_iou[:na, :nb]), (name, na, nb, _describe(got_iou, want_iou[:na, :nb], A, B))
            assert _same(got_ov, want_ov[:na, :nb]), (name, na, nb, _describe(got_ov, want_ov[:na, :nb], A, B))
    print(f"offset {offset}: {n_dropped} of {n_rows} rows dropped for their heading's trig")
    assert n_dropped <= MAX_DROPPED * n_rows, (n_dropped, n_rows)


def test_pair_kernels_on_empty_sets(gpu):
    """(0, 5) and (5, 0): an empty matrix, no error; the next call is right"""
    import torch
    from modest_amd import ops
    from modest_amd.utils.iou3d_nms import iou3d_nms_utils as iu
    A, B = ic.random_sets((0, 0))
    a, none = _dev(A[:5], gpu), torch.zeros((0, 7), dtype=torch.float32, device=gpu)
    for fn in (ops.boxes_iou_bev, lambda x, y: ops.boxes_iou_bev(x, y, overlap_only=True), iu.boxes_iou_bev, iu.boxes_iou3d_gpu):
        assert tuple(fn(none, a).shape) == (0, 5) and tuple(fn(a, none).shape) == (5, 0)
    assert ops.boxes_iou_bev_host(np.zeros((0, 7), np.float32), A[:5]).shape == (0, 5)
    assert ops.boxes_iou_bev_host(A[:5], np.zeros((0, 7), np.float32)).shape == (5, 0)
    assert _same(ops.boxes_iou_bev(a, a).cpu().numpy(), ol.boxes_iou_bev(A[:5], A[:5], arith="f64"))


@pytest.mark.parametrize("offset", ic.OFFSETS)
def test_host_trig_paths_equal_the_glibc_oracle_bit_for_bit(gpu, offset):
    """ops.boxes_iou_bev_host and iou3d_nms_utils.boxes_bev_iou_cpu (the paths that are handed the host's cosf / sinf: the
    label stage's objs_nms) on every family, 500 x 500, against the glibc oracle: np.array_equal, and every sliced shape
    equal to the slice of the full matrix.

    This test found a bug.  The host-trig kernels took cosf / sinf from the host but sorted the clipped polygon's vertices
    by the DEVICE's atan2 ((float)atan2(double, double)), where the reference's CPU path sorts by glibc's atan2f.  Where
    two vertices lie within an ulp of the same polar angle the two orders differ and so does the fan area: 304 of the
    7 250 000 values of offset 0 differed, by at most 8.9e-7 IoU (turned by pi 54, swapped + pi/2 51, heading + 2 pi k 36,
    turned by 1e-7 75, shifted by 1e-5 1, edge sharing 32, edge gaps -0.005 / -0.02 25 / 28, special headings 2), and 23 of
    offset 70, by at most 4.4e-6 (measured on an MI355X, and equal to what a CPU build of the oracle with atan2 alone
    replaced predicts).  None on identical boxes (the self-IoU objs_nms ranks by), random sets or label rows, which is
    all the suite held before.  The kernels now report pairs whose sorted angles lie within 8 ulp of each other and the
    host recomputes those with atan2f (iou3d.hip: box_overlap<TIES>, host_iou_bev)."""
    from modest_amd import ops
    from modest_amd.utils.iou3d_nms import iou3d_nms_utils as iu
    report = []
    for name, (A, B) in ic.families(offset).items():
        want = ic.bev(A, B, False, "glibc")
        full = ops.boxes_iou_bev_host(A, B)
        for label, got in (("ops.boxes_iou_bev_host", full), ("boxes_bev_iou_cpu", iu.boxes_bev_iou_cpu(A.copy(), B.copy()))):
            assert got.shape == want.shape and got.dtype == np.float32
            if not _same(got, want):
                report.append((name, label, _describe(got, want, A, B)))
        for na, nb in SHAPES[:-1]:
            assert _same(ops.boxes_iou_bev_host(A[:na], B[:nb]), full[:na, :nb]), (name, na, nb)
    assert not report, report


# the families on which the host-trig kernels differed from the glibc oracle before near-tied angles were resolved on the host
TIE_FAMILIES = (("turned by pi", 500), ("swapped + pi/2", 257), ("heading + 2 pi k", 129), ("turned by 1e-07", 400),
                ("edge sharing", 300), ("edge gap -0.005", 65), ("edge gap -0.02", 500), ("turned by 1e-05", 450),
                ("shifted by 1e-05", 333))


def _objs8(boxes):
    """(n, 7) float32 boxes -> the (n, 8) float64 object rows {t0, t1, t2, l, w, h, ry, volume} whose objs_nms boxes they
    are (pointcloud_utils.py:322-324: [t0, t2, 0, l, w, h, -ry] as float32; every float32 is exact in double)"""
    b = boxes.astype(np.float64)
    z = np.zeros(len(b))
    return np.ascontiguousarray(np.c_[b[:, 0], z, b[:, 1], b[:, 3], b[:, 4], b[:, 5], -b[:, 6], z])


@pytest.mark.parametrize("offset", ic.OFFSETS)
def test_objs_iou_and_its_batch_on_degenerate_sets(gpu, offset):
    """ops.objs_iou_batch (modest_objs_iou_batch -> pair_sets_kernel: what the label stage of a chain runs) and
    ops.objs_iou on box sets made of the first m rows of both sides of a degenerate family, so that the self-IoU matrix
    holds the family in its off-diagonal blocks: eleven sets of 0 to 1 000 boxes in ONE batch call, an empty set and a set
    of one box among them, each np.array_equal with the glibc oracle.  The oracle built with atan2 alone in double
    (arith="atan2_f64": the kernel's arithmetic before the host resolves near-tied angles) differs from the glibc oracle
    on the batch as a whole and on at least five of the sets, so a batch call that lost its resolution, or resolved from
    another set's tie bytes, fails here.  Values it decides per family set, measured on the CPU: offset 0: 112, 53, 19,
    81, 29, 7, 52, 5, 1; offset 70: 4, 7, 0, 0, 0, 0, 2, 11, 12."""
    from modest_amd import ops
    fam = ic.families(offset)
    sets = []
    for k, (name, m) in enumerate(TIE_FAMILIES):
        A, B = fam[name]
        sets.append(np.concatenate([A[:m], B[:m]]))
        if k == 1:
            sets.append(np.zeros((0, 7), np.float32))
        if k == 4:
            sets.append(np.ascontiguousarray(A[:1]))
    want = [ic.bev(s, s, False, "glibc") for s in sets]
    decided = [int((~((ic.bev(s, s, False, "atan2_f64") == w) | np.isnan(w))).sum()) for s, w in zip(sets, want)]
    print(f"offset {offset}: values the tie resolution decides, per set: {decided}")
    assert sum(d > 0 for d in decided) >= 5, decided
    rows = [_objs8(s) for s in sets]
    got = ops.objs_iou_batch(rows)
    assert len(got) == len(sets)
    for k, (g, w, s) in enumerate(zip(got, want, sets)):
        assert g.shape == w.shape == (len(s), len(s)) and g.dtype == np.float32
        assert _same(g, w), (k, len(s), _describe(g, w, s, s))
    for k in (0, 2, 6, 9, 10):      # the single-set entry point: the same matrices
        assert _same(ops.objs_iou(rows[k]), want[k]), k


# --------------------------------------------------------------------------------------- b. pair kernels, exact geometry
@pytest.mark.parametrize("centre", ic.CENTRES, ids=str)
def test_pair_kernels_against_exact_geometry(gpu, centre):
    """500 x 500 random detector-shaped pairs within 6 m of (0, 0), (70, 40), (-75, 75), (150, -150) against exact
    clipping (tests/rect_exact.py), on the pairs well-conditioned at 0.02 m:
        |overlap - exact| <= (P_a + P_b) * ulp32(R),   |iou - exact| <= 2 * that / (area_a + area_b - exact) + 1e-6
    (derivation: tests/iou3d_cases.py; the reference's own arithmetic reaches 0.255-0.350 of the first).  That at least 95 %
    of the pairs are well-conditioned and 10 000 of those overlap is asserted from the exact geometry."""
    from modest_amd import ops
    A, B = ic.random_sets(centre)
    e = ic.exact(centre)
    e.check_conditions()
    a, b = _dev(A, gpu), _dev(B, gpu)
    iou = ops.boxes_iou_bev(a, b).cpu().numpy()
    ov = ops.boxes_iou_bev(a, b, overlap_only=True).cpu().numpy()
    assert np.isfinite(iou).all() and np.isfinite(ov).all()
    s_ov, s_iou = e.shares(ov, iou)
    print(f"{centre}: share of the bound {s_ov:.3f} overlap, {s_iou:.3f} IoU")
    assert s_ov <= 1, s_ov
    assert s_iou <= 1, s_iou


# --------------------------------------------------------------------------------------- c. boxes_iou3d_gpu
def test_boxes_iou3d_height_cases_at_range(gpu):
    """boxes_iou3d_gpu on (128, 50) boxes near (70, 35) against iou3d_nms_utils.py:54-87 restated in NumPy float32 on the
    twin's BEV overlap, to 2 ulp of the value.  z and dz are dyadic, so among the pairs that overlap in BEV the height
    ranges overlap, touch exactly (top - bot == 0: IoU exactly 0), lie apart, and some boxes have dz = 0."""
    from modest_amd.utils.iou3d_nms import iou3d_nms_utils as iu
    fam = ic.families(70.0)
    A, B = fam["turned by 0.1"][0][:128].copy(), fam["half size turned by 0.4"][1][:50].copy()
    rng = np.random.default_rng(31)
    for X in (A, B):
        X[:, 2] = rng.choice(np.array([-1, -0.5, 0, 0.5, 1, 1.5], np.float32), len(X))
        X[:, 5] = rng.choice(np.array([0, 0.5, 1, 1, 2, 2], np.float32), len(X))
    f = np.float32
    top = np.minimum((A[:, 2] + A[:, 5] / f(2))[:, None], (B[:, 2] + B[:, 5] / f(2))[None, :])
    bot = np.maximum((A[:, 2] - A[:, 5] / f(2))[:, None], (B[:, 2] - B[:, 5] / f(2))[None, :])
    ov = ol.boxes_iou_bev(A, B, overlap_only=True, arith="f64")
    h = top - bot
    in_bev = ov > 0
    assert (in_bev & (h > 0)).sum() >= 100 and (in_bev & (h == 0)).sum() >= 20 and (in_bev & (h < 0)).sum() >= 20
    assert (in_bev & (A[:, 5] == 0)[:, None]).sum() >= 20 and (in_bev & (B[:, 5] == 0)[None, :]).sum() >= 20
    inter = ov * np.maximum(h, f(0))
    vol = (A[:, 3] * A[:, 4] * A[:, 5])[:, None] + (B[:, 3] * B[:, 4] * B[:, 5])[None, :]
    want = inter / np.maximum(vol - inter, f(1e-6))
    assert want.dtype == np.float32 and np.isfinite(want).all() and (want > 0.01).sum() >= 100
    got = iu.boxes_iou3d_gpu(_dev(A, gpu), _dev(B, gpu)).cpu().numpy()
    assert got.shape == (128, 50)
    assert np.all(got[in_bev & (h <= 0)] == 0)
    assert np.all(np.abs(got.astype(np.float64) - want) <= 2 * np.spacing(np.abs(want)).astype(np.float64))


# --------------------------------------------------------------------------------------- d. NMS, keep lists in score order
def _nms_expect(boxes, scores_dev, thresh, rotated, pre_maxsize=None):
    """order[oracle keep]: the order is torch's own descending sort of the device scores (the wrapper's; it is not
    stable, so NumPy's argsort would not do on ties), the greedy walk the twin's (rotated) or the glibc oracle's
    (axis-aligned: no trig)"""
    order = scores_dev.sort(0, descending=True)[1].cpu().numpy()
    if pre_maxsize is not None:
        order = order[:pre_maxsize]
    pos = ol.nms(boxes[order], thresh, rotated=rotated, arith="f64" if rotated else "glibc")
    return order[pos], len(order)


def _nms_both(gpu, boxes, scores, thresh, min_each=0):
    from modest_amd.utils.iou3d_nms import iou3d_nms_utils as iu
    b, sc = _dev(boxes, gpu), _dev(scores, gpu)
    for rotated, fn in ((True, iu.nms_gpu), (False, iu.nms_normal_gpu)):
        want, n = _nms_expect(boxes, sc, thresh, rotated)
        assert min_each <= len(want) <= n - min_each, (rotated, thresh, len(want))
        keep, extra = fn(b, sc, thresh)
        assert extra is None and str(keep.dtype) == "torch.int64"
        assert np.array_equal(keep.cpu().numpy(), want), (rotated, thresh, len(boxes), len(want), len(keep))


@pytest.mark.parametrize("thresh", ic.THRESHOLDS)
@pytest.mark.parametrize("offset", ic.NMS_OFFSETS)
def test_nms_on_detector_like_proposals(gpu, offset, thresh):
    """nms_gpu / nms_normal_gpu on 4 608 clustered proposals (96 jittered copies of 48 objects, a fifth turned by pi,
    exact duplicates) around x = 0 and x = 60 m at thresholds 0.01 to 0.85: the keep list equals order[oracle keep] in
    score order, with at least 20 kept and 20 suppressed (the oracle keeps 44 to 2 434)."""
    p, sc = ic.proposals(offset)
    _nms_both(gpu, p, sc, thresh, min_each=20)


@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 127, 128, 129, 1000))
def test_nms_at_tile_edges(gpu, n):
    """the first n proposals at thresholds 0.1 and 0.7: one box, one tile short of / exactly / one past full (the diagonal
    tile's lane + 1 start, a last column block of 63 and of 1), two row blocks and a grid of 16 x 16 tiles"""
    for offset in ic.NMS_OFFSETS:
        p, sc = ic.proposals(offset)
        for thresh in (0.1, 0.7):
            _nms_both(gpu, p[:n].copy(), sc[:n].copy(), thresh)


@pytest.mark.parametrize("pre_maxsize", (1, 64, 100))
def test_nms_pre_maxsize(gpu, pre_maxsize):
    from modest_amd.utils.iou3d_nms import iou3d_nms_utils as iu
    p, sc = ic.proposals(60.0)
    b, s = _dev(p, gpu), _dev(sc, gpu)
    for thresh in (0.1, 0.7):
        want, n = _nms_expect(p, s, thresh, True, pre_maxsize)
        assert n == pre_maxsize
        keep, _ = iu.nms_gpu(b, s, thresh, pre_maxsize=pre_maxsize)
        assert np.array_equal(keep.cpu().numpy(), want), (pre_maxsize, thresh)


def test_nms_with_equal_scores(gpu):
    """every score 0.5: the order is whatever torch's sort of the device tensor makes of the ties, and the keep list
    follows it"""
    p, _ = ic.proposals(0.0)
    sc = np.full(len(p), 0.5, np.float32)
    for thresh in (0.1, 0.7):
        _nms_both(gpu, p, sc, thresh, min_each=20)


def test_nms_reuses_a_context_without_stale_words(gpu):
    """ops.nms on ONE explicit context with n = 4 608, 129, 65, 1 and 4 608 again, rotated and axis-aligned: the
    suppression words in the context's arena are never cleared, so a tile that failed to write its word would read the
    previous call's.  Each keep equals the oracle's; the last equals the first."""
    from modest_amd import _lib, ops
    p, sc = ic.proposals(60.0)
    ps = p[np.argsort(-sc, kind="stable")]
    ctx = _lib.Context(gpu.index or 0)
    try:
        for rotated in (True, False):
            got = []
            for n in (4608, 129, 65, 1, 4608):
                keep = ops.nms(_dev(ps[:n], gpu), 0.7, rotated=rotated, ctx=ctx)
                want = ol.nms(ps[:n], 0.7, rotated=rotated, arith="f64" if rotated else "glibc")
                assert keep.dtype == np.int64 and np.array_equal(keep, want), (rotated, n, len(keep), len(want))
                got.append(keep.copy())
            assert np.array_equal(got[0], got[-1])
    finally:
        ctx.close()


def test_nms_of_nothing(gpu):
    import torch
    from modest_amd import ops
    from modest_amd.utils.iou3d_nms import iou3d_nms_utils as iu
    none = torch.zeros((0, 7), dtype=torch.float32, device=gpu)
    for rotated in (True, False):
        keep = ops.nms(none, 0.1, rotated=rotated)
        assert keep.shape == (0,) and keep.dtype == np.int64
    for fn in (iu.nms_gpu, iu.nms_normal_gpu):
        keep, _ = fn(none, torch.zeros(0, dtype=torch.float32, device=gpu), 0.1)
        assert tuple(keep.shape) == (0,) and keep.dtype == torch.int64


def test_nms_on_a_side_stream(gpu):
    import torch
    from modest_amd.utils.iou3d_nms import iou3d_nms_utils as iu
    p, sc = ic.proposals(0.0)
    b, s = _dev(p[:1000], gpu), _dev(sc[:1000], gpu)
    main = [fn(b, s, 0.7)[0].cpu().numpy() for fn in (iu.nms_gpu, iu.nms_normal_gpu)]
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        other = [fn(b, s, 0.7)[0] for fn in (iu.nms_gpu, iu.nms_normal_gpu)]
    side.synchronize()
    for m, o, rotated in zip(main, other, (True, False)):
        assert np.array_equal(m, o.cpu().numpy())
        assert np.array_equal(m, _nms_expect(p[:1000], s, 0.7, rotated)[0])


# --------------------------------------------------------------------------------------- e. wrapper errors
def test_wrapper_errors_leave_the_next_call_right(gpu):
    """iou3d_nms_cuda raises RuntimeError where the reference prints and exits: non-contiguous boxes to nms_gpu, float64
    boxes to boxes_iou_bev_gpu, a device keep tensor.  The next valid calls in the same process are right."""
    import torch
    from modest_amd.utils.iou3d_nms import iou3d_nms_cuda as ext
    p, sc = ic.proposals(0.0)
    ps = p[np.argsort(-sc, kind="stable")][:200]
    b = _dev(ps, gpu)
    keep = torch.zeros(200, dtype=torch.int64)
    wide = torch.zeros((200, 14), dtype=torch.float32, device=gpu)
    with pytest.raises(RuntimeError):
        ext.nms_gpu(wide[:, :7], keep, 0.7)
    with pytest.raises(RuntimeError):
        ext.nms_normal_gpu(wide[:, ::2], keep, 0.7)
    with pytest.raises(RuntimeError):
        ext.nms_gpu(b, keep.to(gpu), 0.7)
    out = torch.zeros((200, 200), dtype=torch.float32, device=gpu)
    with pytest.raises(RuntimeError):
        ext.boxes_iou_bev_gpu(b.double(), b, out)
    with pytest.raises(RuntimeError):
        ext.boxes_overlap_bev_gpu(b, b, out.double())
    with pytest.raises(RuntimeError):
        ext.boxes_iou_bev_gpu(b.cpu(), b, out)
    n = ext.nms_gpu(b, keep, 0.7)
    want = ol.nms(ps, 0.7, arith="f64")
    assert n == len(want) and np.array_equal(keep[:n].numpy(), want)
    assert ext.boxes_iou_bev_gpu(b, b, out) == 1
    assert _same(out.cpu().numpy(), ol.boxes_iou_bev(ps, ps, arith="f64"))
