"""CPU: the f64 twin of the BEV IoU oracle (oracle/iou3d_oracle.c built with -DMODEST_ORACLE_TRIG_F64) tied to what the
project already trusts -- the glibc build of the same file (== the reference's iou3d_cpu.cpp, test_oracle_mask.py) and the
exact geometry of tests/rect_exact.py -- on the very inputs tests/test_gpu_iou3d.py feeds the kernels (tests/iou3d_cases.py).

The twin is the yardstick of the kernels that evaluate their trig on the device ((float)cos((double)h), trig_f32.h): it is
the glibc build with the three libm calls replaced, so the kernels are compared with it bit for bit.  The glibc build
remains the yardstick of the host-trig kernels.  Both builds are held to the derived bound of iou3d_cases.py against exact
geometry, which proves that the GPU tests' inputs keep the reference's own arithmetic inside every cap they assert.
"""
import numpy as np
import pytest

import iou3d_cases as ic
from oracle import labels as ol


def _both(a, b, arith):
    return ic.bev(a, b, True, arith), ic.bev(a, b, False, arith)


def test_twin_against_glibc_oracle_near_the_origin():
    """Random detector-shaped pairs within +-6 m of the origin (500 x 500): the twin stays within the project's tolerances
    of the glibc oracle, 2e-6 IoU and 2e-5 overlap, and is no copy of it.  Measured: 500 of 250 000 IoUs differ, by at
    most 2.1e-7 IoU and 9.5e-7 overlap."""
    a, b = ic.random_sets((0, 0))
    (og, ig), (od, id_) = _both(a, b, "glibc"), _both(a, b, "f64")
    assert np.isfinite(ig).all() and np.isfinite(id_).all()
    assert np.abs(ig - id_).max() <= 2e-6
    assert np.abs(og - od).max() <= 2e-5
    assert (ig != id_).any() and (og != od).any()


def test_twin_against_glibc_oracle_at_range():
    """The constructed families at centres near (70, 35): the two builds differ on few pairs, by MORE than the near-origin
    tolerances of 2e-6 IoU / 2e-5 overlap, so the glibc oracle cannot judge a device-trig kernel at detector range at
    those tolerances.  This documents that; it sets no tolerance for the kernel, which is compared with the twin bit for
    bit.  Asserted: on well-conditioned pairs every difference stays within the derived exact-geometry bound.

    Measured over the 29 families x 250 000 pairs (largest differences, all pairs; pairs that differ):
        turned by 0.1            1.2e-5 IoU   1.2e-5 overlap     48
        turned by 0.01           5.3e-6 IoU   2.8e-5 overlap     79
        headings in +-100        5.1e-6 IoU   2.9e-5 overlap    106
        heading + 2 pi k         4.7e-6 IoU   7.4e-6 overlap     48
        shifted by 1e-05         4.4e-6 IoU   6.7e-6 overlap      8
        swapped + pi/2           3.2e-6 IoU   2.5e-5 overlap     36
        half size turned by 0.4  2.9e-6 IoU   1.2e-5 overlap     21
    and none at all on 16 of the families (identical, concentric, edge sharing, ...)."""
    worst_iou = worst_ov = 0.0
    rows_a, rows_b, d_ov, d_iou = [], [], [], []
    for name, (A, B) in ic.families(70.0).items():
        (og, ig), (od, id_) = _both(A, B, "glibc"), _both(A, B, "f64")
        assert not np.isnan(ig).any() and not np.isnan(id_).any(), name
        i, j = np.nonzero((og != od) | (ig != id_))
        if name.startswith("twin-only"):
            assert len(i) == 0, name       # zero extents / axis-aligned rows: no trig rounding to differ by
            continue
        worst_iou = max(worst_iou, float(np.abs(ig - id_).max()))
        worst_ov = max(worst_ov, float(np.abs(og - od).max()))
        rows_a.append(A[i]); rows_b.append(B[j])
        d_ov.append(np.abs(og[i, j].astype(np.float64) - od[i, j])); d_iou.append(np.abs(ig[i, j].astype(np.float64) - id_[i, j]))
    print(f"largest twin-vs-glibc difference at range: {worst_iou:.3g} IoU, {worst_ov:.3g} overlap")
    e = ic.Exact(np.concatenate(rows_a), np.concatenate(rows_b))      # the pairs that differ; the rest differ by 0
    d_ov, d_iou = np.concatenate(d_ov), np.concatenate(d_iou)
    assert np.all(d_ov[e.well] <= e.overlap_bound[e.well])
    assert np.all(d_iou[e.well] <= e.iou_bound[e.well])


@pytest.mark.parametrize("centre", ic.CENTRES, ids=str)
def test_both_builds_against_exact_geometry(centre):
    """500 x 500 random pairs at each centre against rect_exact (exact clipping, independent of the reference's polygon
    walk), on the pairs well-conditioned at 0.02 m:
        |overlap - exact| <= (P_a + P_b) * ulp32(R)                      (derivation: tests/iou3d_cases.py)
        |iou - exact|     <= 2 * that / (area_a + area_b - exact) + 1e-6.
    At least 95 % of the pairs are well-conditioned and at least 10 000 of those overlap.

    Measured, both builds alike (share of the overlap bound / of the IoU bound; largest overlap error; well-conditioned;
    overlapping among them):
        (0, 0)        0.350 / 0.141   4.0e-6 m^2   98.68 %   20 808
        (70, 40)      0.255 / 0.173   4.1e-5 m^2   98.66 %   22 283
        (-75, 75)     0.331 / 0.257   5.8e-5 m^2   98.63 %   21 990
        (150, -150)   0.336 / 0.222   1.2e-4 m^2   98.70 %   22 017
    On ill-conditioned pairs the reference's 1e-2 m margin puts it off by up to 0.014 m^2: those belong to the twin
    comparison, not to this one."""
    a, b = ic.random_sets(centre)
    e = ic.exact(centre)
    e.check_conditions()
    for arith in ("glibc", "f64"):
        ov, iou = _both(a, b, arith)
        s_ov, s_iou = e.shares(ov, iou)
        print(f"{centre} {arith}: share of the bound {s_ov:.3f} overlap, {s_iou:.3f} IoU")
        assert s_ov <= 1 and s_iou <= 1, (arith, s_ov, s_iou)


def test_reference_blow_up_on_coincident_edges_is_kept():
    """A box against the same rectangle written with dx / dy swapped and heading + float32(pi / 2), near the origin: the
    reference's segment intersection divides by D ~ 0 on the near-parallel coincident edges and returns overlaps wrong by
    metres and IoUs far above 1 (measured: up to 1.77e9 here).  That is the contract -- the reference does it -- so both
    builds reproduce it, agree with each other within the near-origin tolerances, and equal the reference's own
    iou3d_cpu.cpp where oracle/_ref is built."""
    A, B = ic.families(0.0)["swapped + pi/2"]
    k = np.arange(ic.K)
    a, b = A, B
    assert np.allclose(ic.Exact(a, b).iou, 1, atol=1e-5)       # geometrically the same rectangle, pair by pair
    ig, id_ = ic.bev(a, b, False, "glibc"), ic.bev(a, b, False, "f64")
    assert (ig[k, k] > 2).any() and (id_[k, k] > 2).any()
    assert np.array_equal(ig > 2, id_ > 2)
    sane = ig <= 2
    assert np.abs(ig - id_)[sane].max() <= 2e-6
    sel = np.r_[np.nonzero(ig[k, k] > 2)[0], k[:100]]      # the pairs that blow up, and a hundred more rows
    ref = ol.boxes_iou_bev_reference(a[sel].copy(), b[sel].copy())
    if ref is not None:                              # oracle/_ref is built only where the reference checkout is present
        assert (ref > 2).any()
        assert np.array_equal(ref, ig[np.ix_(sel, sel)])


@pytest.mark.parametrize("offset", ic.NMS_OFFSETS)
def test_detector_like_nms_on_the_oracle(offset):
    """4 608 clustered proposals (tests/iou3d_cases.py) through the oracle's greedy NMS: at every threshold at least 20 are
    kept and at least 20 suppressed, so the GPU comparison of keep lists decides something, and the greedy walk equals
    the definition on the full IoU matrix (of the first 1 000).  Kept, twin (rotated) / glibc (axis-aligned), at thresholds 0.01 / 0.1 / 0.5 /
    0.7 / 0.85:
        offset 0     44 / 47 / 137 / 466 / 2 415  rotated      44 / 48 / 131 / 381 / 1 643  axis-aligned
        offset 60    47 / 48 / 132 / 468 / 2 434  rotated      44 / 49 / 129 / 386 / 1 706  axis-aligned
    The glibc build keeps the same rotated lists on this input (luck, not a guarantee)."""
    p, sc = ic.proposals(offset)
    ps = p[np.argsort(-sc, kind="stable")]
    m = 1000
    iou = ic.bev(ps[:m], ps[:m], False, "f64")
    for t in ic.THRESHOLDS:
        for rotated, arith in ((True, "f64"), (False, "glibc")):
            keep = ol.nms(ps, t, rotated=rotated, arith=arith)
            assert 20 <= len(keep) <= len(ps) - 20, (t, rotated, len(keep))
            assert np.all(np.diff(keep) > 0)
        want, gone = [], np.zeros(len(ps), bool)      # src/iou3d_nms.cpp:116-135 on the full matrix
        for i in range(m):
            if not gone[i]:
                want.append(i)
                gone[i + 1:m] |= iou[i, i + 1:] > np.float32(t)
        assert np.array_equal(ol.nms(ps[:m], t, arith="f64"), want), t


def test_arith_argument():
    a, _ = ic.random_sets((0, 0))
    assert np.array_equal(ol.boxes_iou_bev(a[:5], a[:7]), ol.boxes_iou_bev(a[:5], a[:7], arith="glibc"))
    with pytest.raises(ValueError):
        ol.boxes_iou_bev(a[:5], a[:7], arith="f32")
