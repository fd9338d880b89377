"""Edge cases of the box decoding by name, shared by tests/test_box_decode_cpu.py and
tests/test_gpu_box_decode.py.  CASES: name -> a case of tests/box_decode_seq.py.  Each is small: a few rows that carry the
edge, padded with ordinary rows; the tile cases set the row count instead."""
import numpy as np

import box_decode_seq as seq

F = np.float32
INF, NAN = F(np.inf), F(np.nan)
CASES = {}


def _ulp_steps(x, steps):
    x = F(x)
    for _ in range(abs(steps)):
        x = np.nextafter(x, F(np.inf) if steps > 0 else F(-np.inf), dtype=F)
    return x


def _argmax_rows(n):
    """(8, n) logits: a tie of all, a tie of the last two at the maximum, a NaN first, two NaNs (the first wins), a NaN after
    the maximum, +inf twice, -inf everywhere, -0 against +0"""
    rows = np.zeros((8, n), dtype=F)
    rows[0] = 0.25
    rows[1] = np.linspace(-1, 0, n)
    rows[1, -2:] = 0.5
    rows[2] = 1.0
    rows[2, 0] = NAN
    rows[3] = 1.0
    rows[3, n // 2] = NAN
    rows[3, -1] = NAN
    rows[4] = np.arange(n, 0, -1)
    rows[4, -1] = NAN
    rows[5] = -1.0
    rows[5, max(n - 2, 0)] = INF
    rows[5, -1] = INF
    rows[6] = -INF
    rows[7] = -0.0
    rows[7, -1] = 0.0
    return rows


# ---- argmax: ties, NaN logits (the first NaN wins), all-equal logits -- in the direction bins and in the classes
for bins in (1, 2, 8):
    c = seq.make_anchor(10 + bins, B=1, N=12, bins=bins)
    c["dir"][0, :8] = _argmax_rows(bins)
    CASES[f"anchor_argmax_bins{bins}"] = c
for K in (1, 3, 32):
    c = seq.make_point(20 + K, N=12, K=K)
    c["cls"][:8] = _argmax_rows(K)
    CASES[f"point_argmax_k{K}"] = c


# ---- direction bins: headings at which v / period + dir_limit_offset is an exact integer, and one ulp either side
def _bin_edges(bins, dir_offset, dir_limit_offset):
    c = seq.make_anchor(30 + bins, B=2, N=16, bins=bins, dir_offset=dir_offset, dir_limit_offset=dir_limit_offset)
    period, off, lim = seq.period_of(bins), F(dir_offset), F(dir_limit_offset)
    c["anchors"][:, 6] = 0.0
    row, found = 0, 0
    for m in (-2, -1, 0, 1, 3):
        h = (F(m) - lim) * period + off
        # the nearest heading at which the kernel's own (h - off) / period + lim is the integer m, float32 throughout
        near = [_ulp_steps(h, s) for s in sorted(range(-8, 9), key=abs)]
        exact = [x for x in near if (x - off) / period + lim == F(m)]
        h = exact[0] if exact else h
        found += bool(exact)
        for step in (-1, 0, 1):
            c["box"][0, row, 6] = _ulp_steps(h, step)
            row += 1
    assert found >= 3, (bins, found)         # exact integers are among them
    return c


CASES["anchor_bin_edges_bins2"] = _bin_edges(2, 0.78539, 0.0)
CASES["anchor_bin_edges_bins1"] = _bin_edges(1, 0.0, 0.5)
CASES["anchor_bin_edges_bins8"] = _bin_edges(8, 0.25, 0.5)


# ---- non-finite encodings, degenerate anchors and rois
def _nonfinite(c, box, sizes):
    """rows 0..7 of the (R, code) encodings `box` against the (R, >= 2) anchor sizes (or None)"""
    for row, v in enumerate((INF, -INF, NAN, F(89.0))):          # exp overflows float32 at 89
        box[row, 3] = v
        box[row, 5] = v
    box[4, 0] = INF                                                # xt = inf with diagonal 0: 0 * inf
    box[5, 1] = -INF
    box[6, 2] = INF                                                # zg infinite
    box[7, 0:3] = [NAN, INF, -INF]
    if sizes is not None:
        sizes[4:6, 0:2] = 0.0                                      # dx = dy = 0
        sizes[8, 0:2] = 0.0                                        # ... with finite encodings
        sizes[9, 0:3] = [0.0, 0.0, -1.0]
    return c


c = seq.make_anchor(40, B=2, N=12, bins=2)
CASES["anchor_nonfinite"] = _nonfinite(c, c["box"][1], c["anchors"][:, 3:6])
c = seq.make_anchor(41, B=1, N=12, bins=2, sincos=True)
CASES["anchor_sincos_nonfinite"] = _nonfinite(c, c["box"][0], c["anchors"][:, 3:6])
c = seq.make_point(42, N=12, K=1)
CASES["point_nonfinite"] = _nonfinite(c, c["box"], None)
c["mean"][0, 0:2] = 0.0                                            # K = 1: every row meets the diagonal of 0
c = seq.make_point(43, N=12, K=3, mean=False)
CASES["point_no_mean_nonfinite"] = _nonfinite(c, c["box"], None)
c = seq.make_roi(44, B=1, M=12)
CASES["roi_nonfinite"] = _nonfinite(c, c["box"], c["rois"][0, :, 3:6])

# ---- angles: atan2(+-0, +-0), atan2(-0., -1), and the sincos coder with cost + cos ra = sint + sin ra = 0
ZEROS = [(0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0), (-0.0, -1.0), (0.0, -1.0), (1.0, 0.0), (-1.0, -0.0)]   # (sint, cost)
c = seq.make_point(50, N=10, K=3)
for row, (s, co) in enumerate(ZEROS):
    c["box"][row, 6], c["box"][row, 7] = co, s
CASES["point_atan2_zeros"] = c
c = seq.make_anchor(51, B=1, N=12, bins=0, sincos=True)
c["anchors"][:8, 6] = 0.0                                          # cos ra = 1, sin ra = 0
c["anchors"][[1, 3, 4], 6] = -0.0                                  # ... sin ra = -0, so that sint = -0 stays -0
for row, (s, co) in enumerate(ZEROS):
    c["box"][0, row, 6], c["box"][0, row, 7] = F(co) - F(1.0), s
for row, ra in ((8, 0.5), (9, 2.5), (10, -1.25)):                  # the sums cancel exactly: atan2(0, 0)
    c["anchors"][row, 6] = ra
    c["box"][0, row, 6] = -seq.f32_of_double(np.cos, F(ra))
    c["box"][0, row, 7] = -seq.f32_of_double(np.sin, F(ra))
CASES["anchor_sincos_zeros"] = c
c = dict(c, dir=np.random.RandomState(52).normal(0, 1, (1, 12, 2)).astype(F))
CASES["anchor_sincos_zeros_dir"] = c

# ---- RoI inputs: zg infinite (above), the roi heading at +-pi and 1e8
c = seq.make_roi(60, B=2, M=6)
c["rois"][0, :, 6] = [np.pi, -np.pi, 1e8, -1e8, 0.0, -0.0]
c["rois"][1, :3, 6] = [np.pi / 2, 3e4, 1e-30]
CASES["roi_headings"] = c

# ---- layout: C = 0, 2 and 9 extra columns, the non-contiguous points view (every point case), no mean size, B = 1
for extra in (0, 2, 9):
    CASES[f"anchor_extra{extra}"] = seq.make_anchor(70 + extra, B=1, N=70, extra=extra, bins=2)
    CASES[f"roi_extra{extra}"] = seq.make_roi(80 + extra, B=1, M=70, extra=extra)
for extra in (0, 2, 8):                                            # 8 + 8 = the code limit of 16
    CASES[f"point_extra{extra}"] = seq.make_point(90 + extra, N=70, K=3, extra=extra)
CASES["anchor_sincos_extra8"] = seq.make_anchor(78, B=2, N=70, extra=8, bins=2, sincos=True)      # code 16 in, 15 out
CASES["anchor_no_dir"] = seq.make_anchor(79, B=3, N=70, bins=0)
CASES["point_no_mean"] = seq.make_point(99, N=70, K=3, mean=False)
CASES["point_k32_extra8"] = seq.make_point(98, N=300, K=32, extra=8)   # the widest tiles the LDS holds

# ---- tile boundaries: every tile tail, the 16-byte and the dword path (code 7: a tile of 63 rows is 441 dwords, no multiple
# of 4, and every tile after the first of 257 rows begins off a 16-byte boundary)
TILE_ROWS = (1, 63, 64, 65, 255, 256, 257, 513)
for n in TILE_ROWS:
    CASES[f"anchor_rows{n}"] = seq.make_anchor(100 + n, B=2, N=n, bins=2)                  # code 7, B = 2: odd tile bases
    CASES[f"anchor_code8_rows{n}"] = seq.make_anchor(200 + n, B=1, N=n, extra=1, bins=2)   # code 8: every tile 16-byte aligned
    CASES[f"point_rows{n}"] = seq.make_point(300 + n, N=n, K=3)                             # 8 in, 7 out
    CASES[f"roi_rows{n}"] = seq.make_roi(400 + n, B=1, M=n)
    CASES[f"roi_code9_rows{n}"] = seq.make_roi(500 + n, B=1, M=n, extra=2)

# ---- one mid-size run per head: more than one tile per workgroup column, not the workload's own size
MID = {"anchor": seq.make_anchor(600, B=2, N=24 * 257, bins=2), "point": seq.make_point(601, N=4 * 1031, K=3),
       "roi": seq.make_roi(602, B=4, M=100)}
