"""Inputs and yardsticks shared by tests/test_iou3d_oracle_cpu.py and tests/test_gpu_iou3d.py.

Boxes are (n, 7) float32 rows [x, y, z, dx, dy, dz, heading] (modest_amd/csrc/iou3d.hip, oracle/iou3d_oracle.c).

  random_sets(centre)    two sets of 500 detector-shaped boxes (dx 0.5-5, dy 0.4-2.2, heading +-3.2) within +-6 m of centre
  families(offset)       constructed families of 500 rows each against a base set of 500 random boxes: the same rectangle in
                         other parametrisations, contained / turned / shifted / edge-sharing boxes, single shapes, special and
                         large headings, thin, zero-size and negative-extent boxes, disjoint pairs
  proposals(offset)      4 608 detector-like NMS proposals: 96 jittered copies of each of 48 objects, 20 % turned by pi, every
                         17th an exact duplicate, in shuffled order (so that a prefix still holds many objects)
  exact(a, b)            exact geometry of all pairs (tests/rect_exact.py, independent of the reference's polygon walk), the
                         well-conditioned mask at 0.02 m and the derived bounds of the float32 polygon walk

The derived bound.  Every vertex of the clipped polygon is a corner or a crossing of two edges, computed in float32 from
coordinates of magnitude <= R, so it is off by a few ulp32(R) at the most on a well-conditioned pair (no corner within
0.02 m of the other box's boundary: no inside test or crossing test turns on a rounding).  Moving the boundary of the
intersection by e changes its area by at most perimeter * e, and the perimeter of the intersection is at most that of
either box, so
    |overlap - exact| <= (P_a + P_b) * ulp32(R),
which leaves the constant of "a few ulp" to the sum of the two perimeters.  The C restatement of the reference reaches
0.255-0.350 of it (tests/test_iou3d_oracle_cpu.py).  For IoU = o / (S - o), S = area_a + area_b, the derivative in o is
S / (S - o)^2 <= 2 / (S - o) because o <= S / 2, hence
    |iou - iou_exact| <= 2 * overlap_bound / (S - exact) + 1e-6,
the 1e-6 covering the float32 roundings of the two areas, the sum and the division (values <= 1, a few ulp of 6e-8).
"""
import functools
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rect_exact as rx  # noqa: E402
from oracle import labels as ol  # noqa: E402

K = 500
CENTRES = ((0, 0), (70, 40), (-75, 75), (150, -150))
OFFSETS = (0.0, 70.0)                      # families: centres near (offset, offset / 2)
NMS_OFFSETS = (0.0, 60.0)
THRESHOLDS = (0.01, 0.1, 0.5, 0.7, 0.85)
PI = np.float32(np.pi)


def _set(rng, k, cx, cy, spread):
    return np.c_[cx + rng.uniform(-spread, spread, k), cy + rng.uniform(-spread, spread, k), np.zeros(k),
                 rng.uniform(0.5, 5, k), rng.uniform(0.4, 2.2, k), np.ones(k), rng.uniform(-3.2, 3.2, k)].astype(np.float32)


@functools.lru_cache(maxsize=None)
def random_sets(centre):
    rng = np.random.default_rng([5, CENTRES.index(tuple(centre))])
    a, b = _set(rng, K, centre[0], centre[1], 6), _set(rng, K, centre[0], centre[1], 6)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def families(offset):
    """{name: (A, B)}: (500, 7) box sets whose row k of B is built from row k of A; the full A x B matrix holds the
    family on its diagonal and cross pairs everywhere else.  Names starting with 'twin-only' hold zero-size or
    negative-extent rows and never meet exact geometry."""
    rng = np.random.default_rng([1, int(offset)])
    base = lambda: _set(rng, K, offset, offset * 0.5, 5)   # noqa: E731
    a = base()
    fam = {}

    def put(name, A, B):
        A, B = np.ascontiguousarray(A, np.float32), np.ascontiguousarray(B, np.float32)
        assert A.shape == B.shape == (K, 7) and np.isfinite(A).all() and np.isfinite(B).all(), name
        A.setflags(write=False)
        B.setflags(write=False)
        fam[name] = (A, B)

    # the same rectangle
    put("identical", a, a)
    b = a.copy(); b[:, 6] += PI; put("turned by pi", a, b)
    b = a.copy(); b[:, 3], b[:, 4] = a[:, 4], a[:, 3]; b[:, 6] += np.float32(np.pi / 2); put("swapped + pi/2", a, b)
    b = a.copy(); b[:, 6] = a[:, 6] + np.float32(2 * np.pi) * rng.integers(-3, 4, K).astype(np.float32); put("heading + 2 pi k", a, b)
    # contained
    b = a.copy(); b[:, 3:5] *= 0.5; put("concentric half size", a, b)
    b = a.copy(); b[:, 3:5] *= 0.5; b[:, 6] += np.float32(0.4); put("half size turned by 0.4", a, b)
    for eps in (1e-1, 1e-2, 1e-3, 1e-5, 1e-7):
        b = a.copy(); b[:, 6] += np.float32(eps); put(f"turned by {eps:g}", a, b)
    for eps in (1e-2, 1e-3, 1e-5):
        b = a.copy(); b[:, 0] += np.float32(eps); put(f"shifted by {eps:g}", a, b)
    # edge to edge: b displaced along a's own x axis
    c, s = np.cos(a[:, 6].astype(np.float64)), np.sin(a[:, 6].astype(np.float64))
    for gap in (0.0, 0.005, 0.02, -0.005, -0.02):
        b = a.copy(); b[:, 0] = a[:, 0] + (a[:, 3] + gap) * c; b[:, 1] = a[:, 1] + (a[:, 3] + gap) * s
        put("edge sharing" if gap == 0 else f"edge gap {gap:+g}", a, b)
    # single shapes
    b = a.copy(); b[:, 0] = a[:, 0] + a[:, 3] * c - a[:, 4] * s; b[:, 1] = a[:, 1] + a[:, 3] * s + a[:, 4] * c
    put("corner touching", a, b)
    b = a.copy(); b[:, 6] += np.float32(np.pi / 2); put("cross at pi/2", a, b)
    sq = a.copy(); sq[:, 4] = sq[:, 3]; b = sq.copy(); b[:, 6] += np.float32(np.pi / 4); put("squares at pi/4", sq, b)
    # headings
    special = np.array([0, np.pi / 2, -np.pi / 2, np.pi, -np.pi], np.float32)
    ax = a.copy(); ax[:, 6] = rng.choice(special, K)
    b = ax.copy(); b[:, 0] += ax[:, 3] * np.float32(0.25); b[:, 6] = rng.choice(special, K); put("special headings", ax, b)
    big = a.copy(); big[:, 6] = rng.uniform(-100, 100, K)
    b = base(); b[:, :2] = big[:, :2] + rng.uniform(-1, 1, (K, 2)); b[:, 6] = rng.uniform(-100, 100, K)
    put("headings in +-100", big, b)
    # odd sizes
    th = a.copy(); th[:, 4] = rng.choice(np.array([0.005, 0.01, 0.02, 0.05], np.float32), K)
    b = base(); b[:, :2] = th[:, :2] + rng.uniform(-0.5, 0.5, (K, 2)); put("thin against neighbours", th, b)
    z = a.copy(); z[:, 3:5] = 0
    put("twin-only zero size against itself", z, z)
    put("twin-only zero size inside a box", a, z)
    # dx = -0.02: half extent + the 1e-2 margin of the inside test is exactly 0, so only a point exactly on the box's
    # axis (local x == 0) can turn the test, and does so between < and <=.  Heading 0 and dyadic centres: the other box's
    # left edge lies exactly on that axis.
    neg = a.copy(); neg[:, :2] = np.round(neg[:, :2] * 4) / 4; neg[:, 3] = np.float32(-0.02); neg[:, 6] = 0
    b = neg.copy(); b[:, 3] = 1; b[:, 4] = np.float32(0.25); b[:, 0] = neg[:, 0] + np.float32(0.5)
    put("twin-only negative extent on the margin", neg, b)
    # control: b far to the side of a (at least 30 m between centres, boxes at most 5.5 m across): exactly 0, not NaN
    b = base(); b[:, 0] += np.float32(30) + 20 * rng.random(K).astype(np.float32); put("disjoint", a, b)
    return fam


def family_disjoint_is_disjoint(A, B):
    d = np.hypot(A[:, None, 0].astype(np.float64) - B[None, :, 0], A[:, None, 1].astype(np.float64) - B[None, :, 1])
    return bool((d > 12).all())


@functools.lru_cache(maxsize=None)
def proposals(offset):
    """(boxes (4608, 7) float32, scores (4608,) float32)"""
    rng = np.random.default_rng([7, int(offset)])
    nobj, per = 48, 96
    obj = np.c_[offset + rng.uniform(-35, 35, nobj), rng.uniform(-35, 35, nobj), np.zeros(nobj), rng.uniform(3.2, 4.8, nobj),
                rng.uniform(1.5, 2.0, nobj), np.full(nobj, 1.5), rng.uniform(-3.2, 3.2, nobj)]
    p = np.repeat(obj, per, 0)
    n = len(p)
    p[:, :2] += rng.normal(0, 0.25, (n, 2))
    p[:, 3:5] *= rng.normal(1, 0.06, (n, 2))
    p[:, 6] += rng.normal(0, 0.08, n) + np.pi * (rng.random(n) < 0.2)
    dup = np.arange(0, n - 1, 17)
    p[dup] = p[dup + 1]                         # exact duplicates
    p = p[rng.permutation(n)].astype(np.float32)
    sc = rng.random(n).astype(np.float32)
    p.setflags(write=False)
    sc.setflags(write=False)
    return p, sc


# ------------------------------------------------------------------------------------------ oracle, all pairs, threaded
def bev(a, b, overlap_only=False, arith="glibc", threads=8):
    """oracle.labels.boxes_iou_bev over row blocks of a in parallel (ctypes releases the GIL; the C code is pure)"""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    if len(a) < 4 * threads:
        return ol.boxes_iou_bev(a, b, overlap_only, arith=arith)
    ol.boxes_iou_bev(a[:1], b[:1], arith=arith)      # load the library once, outside the pool
    cuts = np.linspace(0, len(a), threads + 1).astype(int)
    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(lambda k: ol.boxes_iou_bev(a[cuts[k]:cuts[k + 1]], b, overlap_only, arith=arith), range(threads)))
    return np.concatenate(parts, 0)


# ------------------------------------------------------------------------------------------ exact geometry
def to_rect(x):
    """(n, 7) boxes -> rect_exact's (cx, cy, l, w, ry): its ry turns the other way"""
    x = np.asarray(x)
    return np.c_[x[:, 0], x[:, 1], x[:, 3], x[:, 4], -x[:, 6].astype(np.float64)]


def ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


class Exact:
    """exact overlap and IoU of the pairs (a[k], b[k]), the well-conditioned mask and the two derived bounds"""

    def __init__(self, a, b, margin=0.02, shape=None):
        A, B = to_rect(a), to_rect(b)
        sh = shape or (len(A),)
        self.overlap = rx.inter_area(A, B).reshape(sh)
        self.union = (rx.box_area(A) + rx.box_area(B)).reshape(sh) - self.overlap
        self.iou = self.overlap / self.union
        self.well = rx.well_conditioned(A, B, margin).reshape(sh)
        R = np.maximum(np.abs(rx.corners(A)).max((1, 2)), np.abs(rx.corners(B)).max((1, 2)))
        P = 2 * (A[:, 2] + A[:, 3] + B[:, 2] + B[:, 3])
        self.overlap_bound = (P * ulp32(R)).reshape(sh)
        self.iou_bound = 2 * self.overlap_bound / self.union + 1e-6

    @classmethod
    def all_pairs(cls, a, b, margin=0.02):
        """every pair of a x b, (na, nb) each.  Pairs whose circumscribed circles lie more than 2 * margin apart are
        disjoint and well-conditioned by that alone and skip the clipping (their bounds are computed as for the rest)."""
        a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
        d = np.hypot(a64[:, None, 0] - b64[None, :, 0], a64[:, None, 1] - b64[None, :, 1])
        near = d <= (np.hypot(a64[:, 3], a64[:, 4]) / 2)[:, None] + (np.hypot(b64[:, 3], b64[:, 4]) / 2)[None, :] + 2 * margin
        i, j = np.nonzero(near)
        e = cls(a[i], b[j], margin)
        A, B = to_rect(a), to_rect(b)
        full = cls.__new__(cls)
        sh = near.shape
        full.overlap = np.zeros(sh)
        full.overlap[i, j] = e.overlap
        full.union = rx.box_area(A)[:, None] + rx.box_area(B)[None, :] - full.overlap
        full.iou = full.overlap / full.union
        full.well = np.ones(sh, bool)
        full.well[i, j] = e.well
        R = np.maximum(np.abs(rx.corners(A)).max((1, 2))[:, None], np.abs(rx.corners(B)).max((1, 2))[None, :])
        P = 2 * ((A[:, 2] + A[:, 3])[:, None] + (B[:, 2] + B[:, 3])[None, :])
        full.overlap_bound = P * ulp32(R)
        full.iou_bound = 2 * full.overlap_bound / full.union + 1e-6
        return full

    def check_conditions(self):
        """the inputs keep the comparison meaningful: asserted from the exact geometry alone"""
        assert self.well.mean() >= 0.95, self.well.mean()
        assert int((self.well & (self.overlap > 0)).sum()) >= 10000

    def shares(self, overlap, iou):
        """largest |error| / bound over the well-conditioned pairs, for overlap and IoU"""
        w = self.well
        so = np.abs(overlap.astype(np.float64) - self.overlap)[w] / self.overlap_bound[w]
        si = np.abs(iou.astype(np.float64) - self.iou)[w] / self.iou_bound[w]
        return float(so.max()), float(si.max())


@functools.lru_cache(maxsize=None)
def exact(centre):
    return Exact.all_pairs(*random_sets(centre))
