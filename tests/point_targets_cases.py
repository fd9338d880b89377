"""Inputs for the point-head target tests past the kernel's constants and on its edges (not a test module;
tests/test_point_targets_cpu.py checks on the CPU that every case holds the edge it is named after,
tests/test_gpu_point_targets.py runs them on the device against tests/point_targets_seq.py).

A case is a dict: points (N, 4), gt and ext (B, M, 8), num_class, mean (n_cls, 3) or None, want_box, want_part, and
``present``: a function of the case that says, from the inputs alone (through the restatement), whether the edge is there.
The cases of CASES keep B <= 3, N <= ~1500 and M <= one tile + 1; those of PAST go on from there: up to 40 samples, four
tiles and 20 100 points, where the kernel's tile loop and round loop repeat.  ``past(name)`` builds a PAST case once
per process and hands out the same dict (nobody writes into it).
"""
import functools
import os
import re

import numpy as np

import point_targets_seq as seq
import roipool_seq

F = np.float32
KITTI = np.array([[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]], dtype=F)


def kernel_constants():
    """(lanes per workgroup, boxes per LDS tile) as csrc/point_targets.hip states them"""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "modest_amd", "csrc",
                            "point_targets.hip")).read()
    return tuple(int(re.search(r"constexpr int %s = (\d+);" % n, src).group(1)) for n in ("PT_T", "PT_TILE"))


WG, TILE = kernel_constants()


def case(points, gt, present, ext=None, num_class=3, mean=KITTI, want_box=True, want_part=True):
    gt = np.ascontiguousarray(gt, dtype=F)
    return dict(points=np.ascontiguousarray(points, dtype=F).reshape(-1, 4), gt=gt,
                ext=seq.enlarge(gt) if ext is None else np.ascontiguousarray(ext, dtype=F), num_class=num_class, mean=mean,
                want_box=want_box, want_part=want_part, present=present)


def run(c):
    return seq.assign(c["points"], c["gt"], c["ext"], c["num_class"], c["mean"], c["want_box"], c["want_part"])


def state(c):
    """(k, idx, ext hit, labels) of the case by the restatement"""
    k, idx, hit = seq.membership(c["points"], c["gt"], c["ext"])
    return k, idx, hit, run(c)["point_cls_labels"]


def local_to_world(g, u):
    """u (n, 3) in units of the box's sizes, box frame -> (n, 3) world"""
    c, s = np.cos(np.float64(g[6])), np.sin(np.float64(g[6]))
    x, y, z = u[:, 0] * g[3], u[:, 1] * g[4], u[:, 2] * g[5]
    return np.stack([g[0] + x * c - y * s, g[1] + x * s + y * c, g[2] + z], axis=1)


def random_scene(seed, B, M, N, live=None, shuffle=False):
    """B samples of live[b] random boxes (classes 1..3) and zero rows, N points grouped by sample (or shuffled): most near
    a box of their sample (inside, in the enlarged margin, just outside), the rest anywhere"""
    rs = np.random.RandomState(seed)
    live = [max(M - 2, 0)] * B if live is None else live
    gt = np.zeros((B, M, 8), dtype=F)
    for b in range(B):
        for j in range(live[b]):
            gt[b, j] = [rs.uniform(-40, 40), rs.uniform(-40, 40), rs.uniform(-1, 1), rs.uniform(2, 5), rs.uniform(1, 2.5),
                        rs.uniform(1, 2), rs.uniform(-3.3, 3.3), rs.randint(1, 4)]
    pts = np.zeros((N, 4), dtype=F)
    for i in range(N):
        b = min(i * B // max(N, 1), B - 1) if B else 0
        pts[i, 0] = b
        if B and live[b] and rs.rand() < 0.7:
            g = gt[b, rs.randint(live[b])]
            pts[i, 1:] = local_to_world(g, rs.uniform(-0.62, 0.62, (1, 3)))[0]
        else:
            pts[i, 1:] = [rs.uniform(-45, 45), rs.uniform(-45, 45), rs.uniform(-2, 2)]
    if shuffle:
        pts = pts[rs.permutation(N)]
    return pts, gt


def inside_point(gt, b, j, u=(0.1, -0.2, 0.15)):
    return [b, *local_to_world(gt[b, j], np.array([u]))[0]]


# ---------------------------------------------------------------------------------------------------------- the cases
def n_points(n):
    pts, gt = random_scene(100 + n, 2, 5, n)
    pts[0] = inside_point(gt, int(pts[0, 0]), 0)
    pts[-1] = inside_point(gt, int(pts[-1, 0]), 1)      # the last lane (of the last workgroup) has work to show

    def present(c):
        _, idx, _, _ = state(c)
        return len(c["points"]) == n and idx[0] >= 0 and idx[-1] >= 0
    return case(pts, gt, present)


def no_points():
    _, gt = random_scene(7, 2, 5, 0)
    return case(np.zeros((0, 4), dtype=F), gt, lambda c: len(c["points"]) == 0 and c["gt"].shape[1] > 0)


def no_boxes():
    pts, _ = random_scene(8, 2, 5, 100)
    return case(pts, np.zeros((2, 0, 8), dtype=F), lambda c: c["gt"].shape == (2, 0, 8) and len(c["points"]) == 100)


def no_samples():
    pts, _ = random_scene(9, 2, 5, 70)
    return case(pts, np.zeros((0, 5, 8), dtype=F), lambda c: c["gt"].shape[0] == 0 and (state(c)[0] == -1).all())


def shuffled():
    pts, gt = random_scene(10, 3, 9, 1000, shuffle=True)

    def present(c):
        k, idx, _, _ = state(c)
        mixed = [len(set(k[i:i + 64])) for i in range(0, len(k), 64)]
        fg_samples = set(k[idx >= 0])
        return min(mixed) >= 2 and max(mixed) == 3 and fg_samples == {0, 1, 2}
    return case(pts, gt, present)


def stray_samples():
    pts, gt = random_scene(11, 2, 6, 300)
    where = inside_point(gt, 0, 0)[1:]
    strays = [[-1, *where], [2, *where], [0.5, *where], [np.nan, *where], [-0.0, *where]]
    pts = np.concatenate([pts[:100], np.array(strays, dtype=F), pts[100:]])

    def present(c):
        k, idx, _, lab = state(c)
        p = c["points"]
        at = {v: np.flatnonzero(p[:, 0] == F(v)) for v in (-1, 2, 0.5)}
        would = roipool_seq.inside_mask(p[:, 1:4], c["gt"][0, :, :7]).any(axis=0)
        return (c["gt"].shape[0] == 2 and all(len(i) == 1 and would[i[0]] and k[i[0]] == -1 and lab[i[0]] == 0 for i in at.values())
                and bool(np.isnan(p[:, 0]).any()) and k[104] == 0 and idx[104] == 0 and np.signbit(p[104, 0]))
    return case(pts, gt, present)


def overlapping():
    pts, gt = random_scene(12, 2, 6, 200)
    gt[1, 3] = gt[1, 1]
    gt[1, 3, 3:6] += F(0.5)                  # row 3 encloses row 1: the lower index wins
    gt[1, 3, 7] = 1 + gt[1, 1, 7] % 3
    pts[150:160] = [inside_point(gt, 1, 1, u) for u in np.random.RandomState(1).uniform(-0.45, 0.45, (10, 3))]

    def present(c):
        k, idx, _, lab = state(c)
        sel = np.flatnonzero(k == 1)
        m = roipool_seq.inside_mask(c["points"][sel, 1:4], c["gt"][1, :, :7])
        both = sel[m[1] & m[3]]
        return len(both) >= 10 and (idx[both] == 1).all() and (lab[both] == int(c["gt"][1, 1, 7])).all() \
            and c["gt"][1, 1, 7] != c["gt"][1, 3, 7]
    return case(pts, gt, present)


def last_row_past_the_tile():
    M = TILE + 1
    pts, gt = random_scene(13, 2, M, 400, live=[M, M])
    gt[:, :TILE, 0] += F(500.0)              # every box of the first tile is far from every point
    pts[pts[:, 0] == 1, 1:] = [inside_point(gt, 1, TILE, u)[1:] for u in
                               np.random.RandomState(2).uniform(-0.6, 0.6, (int((pts[:, 0] == 1).sum()), 3))]

    def present(c):
        k, idx, hit, _ = state(c)
        return c["gt"].shape[1] == TILE + 1 and set(idx[k == 1]) == {-1, TILE} and set(idx) == {-1, TILE} \
            and bool((hit & (idx < 0)).any())
    return case(pts, gt, present)


def enlarged_only():
    pts, gt = random_scene(14, 2, 4, 120, live=[2, 2])
    rs = np.random.RandomState(3)
    for i in range(40, 60):
        b = int(pts[i, 0])
        g = gt[b, 0]
        u = np.array([[(0.5 + 0.05 / g[3]) * rs.choice([-1, 1]), rs.uniform(-0.4, 0.4), rs.uniform(-0.4, 0.4)]])
        pts[i, 1:] = local_to_world(g, u)[0]   # 5 cm outside the box, inside the box grown by 20 cm

    def present(c):
        _, idx, hit, lab = state(c)
        only = (idx[40:60] < 0) & hit[40:60]
        return only.all() and (lab[40:60] == -1).all() and bool((lab == 0).any()) and bool((lab > 0).any())
    return case(pts, gt, present)


def enlarged_hit_is_another_box():
    gt = np.zeros((1, 4, 8), dtype=F)
    gt[0, 0] = [0, 0, 0, 4, 2, 2, 0, 1]
    gt[0, 1] = [4.05, 0, 0, 4, 2, 2, 0, 2]
    pts = [[0, 2.08, 0.3, 0.1], [0, 2.03, 0.3, 0.1], [0, 1.0, 0.0, 0.0], [0, 30.0, 0, 0]]

    def present(c):
        _, idx, hit, lab = state(c)
        first_ext = roipool_seq.points_in_boxes(c["ext"][:, :, :7], c["points"][None, :, 1:4])[0]
        return idx[0] == 1 and first_ext[0] == 0 and lab[0] == 2 and idx[1] == -1 and hit[1] and lab[1] == -1
    return case(pts, gt, present)


def origin_in_zero_rows(num_class):
    pts, gt = random_scene(15, 2, 6, 150, live=[3, 4])
    gt[0, :3, 0] += F(60.0)                  # no live box near the origin
    gt[1, :4, 0] += F(60.0)
    pts[10] = [0, 0, 0, 0]
    pts[140] = [1, 0, 0, 0]
    mean = KITTI if num_class > 1 else KITTI[:1]
    if num_class == 1:
        gt[:, :, 7] = np.minimum(gt[:, :, 7], F(1.0))   # one class, one row of mean sizes

    def present(c):
        _, idx, _, lab = state(c)
        out = run(c)
        rows_zero = not c["gt"][0, 3].any() and not c["gt"][1, 4].any()
        fg_targets = bool(out["point_box_labels"][10, 3:6].all()) and (out["point_part_labels"][10] == F(0.5)).all()
        want = 1 if c["num_class"] == 1 else 0
        last = seq.f32_of_double(np.log, seq.TINY / c["mean"][-1])
        return rows_zero and idx[10] == 3 and idx[140] == 4 and lab[10] == want and lab[140] == want and fg_targets \
            and seq.same_bits(out["point_box_labels"][10, 3:6], last)
    return case(pts, gt, present, num_class=num_class, mean=mean)


def class_two_of_three():
    pts, gt = random_scene(16, 2, 5, 200)
    gt[:, :, 7] = np.where(gt[:, :, 7] > 0, F(2.0), F(0.0))

    def present(c):
        _, idx, _, lab = state(c)
        return c["num_class"] == 3 and idx.max() >= 0 and set(lab[idx >= 0]) == {2}
    return case(pts, gt, present)


def zero_dx():
    pts, gt = random_scene(17, 1, 5, 100, live=[3])
    gt[0, 3] = [1.0, 70.0, 0.0, 0.0, 1.6, 1.5, 0.0, 2.0]
    pts[5] = [0, 1.0, 70.25, 0.1]
    pts[6] = [0, F(1.0) + F(2.0 ** -18), 69.5, -0.2]
    pts[7] = [0, F(1.0) - F(2.0 ** -17), 69.5, -0.2]

    def present(c):
        _, idx, _, _ = state(c)
        out = run(c)
        clamp = seq.f32_of_double(np.log, seq.TINY / c["mean"][1, 0:1])[0]
        return c["gt"][0, 3, 3] == 0 and (idx[5:8] == 3).all() and (out["point_box_labels"][5:8, 3] == clamp).all() \
            and out["point_part_labels"][6, 0] == F(F(2.0 ** -18) / seq.TINY + F(0.5))
    return case(pts, gt, present)


def zero_dx_part_alone():
    c = zero_dx()

    def present(c):
        out = run(c)["point_part_labels"]
        return np.isnan(out[5, 0]) and np.isposinf(out[6, 0]) and np.isneginf(out[7, 0])   # the sizes as given: no clamp
    return dict(c, want_box=False, present=present)


def negative_dz():
    pts, gt = random_scene(18, 1, 5, 100, live=[3])
    gt[0, 1, 5] = -gt[0, 1, 5]
    pts[20:30] = [inside_point(gt, 0, 1, u) for u in np.random.RandomState(4).uniform(-0.4, 0.4, (10, 3))]

    def present(c):
        _, idx, hit, lab = state(c)
        g = c["gt"][0, 1].copy()
        g[5] = -g[5]
        would = roipool_seq.inside_mask(c["points"][20:30, 1:4], g[None, :7])[0]
        return c["gt"][0, 1, 5] < 0 and would.all() and (idx[20:30] < 0).all() and (lab[20:30] == 0).all() and not hit[20:30].any()
    return case(pts, gt, present)


def thresholds():
    """points exactly on the predicate's thresholds, the construction tests/roipool_seq.py:fixture_cases looks for: an
    axis-aligned box at x = y = 0, |x| one float inside / outside the side face's double bound, a point on the z face, and
    a dx whose float32 bound dx * 0.5f + 1e-5f lies below the double one with a point at that float32 sum"""
    rs = np.random.RandomState(5)
    dx = next(d for d in (F(rs.uniform(16, 32)) for _ in range(1000)) if roipool_seq.f32_bound_wrong(d))   # 1e-5 is 10.49 floats there
    gt = np.zeros((1, 3, 8), dtype=F)
    gt[0, 0] = [0, 0, 0.25, dx, 2.0, 1.5, 0, 1]
    D = np.float64(dx) / 2.0 + roipool_seq.MARGIN
    up = F(D) if np.float64(F(D)) >= D else np.nextafter(F(D), F(np.inf))
    dn = np.nextafter(up, F(-np.inf))
    f32sum = dx * F(0.5) + F(1e-5)
    zf = F(0.25) + F(0.75)
    pts = [[0, dn, 0.1, 0.3], [0, -dn, -0.1, 0.3], [0, up, 0.1, 0.3], [0, -up, 0.1, 0.3], [0, f32sum, 0.2, 0.3],
           [0, 0.5, 0.3, zf], [0, 0.5, 0.3, np.nextafter(zf, F(9))], [0, 0.5, 0.3, F(0.25) - F(0.75)]]
    # the enlarged box is the gt box, so a point one float outside is background, not ignored
    def present(c):
        _, idx, hit, lab = state(c)
        return list(idx) == [0, 0, -1, -1, 0, 0, -1, 0] and roipool_seq.f32_bound_wrong(c["gt"][0, 0, 3]) \
            and np.float64(c["points"][4, 1]) < D and list(lab) == [1, 1, 0, 0, 1, 1, 0, 1]
    return case(pts, gt, present, ext=gt)


def nan_coordinates():
    pts, gt = random_scene(19, 2, 5, 200)
    w = inside_point(gt, 0, 0)
    pts[30] = [0, np.nan, w[2], w[3]]
    pts[31] = [0, w[1], np.nan, w[3]]
    pts[32] = [0, w[1], w[2], np.nan]       # the predicate's z test is "outside if |z - cz| > dz / 2": false for NaN
    pts[33] = [0, np.nan, np.nan, np.nan]

    def present(c):
        _, idx, hit, lab = state(c)
        return (idx[[30, 31, 33]] < 0).all() and not hit[[30, 31, 33]].any() and (lab[[30, 31, 33]] == 0).all() and idx[32] == 0
    return case(pts, gt, present)


def no_mean_size():
    pts, gt = random_scene(20, 2, 5, 200)
    return case(pts, gt, lambda c: c["mean"] is None and c["want_box"] and (state(c)[1] >= 0).any(), mean=None)


def wants(box, part):
    pts, gt = random_scene(21, 2, 5, 300)
    return case(pts, gt, lambda c: (c["want_box"], c["want_part"]) == (box, part) and (state(c)[1] >= 0).any(),
                want_box=box, want_part=part)


def grouped_big():
    """B = 3, ~1500 points grouped by sample: workgroups of one sample and workgroups across a boundary"""
    pts, gt = random_scene(22, 3, 40, 1500, live=[23, 31, 40])

    def present(c):
        k = state(c)[0]
        per = [len(set(k[i:i + WG])) for i in range(0, len(k), WG)]
        return 1 in per and 2 in per
    return case(pts, gt, present)


CASES = {
    **{f"N = {n}": (lambda n=n: n_points(n)) for n in (1, 63, 65, WG - 1, WG, WG + 1)},
    "N = 0": no_points, "M = 0": no_boxes, "B = 0": no_samples,
    "shuffled bs_idx": shuffled, "bs_idx -1, B, 0.5": stray_samples, "two boxes, the lower index": overlapping,
    "last row past the tile": last_row_past_the_tile, "enlarged box only": enlarged_only,
    "enlarged hit is another box": enlarged_hit_is_another_box,
    "origin in zero rows, class 0 wraps": lambda: origin_in_zero_rows(3),
    "origin in zero rows, num_class 1": lambda: origin_in_zero_rows(1),
    "class 2.0 of 3": class_two_of_three, "dx = 0": zero_dx, "dx = 0, part labels alone": zero_dx_part_alone,
    "negative dz": negative_dz, "thresholds": thresholds, "NaN coordinates": nan_coordinates,
    "no mean size": no_mean_size,
    **{f"want_box {b}, want_part {p}": (lambda b=b, p=p: wants(b, p)) for b in (False, True) for p in (False, True)},
    "grouped, three samples": grouped_big,
}


# ------------------------------------------------------------------------- past 65 boxes, 3 samples and one workgroup
def held(c, s):
    """(rows of sample s holding each of its points (M, n) bool, the indices of those points)"""
    sel = np.flatnonzero(seq.sample_of(c["points"], c["gt"].shape[0]) == s)
    return roipool_seq.inside_mask(c["points"][sel, 1:4], np.ascontiguousarray(c["gt"][s, :, :7])), sel


def first_enlarged(c):
    """(N,) the lowest enlarged row of the point's sample holding it, -1 for none"""
    k = seq.sample_of(c["points"], c["gt"].shape[0])
    out = np.full(len(k), -1, dtype=np.int64)
    for s in range(c["gt"].shape[0]):
        sel = np.flatnonzero(k == s)
        out[sel] = roipool_seq.points_in_boxes(np.ascontiguousarray(c["ext"][s:s + 1, :, :7]), c["points"][None, sel, 1:4])[0]
    return out


def margin_point(gt, b, j, rs):
    """5 cm outside box j of sample b across an x face: inside the box grown by 20 cm only"""
    g = gt[b, j]
    u = np.array([[(0.5 + 0.05 / g[3]) * rs.choice([-1, 1]), rs.uniform(-0.4, 0.4), rs.uniform(-0.4, 0.4)]])
    return [b, *local_to_world(g, u)[0]]


def grown(g, by):
    """a copy of row g with every size grown by `by` metres and the next class"""
    out = g.copy()
    out[3:6] += F(by)
    out[7] = 1 + g[7] % 3
    return out


def two_tiles():
    M = 2 * TILE
    pts, gt = random_scene(30, 2, M, 600, live=[M, M])
    gt[:, M - 1, 0] += F(200.0)              # the last row lies alone: no lower row takes its points
    rs = np.random.RandomState(30)
    pts[290:300] = [inside_point(gt, 0, M - 1, u) for u in rs.uniform(-0.45, 0.45, (10, 3))]
    pts[0:5] = [inside_point(gt, 0, 0, u) for u in rs.uniform(-0.45, 0.45, (5, 3))]

    def present(c):
        _, idx, _, lab = state(c)
        return c["gt"].shape[1] == 2 * TILE and bool(c["gt"][:, :, 3:6].all()) and (idx[290:300] == 2 * TILE - 1).all() \
            and (idx[0:5] == 0).all() and (lab[290:300] > 0).all() and set(idx[idx >= 0] // TILE) == {0, 1}
    return case(pts, gt, present)


def two_tiles_and_a_row():
    M = 2 * TILE + 1
    pts, gt = random_scene(31, 2, M, 500, live=[M, M])
    gt[:, M - 1, 0] += F(300.0)
    pts[400:412] = [inside_point(gt, 1, M - 1, u) for u in np.random.RandomState(31).uniform(-0.45, 0.45, (12, 3))]

    def present(c):
        k, idx, _, _ = state(c)
        m, sel = held(c, 1)
        only = sel[m[2 * TILE] & ~m[:2 * TILE].any(axis=0)]
        return c["gt"].shape[1] == 2 * TILE + 1 and len(only) >= 10 and (idx[only] == 2 * TILE).all() \
            and set(idx[idx >= 0] // TILE) == {0, 1, 2}
    return case(pts, gt, present)


def three_tiles_and_37():
    M = 3 * TILE + 37
    pts, gt = random_scene(32, 2, M, 1500, live=[M, M])

    def present(c):
        idx = state(c)[1]
        return c["gt"].shape[1] == 3 * TILE + 37 and set(idx[idx >= 0] // TILE) == {0, 1, 2, 3} \
            and bool((idx >= 3 * TILE + 32).any())
    return case(pts, gt, present)


def first_hit_wins_across_tiles():
    M = 2 * TILE + 20
    a, b, c_ = 5, TILE + 9, 2 * TILE + 3
    pts, gt = random_scene(33, 2, M, 800, live=[M, M])
    gt[1, a, 0:2] = [150.0, 150.0]           # away from every other box
    gt[1, b] = grown(gt[1, a], 0.5)
    gt[1, c_] = grown(gt[1, b], 0.5)
    rs = np.random.RandomState(33)
    pts[600:610] = [inside_point(gt, 1, a, u) for u in rs.uniform(-0.45, 0.45, (10, 3))]
    for i in range(610, 620):                # 15 cm outside row a, 10 cm inside row b
        u = [(0.5 + 0.15 / gt[1, a, 3]) * rs.choice([-1, 1]), rs.uniform(-0.4, 0.4), rs.uniform(-0.4, 0.4)]
        pts[i] = inside_point(gt, 1, a, u)

    def present(c):
        _, idx, _, lab = state(c)
        g = c["gt"]
        m, sel = held(c, 1)
        three, two = sel[m[a] & m[b] & m[c_]], sel[~m[a] & m[b] & m[c_]]
        across = 0
        for s in range(2):
            ms = held(c, s)[0]
            across += int((sum(ms[t:t + TILE].any(axis=0).astype(int) for t in range(0, M, TILE)) >= 2).sum())
        return len({int(g[1, a, 7]), int(g[1, b, 7]), int(g[1, c_, 7])}) == 3 and a < TILE <= b < 2 * TILE <= c_ \
            and len(three) >= 10 and (idx[three] == a).all() and (lab[three] == int(g[1, a, 7])).all() \
            and len(two) >= 10 and (idx[two] == b).all() and (lab[two] == int(g[1, b, 7])).all() and across >= 30
    return case(pts, gt, present)


def enlarged_rows_elsewhere():
    M = 2 * TILE + 11
    pts, gt = random_scene(34, 2, M, 1400, live=[M, M])
    order = np.roll(np.arange(M), TILE + 7)
    ext = seq.enlarge(gt)[:, order]
    ext[1, :, 0] += F(500.0)                 # sample 1: no enlarged row near any point

    def present(c):
        k, idx, hit, lab = state(c)
        fe = first_enlarged(c)
        ign = (k == 0) & (idx < 0) & (fe >= 0)
        per_tile = [int((fe[ign] // TILE == t).sum()) for t in range(3)]
        apart = (k == 0) & (idx >= 0) & (fe >= 0) & (idx // TILE != fe // TILE)
        one = (k == 1) & (idx >= 0)
        return seq.same_bits(c["ext"][0], seq.enlarge(c["gt"])[0, order]) and min(per_tile) >= 3 and (lab[ign] == -1).all() \
            and int(apart.sum()) >= 10 and int(one.sum()) >= 10 and not hit[k == 1].any() and (lab[one] > 0).all() \
            and (lab[one] == c["gt"][1, idx[one], 7].astype(np.int64)).all()
    return case(pts, gt, present, ext=ext)


def sixteen_samples_in_one_workgroup():
    pts, gt = random_scene(35, 16, 6, WG, live=[4] * 16)
    rs = np.random.RandomState(35)
    for b in range(16):
        pts[16 * b] = inside_point(gt, b, 0)
        pts[16 * b + 1] = margin_point(gt, b, 0, rs)

    def present(c):
        k, idx, _, lab = state(c)
        return len(k) == WG and (k == np.arange(WG) // 16).all() \
            and all((idx[k == b] >= 0).any() and (lab[k == b] == -1).any() for b in range(16))
    return case(pts, gt, present)


def forty_samples_shuffled():
    B, M = 40, TILE + 3
    pts, gt = random_scene(36, B, M, 520, live=[M] * B)
    for b in range(B):
        j = TILE + b % 3
        gt[b, j, 0] += F(200.0)
        pts[13 * b] = inside_point(gt, b, j)                 # a foreground point of every sample, past the first tile
    pts = pts[np.random.RandomState(36).permutation(len(pts))]

    def present(c):
        k, idx, _, _ = state(c)
        full = [len(set(k[i:i + 64])) for i in range(0, len(k) - 63, 64)]     # 520 = 8 wavefronts of 64 and 8 points
        return c["gt"].shape[:2] == (40, TILE + 3) and len(k) == 520 and len(full) == 8 and min(full) >= 20 \
            and set(k[idx >= 0]) == set(range(40)) and bool((idx >= TILE).any()) and len(set(k[512:])) >= 2
    return case(pts, gt, present)


def samples_descending():
    pts, gt = random_scene(37, 5, 12, 1500, live=[10] * 5)
    count = {4: 300, 3: 212, 2: 60, 1: 60, 0: 68}            # 700 points: workgroups of one, two and three samples
    pts = pts[np.concatenate([np.flatnonzero(pts[:, 0] == s)[:count[s]] for s in (4, 3, 2, 1, 0)])]

    def present(c):
        k, idx, _, _ = state(c)
        per = [len(set(k[i:i + WG])) for i in range(0, len(k), WG)]
        return len(k) == 700 and (np.diff(k) <= 0).all() and k[0] == 4 and k[-1] == 0 and 1 in per and 2 in per \
            and set(k[idx >= 0]) == {0, 1, 2, 3, 4}
    return case(pts, gt, present)


def samples_no_point_names():
    pts, gt = random_scene(38, 9, 8, 900, live=[6] * 9)
    pts = pts[np.isin(pts[:, 0], (1, 4, 8))]                 # 100 points each of samples 1, 4 and 8
    gt[4, 6] = grown(gt[1, 2], 0.5)                          # sample 4 has a row around a box of sample 1, and the reverse
    gt[1, 6] = grown(gt[4, 3], 0.5)
    rs = np.random.RandomState(38)
    pts[10:35] = [inside_point(gt, 1, 2, u) for u in rs.uniform(-0.45, 0.45, (25, 3))]
    pts[110:135] = [inside_point(gt, 4, 3, u) for u in rs.uniform(-0.45, 0.45, (25, 3))]
    gt[0], gt[2], gt[3] = gt[4], gt[8], gt[1]                # the rows a sample renumbered by rank would read

    def present(c):
        k, idx, _, _ = state(c)
        g, p = c["gt"], c["points"]

        def misled(s, other):
            """points of sample s that `other`'s rows hold too, in a row that differs from the one s gives them"""
            sel = np.flatnonzero((k == s) & (idx >= 0))
            m = roipool_seq.inside_mask(p[sel, 1:4], np.ascontiguousarray(g[other, :, :7]))
            there = m.any(axis=0)
            differ = (g[other, m.argmax(axis=0)] != g[s, idx[sel]]).any(axis=1)
            return int((there & differ).sum())
        return g.shape[0] == 9 and set(k) == {1, 4, 8} and np.array_equal(g[0], g[4]) and np.array_equal(g[2], g[8]) \
            and np.array_equal(g[3], g[1]) and misled(1, 0) >= 20 and misled(4, 1) >= 20
    return case(pts, gt, present)


STRAYS = (-1.0, 2.0, 0.5, np.nan)


def strays_by_the_wavefront():
    N = 3 * WG + 64
    pts, gt = random_scene(39, 2, 8, N, live=[6, 6])
    rs = np.random.RandomState(39)
    for i in list(range(64, 128)) + list(range(WG, 2 * WG)):
        pts[i] = [STRAYS[i % 4], *inside_point(gt, 0, i % 6, rs.uniform(-0.4, 0.4, 3))[1:]]

    def present(c):
        k, _, _, lab = state(c)
        p = c["points"]
        stray = np.zeros(len(p), dtype=bool)
        stray[64:128] = stray[WG:2 * WG] = True
        would = roipool_seq.inside_mask(p[:, 1:4], np.ascontiguousarray(c["gt"][0, :, :7])).any(axis=0)
        seen = [bool((p[stray, 0] == F(v)).any()) for v in STRAYS[:3]] + [bool(np.isnan(p[stray, 0]).any())]
        return len(p) == 3 * WG + 64 and c["gt"].shape[0] == 2 and (k[stray] == -1).all() and (k[~stray] >= 0).all() \
            and would[stray].all() and (lab[stray] == 0).all() and all(seen) and bool((lab[~stray] > 0).any())
    return case(pts, gt, present)


def one_point_in_the_tail_workgroup():
    N, M = 4 * WG + 1, TILE + 10
    pts, gt = random_scene(40, 3, M, N, live=[M] * 3)
    gt[2, TILE + 5, 0] += F(200.0)
    pts[-1] = inside_point(gt, 2, TILE + 5)

    def present(c):
        k, idx, _, lab = state(c)
        return len(k) == 4 * WG + 1 and k[-1] == c["gt"].shape[0] - 1 and idx[-1] == TILE + 5 and lab[-1] > 0
    return case(pts, gt, present)


def detector_sized():
    B, M, per = 4, 200, 5003
    pts, gt = random_scene(41, B, M, B * per, live=[200, 137, 65, 0])
    pts[-1] = [3, 0, 0, 0]                   # the origin, in a sample of zero rows only

    def present(c):
        k, idx, _, lab = state(c)
        return c["gt"].shape[:2] == (4, 200) and [int((k == s).sum()) for s in range(4)] == [5003] * 4 \
            and not c["gt"][3].any() and k[-1] == 3 and idx[-1] == 0 and bool((idx >= 2 * TILE).any()) \
            and bool((lab == -1).any()) and -(-len(k) // WG) >= 70
    return case(pts, gt, present)


PAST = {
    "M = 2 tiles": two_tiles, "M = 2 tiles + 1": two_tiles_and_a_row, "M = 3 tiles + 37": three_tiles_and_37,
    "first hit wins across tiles": first_hit_wins_across_tiles, "enlarged rows elsewhere": enlarged_rows_elsewhere,
    "16 samples in one workgroup": sixteen_samples_in_one_workgroup,
    "40 samples shuffled, two tiles": forty_samples_shuffled, "samples descending": samples_descending,
    "samples that no point names": samples_no_point_names,
    "a wavefront and a workgroup of strays": strays_by_the_wavefront,
    "one point in the tail workgroup": one_point_in_the_tail_workgroup, "detector-sized": detector_sized,
}


@functools.lru_cache(maxsize=None)
def past(name):
    """the PAST case `name` with its restatement result under "want", built once: shared, so leave it unchanged"""
    c = PAST[name]()
    return dict(c, want=run(c))
