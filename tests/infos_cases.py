"""Edge cases of the dataset-infos kernels by name, shared by tests/test_kitti_infos_cases_cpu.py and
tests/test_gpu_kitti_infos_edges.py.  CASES: name -> a case of tests/infos_seq.py, each at the smallest shape that carries
its edge (a chunk is 512 rows, a workgroup 2 048, a pass at most 256 boxes).  `present(case, want)` asserts that the edge
is really there in the restatement `want = infos_seq.expect(case)`, and that no planted row lies within rounding of +-tau
unless the device's float64 margin is the rational one."""
from fractions import Fraction

import numpy as np

import infos_seq as seq
from modest_amd import kitti_infos as ki

F = np.float32
NAN, INF = F(np.nan), F(np.inf)
CASES = {}
CZ = -0.5
ORDINARY = (40.0, -20.0, CZ, 3.9, 1.6, 1.5, 0.3)


def _far(n, cx, cy):
    """rows at least 50 m from (cx, cy) on both axes"""
    i = np.arange(n)
    return np.stack([cx + 50 + (i % 97) * 0.37, cy + 50 + (i % 89) * 0.41, np.full(n, CZ), np.zeros(n)], axis=1).astype(F)


def _inside(rs, gt7, n, scale=0.9):
    half = np.abs(np.asarray(gt7[3:6])) / 2
    p = seq.to_world(gt7, rs.uniform(-scale, scale, (n, 3)) * half)
    return np.concatenate([p, np.zeros((n, 1), dtype=F)], axis=1)


# ---- 1. row seams: one frame, one box ----------------------------------------------------------------------------------
SEAM_ROWS = (1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4609)
LONELY_AT = (0, 63, 64, 447, 448, 511, 512)


def _seam(n, filling):
    rs = np.random.RandomState(1000 + n)
    rows = _far(n, ORDINARY[0], ORDINARY[1])
    if filling == "lonely":
        at = np.array(sorted({i for i in LONELY_AT + (n - 1,) if i < n}))
    elif filling == "every":
        at = np.arange(n)
    else:
        at = np.arange(0, n, 2)
    rows[at] = _inside(rs, ORDINARY, len(at))
    return seq.make_case([dict(rows=rows, gt=[ORDINARY])], kind="seam", members=at)


for _n in SEAM_ROWS:
    for _fill in ("lonely", "every", "other"):
        CASES[f"seam_{_fill}_rows{_n}"] = _seam(_n, _fill)


# ---- 2. pass seams / 3. frames: a line of overlapping boxes, empty ones between filled ones ---------------------------
def _line(rs, n, nb, origin=10.0):
    """nb boxes 1.5 m apart and 4 m long (a row lies in up to five), every fifth moved 30 m aside (no member); n rows, one
    in ten far behind the sensor"""
    k = np.arange(nb)
    gt = np.stack([origin + 1.5 * k, np.where(k % 5 == 1, 33.0, 3.0), np.full(nb, CZ), np.full(nb, 4.0), np.full(nb, 2.0),
                   np.full(nb, 1.5), 0.05 * (k % 7)], axis=1).reshape(nb, 7)
    rows = np.zeros((n, 4), dtype=F)
    rows[:, :3] = rs.uniform(-60, -50, (n, 3))
    if nb:
        filled = np.nonzero(k % 5 != 1)[0]
        for i in range(n):
            if i % 10 != 9:
                rows[i] = _inside(rs, gt[filled[(i * 7) % len(filled)]], 1)[0]
    else:
        rows[:, :3] = rs.uniform(-30, 30, (n, 3))
    return rows, gt


PASS_SEAMS = ((3, 1), (3, 2), (65, 64), (256, 256), (257, 256), (300, 256), (257, 1))
for _nb, _pass in PASS_SEAMS:
    _rows, _gt = _line(np.random.RandomState(2000 + _nb + _pass), 1100, _nb)
    CASES[f"pass_boxes{_nb}_pass{_pass}"] = seq.make_case([dict(rows=_rows, gt=_gt)], pass_boxes=_pass, kind="pass")

FRAME_ROWS, FRAME_BOXES, FRAME_FOV = (0, 1, 513, 2049, 0, 64, 700), (2, 0, 3, 1, 0, 257, 2), (1, 0, 1, 0, 1, 1, 0)


def _frames(rows_of, boxes_of, seed, fov=FRAME_FOV):
    rs = np.random.RandomState(seed)
    out = []
    for k, (n, nb) in enumerate(zip(rows_of, boxes_of)):
        rows, gt = _line(rs, n, nb, origin=10.0 + 3 * k)
        out.append(dict(rows=rows, gt=gt, calib=(seq.CALIB_A, seq.CALIB_B)[k % 2], fov_only=fov[k % len(fov)]))
    return out


CASES["frames_seven"] = seq.make_case(_frames(FRAME_ROWS, FRAME_BOXES, 3000), kind="frames")
CASES["frames_seven_pass2"] = seq.make_case(_frames(FRAME_ROWS, FRAME_BOXES, 3001), pass_boxes=2, und_cap=1, kind="frames")
CASES["frames_all_empty"] = seq.make_case(_frames((0, 0, 0), (2, 0, 1), 3002), kind="empty")
CASES["frames_no_boxes"] = seq.make_case(_frames((700, 64), (0, 0), 3003, fov=(1, 0)), kind="noboxes")

# ---- 4. database predicate / 5. hull: headings x centres x sizes -------------------------------------------------------
HEADINGS = (0.0, float(F(np.pi / 2)), -float(F(np.pi / 2)), np.pi / 4, 3.0, -1e-3, 7.5)
CENTRES = ((0.0, 0.0), (40.0, -20.0), (-900.0, 700.0), (3000.0, -3000.0))
SIZES = ((3.9, 1.6, 1.5), (0.05, 0.05, 0.05), (12.0, 0.4, 2.0), (0.0, 1.6, 1.5), (-1.0, 1.6, 1.5))


def _boxes_at(centre):
    return np.array([(centre[0], centre[1], CZ) + s + (h,) for h in HEADINGS for s in SIZES], dtype=np.float64)


def _neighbours(p, col, k):
    """(2k + 1, 3): the float32 point p with column `col` moved -k .. k float32 values"""
    up, down = [F(p[col])], [F(p[col])]
    for _ in range(k):
        up.append(np.nextafter(up[-1], INF, dtype=F))
        down.append(np.nextafter(down[-1], -INF, dtype=F))
    out = np.repeat(np.asarray(p, dtype=F)[None], 2 * k + 1, axis=0)
    out[:, col] = np.array(down[:0:-1] + up, dtype=F)
    return out


def _dominant(gt7, axis):
    """the lidar axis along which the normal of a side face (local axis 0 / 1) is larger"""
    c, s = abs(np.cos(gt7[6])), abs(np.sin(gt7[6]))
    return (0 if c >= s else 1) if axis == 0 else (1 if c >= s else 0)


def face_flip(gt7, axis, sign, k=48):
    """two adjacent float32 points between which the database predicate of the box flips at the side face (axis, sign),
    (2, 3), or (0, 3) when none of the 2k + 1 neighbours of the face point shows one"""
    local = [0.0, 0.0, 0.0]
    local[axis] = sign * (gt7[3 + axis] / 2 + 0.01)
    local[1 - axis] = 0.25 * max(gt7[4 - axis], 0.0) / 2
    cand = _neighbours(seq.to_world(gt7, local)[0], _dominant(gt7, axis), k)
    mem = ki.points_in_boxes_host(cand, gt7[None])[0]
    flips = np.nonzero(mem[1:] != mem[:-1])[0]
    if not len(flips):
        return np.zeros((0, 3), dtype=F)
    i = flips[np.argmin(np.abs(flips - k))]
    return cand[i:i + 2]


def _nonfinite_rows(centre):
    c = (F(centre[0]), F(centre[1]), F(CZ))
    rows = []
    for bad in (NAN, INF, -INF):
        for col in range(3):
            r = list(c)
            r[col] = bad
            rows.append(r)
    rows += [[NAN, NAN, c[2]], [c[0], NAN, NAN], [NAN, NAN, NAN]]
    return np.array(rows, dtype=F)


def _db_case(centre):
    gt = _boxes_at(centre)
    pts, flips = [_nonfinite_rows(centre)], [0, 0, 0, 0]
    z_exact = []
    for b in gt:
        for axis in (0, 1):
            for sign in (1, -1):
                pair = face_flip(b, axis, sign)
                flips[2 * axis + (sign < 0)] += len(pair) // 2
                pts.append(pair)
        for sign in (1, -1):                                 # |sz| == dz/2 (exact for the dyadic heights) and 1, 2 values either side
            zf = seq.to_world(b, [0.0, 0.0, sign * b[5] / 2])[0]
            z_exact.append((sum(len(p) for p in pts) + 2, sign))
            pts.append(_neighbours(zf, 2, 2))
        if b[6] == np.pi / 4:                                # the rows farthest from the centre that `reject` must let through
            for off in (0.0099, 0.0101):
                pts.append(seq.to_world(b, [[sx * (b[3] / 2 + off), sy * (b[4] / 2 + off), 0.0] for sx in (1, -1) for sy in (1, -1)]))
    pts = np.concatenate(pts)
    rows = np.concatenate([pts, np.zeros((len(pts), 1), dtype=F)], axis=1)
    return seq.make_case([dict(rows=rows, gt=gt)], kind="db", flips=flips, z_exact=z_exact)


for _c in CENTRES:
    CASES["db_centre_%g_%g" % _c] = _db_case(_c)


def _hull_rows(b, tau):
    """rows at local face offsets +-tau moved 0, +-1, +-2 float32 values, on every axis, and the corners.  An axis without
    extent gets none: at a centre of 0 its rows would have coordinates of about tau, whose float32 neighbours lie closer
    together than delta"""
    half = np.abs(np.asarray(b[3:6])) / 2                 # (the hull of a negative size is that of its absolute value)
    quarter = 0.25 * half
    pts = []
    for axis in range(3):
        col = 2 if axis == 2 else _dominant(b, axis)
        for sign in (1, -1) if half[axis] > 0 else ():
            for t in (tau, -tau):
                local = quarter.copy()
                local[axis] = sign * (half[axis] - t)
                pts.append(_neighbours(seq.to_world(b, local)[0], col, 2))
    for t in (tau, -tau) if (half > 0).all() else ():
        pts.append(seq.to_world(b, [[sx * (half[0] - t), sy * (half[1] - t), sz * (half[2] - t)]
                                    for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]))
    return np.concatenate(pts)


def _hull_case(centre, fov_only):
    gt = _boxes_at(centre)
    corners = ki.boxes_to_corners_3d(gt)
    pts = np.concatenate([_nonfinite_rows(centre)] + [_hull_rows(b, ki.hull_tau(corners[k])) for k, b in enumerate(gt)])
    rows = np.concatenate([pts, np.zeros((len(pts), 1), dtype=F)], axis=1)
    return seq.make_case([dict(rows=rows, gt=gt, fov_only=fov_only)], kind="hull", und_cap=32)


for _c in CENTRES:
    for _fov in (0, 1):
        CASES["hull_centre_%g_%g_fov%d" % (_c + (_fov,))] = _hull_case(_c, _fov)

# the NaN rows on their own, every row counted: a row with a NaN coordinate is neither inside nor undecided
CASES["hull_nan_rows"] = seq.make_case([dict(rows=np.concatenate([np.concatenate([_nonfinite_rows(c), np.zeros((12, 1), dtype=F)], axis=1),
                                                                  _inside(np.random.RandomState(7), _boxes_at(c)[0], 20)]),
                                             gt=_boxes_at(c)[[0, 2, 5, 15]], fov_only=0) for c in CENTRES[:2]], kind="nan")


def _exact_scene(fov_only):
    """heading 0, dyadic centre and sizes, max|corner| <= 128 (tau = 2^-15): rows land on m == tau and m == -tau exactly"""
    b = np.array([32.0, -8.0, CZ, 4.0, 2.0, 1.5, 0.0])
    tau = 2.0 ** -15
    pts = []
    for axis in range(3):
        for sign in (1, -1):
            for t in (tau, -tau):
                p = np.array([b[0] + 0.5, b[1] - 0.25, b[2] + 0.125], dtype=F)
                p[axis] = F(b[axis] + sign * (b[3 + axis] / 2 - t))
                pts.append(_neighbours(p, axis, 1))
    pts = np.concatenate(pts)
    rows = np.concatenate([pts, np.zeros((len(pts), 1), dtype=F)], axis=1)
    return seq.make_case([dict(rows=rows, gt=[b], fov_only=fov_only)], kind="exact")


CASES["hull_exact_fov0"], CASES["hull_exact_fov1"] = _exact_scene(0), _exact_scene(1)


def _cap_scene(und_cap, fov_only):
    """undecided rows (on the +x face, m ~ 1e-7) per box: 40, 1, 3, and 5 on a box behind the sensor"""
    rs = np.random.RandomState(5000)
    gt = np.array([(10.0, 2.0, CZ, 3.9, 1.6, 1.5, 0.3), (20.0, 2.0, CZ, 3.9, 1.6, 1.5, 0.3), (30.0, 2.0, CZ, 3.9, 1.6, 1.5, 0.3),
                   (-10.0, 2.0, CZ, 3.9, 1.6, 1.5, 0.3)])
    rows = [_far(30, 0.0, 0.0)]
    for b, k in zip(gt, (40, 1, 3, 5)):
        face = seq.to_world(b, np.stack([np.full(k, b[3] / 2), rs.uniform(-0.7, 0.7, k), rs.uniform(-0.6, 0.6, k)], axis=1))
        rows += [np.concatenate([face, np.zeros((k, 1), dtype=F)], axis=1), _inside(rs, b, 20)]
    rows = np.concatenate(rows)
    return seq.make_case([dict(rows=rows[rs.permutation(len(rows))], gt=gt, fov_only=fov_only)], und_cap=und_cap, kind="cap")


for _cap in (0, 1, 4, 32):
    for _fov in (0, 1):
        CASES[f"hull_cap{_cap}_fov{_fov}"] = _cap_scene(_cap, _fov)


# ---- 6. FOV in exact arithmetic ---------------------------------------------------------------------------------------
FOV_T_CAM, FOV_T_IMG = (0.25, -0.5, 0.125), (32.0, 16.0, 0.25)
CALIB_F = seq.exact_calib(512.0, 256.0, 128.0, FOV_T_CAM, FOV_T_IMG, (512, 256))
FOV_STEP = Fraction(1, 8)             # of u and v: x, y, z then lie on multiples of 2^-12 times the depth


def _fov_row(u, v, rz):
    """the lidar row whose image point is (u, v) at rectified depth rz, in rationals"""
    f, cu, cv = 512, 256, 128
    tx, ty, tz = (Fraction(t) for t in FOV_T_CAM)
    t0, t1, _ = (Fraction(t) for t in FOV_T_IMG)
    rx, ry = (u * rz - cu * rz - t0) / f, (v * rz - cv * rz - t1) / f
    return [rz - tz, tx - rx, ty - ry]


def fov_rational(row):
    """-> (flag, every partial sum of both chains and, where rect_z != 0, u and v, as rationals) of a finite float32 row
    under CALIB_F; the planted depths are powers of two, so the two divisions are exact as well"""
    x, y, z = (Fraction(float(v)) for v in row)
    tx, ty, tz = (Fraction(t) for t in FOV_T_CAM)
    t0, t1, t2 = (Fraction(t) for t in FOV_T_IMG)
    r = [-y + tx, -z + ty, x + tz]
    terms = [[512 * r[0], 256 * r[2], t0], [512 * r[1], 128 * r[2], t1], [r[2], t2]]
    sums = list(r)
    for t in terms:
        sums += [sum(t[i] for i in range(len(t)) if mask >> i & 1) for mask in range(1, 1 << len(t))]
    h0, h1, depth = sum(terms[0]), sum(terms[1]), r[2]
    if r[2] == 0:
        return False, sums
    u, v = h0 / r[2], h1 / r[2]
    sums += [u, v]
    return (0 <= u < 512 and 0 <= v < 256 and depth >= 0), sums


def _fov_case():
    W, H, g = Fraction(512), Fraction(256), FOV_STEP
    finite = [_fov_row(u, v, rz) for rz in (1, 2, 8, 32) for u in (Fraction(0), -g, W, W - g, Fraction(201, 2))
              for v in (Fraction(0), -g, H, H - g, Fraction(241, 4))]
    tz = Fraction(FOV_T_CAM[2])
    finite += [[-tz, Fraction(1, 4) + Fraction(1, 16), Fraction(-1, 2) + Fraction(1, 32)],     # rect_z == 0 and hom == 0: 0 / 0
               [-tz, Fraction(-3, 4), Fraction(1)],                                              # rect_z == 0, hom != 0: +-inf
               [-4 - tz, Fraction(1, 4), Fraction(-1, 2)], [-4 - tz, Fraction(3), Fraction(1)],  # rect_z < 0 (u, v inside the image)
               [8 - tz, Fraction(0), Fraction(0)]]
    finite = np.array([[float(v) for v in r] for r in finite], dtype=np.float64)
    zeros = np.array([[-0.0, -0.0, -0.0], [7.875, -0.0, -0.0], [-0.125, -0.0, 0.0]])         # the last: rect_z = -0.125 + 0.125 = +0
    pts = np.concatenate([finite, zeros]).astype(F)
    assert np.array_equal(pts.astype(np.float64), np.concatenate([finite, zeros]))             # every coordinate is a float32
    bad = _nonfinite_rows((8.0, 0.25))
    rows = np.concatenate([np.concatenate([pts, bad]), np.zeros((len(pts) + len(bad), 1), dtype=F)], axis=1)
    big = np.array([[16.0, 0.0, 0.0, 100.0, 100.0, 100.0, 0.0]])
    return seq.make_case([dict(rows=rows, calib=CALIB_F, fov_only=1), dict(rows=rows, gt=big, calib=CALIB_F, fov_only=1)],
                         kind="fov", n_finite=len(pts))


CASES["fov_exact"] = _fov_case()


_restated = {}


def restated(name):
    """the restatement of a named case, computed once and left unchanged"""
    if name not in _restated:
        _restated[name] = seq.expect(CASES[name])
    return _restated[name]


# ---- present ----------------------------------------------------------------------------------------------------------
def _is_f32(q):
    return q == 0 or Fraction(float(F(float(q)))) == q and abs(q) > Fraction(2) ** -126


def check_band(case, want):
    """no row within delta of +-tau unless the device's float64 margin is the rational one; -> the number of exact rows"""
    exact = 0
    for f, j, i in seq.band_rows(case):
        box = seq.frame_boxes(case, f)[j]
        true, dev = seq.exact_pair(seq.frame_rows(case, f)[i, :3], box)
        assert true == dev, ("a planted row sits within delta of tau and its float64 margin is not exact", f, j, i, float(true - dev))
        exact += 1
    return exact


def present(case, want):
    kind, fr = case["kind"], case["frames"]
    exact = check_band(case, want)
    assert exact == 0 or kind in ("exact", "db", "hull"), exact
    total = int(want["db_count"].sum())
    tagged = want["gathered"][:, 3].view(np.uint32)
    assert total == len(want["gathered"])
    if kind in ("seam", "pass", "frames") and total >= 14:
        assert (tagged == seq.NAN_PAYLOAD).any()                      # a NaN payload among the members
    if kind == "seam":
        d, n = want["dense"][0][0], int(fr["n"][0])
        assert np.array_equal(np.nonzero(d)[0], case["members"]) and want["hull_count"][0] == len(case["members"])
        rows, box = seq.frame_rows(case, 0), case["boxes"][0]
        off = np.maximum(np.abs(rows[:, 0] - box["bf"][0]), np.abs(rows[:, 1] - box["bf"][1]))
        assert (off[d == 0] >= 50).all() and (off[d > 0] <= box["reject"]).all() and len(d) == n
    elif kind == "pass":
        d, nb = want["dense"][0], len(case["boxes"])
        per_row, per_box = d.sum(axis=0), d.sum(axis=1)
        assert per_row.max() >= (3 if nb > 3 else 2) and (per_row == 0).any()
        empty = np.nonzero(per_box == 0)[0]
        assert any(per_box[:e].any() and per_box[e + 1:].any() for e in empty)       # a box without members between filled ones
        assert nb >= case["pass_boxes"] and int(fr["n"][0]) == 1100
    elif kind == "frames":
        assert tuple(fr["n"]) == FRAME_ROWS and tuple(fr["box_count"]) == FRAME_BOXES and len(set(fr["fov_only"])) == 2
        assert not np.array_equal(fr["m1"][0], fr["m1"][1]) and 0 < want["fov"].sum() < len(want["fov"])
        assert all(want["db_count"][b] > 0 for b in (2, 4, 5, 263)) and not want["db_count"][:2].any() and want["hull_count"].sum() > 0
    elif kind == "empty":
        assert not fr["n"].any() and len(case["boxes"]) == 3 and total == 0
    elif kind == "noboxes":
        assert len(case["boxes"]) == 0 and 0 < want["fov"].sum() < len(want["fov"])
    elif kind == "db":
        assert min(case["flips"]) >= 1, case["flips"]
        rows, d = seq.frame_rows(case, 0), want["dense"][0]
        nan_z = np.isnan(rows[:, 2]) & ~np.isnan(rows[:, 0]) & ~np.isnan(rows[:, 1])
        assert d[:, nan_z].any(), "a NaN-z member"
        assert not d[:, np.isnan(rows[:, 0]) | np.isnan(rows[:, 1]) | np.isinf(rows[:, :3]).any(axis=1)].any()
        for k, b in enumerate(case["gts"][0]):
            if b[5] in (1.5, 2.0) and b[3] > 0:                      # dyadic heights: the face value is hit exactly
                for at, sign in case["z_exact"][2 * k:2 * k + 2]:
                    assert abs(float(rows[at, 2]) - b[2]) == b[5] / 2 and d[k, at] == 1
                    beyond = d[k, at + 1:at + 3] if sign > 0 else d[k, at - 2:at][::-1]
                    assert not beyond.all() and not beyond[1], "within two float32 values beyond the face the row is no member"
            if b[6] == np.pi / 4 and b[3] > 0 and abs(b[0]) <= 64:
                for off, member in ((0.0099, True), (0.0101, False)):
                    pin = seq.to_world(b, [[sx * (b[3] / 2 + off), sy * (b[4] / 2 + off), 0.0] for sx in (1, -1) for sy in (1, -1)])
                    at = (rows[:, None, :3] == pin[None]).all(axis=2).any(axis=1)
                    assert at.sum() >= 4 and (d[k, at] == int(member)).all()
        assert total > 100
    elif kind in ("hull", "cap", "nan", "exact"):
        rows = seq.frame_rows(case, 0)
        bad = np.isnan(rows[:, :3]).any(axis=1)
        for k, (f, j) in enumerate(seq.box_frame(case)):
            badk = np.nonzero(np.isnan(seq.frame_rows(case, f)[:, :3]).any(axis=1))[0]
            assert not np.intersect1d(badk, want["inside"][k]).size and not np.intersect1d(badk, want["und"][k]).size
        if kind == "hull":
            assert bad.any() and (want["und_n"] > 0).sum() >= 20 and (want["hull_count"] > 0).sum() >= 10 or int(fr["fov_only"][0])
            assert (want["und_n"] > case["und_cap"]).any() or int(fr["fov_only"][0])
        if kind == "nan":
            assert bad.sum() >= 6 and want["hull_count"][0] >= 20
        if kind == "cap":
            n = want["und_n"]
            if int(fr["fov_only"][0]) == 0:
                assert tuple(n) == (40, 1, 3, 5)
            else:
                assert tuple(n[:3]) == (40, 1, 3) and n[3] == 0 and want["hull_count"][3] == 0
        if kind == "exact":
            m = seq.margin_ld(rows[:, :3], case["boxes"][0])
            tau = np.longdouble(case["boxes"][0]["tau"])
            assert tau == 2.0 ** -15 and (m == tau).sum() >= 6 and (m == -tau).sum() >= 6 and exact >= 12
            if int(fr["fov_only"][0]) == 0:
                assert set(np.nonzero(m == tau)[0]) <= set(want["inside"][0])
                assert not set(np.nonzero(m == -tau)[0]) & (set(want["inside"][0]) | set(want["und"][0]))
    elif kind == "fov":
        rows, n = seq.frame_rows(case, 0), case["n_finite"]
        flags = []
        for r in rows[:n, :3]:
            flag, sums = fov_rational(r)
            assert all(_is_f32(q) for q in sums), ("the float32 chain is not exact on", r)
            flags.append(flag)
        assert np.array_equal(want["fov"][:n], flags) and not want["fov"][n:len(rows)].any()
        assert sum(flags) >= 16 and len(flags) - sum(flags) >= 20
        assert np.array_equal(want["fov"][len(rows):], want["fov"][:len(rows)])
        assert set(want["inside"][0]) == set(np.nonzero(want["fov"][:len(rows)])[0])       # the big box holds every FOV row
    else:
        raise AssertionError(kind)
