"""Restatement of the dataset-infos kernels (modest_amd/csrc/kitti_infos.hip: infos_count, infos_scan, infos_gather;
DESIGN.md section 7c) in plain numpy, shared by tests/test_kitti_infos_cases_cpu.py and tests/test_gpu_kitti_infos_edges.py.

A case (`make_case`) is what one modest_infos_count call sees: packed (R, 4) float32 rows, an ops.INFOS_FRAME table whose
frames carry their own m1 / p2t / height / width / fov_only, the float64 (nb, 7) boxes of every frame turned into
ops.INFOS_BOX rows by the package's own `_box_table(gt, boxes_to_corners_3d(gt))` (so the shipped reject and tau are under
test), `pass_boxes` and `und_cap`.

`expect(case)` gives, per frame: the FOV flag of every row (kitti_infos.get_fov_flag), the dense database mask
(kitti_infos.points_in_boxes_host) and its row sums, the gathered rows (box after box in table order, the members of a box
in file order, xyz = float32(float64(p) - centre), column 3 with its bits), and the hull: the margin m of every counted
row in np.longdouble from the table's own cs / b / tau, inside = m >= tau, undecided = not inside and m > -tau.  A row
with a NaN coordinate has a NaN margin and is neither: that is the answer of the reference's Delaunay.find_simplex.

The device evaluates m in float64 with one fma, so a row whose |m| lies within rounding of tau could fall either way:
`delta(case)` = 2^-40 * max(1, max|corner|) is about a thousand times the measured float64-to-longdouble difference of m
(8.8e-16 x reach), and `band_rows` lists the (box, row) pairs closer to +-tau than that.  Such a pair is allowed only when
`exact_pair` shows that the device's float64 evaluation IS the rational margin (the deciding axis is z, or the heading is
0 with cs = (1, 0)); there m == tau is inside and m == -tau is outside and not undecided."""
from fractions import Fraction

import numpy as np

from modest_amd import kitti_infos as ki
from modest_amd import ops

F = np.float32
LD = np.longdouble
CHUNK = 512                # rows of a wavefront's chunk (modest_infos_chunk_rows(); asserted on the device by the GPU file)
WG_ROWS = 4 * CHUNK
NAN_PAYLOAD = 0x7FC12345


# ---- calibrations in exact arithmetic ---------------------------------------------------------------------------------
def exact_calib(focal=512.0, cu=256.0, cv=128.0, t_cam=(0.0, 0.0, 0.0), t_img=(0.0, 0.0, 0.0), size=(512, 256)):
    """-> dict(m1 (12,), p2t (12,), width, height, text).  Tr_velo_to_cam is the signed permutation cam = (-y, -z, x) + t_cam,
    R0 = I, P2 = [[f 0 cu t0] [0 f cv t1] [0 0 1 t2]]: with dyadic entries and rows every product of the chain is exact,
    and with t_img = 0 every output takes one rounding whatever the order or fusing.  `text` is the calib file."""
    V2C = np.array([[0, -1, 0, t_cam[0]], [0, 0, -1, t_cam[1]], [1, 0, 0, t_cam[2]]], dtype=np.float64)
    P2 = np.array([[focal, 0, cu, t_img[0]], [0, focal, cv, t_img[1]], [0, 0, 1, t_img[2]]], dtype=np.float64)
    line = lambda k, a: k + ": " + " ".join(repr(float(v)) for v in np.ravel(a))      # noqa: E731
    text = "\n".join([line("P0", P2), line("P1", P2), line("P2", P2), line("P3", P2), line("R0_rect", np.eye(3)),
                      line("Tr_velo_to_cam", V2C), line("Tr_imu_to_velo", V2C)]) + "\n"
    m1 = np.dot(V2C.astype(F).T, np.eye(3, dtype=F).T)                                   # Calibration.lidar_to_rect_matrix
    return dict(m1=m1.reshape(-1).astype(F), p2t=np.ascontiguousarray(P2.astype(F).T).reshape(-1), width=int(size[0]),
                height=int(size[1]), text=text)


CALIB_A = exact_calib(t_cam=(0.25, -0.5, 0.125))
CALIB_B = exact_calib(256.0, 128.0, 64.0, t_cam=(-1.0, 0.75, 2.0), size=(256, 128))


class TableCalib(ki.Calibration):
    """kitti_infos.Calibration standing on a frame's m1 / p2t instead of a calib file"""

    def __init__(self, m1, p2t):
        self._m1 = np.ascontiguousarray(m1, dtype=F).reshape(4, 3)
        self.P2 = np.ascontiguousarray(np.asarray(p2t, dtype=F).reshape(4, 3).T)     # P2.T is then the view Calibration multiplies by

    def lidar_to_rect_matrix(self):
        return self._m1


# ---- a case -----------------------------------------------------------------------------------------------------------
def make_case(frames, pass_boxes=256, und_cap=32, **notes):
    """frames: [dict(rows (n, 4) float32, gt (nb, 7) float64, calib, fov_only)] -> the case"""
    fr = np.zeros(len(frames), dtype=ops.INFOS_FRAME)
    rows, tabs, gts, corners = [], [], [], []
    off = nb_run = cnt_run = 0
    for k, f in enumerate(frames):
        r = tag_intensity(np.array(f["rows"], dtype=F).reshape(-1, 4))
        gt = np.ascontiguousarray(f.get("gt", np.zeros((0, 7))), dtype=np.float64).reshape(-1, 7)
        co = ki.boxes_to_corners_3d(gt) if len(gt) else np.zeros((0, 8, 3), dtype=F)
        cal = f.get("calib", CALIB_A)
        fr["row_offset"][k], fr["n"][k], fr["box_begin"][k], fr["box_count"][k], fr["cnt_offset"][k] = off, len(r), nb_run, len(gt), cnt_run
        fr["m1"][k], fr["p2t"][k], fr["height"][k], fr["width"][k] = cal["m1"], cal["p2t"], cal["height"], cal["width"]
        fr["fov_only"][k] = int(f.get("fov_only", 0))
        off += len(r)
        nb_run += len(gt)
        cnt_run += -(-len(r) // CHUNK) * len(gt)
        rows.append(r), tabs.append(ki._box_table(gt, co)), gts.append(gt), corners.append(co)
    case = dict(rows=np.concatenate(rows) if rows else np.zeros((0, 4), dtype=F), frames=fr, boxes=np.concatenate(tabs), gts=gts,
                corners=corners, pass_boxes=int(pass_boxes), und_cap=int(und_cap), wcount_words=cnt_run)
    case.update(notes)
    return case


def frame_rows(case, f):
    fr = case["frames"][f]
    return case["rows"][int(fr["row_offset"]):int(fr["row_offset"]) + int(fr["n"])]


def frame_boxes(case, f):
    fr = case["frames"][f]
    return case["boxes"][int(fr["box_begin"]):int(fr["box_begin"]) + int(fr["box_count"])]


def tag_intensity(rows, nan_every=7):
    """column 3 := the row number, every `nan_every`-th a NaN with a payload: order and bit preservation both show"""
    rows = np.ascontiguousarray(rows, dtype=F)
    rows[:, 3] = np.arange(len(rows), dtype=F)
    rows[nan_every - 1::nan_every, 3] = np.array([NAN_PAYLOAD], dtype=np.uint32).view(F)[0]
    return rows


def to_world(gt7, local):
    """local (k, 3) offsets in the box's frame -> float32 lidar points (the float64 point rounded once)"""
    b = np.asarray(gt7, dtype=np.float64)
    l = np.asarray(local, dtype=np.float64).reshape(-1, 3)
    c, s = np.cos(b[6]), np.sin(b[6])
    return np.stack([b[0] + l[:, 0] * c - l[:, 1] * s, b[1] + l[:, 0] * s + l[:, 1] * c, b[2] + l[:, 2]], axis=1).astype(F)


def steps(x, k):
    """x moved k float32 values up (k > 0) or down"""
    x = F(x)
    for _ in range(abs(int(k))):
        x = np.nextafter(x, F(np.inf) if k > 0 else F(-np.inf), dtype=F)
    return x


# ---- the hull margin --------------------------------------------------------------------------------------------------
def margin_ld(xyz, box):
    """(n,) np.longdouble margin of float32 points against one INFOS_BOX row, from its own b and cs"""
    p = np.asarray(xyz, dtype=F).astype(LD)
    b, cs = box["b"].astype(LD), box["cs"].astype(LD)
    with np.errstate(invalid="ignore"):
        sx, sy, sz = p[:, 0] - b[0], p[:, 1] - b[1], p[:, 2] - b[2]
        lx, ly = sy * cs[1] + sx * cs[0], sy * cs[0] - sx * cs[1]
        m = np.minimum(np.minimum(b[3] / 2 - np.abs(lx), b[4] / 2 - np.abs(ly)), b[5] / 2 - np.abs(sz))
    return m                                           # np.minimum hands a NaN on: a NaN coordinate is a NaN margin


def delta(case):
    reach = max([1.0] + [float(np.max(np.abs(c))) for c in case["corners"] if c.size])
    return 2.0 ** -40 * reach


def band_rows(case):
    """[(frame, box in frame, row)] of every pair with ||m| - tau| < delta, all rows (counted or not)"""
    d, out = LD(delta(case)), []
    for f in range(len(case["frames"])):
        rows = frame_rows(case, f)
        for j, box in enumerate(frame_boxes(case, f)):
            with np.errstate(invalid="ignore"):
                near = np.abs(np.abs(margin_ld(rows[:, :3], box)) - LD(box["tau"])) < d
            out += [(f, j, int(i)) for i in np.nonzero(near)[0]]
    return out


def _rn(q):
    return Fraction(float(q))      # a rational rounded to the nearest float64 (Fraction.__float__ rounds correctly)


def exact_pair(xyz, box):
    """-> (the rational margin, the device's float64 margin as a rational): kitti_infos.hip hull_margin operation for
    operation, every rounding of it written out (_rn), against the same expression without any"""
    x, y, z = (Fraction(float(v)) for v in xyz)
    b = [Fraction(float(v)) for v in box["b"]]
    c, s = Fraction(float(box["cs"][0])), Fraction(float(box["cs"][1]))
    sx, sy, sz = x - b[0], y - b[1], z - b[2]
    true = min(b[3] / 2 - abs(sy * s + sx * c), b[4] / 2 - abs(sy * c - sx * s), b[5] / 2 - abs(sz))
    dx, dy, dz = _rn(sx), _rn(sy), _rn(sz)
    lx = _rn(dy * s + _rn(dx * c))
    ly = _rn(dy * c - _rn(dx * s))
    dev = min(_rn(b[3] / 2 - abs(lx)), _rn(b[4] / 2 - abs(ly)), _rn(b[5] / 2 - abs(dz)))
    return true, dev


# ---- the restatement --------------------------------------------------------------------------------------------------
def nondegenerate(gt7):
    return bool((np.asarray(gt7)[3:6] != 0).all())      # (a negative size has the corners, and so the hull, of its absolute value)


def expect(case, end_to_end=True):
    """-> dict(fov (R,) bool, dense [per frame (nb, n) int32], db_count (NB,), gathered (total, 4) float32, inside / und
    [per global box: sorted row numbers], hull_count, und_n (NB,), hull_ref [per global box: the reference's in_hull count
    of the counted rows, None for a degenerate box or when end_to_end is off])"""
    fovs, dense, parts, inside, und, hull_ref = [], [], [], [], [], []
    for f, fr in enumerate(case["frames"]):
        rows, gt, tab = frame_rows(case, f), case["gts"][f], frame_boxes(case, f)
        fov = ki.get_fov_flag(rows, TableCalib(fr["m1"], fr["p2t"]), (int(fr["height"]), int(fr["width"]))) if len(rows) else np.zeros(0, dtype=bool)
        fovs.append(np.asarray(fov, dtype=bool))
        counted = fovs[-1] | (int(fr["fov_only"]) == 0)
        d = ki.points_in_boxes_host(rows[:, :3], gt)
        dense.append(d)
        for j in range(len(gt)):
            sel = rows[d[j] > 0].copy()
            sel[:, :3] = (sel[:, :3].astype(np.float64) - gt[j, :3]).astype(F)
            parts.append(sel)
            m = margin_ld(rows[:, :3], tab[j])
            tau = LD(tab[j]["tau"])
            with np.errstate(invalid="ignore"):
                ins = counted & (m >= tau)
                u = counted & ~ins & (m > -tau)
            inside.append(np.nonzero(ins)[0])
            und.append(np.nonzero(u)[0])
            ref = None
            if end_to_end and nondegenerate(gt[j]):
                ref = int(ki.in_hull(rows[counted][:, :3], case["corners"][f][j]).sum())
            hull_ref.append(ref)
    return dict(fov=np.concatenate(fovs) if fovs else np.zeros(0, dtype=bool), dense=dense,
                db_count=np.array([len(p) for p in parts], dtype=np.int32),
                gathered=np.concatenate(parts) if parts else np.zeros((0, 4), dtype=F), inside=inside, und=und,
                hull_count=np.array([len(i) for i in inside], dtype=np.int32), und_n=np.array([len(u) for u in und], dtype=np.int32),
                hull_ref=hull_ref)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def box_frame(case):
    """per global box: (frame, box in frame)"""
    return [(f, j) for f, fr in enumerate(case["frames"]) for j in range(int(fr["box_count"]))]
