"""numpy restatement of csrc/box_decode.hip under its arithmetic contract: float32, one rounding per
operation in the written order, sqrt and / correctly rounded (numpy's float32 sqrt and divide are), exp / sin / cos / atan2 via
float64 and ONE cast, x ** 2 as x * x, Python's scalars rounded to float32 first.  ARGMAX: the first index of the maximum, a NaN
counts as the maximum and the first NaN wins (torch's max(dim=-1) on the CPU).

A *case* is a dict: kind "anchor" (box (B, N, code), anchors (N, cols), dir (B, N, bins) | None, dir_offset, dir_limit_offset,
sincos), "point" (box (N, 8 + C), coords (N, 4) whose columns 1:4 are the points, cls (N, K), mean (K, 3) | None) or "roi"
(rois (B, M, code), box (B M, code)).  restate(case) -> the float32 boxes; exact(case) -> (value float64, bound, period): the
expression evaluated in float64 on the same float32 inputs and constants, and per element a bound on the float32 error of ANY
evaluation that rounds + - * / once (relative u = 2^-24 each) and whose sqrt, exp, sin, cos and atan2 are within one ulp
(relative 2 u) -- ours (half an ulp) and the reference's CPU torch alike:
    diag  = sqrt(dxa^2 + dya^2): squares u each, sum u -> 2 u under the root -> u, plus the root's own 2 u          = 3 u
    x, y  = t diag + a: |t| diag (3 u + u) + u |result|                          z = t dza + a: u |t dza| + u |result|
    sizes = exp(t) a: 2 u + u = 3 u                                              (exp(t) alone: 2 u)
    heading atan2(s, c) of s = sint + sin ra, c = cost + cos ra: e_s = 2 u |sin ra| + u |s|, e_c alike, and
          (|c| e_s + |s| e_c) / (c^2 + s^2) + 2 u |angle|; atan2(sint, cost) of given values: 2 u |angle|
    the direction rule adds 8 roundings of magnitudes below |angle| + |dir_offset| + 2 pi, and its floor may land one period
          away: a heading is compared modulo `period` (2 pi without the rule; None: not an angle)
    RoI x = ((xg c + yg (-s)) + zg 0) + roi x with xg = t diag (4 u), c and s 2 u each, a product u, two sums u:
          (4 u + 3 u) (|xg c| + |yg s|) + u |xg c - yg s| + u |x|, y alike
each times 1.01 for the second-order terms, plus 2^-149.  Columns that use + - * / floor only (z, the extra columns, rt + ra and
the direction rule on it, the RoI heading) get the same kind of bound but are compared bit for bit by the tests.  Elements
whose exact value is not a finite float32 get no bound (nan): there the patterns of NaN / inf / zero are compared.
"""
import json
import types

import numpy as np

F = np.float32
U = 2.0 ** -24
TINY = 2.0 ** -149
SLACK = 1.01
TWO_PI = 2 * np.pi
MAX_CODE, MAX_BINS, MAX_CLASS, MAX_ROWS = 16, 8, 32, (1 << 31) - 1
TILE = 256


def f32_of_double(fn, *xs):
    """the double function of float32 arguments, rounded once"""
    with np.errstate(all="ignore"):
        return np.asarray(fn(*[np.asarray(x, dtype=F).astype(np.float64) for x in xs])).astype(F)


def argmax_rule(x):
    """(R, n) -> (R,) the ARGMAX rule"""
    x = np.asarray(x)
    best = np.zeros(x.shape[0], dtype=np.int64)
    bv = x[:, 0].copy()
    for k in range(1, x.shape[1]):
        v = x[:, k]
        with np.errstate(all="ignore"):
            take = (bv == bv) & ((v > bv) | (v != v))
        bv = np.where(take, v, bv)
        best = np.where(take, k, best)
    return best


def period_of(bins):
    return F(2 * np.pi / bins)


def _residual(t, a_xyz, a_size):
    """xg yg zg dxg dyg dzg of encodings t (R, >= 6) against anchor centres and sizes (R, 3) each, float32"""
    dxa, dya, dza = a_size[:, 0], a_size[:, 1], a_size[:, 2]
    diag = np.sqrt(dxa * dxa + dya * dya)
    return [t[:, 0] * diag + a_xyz[:, 0], t[:, 1] * diag + a_xyz[:, 1], t[:, 2] * dza + a_xyz[:, 2],
            f32_of_double(np.exp, t[:, 3]) * dxa, f32_of_double(np.exp, t[:, 4]) * dya, f32_of_double(np.exp, t[:, 5]) * dza]


def anchor_decode(box, anchors, dirp=None, dir_offset=0.0, dir_limit_offset=0.0, sincos=False):
    box, anchors = np.asarray(box, dtype=F), np.asarray(anchors, dtype=F)
    B, N, code = box.shape
    cols = anchors.shape[1]
    t = box.reshape(B * N, code)
    a = np.broadcast_to(anchors[None], (B, N, cols)).reshape(B * N, cols)
    with np.errstate(all="ignore"):
        out = _residual(t, a[:, 0:3], a[:, 3:6])
        ra = a[:, 6]
        if sincos:
            rg = f32_of_double(np.arctan2, t[:, 7] + f32_of_double(np.sin, ra), t[:, 6] + f32_of_double(np.cos, ra))
        else:
            rg = t[:, 6] + ra
        if dirp is not None:
            dirp = np.asarray(dirp, dtype=F)
            bins = dirp.shape[-1]
            label = argmax_rule(dirp.reshape(B * N, bins)).astype(F)
            off, lim, period = F(dir_offset), F(dir_limit_offset), period_of(bins)
            v = rg - off
            rot = v - np.floor(v / period + lim) * period
            rg = (rot + off) + period * label
        first = 8 if sincos else 7
        extras = [t[:, first + k] + a[:, 7 + k] for k in range(cols - 7)]
    return np.stack(out + [rg] + extras, axis=1).astype(F).reshape(B, N, cols)


def point_decode(box, points, cls, mean=None):
    box, points, cls = np.asarray(box, dtype=F), np.asarray(points, dtype=F), np.asarray(cls, dtype=F)
    c = argmax_rule(cls)
    with np.errstate(all="ignore"):
        if mean is not None:
            out = _residual(box, points, np.asarray(mean, dtype=F)[c])
        else:
            out = [box[:, 0] + points[:, 0], box[:, 1] + points[:, 1], box[:, 2] + points[:, 2]] + [
                f32_of_double(np.exp, box[:, k]) for k in (3, 4, 5)]
        rg = f32_of_double(np.arctan2, box[:, 7], box[:, 6])
    return np.stack(out + [rg] + [box[:, k] for k in range(8, box.shape[1])], axis=1).astype(F)


def roi_decode(rois, box):
    rois, box = np.asarray(rois, dtype=F), np.asarray(box, dtype=F)
    code = box.shape[-1]
    r, t = rois.reshape(-1, code), box.reshape(-1, code)
    zero, one = F(0), F(1)
    with np.errstate(all="ignore"):
        xg, yg, zg, dx, dy, dz = _residual(t, np.zeros((len(r), 3), dtype=F), r[:, 3:6])
        ra = r[:, 6]
        c, s = f32_of_double(np.cos, ra), f32_of_double(np.sin, ra)
        x = ((xg * c + yg * (-s)) + zg * zero) + r[:, 0]
        y = ((xg * s + yg * c) + zg * zero) + r[:, 1]
        z = (((xg * zero) + (yg * zero)) + zg * one) + r[:, 2]
        rest = [t[:, k] + r[:, k] for k in range(6, code)]
    return np.stack([x, y, z, dx, dy, dz] + rest, axis=1).astype(F)


def restate(case):
    if case["kind"] == "anchor":
        return anchor_decode(case["box"], case["anchors"], case.get("dir"), case.get("dir_offset", 0.0),
                             case.get("dir_limit_offset", 0.0), case.get("sincos", False))
    if case["kind"] == "point":
        return point_decode(case["box"], case["coords"][:, 1:4], case["cls"], case.get("mean"))
    return roi_decode(case["rois"], case["box"])


# ---------------------------------------------------------------------------------------------------- exact value and bound
def _d(x):
    return np.asarray(x, dtype=F).astype(np.float64)


def _exact_residual(t, a_xyz, a_size):
    """-> ([values], [bounds]) of the six columns, float64"""
    dxa, dya, dza = a_size[:, 0], a_size[:, 1], a_size[:, 2]
    D = np.sqrt(dxa * dxa + dya * dya)
    vals, bnds = [], []
    for k in (0, 1):
        v = t[:, k] * D + a_xyz[:, k]
        vals.append(v)
        bnds.append(4 * U * np.abs(t[:, k]) * D + U * np.abs(v))
    v = t[:, 2] * dza + a_xyz[:, 2]
    vals.append(v)
    bnds.append(U * np.abs(t[:, 2] * dza) + U * np.abs(v))
    for k, a in ((3, dxa), (4, dya), (5, dza)):
        e = np.exp(t[:, k])
        v = e * a
        vals.append(v)
        bnds.append(np.where(e <= np.finfo(F).max, 3 * U * np.abs(v), np.nan))      # exp overflows float32: no bound (inf * 0)
    return vals, bnds


def _finish(vals, bnds, shape):
    val, bnd = np.stack(vals, axis=1), np.stack(bnds, axis=1) * SLACK + TINY
    with np.errstate(all="ignore"):
        ok = np.isfinite(val) & (np.abs(val) <= np.finfo(F).max) & np.isfinite(bnd)
    return val.reshape(shape), np.where(ok, bnd, np.nan).reshape(shape)


def exact(case):
    """-> (value, bound, period): float64 arrays of the output's shape, bound nan where no bound holds; period of the heading
    column (column 6) for the comparison modulo it, or None where the heading is no angle out of atan2"""
    with np.errstate(all="ignore"):
        if case["kind"] == "anchor":
            box, anchors = _d(case["box"]), _d(case["anchors"])
            B, N, code = box.shape
            cols = anchors.shape[1]
            sincos = bool(case.get("sincos", False))
            t = box.reshape(B * N, code)
            a = np.broadcast_to(anchors[None], (B, N, cols)).reshape(B * N, cols)
            vals, bnds = _exact_residual(t, a[:, 0:3], a[:, 3:6])
            ra = a[:, 6]
            period = None
            if sincos:
                s, c = t[:, 7] + np.sin(ra), t[:, 6] + np.cos(ra)
                es, ec = 2 * U * np.abs(np.sin(ra)) + U * np.abs(s), 2 * U * np.abs(np.cos(ra)) + U * np.abs(c)
                rg = np.arctan2(s, c)
                brg = (np.abs(c) * es + np.abs(s) * ec) / (c * c + s * s) + 2 * U * np.abs(rg)
                period = TWO_PI
            else:
                rg = t[:, 6] + ra
                brg = U * np.abs(rg)
            if case.get("dir") is not None:
                dirp = np.asarray(case["dir"], dtype=F)
                bins = dirp.shape[-1]
                label = argmax_rule(dirp.reshape(B * N, bins)).astype(np.float64)
                off, lim, per = float(F(case["dir_offset"])), float(F(case["dir_limit_offset"])), float(period_of(bins))
                v = rg - off
                brg = brg + 8 * U * (np.abs(rg) + abs(off) + TWO_PI)
                rg = (v - np.floor(v / per + lim) * per) + off + per * label
                period = per
            first = 8 if sincos else 7
            for k in range(cols - 7):
                v = t[:, first + k] + a[:, 7 + k]
                vals.append(v)
                bnds.append(U * np.abs(v))
            vals.insert(6, rg)
            bnds.insert(6, brg)
            val, bnd = _finish(vals, bnds, (B, N, cols))
            return val, bnd, period
        if case["kind"] == "point":
            box, pts = _d(case["box"]), _d(case["coords"])[:, 1:4]
            c = argmax_rule(np.asarray(case["cls"], dtype=F))
            if case.get("mean") is not None:
                vals, bnds = _exact_residual(box, pts, _d(case["mean"])[c])
            else:
                vals = [box[:, k] + pts[:, k] for k in range(3)] + [np.exp(box[:, k]) for k in (3, 4, 5)]
                bnds = [U * np.abs(v) for v in vals[:3]] + [2 * U * np.abs(v) for v in vals[3:]]
            rg = np.arctan2(box[:, 7], box[:, 6])
            vals.append(rg)
            bnds.append(2 * U * np.abs(rg))
            for k in range(8, box.shape[1]):
                vals.append(box[:, k])
                bnds.append(np.zeros(len(box)))
            val, bnd = _finish(vals, bnds, (len(box), box.shape[1] - 1))
            return val, bnd, TWO_PI
        rois, box = _d(case["rois"]), _d(case["box"])
        code = box.shape[-1]
        r, t = rois.reshape(-1, code), box.reshape(-1, code)
        vals, bnds = _exact_residual(t, np.zeros((len(r), 3)), r[:, 3:6])
        xg, yg, zg = vals[:3]
        ra = r[:, 6]
        c, s = np.cos(ra), np.sin(ra)
        xr, yr = (xg * c + yg * (-s)) + zg * 0.0, (xg * s + yg * c) + zg * 0.0
        zr = ((xg * 0.0) + (yg * 0.0)) + zg * 1.0
        x, y, z = xr + r[:, 0], yr + r[:, 1], zr + r[:, 2]
        bx = 7 * U * (np.abs(xg * c) + np.abs(yg * s)) + U * np.abs(xr) + U * np.abs(x)
        by = 7 * U * (np.abs(xg * s) + np.abs(yg * c)) + U * np.abs(yr) + U * np.abs(y)
        bz = bnds[2] + U * np.abs(z)
        vals[:3], bnds[:3] = [x, y, z], [bx, by, bz]
        for k in range(6, code):
            v = t[:, k] + r[:, k]
            vals.append(v)
            bnds.append(U * np.abs(v))
        val, bnd = _finish(vals, bnds, (len(r), code))
        return val, bnd, None


def bound_report(got, ex, who="the result"):
    """got against exact()'s triple -> (text of the elements beyond their bound, '' if none; the largest error / bound)"""
    val, bnd, period = ex
    got = np.asarray(got, dtype=F).astype(np.float64).reshape(val.shape)
    with np.errstate(all="ignore"):
        err = np.abs(got - val)
        if period is not None:
            d = np.abs(got[..., 6] - val[..., 6]) % period
            err[..., 6] = np.minimum(d, period - d)
        check = np.isfinite(bnd)
        bad = check & ~(err <= bnd)
        ratio = np.where(check & (bnd > 0), err / np.where(bnd > 0, bnd, 1.0), 0.0)
    lines = [f"{who}: element {idx} = {got[idx]!r}, exact {val[idx]!r}, bound {bnd[idx]!r}" for idx in zip(*np.nonzero(bad))][:10]
    return "\n".join(lines), float(ratio.max()) if ratio.size else 0.0


def bits(a):
    """the bit patterns of float32 values, every NaN as the one quiet NaN: which sign and payload an invalid operation leaves
    differs between processors and is no part of the contract; the sign of a zero and of an infinity is"""
    a = np.ascontiguousarray(a, dtype=F)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def report(got, want, what=""):
    """bit-for-bit comparison -> text naming the first differing elements, '' if none"""
    got, want = np.ascontiguousarray(got, dtype=F), np.ascontiguousarray(want, dtype=F)
    if got.shape != want.shape:
        return f"{what} shape {got.shape}, expected {want.shape}"
    diff = np.nonzero(bits(got) != bits(want))
    return "\n".join(f"{what} element {idx}: {got[idx]!r}, expected {want[idx]!r}" for idx in list(zip(*diff))[:10])


def pattern_report(got, want, what=""):
    """the places of NaN, +inf, -inf and zero -> text naming the first that differ, '' if none"""
    got, want = np.asarray(got, dtype=F), np.asarray(want, dtype=F).reshape(np.shape(got))
    lines = []
    for name, fn in (("NaN", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf), ("zero", lambda v: v == 0)):
        where = np.nonzero(fn(got) != fn(want))
        lines += [f"{what} {name} pattern differs at {idx}: {got[idx]!r}, expected {want[idx]!r}" for idx in list(zip(*where))[:5]]
    return "\n".join(lines)


def exact_columns(case):
    """the columns of the output that use + - * / floor only: compared with the recording bit for bit"""
    cols = restate_shape(case)[-1]
    extras = list(range(7, cols))
    if case["kind"] == "anchor":
        return [2] + ([] if case.get("sincos") else [6]) + extras
    if case["kind"] == "point":
        return [2] + extras
    return [2, 6] + extras


def restate_shape(case):
    if case["kind"] == "anchor":
        B, N, _ = np.shape(case["box"])
        return (B, N, np.shape(case["anchors"])[1])
    if case["kind"] == "point":
        N, code = np.shape(case["box"])
        return (N, code - 1)
    return tuple(np.shape(case["box"]))


# ---------------------------------------------------------------------------------------------------- inputs
def anchor_grid(nx=3, ny=2, sizes=((3.9, 1.6, 1.56), (0.8, 0.6, 1.73)), rotations=(0.0, 1.57), extra=0, seed=0):
    """(1, ny, nx, classes, rotations, 7 + extra) anchors as the reference's generator lays them out, one tensor per class ->
    the list of per-class arrays (1, ny, nx, 1, rotations, 7 + extra)"""
    rs = np.random.RandomState(seed)
    per_class = []
    for ci, size in enumerate(sizes):
        a = np.zeros((1, ny, nx, 1, len(rotations), 7 + extra), dtype=F)
        for iy in range(ny):
            for ix in range(nx):
                for ir, rot in enumerate(rotations):
                    a[0, iy, ix, 0, ir, :7] = [4.0 * ix + 2.0, 4.0 * iy - 2.0, -1.0 - 0.4 * ci, *size, rot]
                    if extra:
                        a[0, iy, ix, 0, ir, 7:] = rs.uniform(-1, 1, extra)
        per_class.append(a)
    return per_class


def flat_anchors(per_class):
    flat = np.concatenate(per_class, axis=-3) if len(per_class) > 1 else per_class[0]
    return np.ascontiguousarray(flat.reshape(-1, flat.shape[-1]), dtype=F)


def random_anchors(rs, N, extra=0):
    a = np.zeros((N, 7 + extra), dtype=F)
    a[:, 0:2] = rs.uniform(-70, 70, (N, 2))
    a[:, 2] = rs.uniform(-3, 1, N)
    a[:, 3:6] = rs.uniform(0.5, 5.0, (N, 3))
    a[:, 6] = rs.uniform(-3.2, 3.2, N)
    a[:, 7:] = rs.uniform(-2, 2, (N, extra))
    return a


def make_anchor(seed, B, N, extra=0, bins=2, sincos=False, dir_offset=0.78539, dir_limit_offset=0.0, anchors=None):
    rs = np.random.RandomState(seed)
    anchors = random_anchors(rs, N, extra) if anchors is None else np.asarray(anchors, dtype=F)
    code = 7 + extra + (1 if sincos else 0)
    box = rs.normal(0, 0.6, (B, N, code)).astype(F)
    case = dict(kind="anchor", box=box, anchors=anchors, dir=None, dir_offset=dir_offset, dir_limit_offset=dir_limit_offset,
                sincos=sincos)
    if bins:
        case["dir"] = rs.normal(0, 1, (B, N, bins)).astype(F)
    return case


def make_point(seed, N, K=3, extra=0, mean=True):
    rs = np.random.RandomState(seed)
    kitti = [[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]]
    coords = np.concatenate([rs.randint(0, 2, (N, 1)), rs.uniform(-40, 40, (N, 3))], axis=1).astype(F)
    box = rs.normal(0, 0.6, (N, 8 + extra)).astype(F)
    m = None
    if mean:
        m = np.asarray([kitti[k % 3] for k in range(K)], dtype=F) + F(0.01) * (np.arange(K, dtype=F)[:, None] // 3)
    return dict(kind="point", box=box, coords=coords, cls=rs.normal(0, 1, (N, K)).astype(F), mean=m)


def make_roi(seed, B, M, extra=0):
    rs = np.random.RandomState(seed)
    rois = random_anchors(rs, B * M, extra).reshape(B, M, 7 + extra)
    return dict(kind="roi", rois=rois, box=rs.normal(0, 0.5, (B * M, 7 + extra)).astype(F))


# ---------------------------------------------------------------------------------------------------- stand-in heads
def coder_stub(name, **attrs):
    """an object of a class named `name` with these attributes: the methods look at the coder's class name"""
    obj = type(name, (), {})()
    for k, v in attrs.items():
        setattr(obj, k, v)
    return obj


_coder = coder_stub


def bare_head(case, device=None, per_class=None):
    """a minimal stand-in head with the attributes the drop-in method of its kind reads, and the method's arguments
    -> (head, args): torch tensors on `device` (the CPU without)"""
    import torch
    from modest_amd.utils import box_decode as bd
    to = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device or "cpu")      # noqa: E731
    kind = case["kind"]
    if kind == "anchor":
        B, N, code = case["box"].shape
        sincos = bool(case.get("sincos", False))
        coder = _coder("ResidualCoder", code_size=code, encode_angle_by_sincos=sincos)
        anchors = [to(a) for a in per_class] if per_class is not None else to(case["anchors"])
        cfg = {}
        if case.get("dir") is not None:
            cfg = dict(DIR_OFFSET=case["dir_offset"], DIR_LIMIT_OFFSET=case["dir_limit_offset"], NUM_DIR_BINS=case["dir"].shape[-1])
        head = types.SimpleNamespace(anchors=anchors, box_coder=coder, model_cfg=cfg, use_multihead=False, num_class=2)
        head.generate_predicted_boxes = types.MethodType(bd.anchor_generate_predicted_boxes, head)
        cls = torch.zeros((B, N * 2), device=device or "cpu", requires_grad=True)
        return head, (B, cls, to(case["box"]).reshape(B, -1), None if case.get("dir") is None else to(case["dir"]).reshape(B, -1))
    if kind == "point":
        kw = {} if case.get("mean") is None else dict(mean_size=to(case["mean"]))
        coder = _coder("PointResidualCoder", code_size=case["box"].shape[1], use_mean_size=case.get("mean") is not None, **kw)
        head = types.SimpleNamespace(box_coder=coder, num_class=case["cls"].shape[1])
        head.generate_predicted_boxes = types.MethodType(bd.point_generate_predicted_boxes, head)
        coords = to(case["coords"])
        return head, (coords[:, 1:4], to(case["cls"]).requires_grad_(True), to(case["box"]))
    B, M, code = case["rois"].shape
    coder = _coder("ResidualCoder", code_size=code, encode_angle_by_sincos=False)
    head = types.SimpleNamespace(box_coder=coder)
    head.generate_predicted_boxes = types.MethodType(bd.roi_generate_predicted_boxes, head)
    cls = torch.zeros((B * M, 1), device=device or "cpu", requires_grad=True)
    return head, (B, to(case["rois"]), cls, to(case["box"]))


# ---------------------------------------------------------------------------------------------------- the recorded scenes
FIELDS = {"anchor": ("box", "anchors", "dir"), "point": ("box", "coords", "cls", "mean"), "roi": ("rois", "box")}


def scenes(rec):
    """the recorded file -> [(name, case, recorded boxes)]"""
    out = []
    for name in json.loads(str(rec["scenes"])):
        cfg = json.loads(str(rec[name + "_cfg"]))
        case = dict(cfg)
        for f in FIELDS[cfg["kind"]]:
            case[f] = rec[f"{name}_{f}"] if f"{name}_{f}" in rec else None
        out.append((name, case, rec[name + "_out"]))
    return out
