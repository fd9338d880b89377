"""numpy restatement of ``RoIHeadTemplate.get_loss`` and its gradients under the contract of DESIGN.md section 7q (not a test
module; tests/test_roi_loss_cpu.py, tests/test_gpu_roi_loss.py, tools/make_golden_roi_loss.py and tools/roi_loss_bench.py
import it).

``restate(inp, cfg)`` is the kernel's arithmetic: float32 in the written order, Python's scalars rounded to float32 first,
exp / log / log1p / sin / cos and the sigmoid as the double function of the float32 argument rounded once, sqrt and / as numpy
rounds them (correctly), the sums over the tree of section 7p (``anchor_loss_seq.tree_sum`` with one sample of R lanes).
``exact(inp, cfg, dec)`` evaluates the SAME statement (one function, ``_evaluate``, serves both) in float64 on the float32
inputs along every branch float32 took (``dec``: the -100 and 1e-12 clamps, the size clamps, the NaN replacement, the
smooth-L1 sides and signs, the side of the ``min``, its ties, the zero norms) and carries a running bound of what float32
can be off by (``anchor_loss_seq.Bounded``; ``sqrt``, the 3-term dot and sin / cos of bounded arguments are added here).

``faults`` (a set of names of ``FAULTS``) mis-states the contract on purpose: tests show that each changes a named case.

A config is a plain dict (what the fixture records as JSON):
    B, M (rois per sample), code, gt_cols (columns of gt_of_rois / gt_of_rois_src, >= code), corner, beta, cls_weight,
    reg_weight, corner_weight, code_weights, seed, labels ("cls": 1 / 0 / -1, "iou": soft float labels), label_dtype
    ("int32" | "int64" | "float32"), mask_dtype ("int32" | "int64"), samples (per sample "mixed" | "nofg" | "allfg" |
    "ignore"), fg (fraction of foreground rows in a mixed sample), specials (names of ``SPECIALS``)
"""
import json

import numpy as np

from anchor_loss_seq import (FUNC_U, U, Bounded, F, _abs, _exp, _is_b, _log, _log1p, _mask, _scale, _sigmoid, _total,  # noqa: F401
                             _trig, _where, error_over_bound, tree_sum)      # U and tree_sum: for the modules that import this one

OUTPUTS = ("table", "grad_cls", "grad_reg")
TABLE = ("rcnn_loss_cls", "rcnn_loss_reg", "rcnn_loss_corner", "rcnn_loss", "fg_sum", "cls_valid")
FAULTS = ("decode_clamps_roi", "flip_by_2pi", "tie_to_first", "reg_reports_corner", "zero_norm_divides", "corner_on_extra")
NO_DEAD_SHARE = "no_dead_share"      # one more fault, shown on the recorded non-finite scene: the smooth-L1 gradient without the
#                                      zero that where() hands the branch not taken
# the 8 corners of boxes_to_corners_3d: the template's signs, times 0.5
SIGN_X = (1, 1, -1, -1, 1, 1, -1, -1)
SIGN_Y = (1, -1, -1, 1, 1, -1, -1, 1)
SIGN_Z = (-1, -1, -1, -1, 1, 1, 1, 1)


# ---- what anchor_loss_seq lacks ----------------------------------------------------------------------------------------------
def _sqrt(x):
    if not _is_b(x):
        with np.errstate(invalid="ignore"):
            return np.sqrt(x)          # IEEE: correctly rounded
    with np.errstate(invalid="ignore"):
        v = np.sqrt(x.v)
        carried = np.where(x.e > 0, v - np.sqrt(np.maximum(x.v - x.e, 0.0)), 0.0)      # sqrt is concave: the lower side is the wider
        # a whole ulp, not half: the contract's root is correctly rounded, torch's vectorised CPU root is within one ulp of it
        return Bounded(v, carried + FUNC_U * (np.abs(v) + carried))


def dot3(ax, ay, az):
    """(ax ax + ay ay) + az az"""
    return (ax * ax + ay * ay) + az * az


def _stack(cols):
    if _is_b(cols[0]):
        return Bounded(np.stack([c.v for c in cols], axis=-1), np.stack([c.e for c in cols], axis=-1))
    return np.stack(cols, axis=-1)


def _sign(a):
    return np.sign(np.where(np.isnan(a), F(0), a)).astype(F)      # torch's sgn: 0 for a NaN


# ---- the statement -----------------------------------------------------------------------------------------------------------
def scalars32(cfg):
    """Python's scalars as they meet a float32 tensor"""
    beta = F(cfg["beta"])
    return dict(beta=beta, half_beta=F(0.5 * float(beta)), l1=float(beta) < 1e-5, w_cls=F(cfg["cls_weight"]),
                w_reg=F(cfg["reg_weight"]), w_corner=F(cfg["corner_weight"]), tiny=F(1e-5), pi=F(np.pi), two_pi=F(2 * np.pi),
                floor=F(-100.0), eps=F(1e-12))


def decisions(inp, cfg):
    """every branch float32 decides, from the float32 statement"""
    return _evaluate(inp, cfg, None)[1]


def _evaluate(inp, cfg, dec, faults=()):
    """dec None: float32 (the restatement) -> (outputs, decisions); else float64 with bounds along `dec`"""
    f32 = dec is None
    d = {} if f32 else dec
    S = scalars32(cfg)
    wrap = (lambda a: np.asarray(a, dtype=F)) if f32 else (lambda a: Bounded(np.asarray(a, dtype=F).astype(np.float64)))
    const = (lambda a: F(a)) if f32 else (lambda a: Bounded(np.float64(F(a))))
    zero = F(0) if f32 else 0.0

    def D(name, fn):
        """a branch: float32 decides it (and records it), float64 follows"""
        if f32:
            d[name] = fn()
        return d[name]

    def at_least(name, a, lo):
        return _where(D(name, lambda: a < lo), const(lo), a)

    code = int(cfg["code"])
    labels = np.asarray(inp["labels"])
    R = labels.shape[0]
    with np.errstate(invalid="ignore"):
        valid = labels >= 0
    fg = np.asarray(inp["mask"]) > 0
    n_fg, n_valid = int(fg.sum()), int(valid.sum())
    den_v, den_f = const(max(n_valid, 1)), const(max(n_fg, 1))
    with_corner = bool(cfg["corner"]) and n_fg > 0
    out = {}
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        # ---- classification
        x, t = wrap(inp["cls"]), wrap(labels.astype(F))
        s = _sigmoid(x)
        la = at_least("floor_a", _log1p(-s), S["floor"])
        lb = at_least("floor_b", _log(s), S["floor"])
        lane_cls = _mask((t - const(1)) * la - t * lb, valid)
        sum_cls = _total(lane_cls.reshape(1, R) if f32 else Bounded(lane_cls.v.reshape(1, R), lane_cls.e.reshape(1, R)), 1, R, 0)
        g0 = const(S["w_cls"]) / den_v
        oms = const(1) - s
        g_s = (g0 * (s - t)) / at_least("eps", oms * s, S["eps"])
        out["grad_cls"] = _mask((g_s * oms) * s, valid)
        # ---- smooth L1 of the encoding
        p, g, roi = wrap(inp["reg"]), wrap(np.asarray(inp["gt"])[:, :code]), wrap(inp["rois"])
        cw = wrap(inp["cw"])
        col = lambda a, k: a[:, k]      # noqa: E731
        ca, cb, cz = (at_least(f"roi_size{k}", col(roi, k), S["tiny"]) for k in (3, 4, 5))
        ga, gb, gz = (at_least(f"gt_size{k}", col(g, k), S["tiny"]) for k in (3, 4, 5))
        diag_c = _sqrt(ca * ca + cb * cb)
        tg = [col(g, 0) / diag_c, col(g, 1) / diag_c, col(g, 2) / cz, _log(ga / ca), _log(gb / cb), _log(gz / cz), col(g, 6)]
        tg += [col(g, k) - col(roi, k) for k in range(7, code)]
        tg = _stack(tg)
        replaced = D("replaced", lambda: np.isnan(tg))
        tg = _where(replaced, p, tg)
        diff = (p - tg) * (cw[None, :] if f32 else Bounded(cw.v[None, :], cw.e[None, :]))
        nrm = _abs(diff)
        quad = D("quad", lambda: (nrm < S["beta"]) & (not S["l1"]))
        sign_d = D("sign_d", lambda: _sign(diff))
        beta, half = const(S["beta"]), const(S["half_beta"])
        v = nrm if S["l1"] else _where(quad, (const(0.5) * (nrm * nrm)) / beta, nrm - half)
        lane_reg = zero
        for k in range(code):
            lane_reg = lane_reg + v[:, k]
        lane_reg = _mask(lane_reg, fg)
        sum_reg = _total(lane_reg.reshape(1, R) if f32 else Bounded(lane_reg.v.reshape(1, R), lane_reg.e.reshape(1, R)), 1, R, code)
        gl = const(S["w_reg"]) / den_f
        if S["l1"]:
            g_n = gl * (np.ones(nrm.shape, dtype=F) if f32 else Bounded(np.ones(nrm.v.shape)))
        else:
            # where() hands the branch not taken a zero and pow's backward multiplies it by 2 n: +0 for a finite n (gl + 0 is
            # gl, exactly: a float32 decision, no rounding), a NaN for an infinite or NaN one
            dead_nan = D("dead_nan", lambda: np.isnan(((F(0) / beta) * F(0.5)) * (F(2) * nrm)) & (NO_DEAD_SHARE not in faults))
            g_n = _where(quad, ((gl / beta) * const(0.5)) * (const(2) * nrm), _where(dead_nan, const(np.nan), gl))
        cwr = cw[None, :] if f32 else Bounded(cw.v[None, :], cw.e[None, :])
        g_d = _scale(g_n, sign_d) * cwr
        g_in = _where(replaced, g_d + (-g_d), g_d)
        # ---- the corner term
        lane_corner = None
        gc = None
        if with_corner:
            q = wrap(np.asarray(inp["src"])[:, :7])
            rdx, rdy, rdz, rh = col(roi, 3), col(roi, 4), col(roi, 5), col(roi, 6)
            if "decode_clamps_roi" in faults:
                rdx, rdy, rdz = ca, cb, cz
            diag = _sqrt(rdx * rdx + rdy * rdy)
            e3, e4, e5 = _exp(col(p, 3)), _exp(col(p, 4)), _exp(col(p, 5))
            x0, y0, z0 = col(p, 0) * diag, col(p, 1) * diag, col(p, 2) * rdz
            dx, dy, dz = e3 * rdx, e4 * rdy, e5 * rdz
            hp = col(p, 6) + rh
            cr, sr = _trig(rh, np.cos), _trig(rh, np.sin)
            cx, cy, cz_ = (x0 * cr - y0 * sr) + col(roi, 0), (x0 * sr + y0 * cr) + col(roi, 1), z0 + col(roi, 2)
            cp, sp = _trig(hp, np.cos), _trig(hp, np.sin)
            qx, qy, qz, qdx, qdy, qdz, qh = (col(q, k) for k in range(7))
            cg, sg = _trig(qh, np.cos), _trig(qh, np.sin)
            qf = qh + const(S["two_pi"] if "flip_by_2pi" in faults else S["pi"])
            cf, sf = _trig(qf, np.cos), _trig(qf, np.sin)
            g_c = (const(S["w_corner"]) / const(n_fg)) / const(8)
            csum = gcx = gcy = gcz = gdx = gdy = gdz = G00 = G01 = G10 = G11 = zero
            for k in range(8):
                ax, ay, az = const(0.5 * SIGN_X[k]), const(0.5 * SIGN_Y[k]), const(0.5 * SIGN_Z[k])
                lx, ly, lz = dx * ax, dy * ay, dz * az
                PX, PY, PZ = (lx * cp - ly * sp) + cx, (lx * sp + ly * cp) + cy, lz + cz_
                mx, my, mz = qdx * ax, qdy * ay, qdz * az
                GX, GY, GZ = (mx * cg - my * sg) + qx, (mx * sg + my * cg) + qy, mz + qz
                FX, FY = (mx * cf - my * sf) + qx, (mx * sf + my * cf) + qy
                ax_, ay_, az_ = PX - GX, PY - GY, PZ - GZ
                bx_, by_ = PX - FX, PY - FY
                na, nb = _sqrt(dot3(ax_, ay_, az_)), _sqrt(dot3(bx_, by_, az_))
                # a squared distance past float32's range is an infinite norm in float32: a branch float32 decides
                na = _where(D(f"na_inf{k}", lambda: np.isposinf(na)), const(np.inf), na)
                nb = _where(D(f"nb_inf{k}", lambda: np.isposinf(nb)), const(np.inf), nb)
                second = D(f"second{k}", lambda: nb < na)
                m = _where(second, nb, na)
                cquad = D(f"cquad{k}", lambda: m < F(1))
                csum = csum + _where(cquad, const(0.5) * (m * m), m - const(0.5))
                # the corner distances go through the same smooth L1 (beta = 1): the same zero from where() times 2 m
                cdead = D(f"cdead{k}", lambda: np.isnan(F(0) * (F(2) * m)) & (NO_DEAD_SHARE not in faults))
                g_m = _scale(_where(cquad, (g_c * const(0.5)) * (const(2) * m), _where(cdead, const(np.nan), g_c)),
                             D(f"sign_m{k}", lambda: _sign(m)))
                tie = D(f"tie{k}", lambda: na == nb)
                g_h = g_m if "tie_to_first" in faults else _where(tie, g_m / const(2), g_m)
                first_less = D(f"first_less{k}", lambda: na < nb)
                g_a = _mask(g_h, ~second)
                g_b = _mask(g_h, ~(first_less | tie) if "tie_to_first" in faults else ~first_less)
                za, zb = D(f"zero_a{k}", lambda: na == 0), D(f"zero_b{k}", lambda: nb == 0)
                if "zero_norm_divides" in faults:
                    za = zb = np.zeros_like(za)
                uax, uay, uaz = (_mask(c / na, ~za) for c in (ax_, ay_, az_))
                ubx, uby, ubz = (_mask(c / nb, ~zb) for c in (bx_, by_, az_))
                gPX, gPY, gPZ = g_a * uax + g_b * ubx, g_a * uay + g_b * uby, g_a * uaz + g_b * ubz
                gcx, gcy, gcz = gcx + gPX, gcy + gPY, gcz + gPZ
                G00, G11, G01, G10 = G00 + lx * gPX, G11 + ly * gPY, G01 + lx * gPY, G10 + ly * gPX
                glx, gly = gPX * cp + gPY * sp, gPY * cp - gPX * sp
                gdx, gdy, gdz = gdx + glx * ax, gdy + gly * ay, gdz + gPZ * az
            lane_corner = _mask(csum / const(8), fg)
            g_cos, g_sin = G00 + G11, G01 - G10
            gx0, gy0 = gcx * cr + gcy * sr, gcy * cr - gcx * sr
            gc = [gx0 * diag, gy0 * diag, gcz * rdz, (gdx * rdx) * e3, (gdy * rdy) * e4, (gdz * rdz) * e5, g_sin * cp - g_cos * sp]
        cols = []
        for k in range(code):
            share = gc[k] if gc is not None and k < 7 else (gc[6] if gc is not None and "corner_on_extra" in faults else None)
            cols.append(g_in[:, k] if share is None else g_in[:, k] + share)
        out["grad_reg"] = _mask(_stack(cols), fg[:, None])
        # ---- the table
        cls = (sum_cls / den_v) * const(S["w_cls"])
        reg = (sum_reg / den_f) * const(S["w_reg"])
        if with_corner:
            sum_corner = _total(lane_corner.reshape(1, R) if f32 else Bounded(lane_corner.v.reshape(1, R), lane_corner.e.reshape(1, R)),
                                1, R, 8)
            corner = (sum_corner / const(n_fg)) * const(S["w_corner"])
            loss = cls + (reg + corner)
        else:
            corner = const(0)
            loss = cls + reg
        if "reg_reports_corner" in faults and with_corner:
            reg = reg + corner
        vals = (cls, reg, corner, loss, const(n_fg), const(n_valid))
        if f32:
            out["table"] = np.array(vals, dtype=F)
        else:
            out["table"] = Bounded(np.array([float(q.v) for q in vals]), np.array([float(q.e) for q in vals]))
    if f32:
        out = {k: np.asarray(v, dtype=F) for k, v in out.items()}
    return out, d


def restate(inp, cfg, faults=()):
    """the kernel's float32 results: {"table" (6), "grad_cls" (R), "grad_reg" (R, code)}"""
    return _evaluate(inp, cfg, None, faults)[0]


def exact(inp, cfg, dec=None):
    """the same statement in float64 along float32's branches -> {name: (value float64, bound float64)}"""
    out = _evaluate(inp, cfg, decisions(inp, cfg) if dec is None else dec)[0]
    return {k: (v.v, v.e) for k, v in out.items()}


# ---- comparisons -------------------------------------------------------------------------------------------------------------
def _place(name, idx):
    if name == "table":
        return TABLE[int(idx[0])]
    return "(row %d)" % int(idx[0]) if len(idx) == 1 else "(row %d, column %d)" % tuple(int(v) for v in idx)


def bound_report(got, ex, what="ours"):
    """every element of every output against exact(): |got - value| <= bound, a NaN exactly where the value is one.
    -> (text naming the row and column of each output's worst miss, or "", {output: largest error / bound})"""
    lines, ratios = [], {}
    for name in OUTPUTS:
        v, e = ex[name]
        g = np.asarray(got[name], dtype=np.float64)
        if g.shape != v.shape:
            lines.append(f"{what} {name}: shape {g.shape}, expected {v.shape}")
            continue
        ratio, nan_v, nan_g = error_over_bound(g, v, e)
        ratios[name] = float(ratio.max()) if ratio.size else 0.0
        bad = (ratio > 1.0) | (nan_v != nan_g)
        if bad.any():
            idx = np.unravel_index(int(np.argmax(np.where(nan_v != nan_g, np.inf, ratio))), g.shape)
            lines.append(f"{what} {name}: {int(bad.sum())} of {g.size} elements outside the bound, the worst at {_place(name, idx)}: "
                         f"{got[name][idx]!r} against {v[idx]!r} +- {e[idx]!r}")
    return "\n".join(lines), ratios


def zero_report(a, b, what="the zero pattern"):
    """the gradient elements that are == 0 in one and not in the other (a NaN is not 0)"""
    lines = []
    for name in OUTPUTS[1:]:
        za, zb = np.asarray(a[name]) == 0, np.asarray(b[name]) == 0
        if za.shape != zb.shape or (za != zb).any():
            idx = np.argwhere(za != zb)[0] if za.shape == zb.shape else (0,)
            lines.append(f"{what} of {name} differs at {_place(name, idx)}")
    return "\n".join(lines)


def report(got, want, what="the device"):
    """bit for bit: every element of every output, NaNs included -> text naming the row and column, or "" """
    lines = []
    for name in OUTPUTS:
        g, w = np.asarray(got[name], dtype=F), np.asarray(want[name], dtype=F)
        if g.shape != w.shape:
            lines.append(f"{what} {name}: shape {g.shape}, expected {w.shape}")
            continue
        bad = g.view(np.uint32) != w.view(np.uint32)
        bad &= ~(np.isnan(g) & np.isnan(w))
        bad &= ~((g == 0) & (w == 0))     # the sign of a zero carries nothing
        if bad.any():
            idx = np.argwhere(bad)[0]
            lines.append(f"{what} {name}: {int(bad.sum())} of {g.size} elements differ, the first at {_place(name, idx)}: "
                         f"{g[tuple(idx)]!r} ({g.view(np.uint32)[tuple(idx)]:#010x}) against {w[tuple(idx)]!r} "
                         f"({w.view(np.uint32)[tuple(idx)]:#010x})")
    return "\n".join(lines)


# ---- seeded inputs -----------------------------------------------------------------------------------------------------------
def base_cfg(**kw):
    cfg = dict(B=2, M=64, code=7, gt_cols=None, corner=True, beta=1.0 / 9.0, cls_weight=1.0, reg_weight=1.0, corner_weight=1.0,
               code_weights=None, seed=1, labels="cls", label_dtype=None, mask_dtype="int64", samples=None, fg=0.3, specials=[])
    cfg.update(kw)
    if cfg["code_weights"] is None:
        cfg["code_weights"] = [1.0] * cfg["code"]
    if cfg["samples"] is None:
        cfg["samples"] = ["mixed"] * cfg["B"]
    if cfg["gt_cols"] is None:
        cfg["gt_cols"] = cfg["code"]
    if cfg["label_dtype"] is None:
        cfg["label_dtype"] = "int64" if cfg["labels"] == "cls" else "float32"
    assert len(cfg["samples"]) == cfg["B"] and len(cfg["code_weights"]) == cfg["code"] and cfg["gt_cols"] >= cfg["code"]
    assert cfg["labels"] == "cls" or cfg["label_dtype"] == "float32"
    return cfg


def _sp_logits(inp, cfg, rows, recorded=False):
    """logits of exactly +0 and -0, +-30 and +-100 against labels of exactly 0, 1 and (soft labels) 0.5.  `recorded`: -80 in
    place of -100 where the label is above 0 -- there a float32 sigmoid evaluated as 1 / (1 + exp(-x)) is exactly 0 (exp(100)
    overflows float32) and hands on a gradient of exactly 0, where the contract's sigmoid is 3.8e-44 and the gradient -2.9e-34
    (DESIGN.md section 7q): the zero patterns differ, so that point is a case against the restatement, not a recorded one"""
    vals = np.array([0.0, -0.0, 30.0, -30.0, 100.0, -100.0], dtype=F)
    soft = inp["labels"].dtype == F
    targets = (0.0, 1.0, 0.5) if soft else (0, 1)
    r = 0
    for tv in targets:
        for v in vals:
            inp["cls"][rows[r] + 1] = F(-80.0) if recorded and tv > 0 and v == F(-100.0) else v      # a row that is not foreground
            inp["labels"][rows[r] + 1] = tv
            r += 1


def _sp_logits_recorded(inp, cfg, rows):
    _sp_logits(inp, cfg, rows, recorded=True)


def _sp_beta(inp, cfg, rows):
    """|d| == beta exactly (the linear side) and d == 0 (gradient 0), in column 6, whose target is the gt's heading itself"""
    a, b = rows[0], rows[1]
    inp["gt"][a, 6] = F(0)
    inp["reg"][a, 6] = F(cfg["beta"]) / F(cfg["code_weights"][6])
    inp["reg"][b, 6] = inp["gt"][b, 6]


def _sp_zero_distance(inp, cfg, rows):
    """a prediction that decodes to its gt exactly: every corner at distance 0 from the gt (the norm hands on 0)"""
    r = rows[2]
    inp["rois"][r, :7] = np.array([8, -4, 1, 3, 4, 2, 0], dtype=F)      # diagonal 5, heading 0: cos 1, sin 0
    inp["reg"][r, :7] = 0
    inp["src"][r, :7] = inp["rois"][r, :7]


def _sp_sizes(inp, cfg, rows):
    """a gt size <= 0 (clamped at 1e-5 by the encoding) and a roi size of 0 (clamped there, not in the decode)"""
    inp["gt"][rows[3], 3] = F(-1.0)
    inp["gt"][rows[3], 5] = F(0.0)
    inp["rois"][rows[4], 4] = F(0.0)


def _sp_nan(inp, cfg, rows):
    inp["gt"][rows[5], 1] = F(np.nan)


def _sp_headings(inp, cfg, rows):
    """headings beyond +-pi in the roi, the prediction and the gt"""
    r = rows[6]
    inp["rois"][r, 6], inp["reg"][r, 6], inp["src"][r, 6], inp["gt"][r, 6] = F(4.0), F(2.5), F(-5.0), F(3.5)


def _sp_tie(inp, cfg, rows):
    """four of the 8 corners exactly as far from the gt as from the flipped gt, in different directions.  The gt is 8 x 4 at the
    origin with heading 0: its corners are (+-4, +-2), and those of the flipped gt their negatives exactly (4 sin(pi_f32) is
    below half an ulp of 2, 2 sin(pi_f32) below half an ulp of 4).  The prediction is centred at (1, -2) with half sizes
    (0.5, -1) (a roi of negative width, which the decode does not clamp), so its corners 0 and 2 of either level are (1.5, -3)
    and (0.5, -1), on the bisector of (4, 2) and (-4, -2): squared distances 6.25 + 25 = 30.25 + 1 and 20.25 + 1 = 12.25 + 9.
    The two tied corners lie at different distances, so handing the tie whole to one side changes the centre's gradient"""
    r = rows[7]
    inp["rois"][r, :7] = np.array([1, -2, 1, 1, -2, 2, 0], dtype=F)
    inp["reg"][r, :7] = np.array([0, 0, -0.5, 0, 0, -0.25, 0], dtype=F)
    inp["src"][r, :7] = np.array([0, 0, 1, 8, 4, 2, 0], dtype=F)


def _sp_mask_values(inp, cfg, rows):
    """mask values other than 0 / 1: 2 is foreground, -1 is not"""
    inp["mask"][rows[8]] = 2
    inp["mask"][rows[9]] = -1


def _sp_nonfinite(inp, cfg, rows):
    """on foreground rows: NaN, +inf, -inf in rcnn_reg's column 1 and in its column 6; inf in a gt's column 1 and in another
    gt's column 6 (the encoded targets are those infinities)"""
    for j, v in enumerate((np.nan, np.inf, -np.inf)):
        inp["reg"][rows[10 + j], 1] = F(v)
        inp["reg"][rows[13 + j], 6] = F(v)
    inp["gt"][rows[16], 1] = F(np.inf)
    inp["gt"][rows[17], 6] = F(np.inf)


def _sp_inf_reg(inp, cfg, rows):
    """infinities alone: rcnn_loss_reg is +inf, not a NaN"""
    inp["reg"][rows[10], 1], inp["reg"][rows[11], 2], inp["gt"][rows[12], 0] = F(np.inf), F(-np.inf), F(np.inf)


def _sp_nonfinite_cls(inp, cfg, rows, vals=(np.inf, -np.inf)):
    """inf and -inf in rcnn_cls, on rows that are not foreground, against labels of 0 and 1"""
    for j, v in enumerate(vals * 2):
        inp["cls"][rows[20 + j] + 1] = F(v)
        inp["labels"][rows[20 + j] + 1] = j // len(vals)


def _sp_nan_cls(inp, cfg, rows):
    """a NaN in rcnn_cls: the reference's binary_cross_entropy raises on the CPU (its input is not within [0, 1]), so this
    is a case against the restatement, not a recorded one"""
    _sp_nonfinite_cls(inp, cfg, rows, vals=(np.nan,))


def _sp_extreme(inp, cfg, rows, recorded=False):
    """finite and huge: logits +-88.9 (exp(88.9) is past float32) and +-1e30 against labels 0 and 1, rcnn_reg values 1e20 and
    -1e30, a gt centre of 1e20, and (without the corner term, where column 6 is a plain difference) headings 1e10 in a gt
    and -3e38 in rcnn_reg -- one value of that size, so that no float32 sum overflows where the exact one does not.
    `recorded`: without -88.9 against label 1, the point of ``_sp_logits`` (a float32 sigmoid evaluated as 1 / (1 + exp(-x))
    is exactly 0 there, the contract's is 2.4e-39)"""
    for j, v in enumerate((88.9, -88.9, 1e30, -1e30) * 2):
        if not (recorded and j == 5):
            inp["cls"][rows[20 + j] + 1] = F(v)
        inp["labels"][rows[20 + j] + 1] = j // 4
    inp["reg"][rows[10], 0] = F(1e20)
    inp["reg"][rows[11], 2] = F(-1e30)
    inp["gt"][rows[16], 0] = F(1e20)
    if not cfg["corner"]:
        inp["reg"][rows[13], 6] = F(-3e38)
        inp["gt"][rows[14], 6] = F(1e10)


def _sp_extreme_recorded(inp, cfg, rows):
    _sp_extreme(inp, cfg, rows, recorded=True)


SPECIALS = {"nonfinite": _sp_nonfinite, "inf_reg": _sp_inf_reg, "nonfinite_cls": _sp_nonfinite_cls, "nan_cls": _sp_nan_cls, "extreme": _sp_extreme, "extreme_recorded": _sp_extreme_recorded,
            "logits": _sp_logits, "logits_recorded": _sp_logits_recorded, "beta": _sp_beta, "zero_distance": _sp_zero_distance, "sizes": _sp_sizes, "nan": _sp_nan,
            "headings": _sp_headings, "tie": _sp_tie, "mask_values": _sp_mask_values}
EDGE = ["logits", "beta", "zero_distance", "sizes", "nan", "headings"]      # the `edge` case
EDGE_RECORDED = ["logits_recorded"] + EDGE[1:]                              # what the recorded `edge` scene holds


def make_inputs(cfg):
    """{"cls" (R), "reg" (R, code), "labels" (R), "mask" (R), "gt" (R, gt_cols), "src" (R, gt_cols), "rois" (R, code), "cw" (code)}
    from the config's seed, R = B * M"""
    rs = np.random.RandomState(int(cfg["seed"]))
    B, M, code, cols = (int(cfg[k]) for k in ("B", "M", "code", "gt_cols"))
    R = B * M
    fg = np.zeros((B, M), dtype=bool)
    ignore = np.zeros((B, M), dtype=bool)
    for b, mode in enumerate(cfg["samples"]):
        draw = rs.uniform(size=M)
        if mode == "mixed":
            fg[b] = draw < cfg["fg"]
            ignore[b] = draw > 0.8
        elif mode == "allfg":
            fg[b] = True
        elif mode == "ignore":
            ignore[b] = True
        elif mode != "nofg":
            raise ValueError(mode)
    fg, ignore = fg.reshape(R), ignore.reshape(R)
    if cfg["specials"]:
        assert R >= 120, "the specials sit in the first 120 rows"
        fg[:120:3] = True
        fg[1:120:3] = False
        ignore[:120] = False
    if cfg["labels"] == "cls":
        labels = np.where(fg, 1, np.where(ignore, -1, 0)).astype(cfg["label_dtype"])
    else:
        iou = rs.uniform(0.0, 1.0, size=R)
        labels = np.where(fg, 0.55 + 0.45 * iou, np.where(ignore, 0.0, 0.5 * iou)).astype(F)
    rois = np.zeros((R, code), dtype=F)
    rois[:, :3] = rs.uniform(-40, 40, size=(R, 3))
    rois[:, 3:6] = np.array([3.9, 1.6, 1.56]) * rs.uniform(0.8, 1.2, size=(R, 3))
    rois[:, 6] = rs.uniform(-np.pi, np.pi, size=R)
    rois[:, 7:] = rs.standard_normal((R, code - 7))
    gt = np.zeros((R, cols), dtype=F)
    gt[:, :3] = rs.standard_normal((R, 3)) * 0.4
    gt[:, 3:6] = rois[:, 3:6] * rs.uniform(0.8, 1.25, size=(R, 3))
    gt[:, 6] = rs.uniform(-np.pi / 2, np.pi / 2, size=R)
    gt[:, 7:] = rs.standard_normal((R, cols - 7))          # with gt_cols > code the last columns are what the kernel must not read
    src = gt.copy()
    src[:, :3] = rois[:, :3] + rs.standard_normal((R, 3)) * 0.4
    src[:, 6] = rois[:, 6] + gt[:, 6]
    inp = {"cls": (rs.standard_normal(R) * 2).astype(F), "reg": (rs.standard_normal((R, code)) * 0.3).astype(F),
           "labels": labels, "mask": fg.astype(cfg["mask_dtype"]), "gt": gt, "src": src.astype(F), "rois": rois,
           "cw": np.asarray(cfg["code_weights"], dtype=F)}
    if cfg["specials"]:
        rows = np.arange(0, 120, 3)
        for name in cfg["specials"]:
            SPECIALS[name](inp, cfg, rows)
    return inp


def edge_scene_cfgs():
    """the second config set: what tools/make_golden_roi_loss.py records into tests/golden/roi_loss_edges.npz and
    tests/roi_loss_cases.py runs as cases: non-finite and huge values on foreground rows, with and without the corner term"""
    c = base_cfg
    return {"nonfinite": c(B=1, M=130, seed=51, corner=False, specials=["nonfinite", "nonfinite_cls"]),
            "nonfinite_inf": c(B=1, M=130, seed=52, corner=False, specials=["inf_reg"]),
            "nonfinite_l1": c(B=1, M=130, seed=53, corner=False, beta=0.0, specials=["nonfinite"]),
            "nonfinite_corner": c(B=1, M=130, seed=54, specials=["nonfinite"]),
            "extreme": c(B=1, M=130, seed=55, corner=False, specials=["extreme_recorded"]),
            "extreme_corner": c(B=1, M=130, seed=56, specials=["extreme_recorded"])}


# ---- the fixture -------------------------------------------------------------------------------------------------------------
def scenes(gold):
    """[(name, cfg)] of tests/golden/roi_loss.npz"""
    return [(n, json.loads(str(gold[f"{n}/cfg"]))) for n in json.loads(str(gold["scenes"]))]


def recorded(gold, name):
    return {k: gold[f"{name}/{k}"] for k in OUTPUTS}


# ---- a bare head: the attributes get_loss reads ---------------------------------------------------------------------------
class Cfg(dict):
    """a dict with attribute access (what the reference's EasyDict gives its classes)"""
    __getattr__ = dict.__getitem__


def loss_stub(name, **attrs):
    """an object whose class carries a reference class's name and the attributes get_loss reads from it"""
    obj = type(name, (), {})()
    for k, v in attrs.items():
        setattr(obj, k, v)
    return obj


def model_cfg(cfg, **kw):
    loss = Cfg(CLS_LOSS="BinaryCrossEntropy", REG_LOSS="smooth-l1", CORNER_LOSS_REGULARIZATION=bool(cfg["corner"]),
               LOSS_WEIGHTS=dict(rcnn_cls_weight=cfg["cls_weight"], rcnn_reg_weight=cfg["reg_weight"],
                                 rcnn_corner_weight=cfg["corner_weight"], code_weights=list(cfg["code_weights"])))
    loss.update(kw)
    return Cfg(LOSS_CONFIG=loss)


def bare_head(cfg, inp, device="cpu", head_class=None, requires_grad=True):
    """-> (head, preds): an object with model_cfg, box_coder, reg_loss_func and forward_ret_dict as RoIHeadTemplate holds them
    after assign_targets and the head's forward; preds the leaf tensors {"cls" (R, 1), "reg" (R, code)}"""
    import torch
    head = (head_class or type("Head", (), {}))()
    head.model_cfg = model_cfg(cfg)
    B, M, code = int(cfg["B"]), int(cfg["M"]), int(cfg["code"])
    head.box_coder = loss_stub("ResidualCoder", code_size=code, encode_angle_by_sincos=False)
    cw = torch.from_numpy(np.asarray(inp["cw"], dtype=F).copy()).to(device)
    head.reg_loss_func = loss_stub("WeightedSmoothL1Loss", beta=cfg["beta"], code_weights=cw)
    preds = {"cls": torch.from_numpy(inp["cls"].copy()).view(-1, 1).to(device).requires_grad_(requires_grad),
             "reg": torch.from_numpy(inp["reg"].copy()).to(device).requires_grad_(requires_grad)}
    dev = lambda a, *shape: torch.from_numpy(np.ascontiguousarray(a).copy()).view(*shape).to(device)      # noqa: E731
    head.forward_ret_dict = dict(rcnn_cls=preds["cls"], rcnn_reg=preds["reg"], rcnn_cls_labels=dev(inp["labels"], B, M),
                                 reg_valid_mask=dev(inp["mask"], B, M), gt_of_rois=dev(inp["gt"], B, M, -1),
                                 gt_of_rois_src=dev(inp["src"], B, M, -1), rois=dev(inp["rois"], B, M, code))
    return head, preds
