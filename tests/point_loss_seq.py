"""numpy restatement of the point heads' ``get_loss`` and its gradients under the contract of DESIGN.md section 7r (not a test
module; tests/test_point_loss_cpu.py, tests/test_gpu_point_loss.py, tools/make_golden_point_loss.py and
tools/point_loss_bench.py import it).

``restate(inp, cfg)`` is the kernel's arithmetic: float32 in the written order, Python's scalars rounded to float32 first,
exp / log / log1p and the sigmoid as the double function of the float32 argument rounded once, / as numpy rounds it
(correctly), the sums over the tree of section 7p (``anchor_loss_seq.tree_sum`` with one sample of all B * N lanes: the
stacked batch is one array).  ``exact(inp, cfg, dec)`` evaluates the SAME statement (one function, ``_evaluate``, serves both)
in float64 on the float32 inputs along every branch float32 took (``dec``: the -100 and 1e-12 clamps, the NaN replacement,
the smooth-L1 sides and signs) and carries a running bound of what float32 can be off by (``anchor_loss_seq.Bounded``).

``faults`` (a set of names of ``FAULTS``) mis-states the contract on purpose: tests show that each changes a named case.

A config is a plain dict (what the fixture records as JSON):
    head ("PointHeadBox": cls + box | "PointIntraPartOffsetHead": cls + part, + box with box_layers | "PointHeadSimple": cls),
    box_layers, B, N (points per sample; the stacked batch has B * N rows), num_class, code, beta, cls_weight, part_weight,
    box_weight, code_weights, seed, samples (per sample "mixed" | "none" | "all" | "ignore"), pos (fraction of positives in a
    mixed sample), label_max (labels are drawn from 1 .. label_max), int64 (labels), specials (names of ``SPECIALS``)
"""
import json

import numpy as np

from anchor_loss_seq import (FUNC_U, U, Bounded, F, _abs, _exp, _is_b, _log, _log1p, _mask, _scale, _sigmoid, _total,  # noqa: F401
                             _where, error_over_bound, tree_depth, tree_sum)      # U, tree_sum, tree_depth: for the modules that import this one

OUTPUTS = ("table", "grad_cls", "grad_part", "grad_box")
TABLE = ("point_loss_cls", "point_loss_part", "point_loss_box", "point_loss", "point_pos_num")
FAULTS = ("count_per_sample", "part_divisor_without_3", "ignored_rows_weighted", "target_at_label", "box_for_background",
          "part_grad_off_positives")
NO_DEAD_SHARE = "no_dead_share"      # one more fault, shown on the recorded non-finite scene: the smooth-L1 gradient without the
#                                      zero that where() hands the branch not taken
ALPHA, GAMMA = 0.25, 2.0
HEADS = ("PointHeadBox", "PointIntraPartOffsetHead", "PointHeadSimple")


def terms_of(cfg):
    """the terms of a head: ("cls",) + ("part",) + ("box",)"""
    head = cfg["head"]
    if head == "PointHeadSimple":
        return ("cls",)
    if head == "PointHeadBox":
        return ("cls", "box")
    assert head == "PointIntraPartOffsetHead", head
    return ("cls", "part", "box") if cfg["box_layers"] else ("cls", "part")


def _sign(a):
    return np.sign(np.where(np.isnan(a), F(0), a)).astype(F)      # torch's sgn: 0 for a NaN


def _col(a, k):
    return a[:, k]


# ---- the statement -----------------------------------------------------------------------------------------------------------
def scalars32(cfg):
    """Python's scalars as they meet a float32 tensor"""
    beta = F(cfg["beta"])
    return dict(beta=beta, half_beta=F(0.5 * float(beta)), l1=float(beta) < 1e-5, w_cls=F(cfg["cls_weight"]),
                w_part=F(cfg["part_weight"]), w_box=F(cfg["box_weight"]), floor=F(-100.0), eps=F(1e-12))


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

    def rows(x):
        return x.reshape(1, -1) if f32 else Bounded(x.v.reshape(1, -1), x.e.reshape(1, -1))

    terms = terms_of(cfg)
    B, N, C, code = int(cfg["B"]), int(cfg["N"]), int(cfg["num_class"]), int(cfg["code"])
    R = B * N
    labels = np.asarray(inp["labels"]).astype(np.int64).reshape(R)
    pos, cared = labels > 0, labels >= 0
    P = int(pos.sum())
    out = {}
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        if "count_per_sample" in faults:
            den = np.repeat(np.maximum(pos.reshape(B, N).sum(axis=1), 1).astype(F), N)
        else:
            den = np.full(R, F(max(P, 1)))
        w = F(1) / den if f32 else Bounded(1.0 / den.astype(np.float64), U / den.astype(np.float64))      # one division
        wc = w if "ignored_rows_weighted" in faults else _mask(w, cared)
        box_rows = cared if "box_for_background" in faults else pos
        wr = _mask(w, box_rows)
        # ---- classification
        x = wrap(np.asarray(inp["cls"]).reshape(R, C))
        x32 = np.asarray(inp["cls"], dtype=F).reshape(R, C)
        col = np.arange(C)[None, :]
        tmask = labels[:, None] == (col if "target_at_label" in faults else col + 1)
        t = tmask.astype(F)
        s = _sigmoid(x)
        aw = np.where(tmask, F(ALPHA), F(1 - ALPHA))                                   # t alpha + (1 - t)(1 - alpha): exact
        oms = const(1) - s
        pt = _where(tmask, oms, s)                                                     # t (1 - s) + (1 - t) s: one term is 0
        fw = (aw if f32 else Bounded(aw.astype(np.float64))) * (pt * pt)
        e = _exp(-_abs(x))
        xt = x32 * t if f32 else _where(np.isinf(x32) & ~tmask, Bounded(np.full((), np.nan)), _mask(x, tmask))       # x * t: inf * 0
        relu = np.maximum(x32, F(0)) if f32 else _mask(x, x32 > 0)
        bce = (relu - xt) + _log1p(e)
        lane_cls = zero
        for c in range(C):
            lane_cls = lane_cls + (_col(fw, c) * _col(bce, c)) * wc
        sum_cls = _total(rows(lane_cls), 1, R, C)
        gw = (const(S["w_cls"]) * wc)[:, None]
        g_fw, g_bce = gw * bce, gw * fw
        c1 = _mask(g_bce, x32 >= 0)
        c2 = -_mask(g_bce, tmask)
        c3 = _scale(-((g_bce / (e + const(1))) * e), np.sign(x32))
        g_pt = (g_fw * (aw if f32 else Bounded(aw.astype(np.float64)))) * (const(2) * pt)
        g_s = _scale(g_pt, np.where(tmask, F(-1), F(1)))
        out["grad_cls"] = ((c1 + c2) + c3) + (g_s * oms) * s
        cls = sum_cls * const(S["w_cls"])
        # ---- part
        part = None
        if "part" in terms:
            xp, tp = wrap(np.asarray(inp["part"]).reshape(R, 3)), wrap(np.asarray(inp["part_t"]).reshape(R, 3))
            sp = _sigmoid(xp)
            la = at_least("part_floor_a", _log1p(-sp), S["floor"])
            lb = at_least("part_floor_b", _log(sp), S["floor"])
            v = (tp - const(1)) * la - tp * lb
            lane_part = zero
            for k in range(3):
                lane_part = lane_part + _col(v, k)
            sum_part = _total(rows(_mask(lane_part, pos)), 1, R, 3)
            den3 = const(max(P, 1) if "part_divisor_without_3" in faults else 3 * max(P, 1))      # the Python integer as float32
            part = (sum_part / den3) * const(S["w_part"])
            g0 = const(S["w_part"]) / den3
            omp = const(1) - sp
            g_sp = (g0 * (sp - tp)) / at_least("part_eps", omp * sp, S["eps"])
            g_xp = (g_sp * omp) * sp
            out["grad_part"] = g_xp if "part_grad_off_positives" in faults else _mask(g_xp, pos[:, None])
        # ---- box
        box = None
        if "box" in terms:
            p_, r_ = wrap(np.asarray(inp["box"]).reshape(R, code)), wrap(np.asarray(inp["box_t"]).reshape(R, code))
            cw = wrap(inp["cw"])
            cw = cw[None, :]
            replaced = D("replaced", lambda: np.isnan(r_))
            tg = _where(replaced, p_, r_)
            diff = (p_ - tg) * cw
            nrm = _abs(diff)
            quad = D("quad", lambda: (nrm < S["beta"]) & (not S["l1"]))
            sign_d = D("sign_d", lambda: _sign(diff))
            beta, half = const(S["beta"]), const(S["half_beta"])
            v = nrm if S["l1"] else _where(quad, (const(0.5) * (nrm * nrm)) / beta, nrm - half)
            lane_box = zero
            for k in range(code):
                lane_box = lane_box + _col(v, k) * wr
            sum_box = _total(rows(_mask(lane_box, box_rows)), 1, R, code)
            box = sum_box * const(S["w_box"])
            gl = (const(S["w_box"]) * wr)[:, None]
            if S["l1"]:
                g_n = gl * (np.ones(nrm.shape, dtype=F) if f32 else Bounded(np.ones(nrm.v.shape)))
            else:
                # where() hands the branch not taken a zero and pow's backward multiplies it by 2 n: +0 for a finite n (gl + 0
                # is gl, exactly: a float32 decision, no rounding), a NaN for an infinite or NaN one
                dead_nan = D("dead_nan", lambda: np.isnan(((F(0) / beta) * F(0.5)) * (F(2) * nrm)) & (NO_DEAD_SHARE not in faults))
                g_n = _where(quad, ((gl / beta) * const(0.5)) * (const(2) * nrm), _where(dead_nan, const(np.nan), gl))
            g_d = _scale(g_n, sign_d) * cw
            g_in = _where(replaced, g_d + (-g_d), g_d)
            out["grad_box"] = _mask(g_in, box_rows[:, None])
        # ---- the table: absent terms are skipped, not added as 0
        loss = cls
        if part is not None:
            loss = loss + part
        if box is not None:
            loss = loss + box
        vals = (cls, const(0) if part is None else part, const(0) if box is None else box, loss, const(P))
        if f32:
            out["table"] = np.array(vals, dtype=F)
        else:
            out["table"] = Bounded(np.array([float(q.v) for q in vals]), np.array([float(q.e) for q in vals]))
    if f32:
        out = {k: np.asarray(v, dtype=F) for k, v in out.items()}
    return out, d


def restate(inp, cfg, faults=()):
    """the kernel's float32 results: {"table" (5), "grad_cls" (R, C), "grad_part" (R, 3) and "grad_box" (R, code) for the terms
    of the head}"""
    return _evaluate(inp, cfg, None, faults)[0]


def exact(inp, cfg, dec=None):
    """the same statement in float64 along float32's branches -> {name: (value float64, bound float64)}"""
    out = _evaluate(inp, cfg, decisions(inp, cfg) if dec is None else dec)[0]
    return {k: (v.v, v.e) for k, v in out.items()}


# ---- comparisons -------------------------------------------------------------------------------------------------------------
def _place(name, idx):
    if name == "table":
        return TABLE[int(idx[0])]
    return "(row %d, column %d)" % tuple(int(v) for v in idx)


def bound_report(got, ex, what="ours"):
    """every element of every output against exact(): |got - value| <= bound, a NaN exactly where the value is one.
    -> (text naming the row and column of each output's worst miss, or "", {output: largest error / bound})"""
    lines, ratios = [], {}
    for name in OUTPUTS:
        if name not in ex:
            if got.get(name) is not None:
                lines.append(f"{what} has a {name} that is not expected")
            continue
        v, e = ex[name]
        if got.get(name) is None:
            lines.append(f"{what} lacks {name}")
            continue
        g = np.asarray(got[name], dtype=np.float64)
        if g.shape != v.shape:
            lines.append(f"{what} {name}: shape {g.shape}, expected {v.shape}")
            continue
        ratio, nan_v, nan_g = error_over_bound(g, v, e)
        ratios[name] = float(ratio.max()) if ratio.size else 0.0
        bad = (ratio >= 1.0) | (nan_v != nan_g)
        if bad.any():
            idx = np.unravel_index(int(np.argmax(np.where(nan_v != nan_g, np.inf, ratio))), g.shape)
            lines.append(f"{what} {name}: {int(bad.sum())} of {g.size} elements outside the bound, the worst at {_place(name, idx)}: "
                         f"{got[name][idx]!r} against {v[idx]!r} +- {e[idx]!r}")
    return "\n".join(lines), ratios


def zero_report(a, b, what="the zero pattern"):
    """the gradient elements that are == 0 in one and not in the other (a NaN is not 0)"""
    lines = []
    for name in OUTPUTS[1:]:
        if (name in a) != (name in b):
            lines.append(f"{name} is in one and not in the other")
        elif name in a:
            za, zb = np.asarray(a[name]) == 0, np.asarray(b[name]) == 0
            if za.shape != zb.shape or (za != zb).any():
                idx = np.argwhere(za != zb)[0] if za.shape == zb.shape else (0, 0)
                lines.append(f"{what} of {name} differs at {_place(name, idx)}")
    return "\n".join(lines)


def report(got, want, what="the device"):
    """bit for bit: every element of every output, NaNs included -> text naming the row and column, or "" """
    lines = []
    for name in OUTPUTS:
        if name not in want:
            if got.get(name) is not None:
                lines.append(f"{what} has a {name} that is not expected")
            continue
        if got.get(name) is None:
            lines.append(f"{what} lacks {name}")
            continue
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
    cfg = dict(head="PointHeadBox", box_layers=True, B=2, N=128, num_class=1, code=8, beta=1.0 / 9.0, cls_weight=1.0, part_weight=1.0,
               box_weight=1.0, code_weights=None, seed=1, samples=None, pos=0.1, label_max=None, int64=True, specials=[])
    cfg.update(kw)
    if cfg["code_weights"] is None:
        cfg["code_weights"] = [1.0] * cfg["code"]
    if cfg["samples"] is None:
        cfg["samples"] = ["mixed"] * cfg["B"]
    if cfg["label_max"] is None:
        cfg["label_max"] = cfg["num_class"]
    assert cfg["head"] in HEADS and len(cfg["samples"]) == cfg["B"] and len(cfg["code_weights"]) == cfg["code"]
    return cfg


SPECIAL_ROWS = np.arange(0, 120, 3)      # positives at fixed places; SPECIAL_ROWS + 1 are background rows
LOGITS = (0.0, -0.0, 30.0, -30.0, 100.0, -100.0)
PART_LABELS = (0.0, 1.0, 0.5)


def _sp_logits(inp, cfg, rows):
    """focal logits of exactly +0 and -0, +-30 and +-100 in every class column of a positive and of a background row, and 100
    on an ignored row"""
    for j, v in enumerate(LOGITS):
        inp["cls"][rows[j], :] = F(v)
        inp["cls"][rows[j] + 1, :] = F(v)
    inp["labels"][rows[6] + 1] = -1
    inp["cls"][rows[6] + 1, :] = F(100.0)


def _sp_part(inp, cfg, rows, recorded=False):
    """part logits of exactly +0 and -0, +-30, 100 and -100 against part labels of exactly 0, 1 and 0.5, on positive rows.
    `recorded`: -80 in place of -100 -- at -100 a float32 sigmoid evaluated as 1 / (1 + exp(-x)) is exactly 0 (exp(100) overflows
    float32) and hands on a gradient of exactly 0, where the contract's sigmoid is 3.8e-44 and the gradient is not 0 (DESIGN.md
    section 7q): the zero patterns differ, so -100 is a case against the restatement, not a recorded point"""
    if "part" not in inp:
        return
    for j, v in enumerate(LOGITS):
        r = rows[8 + j]
        inp["part"][r, :] = F(-80.0) if recorded and v == -100.0 else F(v)
        inp["part_t"][r, :] = np.array(PART_LABELS, dtype=F)


def _sp_part_recorded(inp, cfg, rows):
    _sp_part(inp, cfg, rows, recorded=True)


def _sp_beta(inp, cfg, rows):
    """|d| == beta exactly (the linear side) and d == 0 (gradient 0)"""
    if "box" not in inp:
        return
    a, b = rows[16], rows[17]
    inp["box_t"][a, 0] = F(0)
    inp["box"][a, 0] = F(cfg["beta"]) / F(cfg["code_weights"][0])
    inp["box"][b, 1] = inp["box_t"][b, 1]


def _sp_nan(inp, cfg, rows):
    """a NaN in a box label column of a positive row: replaced by the input"""
    if "box" in inp:
        inp["box_t"][rows[18], 2] = F(np.nan)


def _sp_part_outside(inp, cfg, rows):
    """part labels just outside [0, 1]: the formula is simply evaluated"""
    if "part" in inp:
        inp["part_t"][rows[20], 0] = F(1.0) + F(2.0 ** -23)
        inp["part_t"][rows[20], 1] = -F(2.0 ** -24)


def _sp_label_above(inp, cfg, rows):
    """a label above num_class: it matches no class column and counts as a positive"""
    inp["labels"][rows[22]] = cfg["num_class"] + 5


def _sp_nonfinite_off(inp, cfg, rows):
    """NaN and infinite part and box values, predictions and labels, in rows that are not positive (background and ignored):
    the reference's sums are poisoned through NaN * 0, ours do not read these rows"""
    a, b = rows[24] + 1, rows[25] + 1
    inp["labels"][b] = -1
    for key in ("part", "part_t", "box", "box_t"):
        if key in inp:
            inp[key][a, :] = F(np.nan)
            inp[key][b, 0] = F(np.inf)
            inp[key][b, 1] = -F(np.inf)


def _sp_nonfinite_box(inp, cfg, rows, vals=(np.nan, np.inf, -np.inf)):
    """on positive rows: NaN, +inf, -inf in a box prediction's column 1, inf in a box label's column 1"""
    if "box" in inp:
        for j, v in enumerate(vals):
            inp["box"][rows[26 + j], 1] = F(v)
        inp["box_t"][rows[29], 1] = F(np.inf)


def _sp_inf_box(inp, cfg, rows):
    """infinities alone: point_loss_box is +inf, not a NaN"""
    _sp_nonfinite_box(inp, cfg, rows, vals=(np.inf, -np.inf))


def _sp_nonfinite_cls(inp, cfg, rows):
    """inf, -inf and NaN in a focal logit: of a positive (the first and the last class column) and of a background row"""
    for j, v in enumerate((np.inf, -np.inf, np.nan)):
        inp["cls"][rows[30 + j], 0] = F(v)
        inp["cls"][rows[33 + j], -1] = F(v)
        inp["cls"][rows[30 + j] + 1, 0] = F(v)


def _sp_inf_part(inp, cfg, rows):
    """inf and -inf in a part logit of a positive row, against part labels of 0, 1 and 0.5"""
    if "part" in inp:
        for j, v in enumerate((np.inf, -np.inf)):
            inp["part"][rows[36 + j], :] = F(v)
            inp["part_t"][rows[36 + j], :] = np.array(PART_LABELS, dtype=F)


def _sp_nan_part(inp, cfg, rows):
    """a NaN part logit of a positive row: the reference's binary_cross_entropy raises on the CPU (its input is not within
    [0, 1]), so this is a case against the restatement, not a recorded one"""
    if "part" in inp:
        inp["part"][rows[38], 1] = F(np.nan)


def _sp_extreme(inp, cfg, rows, recorded=False):
    """finite and huge, on positive rows: focal logits +-88.9 (exp(88.9) is past float32) and +-1e30, also on background rows;
    part logits of the same values against part labels 0, 1 and 0.5; box values 1e20 and -1e30, a box label of 1e20, and one
    value of -3e38 (one, so that no float32 sum overflows where the exact one does not).  `recorded`: -88.9 against part
    labels of 0 alone, the point of ``_sp_part`` (a float32 sigmoid evaluated as 1 / (1 + exp(-x)) is exactly 0 there)"""
    for j, v in enumerate((88.9, -88.9, 1e30, -1e30)):
        inp["cls"][rows[26 + j], :] = F(v)
        inp["cls"][rows[26 + j], 0] = F(-v)
        inp["cls"][rows[26 + j] + 1, :] = F(v)
        if "part" in inp:
            inp["part"][rows[30 + j], :] = F(v)
            inp["part_t"][rows[30 + j], :] = F(0) if recorded and v == -88.9 else np.array(PART_LABELS, dtype=F)
    if "box" in inp:
        inp["box"][rows[34], 0] = F(1e20)
        inp["box"][rows[35], 2] = F(-1e30)
        inp["box_t"][rows[36], 3] = F(1e20)
        inp["box"][rows[37], 4] = F(-3e38)


def _sp_extreme_recorded(inp, cfg, rows):
    _sp_extreme(inp, cfg, rows, recorded=True)


SPECIALS = {"nonfinite_box": _sp_nonfinite_box, "inf_box": _sp_inf_box, "nonfinite_cls": _sp_nonfinite_cls, "inf_part": _sp_inf_part,
            "nan_part": _sp_nan_part, "extreme": _sp_extreme, "extreme_recorded": _sp_extreme_recorded,
            "logits": _sp_logits, "part": _sp_part, "part_recorded": _sp_part_recorded, "beta": _sp_beta, "nan": _sp_nan,
            "part_outside": _sp_part_outside, "label_above": _sp_label_above, "nonfinite_off": _sp_nonfinite_off}
EDGE = ["logits", "part", "beta", "nan"]                      # the `edge` case
EDGE_RECORDED = ["logits", "part_recorded", "beta", "nan"]    # what the recorded `edge` scene holds


def make_inputs(cfg):
    """{"cls" (R, C), "labels" (R), "part" (R, 3), "part_t" (R, 3), "box" (R, code), "box_t" (R, code), "cw" (code)} from the
    config's seed, R = B * N; the part and box entries only with those terms; the labels of the part and box terms are zero
    off the positives, as the target assignment leaves them"""
    rs = np.random.RandomState(int(cfg["seed"]))
    B, N, C, code = (int(cfg[k]) for k in ("B", "N", "num_class", "code"))
    R = B * N
    terms = terms_of(cfg)
    labels = np.zeros((B, N), dtype=np.int64)
    for b, mode in enumerate(cfg["samples"]):
        draw, cls = rs.uniform(size=N), rs.randint(1, int(cfg["label_max"]) + 1, size=N)
        if mode == "mixed":
            labels[b] = np.where(draw < cfg["pos"], cls, np.where(draw > 0.9, -1, 0))
        elif mode == "none":
            labels[b] = np.where(draw > 0.9, -1, 0)
        elif mode == "all":
            labels[b] = cls
        elif mode == "ignore":
            labels[b] = -1
        else:
            raise ValueError(mode)
    labels = labels.reshape(R)
    if cfg["specials"]:
        assert R >= 121, "the specials sit in the first 121 rows"
        labels[SPECIAL_ROWS] = 1 + np.arange(len(SPECIAL_ROWS)) % int(cfg["label_max"])
        labels[SPECIAL_ROWS + 1] = 0
    pos = labels > 0
    inp = {"cls": (rs.standard_normal((R, C)) * 3).astype(F), "labels": labels.astype(np.int64 if cfg["int64"] else np.int32)}
    part = (rs.standard_normal((R, 3)) * 2).astype(F)
    part_t = np.where(pos[:, None], rs.uniform(0.0, 1.0, size=(R, 3)), 0.0).astype(F)
    box = (rs.standard_normal((R, code)) * 0.5).astype(F)
    box_t = np.where(pos[:, None], rs.standard_normal((R, code)) * 0.5, 0.0).astype(F)
    if "part" in terms:
        inp.update(part=part, part_t=part_t)
    if "box" in terms:
        inp.update(box=box, box_t=box_t, cw=np.asarray(cfg["code_weights"], dtype=F))
    for name in cfg["specials"]:
        SPECIALS[name](inp, cfg, SPECIAL_ROWS)
    return inp


def edge_scene_cfgs():
    """the second config set: what tools/make_golden_point_loss.py records into tests/golden/point_loss_edges.npz and
    tests/point_loss_cases.py runs as cases: non-finite and huge values on positive rows"""
    c = base_cfg
    box, part, simple = HEADS
    return {"nonfinite": c(head=part, B=1, N=130, num_class=3, seed=61, specials=["nonfinite_box", "nonfinite_cls", "inf_part"]),
            "nonfinite_inf": c(head=box, B=1, N=130, seed=62, specials=["inf_box"]),
            "nonfinite_l1": c(head=box, B=1, N=130, seed=63, beta=0.0, specials=["nonfinite_box"]),
            "extreme": c(head=part, B=1, N=130, num_class=3, seed=64, specials=["extreme_recorded"]),
            "extreme_box": c(head=box, B=1, N=130, seed=65, specials=["extreme_recorded"])}


# ---- the fixture -------------------------------------------------------------------------------------------------------------
def scenes(gold):
    """[(name, cfg)] of tests/golden/point_loss.npz"""
    return [(n, json.loads(str(gold[f"{n}/cfg"]))) for n in json.loads(str(gold["scenes"]))]


def recorded(gold, name):
    return {k: gold[f"{name}/{k}"] for k in OUTPUTS if f"{name}/{k}" in gold}


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
    loss = Cfg(LOSS_REG="WeightedSmoothL1Loss",
               LOSS_WEIGHTS=dict(point_cls_weight=cfg["cls_weight"], point_part_weight=cfg["part_weight"],
                                 point_box_weight=cfg["box_weight"], code_weights=list(cfg["code_weights"])))
    loss.update(kw)
    return Cfg(LOSS_CONFIG=loss)


_head_classes = {}


def bound_class(name):
    """a class of the reference head's name with modest_amd.utils.point_head_loss.get_loss bound on it (made once per name)"""
    if name not in _head_classes:
        from modest_amd.utils import point_head_loss
        _head_classes[name] = point_head_loss.bind(type(name, (), {}))
    return _head_classes[name]


def bare_head(cfg, inp, device="cpu", head_class=None, requires_grad=True):
    """-> (head, preds): an object with model_cfg, num_class, box_layers, the two loss objects and forward_ret_dict as a point
    head holds them after assign_stack_targets and its forward; preds the leaf tensors {"cls", "part", "box"} of its terms.
    head_class None: a class of cfg["head"]'s name with our get_loss bound"""
    import torch
    head = (head_class or bound_class(cfg["head"]))()
    head.model_cfg = model_cfg(cfg)
    head.num_class = int(cfg["num_class"])
    terms = terms_of(cfg)
    if cfg["head"] == "PointIntraPartOffsetHead":
        head.box_layers = object() if "box" in terms else None
    head.cls_loss_func = loss_stub("SigmoidFocalClassificationLoss", alpha=ALPHA, gamma=GAMMA)
    if "box" in terms:
        cw = torch.from_numpy(np.asarray(inp["cw"], dtype=F).copy()).to(device)
        head.reg_loss_func = loss_stub("WeightedSmoothL1Loss", beta=cfg["beta"], code_weights=cw)
    else:
        head.reg_loss_func = torch.nn.functional.smooth_l1_loss      # what build_losses leaves without LOSS_REG
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).to(device)      # noqa: E731
    preds = {k: dev(inp[k]).requires_grad_(requires_grad) for k in ("cls", "part", "box") if k in inp}
    head.forward_ret_dict = dict(point_cls_preds=preds["cls"], point_cls_labels=dev(inp["labels"]))
    if "part" in terms:
        head.forward_ret_dict.update(point_part_preds=preds["part"], point_part_labels=dev(inp["part_t"]))
    if "box" in terms:
        head.forward_ret_dict.update(point_box_preds=preds["box"], point_box_labels=dev(inp["box_t"]))
    return head, preds


def outputs_of(loss, tb, preds):
    """the loss, tb_dict's floats and the leaf gradients as the outputs of restate()"""
    table = np.array([tb["point_loss_cls"], tb.get("point_loss_part", 0.0), tb.get("point_loss_box", 0.0), float(loss),
                      tb["point_pos_num"]], dtype=F)
    got = {"table": table}
    for k, p in preds.items():
        got[f"grad_{k}"] = p.grad.detach().cpu().numpy().reshape(-1, p.shape[-1])
    return got
