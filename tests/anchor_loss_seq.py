"""numpy restatement of ``AnchorHeadTemplate.get_loss`` and its gradients under the contract of DESIGN.md section 7p (not a
test module; tests/test_anchor_loss_cpu.py, tests/test_gpu_anchor_loss.py, tools/make_golden_anchor_loss.py and
tools/anchor_loss_bench.py import it).

``restate(inp, cfg)`` is the kernel's arithmetic: float32 in the written order (numpy does not fuse), Python's scalars rounded
to float32 first, exp / log / log1p / sin / cos and the sigmoid as the double function of the float32 argument rounded once,
the sums over the kernel's tree.  ``exact(inp, cfg, dec)`` evaluates the SAME statement (one function, ``_evaluate``, serves
both) in float64 on the float32 inputs, taking every branch float32 decided (``dec``: the class column, the direction bin, the
smooth-L1 side, the NaN replacement, the signs behind |x| and |d|) as float32 took it, and carries with every value a running
bound of what float32 can be off by: a ``Bounded`` number is (value, bound), every operation adds its own rounding,
2^-24 of its result's magnitude, to what its operands hand on (section 7p derives it).  A transcendental is budgeted one ulp
(2 * 2^-24), which covers both the rounded double function and a float32 library function of 1-ulp accuracy; the sigmoid is
evaluated as 1 / (1 + exp(-x)), so its budget is that of the composite.

A config is a plain dict (what the fixture records as JSON):
    B, N, num_class, code, bins (0: no direction head), beta, dir_offset, cls_weight, loc_weight, dir_weight, code_weights,
    seed, samples (per sample "mixed" | "none" | "all" | "ignore"), pos (fraction of positives in a mixed sample),
    label_max (labels are drawn from 1 .. label_max), int64 (labels), specials (names of ``SPECIALS`` written over the seeded
    draw, each at a fixed positive anchor of sample 0), layout (optional (H, W): the head's real layout, three anchor tensors
    of two rotations each and predictions shaped (B, H, W, 6 * columns))
"""
import json

import numpy as np

F = np.float32
U = 2.0 ** -24           # half an ulp, relative: one float32 rounding
TINY = 2.0 ** -149       # ... and absolute, where a product underflows
FUNC_U = 2 * U           # one ulp: the budget of a transcendental
FLT_MAX = float(np.finfo(np.float32).max)
T = 256                  # anchors of a workgroup
ALPHA, GAMMA = 0.25, 2.0
OUTPUTS = ("losses", "grad_cls", "grad_box", "grad_dir")


# ---- (value, bound) arithmetic ---------------------------------------------------------------------------------------------
class Bounded:
    """float64 values with a bound of |float32 value - value| for a float32 evaluation of the same operations"""
    __array_priority__ = 100

    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.broadcast_to(np.asarray(e, dtype=np.float64), self.v.shape)

    @staticmethod
    def of(x):
        return x if isinstance(x, Bounded) else Bounded(np.asarray(x, dtype=np.float64))

    def _rounded(self, v, carried, product=False, definite=None):
        """the operation's own rounding on top of what its operands hand on.  An infinite value whose sign cannot be another
        (`definite`: an infinity plus something finite, a product or quotient of operands that cannot cross 0) is that
        infinity in float32 as well: bound 0"""
        with np.errstate(invalid="ignore", over="ignore"):
            e = carried + U * (np.abs(v) + carried) + (TINY if product else 0.0)
            return Bounded(v, np.where(np.isinf(v) & (np.isfinite(carried) if definite is None else definite), 0.0, e))

    def __add__(self, o):
        o = Bounded.of(o)
        with np.errstate(invalid="ignore"):
            return self._rounded(self.v + o.v, self.e + o.e)
    __radd__ = __add__

    def __neg__(self):
        return Bounded(-self.v, self.e)

    def __sub__(self, o):
        return self + (-Bounded.of(o))

    def __rsub__(self, o):
        return Bounded.of(o) + (-self)

    def __mul__(self, o):
        o = Bounded.of(o)
        with np.errstate(invalid="ignore", over="ignore"):
            v = self.v * o.v
            carried = np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e
            carried = np.where(np.isnan(carried) & ~np.isnan(v), np.inf, carried)      # 0 times an unbounded factor: unbounded
            return self._rounded(v, carried, True, (np.abs(self.v) > self.e) & (np.abs(o.v) > o.e))
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Bounded.of(o)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            v = self.v / o.v
            room = np.abs(o.v) - o.e
            carried = np.where(room > 0, (self.e + np.abs(v) * o.e) / np.where(room > 0, room, 1.0), np.inf)
            carried = np.where((self.e == 0) & (o.e == 0), 0.0, carried)
            return self._rounded(v, carried, True, (np.abs(self.v) > self.e) & (np.abs(o.v) > o.e))

    def __rtruediv__(self, o):
        return Bounded.of(o) / self

    def __getitem__(self, k):
        return Bounded(self.v[k], self.e[k])

    def exact_scale(self, s):
        """times a float32 value that is 0, 1 or -1 (a mask, a sign): no rounding"""
        s = np.asarray(s, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            return Bounded(self.v * s, self.e * np.abs(s))


def _is_b(x):
    return isinstance(x, Bounded)


def _fn32(fn, x):
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        return fn(x.astype(np.float64)).astype(F)


def _exp(x):
    if not _is_b(x):
        return _fn32(np.exp, x)
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.exp(x.v)
        carried = np.where(x.e > 0, np.exp(x.v + x.e) - v, 0.0)
        # past float64's range (and float32's long before): the same infinity on both sides
        return Bounded(v, np.where(np.isinf(v) & np.isfinite(x.e), 0.0, carried + FUNC_U * (v + carried) + TINY))


def _log(x, fn=np.log, low=0.0):
    if not _is_b(x):
        return _fn32(fn, x)
    with np.errstate(invalid="ignore", divide="ignore"):
        v = fn(x.v)
        ok = x.v - x.e > low
        carried = np.where(x.e > 0, np.where(ok, v - fn(np.where(ok, x.v - x.e, 1.0)), np.inf), 0.0)
        return Bounded(v, np.where(np.isposinf(x.v) & np.isfinite(x.e), 0.0, carried + FUNC_U * (np.abs(v) + carried) + TINY))


def _log1p(x):
    return _log(x, np.log1p, -1.0)


def _trig(x, fn):
    if not _is_b(x):
        return _fn32(fn, x)
    with np.errstate(invalid="ignore"):
        v = fn(x.v)
        return Bounded(v, x.e + FUNC_U * (np.abs(v) + x.e))


def _sigmoid(x):
    if not _is_b(x):
        with np.errstate(over="ignore"):
            return (1.0 / (1.0 + np.exp(-x.astype(np.float64)))).astype(F)
    return 1.0 / (1.0 + _exp(-x))


def _abs(x):
    return Bounded(np.abs(x.v), x.e) if _is_b(x) else np.abs(x)


def _where(c, a, b):
    if _is_b(a) or _is_b(b):
        a, b = Bounded.of(a), Bounded.of(b)
        return Bounded(np.where(c, a.v, b.v), np.where(c, a.e, b.e))
    return np.where(c, a, b)


def _mask(x, m):
    """x where m else a true 0 (what a masked route of autograd, or a lane that does no work, contributes)"""
    return _where(m, x, np.zeros((), dtype=np.float64 if _is_b(x) else F))


def _scale(x, s):
    return x.exact_scale(s) if _is_b(x) else x * s.astype(F)


# ---- the kernel's summation tree -----------------------------------------------------------------------------------------
def _wave_tree(x):
    """(..., 64) float32 -> (...): v += v[lane ^ off] for off = 32, 16, .., 1"""
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        x = x + x[..., lane ^ off]
    return x[..., 0]


def _group_tree(x):
    """(..., 256) float32 -> (...): the wavefronts' trees, then (w0 + w1) + (w2 + w3)"""
    w = _wave_tree(x.reshape(x.shape[:-1] + (4, 64)))
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def tree_sum(lanes, rows_read=None):
    """(B, N) float32 lane values -> float32: al_loss's workgroup sums, then al_finish (lane t adds partials t, t + 256, ..
    in ascending order, then the same tree).  `rows_read` mis-states al_finish on purpose: only that many rows of 256"""
    B, N = lanes.shape
    blocks = (N + T - 1) // T
    pad = np.zeros((B, blocks * T), dtype=F)
    pad[:, :N] = lanes
    with np.errstate(invalid="ignore", over="ignore"):
        part = _group_tree(pad.reshape(B, blocks, T)).reshape(-1)
        rows = (part.size + T - 1) // T
        grid = np.zeros((rows * T,), dtype=F)
        grid[:part.size] = part
        acc = np.zeros((T,), dtype=F)
        for r in grid.reshape(rows, T)[:rows_read]:
            acc = acc + r
        return _group_tree(acc)


def tree_depth(B, N, lane_adds):
    """additions on the longest path from a term to the sum"""
    blocks = (N + T - 1) // T
    return lane_adds + 8 + (B * blocks + T - 1) // T + 8


def _total(lanes, B, N, lane_adds, rows_read=None):
    if not _is_b(lanes):
        return tree_sum(lanes, rows_read)
    with np.errstate(invalid="ignore"):
        v = lanes.v.sum(dtype=np.float64)
        carried = lanes.e.sum(dtype=np.float64)
        e = carried + tree_depth(B, N, lane_adds) * U * (np.abs(lanes.v).sum(dtype=np.float64) + carried)
        return Bounded(v, np.where(np.isinf(v) & np.isfinite(carried), 0.0, e))      # infinities of one sign among finite terms


# ---- the statement ---------------------------------------------------------------------------------------------------------
def scalars32(cfg):
    """Python's scalars as they meet a float32 tensor"""
    bins = int(cfg["bins"])
    return dict(beta=F(cfg["beta"]), half_beta=F(0.5 * float(F(cfg["beta"]))), l1=float(F(cfg["beta"])) < 1e-5,
                dir_offset=F(cfg["dir_offset"]), two_pi=F(2 * np.pi), bin_width=F(2 * np.pi / max(bins, 1)),
                alpha=F(ALPHA), one_m_alpha=F(1 - ALPHA), w_cls=F(cfg["cls_weight"]), w_loc=F(cfg["loc_weight"]),
                w_dir=F(cfg["dir_weight"]), fb=F(cfg["B"]))


def decisions(inp, cfg):
    """every branch float32 decides, from the float32 statement"""
    return _evaluate(inp, cfg, None)[1]


FAULTS = ("trunc_period", "no_upper_clamp", "no_dead_share", "finish_256", "finish_2048")


def _evaluate(inp, cfg, dec, faults=()):
    """dec None: float32 (the restatement) -> (outputs, decisions); else float64 with bounds along `dec`.  `faults` (names of
    FAULTS) mis-states the contract on purpose: truncation instead of floor in limit_period, no upper clamp of the bin, the
    smooth-L1 gradient without the dead branch's share, al_finish reading only its first 256 / 2048 partials"""
    assert set(faults) <= set(FAULTS), faults
    rows_read = 1 if "finish_256" in faults else (8 if "finish_2048" in faults else None)
    f32 = dec is None
    S = scalars32(cfg)
    wrap = (lambda a: np.asarray(a, dtype=F)) if f32 else (lambda a: Bounded(np.asarray(a, dtype=np.float64)))
    const = (lambda a: a) if f32 else (lambda a: Bounded(np.float64(a)))
    B, N, C, code, bins = int(cfg["B"]), int(cfg["N"]), int(cfg["num_class"]), int(cfg["code"]), int(cfg["bins"])
    labels = np.asarray(inp["labels"]).astype(np.int64)
    pos, cared = labels > 0, labels >= 0
    cnt = pos.sum(axis=1).astype(F)
    w32 = (F(1.0) / np.maximum(cnt, F(1.0)))[:, None] * np.ones((1, N), dtype=F)         # (B, N)
    w64 = (1.0 / np.maximum(cnt, F(1.0)).astype(np.float64))[:, None] * np.ones((1, N))
    w = wrap(w32) if f32 else Bounded(w64, U * w64)                                          # one division
    wc, wr = _mask(w, cared), _mask(w, pos)
    g_cls, g_loc, g_dir = (const(S[k]) / const(S["fb"]) for k in ("w_cls", "w_loc", "w_dir"))
    out, d = {}, ({} if f32 else dec)

    def lane_sum(terms):
        """a lane's accumulator starts at +0 and takes its terms in order"""
        acc = np.zeros((B, N), dtype=F) if f32 else 0.0
        for term in terms:
            acc = acc + term
        return acc

    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        # ---- classification
        x = wrap(inp["cls"])
        x32 = np.asarray(inp["cls"], dtype=F)
        col = np.arange(C)[None, None, :]
        tmask = (labels[..., None] == col + 1) | ((C == 1) & pos[..., None])
        t = tmask.astype(F)
        s = _sigmoid(x)
        aw = t * S["alpha"] + (F(1) - t) * S["one_m_alpha"]                          # 0.25 or 0.75: exact
        oms = 1.0 - s if not f32 else F(1) - s
        pt = _where(tmask, oms, s)                                                   # t (1 - s) + (1 - t) s: one term is 0
        fw = const(aw) * (pt * pt) if not f32 else aw * (pt * pt)
        e = _exp(-_abs(x))
        xt = x32 * t if f32 else _where(np.isinf(x32) & ~tmask, Bounded(np.full((), np.nan)), _mask(x, tmask))     # x * t: inf * 0
        relu = _mask(x, x32 > 0) if not f32 else np.maximum(x32, F(0))
        bce = (relu - xt) + _log1p(e)
        sum_cls = _total(lane_sum((fw[..., c] * bce[..., c]) * wc for c in range(C)), B, N, C, rows_read)
        gw = (g_cls * wc)[..., None]
        g_fw, g_bce = gw * bce, gw * fw
        c1 = _mask(g_bce, x32 >= 0)
        c2 = -_mask(g_bce, tmask)
        c3 = _scale(-((g_bce / (e + 1.0 if not f32 else e + F(1))) * e), np.sign(x32))
        g_pt = (g_fw * (const(aw) if not f32 else aw)) * ((2.0 if not f32 else F(2)) * pt)
        g_s = _scale(g_pt, np.where(tmask, F(-1), F(1)))
        p1 = (g_s * oms) * s
        out["grad_cls"] = ((c1 + c2) + c3) + p1
        # ---- box regression
        p_, r_ = wrap(inp["box"]), wrap(inp["tg"])
        cw = wrap(np.asarray(inp["cw"], dtype=F))[None, None, :]
        sp, cp = _trig(p_[..., 6], np.sin), _trig(p_[..., 6], np.cos)
        sr, cr = _trig(r_[..., 6], np.sin), _trig(r_[..., 6], np.cos)
        is6 = (np.arange(code) == 6)[None, None, :]
        in6, tg6 = sp * cr, cp * sr
        if f32:
            xin = np.where(is6, in6[..., None], p_)
            tg = np.where(is6, tg6[..., None], r_)
            d["replaced"] = np.isnan(tg)
        else:
            xin = Bounded(np.where(is6, in6.v[..., None], p_.v), np.where(is6, in6.e[..., None], p_.e))
            tg = Bounded(np.where(is6, tg6.v[..., None], r_.v), np.where(is6, tg6.e[..., None], r_.e))
        replaced = d["replaced"]
        tg = _where(replaced, xin, tg)
        diff = (xin - tg) * cw
        nrm = _abs(diff)
        if f32:
            d["quad"] = (nrm < S["beta"]) & (not S["l1"])
            d["sign_d"] = np.sign(np.where(np.isnan(diff), F(0), diff)).astype(F)
        quad, sign_d = d["quad"], d["sign_d"]
        beta, half = const(S["beta"]), const(S["half_beta"])
        half_c, two_c = (F(0.5), F(2)) if f32 else (0.5, 2.0)
        if S["l1"]:
            v = nrm
        else:
            v = _where(quad, (half_c * (nrm * nrm)) / beta, nrm - half)
        sum_loc = _total(lane_sum(_mask(v[..., k] * wr, pos) for k in range(code)), B, N, code, rows_read)
        gl = (g_loc * wr)[..., None]
        if S["l1"]:
            g_n = gl
        else:
            # where() hands the branch not taken a zero, and pow's backward multiplies it by 2 n: +0 for a finite n, a NaN
            # for an infinite or NaN one.  The quadratic side's zero goes through a subtraction only and stays a zero
            if f32:
                dead = ((np.zeros((B, N, 1), dtype=F) / beta) * half_c) * (two_c * nrm)
                d["dead_nan"] = np.isnan(dead) & ("no_dead_share" not in faults)
                dead = np.where(d["dead_nan"], dead, F(0))
                linear = gl + dead
            else:      # gl + (+0) is gl, exactly: the share is a float32 decision, not an operation with a rounding
                linear = _where(d["dead_nan"], Bounded(np.full((), np.nan)), gl)
            g_n = _where(quad, ((gl / beta) * half_c) * (two_c * nrm), linear)
        g_d = _scale(g_n, sign_d) * cw
        g_t = _mask(-g_d, ~replaced)
        g_in = _where(replaced, g_d + (-g_d), g_d)
        g6 = ((g_in[..., 6] * cr) * cp) + ((g_t[..., 6] * sr) * (-sp))
        if f32:
            gb = np.where(is6, g6[..., None], g_in)
        else:
            gb = Bounded(np.where(is6, g6.v[..., None], g_in.v), np.where(is6, g6.e[..., None], g_in.e))
        out["grad_box"] = _mask(gb, pos[..., None])
        # ---- direction
        if bins:
            z = wrap(inp["dir"])
            z32 = np.asarray(inp["dir"], dtype=F)
            if f32:
                rot = np.asarray(inp["tg"], dtype=F)[..., 6] + np.asarray(inp["anchors"], dtype=F)[None, :, 6]
                val = rot - S["dir_offset"]
                lim = val - (np.trunc if "trunc_period" in faults else np.floor)(val / S["two_pi"] + F(0)) * S["two_pi"]
                fl = np.floor(lim / S["bin_width"])
                top = F(np.inf) if "no_upper_clamp" in faults else F(bins - 1)      # unclamped: a bin that is no column
                b_ = np.where(~(fl >= 0), F(0), np.where(fl >= top, top, np.minimum(fl, F(bins)))).astype(np.int64)
                d["bin"] = np.where(pos, b_, 0)
            bin_ = d["bin"]
            m = z32.max(axis=-1, keepdims=True)                                      # a selection: exact
            zm = z - (m if f32 else Bounded(m.astype(np.float64)))
            ez = _exp(zm)
            lse = _log(lane_sum(ez[..., j] for j in range(bins)))
            onehot = np.arange(bins)[None, None, :] == bin_[..., None]
            if f32:
                lsm = zm - lse[..., None]
                picked = np.take_along_axis(lsm, np.minimum(bin_, bins - 1)[..., None], axis=-1)[..., 0]
            else:
                lsm = zm - Bounded(lse.v[..., None], lse.e[..., None])
                picked = Bounded(np.take_along_axis(lsm.v, np.minimum(bin_, bins - 1)[..., None], axis=-1)[..., 0],
                                 np.take_along_axis(lsm.e, np.minimum(bin_, bins - 1)[..., None], axis=-1)[..., 0])
            lane_dir = _mask((-picked) * wr, pos)
            sum_dir = _total(lane_dir, B, N, 0, rows_read)
            g = (-(g_dir * wr))[..., None]
            prob = _exp(lsm)
            out["grad_dir"] = _mask(_mask(g, onehot) - prob * g, pos[..., None])
        # ---- the four scalars
        cls = (sum_cls / const(S["fb"])) * const(S["w_cls"])
        loc = (sum_loc / const(S["fb"])) * const(S["w_loc"])
        if bins:
            dr = (sum_dir / const(S["fb"])) * const(S["w_dir"])
            rpn = cls + (loc + dr)
        else:
            dr = const(F(0))
            rpn = cls + loc
        if f32:
            out["losses"] = np.array([cls, loc, dr, rpn], dtype=F)
        else:
            out["losses"] = Bounded(np.array([q.v for q in (cls, loc, dr, rpn)]), np.array([q.e for q in (cls, loc, dr, rpn)]))
    if f32:
        d["count"] = pos.sum(axis=1)
        out = {k: np.asarray(v, dtype=F) for k, v in out.items()}
    return out, d


def restate(inp, cfg, faults=()):
    """the kernel's float32 results: {"losses" (4), "grad_cls", "grad_box", "grad_dir" (with a direction head)}"""
    return _evaluate(inp, cfg, None, faults)[0]


def exact(inp, cfg, dec=None):
    """the same statement in float64 along float32's branches -> {name: (value float64, bound float64)}"""
    out = _evaluate(inp, cfg, decisions(inp, cfg) if dec is None else dec)[0]
    return {k: (v.v, v.e) for k, v in out.items()}


# ---- comparisons -------------------------------------------------------------------------------------------------------------
def _where3(name, idx):
    if name == "losses":
        return ("rpn_loss_cls", "rpn_loss_loc", "rpn_loss_dir", "rpn_loss")[int(idx[0])]
    return "(sample %d, anchor %d, column %d)" % tuple(int(v) for v in idx)


def error_over_bound(g, v, e):
    """float32 results g against exact()'s (v, e) -> (|g - v| / e per element, where v is a NaN, where g is one).  A NaN
    bound counts as a NaN value.  A value past float32's range even after its bound is that infinity in float32: equal
    infinities agree, anything else there is infinitely far off"""
    nan_v, nan_g = np.isnan(v) | np.isnan(e), np.isnan(g)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        over = ~nan_v & (np.abs(v) - e > FLT_MAX)
        same_inf = over & np.isinf(g) & (np.sign(g) == np.sign(v))
        err = np.where(nan_v | nan_g | same_inf, 0.0, np.where(over, np.inf, np.abs(g - np.where(nan_v | same_inf, 0.0, v))))
        ratio = np.where(err == 0, 0.0, np.where(e > 0, err / np.where(e > 0, e, 1.0), np.inf))
    return ratio, nan_v, nan_g


def bound_report(got, ex, what="ours"):
    """every element of every output against exact(): |got - value| <= bound, a NaN exactly where the value is one.
    -> (text naming (sample, anchor, column) of each output's worst miss, or "", {output: largest error / bound})"""
    lines, ratios = [], {}
    for name in OUTPUTS:
        if name not in ex:
            continue
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
            lines.append(f"{what} {name}: {int(bad.sum())} of {g.size} elements outside the bound, the worst at {_where3(name, idx)}: "
                         f"{got[name][idx]!r} against {v[idx]!r} +- {e[idx]!r}")
    return "\n".join(lines), ratios


def zero_report(a, b, what="the zero pattern"):
    """the elements that are == 0 in one and not in the other (a NaN is not 0)"""
    lines = []
    for name in OUTPUTS[1:]:
        if name in a or name in b:
            za, zb = np.asarray(a[name]) == 0, np.asarray(b[name]) == 0
            if za.shape != zb.shape or (za != zb).any():
                idx = np.argwhere(za != zb)[0] if za.shape == zb.shape else (0, 0, 0)
                lines.append(f"{what} of {name} differs at {_where3(name, idx)}")
    return "\n".join(lines)


def report(got, want, what="the device"):
    """bit for bit: every element of every output, NaNs included -> text naming (sample, anchor, column), or "" """
    lines = []
    for name in OUTPUTS:
        if name not in want:
            if got.get(name) is not None:
                lines.append(f"{what} has a {name} that is not expected")
            continue
        g, w = np.asarray(got[name], dtype=F), np.asarray(want[name], dtype=F)
        if g.shape != w.shape:
            lines.append(f"{what} {name}: shape {g.shape}, expected {w.shape}")
            continue
        bad = g.view(np.uint32) != w.view(np.uint32)
        bad &= ~(np.isnan(g) & np.isnan(w))
        bad &= ~((g == 0) & (w == 0)) if name != "losses" else True     # the sign of a zero gradient carries nothing
        if bad.any():
            idx = np.argwhere(bad)[0]
            lines.append(f"{what} {name}: {int(bad.sum())} of {g.size} elements differ, the first at {_where3(name, idx)}: "
                         f"{g[tuple(idx)]!r} ({g.view(np.uint32)[tuple(idx)]:#010x}) against {w[tuple(idx)]!r} "
                         f"({w.view(np.uint32)[tuple(idx)]:#010x})")
    return "\n".join(lines)


# ---- seeded inputs -----------------------------------------------------------------------------------------------------------
def base_cfg(**kw):
    cfg = dict(B=2, N=300, num_class=3, code=7, bins=2, beta=1.0 / 9.0, dir_offset=0.78539, cls_weight=1.0, loc_weight=2.0,
               dir_weight=0.2, code_weights=None, seed=1, samples=None, pos=0.05, label_max=None, int64=False, specials=[])
    cfg.update(kw)
    if cfg["code_weights"] is None:
        cfg["code_weights"] = [1.0] * cfg["code"]
    if cfg["samples"] is None:
        cfg["samples"] = ["mixed"] * cfg["B"]
    if cfg["label_max"] is None:
        cfg["label_max"] = cfg["num_class"]
    assert len(cfg["samples"]) == cfg["B"] and len(cfg["code_weights"]) == cfg["code"]
    return cfg


def _first_positives(inp, count):
    rows = np.flatnonzero(inp["labels"][0] > 0)
    assert rows.size >= count, "sample 0 has too few positives for the specials"
    return rows


def _sp_logits(inp, cfg, rows):
    """logits of exactly +0 and -0, +-30 and +-100, in the target column and in another, on a positive, a background and an
    ignored anchor"""
    vals = np.array([0.0, -0.0, 30.0, -30.0, 100.0, -100.0], dtype=F)
    back = np.flatnonzero(inp["labels"][0] == 0)[:len(vals)]
    for j, v in enumerate(vals):
        inp["cls"][0, rows[j], :] = v
        inp["cls"][0, back[j], :] = v
    inp["labels"][0, back[-1] + 1] = -1
    inp["cls"][0, back[-1] + 1, :] = F(100.0)


def _sp_beta(inp, cfg, rows):
    """|d| == beta exactly (the second branch) and d == 0 (gradient 0)"""
    r = rows[6]
    inp["tg"][0, r, 0] = F(0)
    inp["box"][0, r, 0] = F(cfg["beta"]) / F(cfg["code_weights"][0])
    inp["box"][0, r, 1] = inp["tg"][0, r, 1]


def _sp_nan2(inp, cfg, rows):
    inp["tg"][0, rows[7], 2] = F(np.nan)


def _sp_nan6(inp, cfg, rows):
    inp["tg"][0, rows[8], 6] = F(np.nan)


def _sp_label_above(inp, cfg, rows):
    inp["labels"][0, rows[9]] = cfg["num_class"] + 5


def edge_headings(bins, dir_offset):
    """float32 headings at and around every bin edge: j * bin_width and j * bin_width + dir_offset for j in [-2 bins, 3 bins],
    each computed in float32 and in float64 rounded once, each with its +-1, +-2, +-3 float32 neighbours; then +-0, +-1e-30,
    -1e-7 (lim rounds to 2 pi: only the upper clamp keeps the bin in range), +-50, +-1e4, 3e38.  -> (L,) float32, the
    -1e-7 entry at index L - 6"""
    bw32, bw64, off32 = F(2 * np.pi / bins), 2 * np.pi / bins, F(dir_offset)
    base = []
    for j in range(-2 * bins, 3 * bins + 1):
        base += [F(j) * bw32, F(j) * bw32 + off32, F(j * bw64), F(j * bw64 + float(dir_offset))]
    out = []
    for v in base:
        lo = hi = F(v)
        near = [F(v)]
        for _ in range(3):
            lo, hi = np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))
            near += [lo, hi]
        out += near
    out = sorted(set(float(v) for v in out))
    return np.array(out + [0.0, -0.0, 1e-30, -1e-30, -1e-7, 50.0, -50.0, 1e4, -1e4, 3e38], dtype=F)


def edge_shape(bins, dir_offset, most=600):
    """(B, N) that hold every edge heading twice (an anchor of heading 0, then one of 1.57), N even and at most `most`"""
    need = 2 * len(edge_headings(bins, dir_offset))
    B = -(-need // most)
    N = -(-need // B)
    return B, N + N % 2


def _sp_dir_edges(inp, cfg, rows):
    """every anchor positive (samples "all"); the edge headings over the anchors in order, each on an anchor of heading 0 and
    on its neighbour of heading 1.57, the rest +0; ONE row of direction logits for all (the scene is about the bin)"""
    h = np.repeat(edge_headings(int(cfg["bins"]), cfg["dir_offset"]), 2)
    flat = np.zeros(inp["tg"].shape[:2], dtype=F).reshape(-1)
    assert h.size <= flat.size and inp["tg"].shape[1] % 2 == 0 and (inp["labels"] > 0).all()
    flat[:h.size] = h
    inp["tg"][..., 6] = flat.reshape(inp["tg"].shape[:2])
    inp["dir"][...] = inp["dir"][0, 0].copy()


def _sp_dir_logits(inp, cfg, rows):
    """direction logits that saturate, tie, overflow exp's argument and are infinite, on positives (2 bins)"""
    for j, z in enumerate(([100.0, -100.0], [0.0, 0.0], [-0.0, 0.0], [88.8, -88.8], [1e30, -1e30], [np.inf, 0.0])):
        inp["dir"][0, rows[j], :2] = np.array(z, dtype=F)


def _sp_nonfinite_box(inp, cfg, rows, vals=(np.nan, np.inf, -np.inf), col6=True):
    """NaN, +inf, -inf in box column 1 of three positives and in column 6 of three others; inf in a target's column 1 and in
    another target's column 6"""
    for j, v in enumerate(vals):
        inp["box"][0, rows[j], 1] = F(v)
        if col6:
            inp["box"][0, rows[3 + j], 6] = F(v)
    inp["tg"][0, rows[6], 1] = F(np.inf)
    if col6:
        inp["tg"][0, rows[7], 6] = F(np.inf)


def _sp_inf_box(inp, cfg, rows):
    """infinities alone, outside the heading column (sin of an infinity is a NaN): rpn_loss_loc is +inf, not a NaN"""
    _sp_nonfinite_box(inp, cfg, rows, vals=(np.inf, -np.inf), col6=False)


def _sp_nonfinite_cls(inp, cfg, rows):
    """inf, -inf and NaN in a class logit: of a positive (the target column and another) and of a background anchor"""
    back = np.flatnonzero(inp["labels"][0] == 0)
    for j, v in enumerate((np.inf, -np.inf, np.nan)):
        inp["cls"][0, rows[8 + j], 0] = F(v)
        inp["cls"][0, rows[11 + j], -1] = F(v)
        inp["cls"][0, back[j], 0] = F(v)


def _sp_extreme(inp, cfg, rows):
    """finite and huge: class logits +-88.9 (exp(88.9) is past float32) and +-1e30 on positives and a background anchor, box
    values 1e20 and -1e30, headings 1e10 and -3e38 in a prediction and in a target"""
    back = np.flatnonzero(inp["labels"][0] == 0)
    for j, v in enumerate((88.9, -88.9, 1e30, -1e30)):
        inp["cls"][0, rows[j], :] = F(v)
        inp["cls"][0, rows[j], 0] = F(-v)
        inp["cls"][0, back[j], :] = F(v)
    inp["box"][0, rows[4], 0] = F(1e20)
    inp["box"][0, rows[5], 2] = F(-1e30)
    inp["tg"][0, rows[6], 3] = F(1e20)
    inp["box"][0, rows[7], 6] = F(1e10)
    inp["box"][0, rows[8], 6] = F(-3e38)
    inp["tg"][0, rows[9], 6] = F(1e10)
    inp["tg"][0, rows[10], 6] = F(-3e38)


def _sp_labels_wide(inp, cfg, rows):
    """int64 labels that a truncating cast would change: 2^32 + 1 (to class 1), 2^31 (to a negative label), -2^40 and
    INT64_MIN (to 0: background instead of ignored); int32: -7, ignored as -1 is"""
    if inp["labels"].dtype == np.int64:
        for j, v in enumerate((2 ** 32 + 1, 2 ** 31, -2 ** 40, -2 ** 63)):
            inp["labels"][0, rows[j]] = v
    else:
        inp["labels"][0, rows[0]] = -7
    for r in rows[:4]:
        if inp["labels"][0, r] <= 0:
            inp["tg"][0, r] = 0


SPECIALS = {"logits": _sp_logits, "beta": _sp_beta, "nan2": _sp_nan2, "nan6": _sp_nan6, "label_above": _sp_label_above,
            "dir_edges": _sp_dir_edges, "dir_logits": _sp_dir_logits, "nonfinite_box": _sp_nonfinite_box, "inf_box": _sp_inf_box,
            "nonfinite_cls": _sp_nonfinite_cls, "extreme": _sp_extreme, "labels_wide": _sp_labels_wide}
WHOLE_SCENE = ("dir_edges",)     # specials that lay out every anchor themselves: no fixed positives are written first
LAYOUT_ROT = ((0.0, 1.57), (0.5, 2.2), (-1.0, 3.0))      # a layout's three anchor tensors: two rotations each
LAYOUT_SIZE = ((3.9, 1.6, 1.56), (0.8, 0.6, 1.73), (1.76, 0.6, 1.73))


def make_inputs(cfg):
    """{"cls" (B, N, C), "box" (B, N, code), "dir" (B, N, bins) or None, "labels" (B, N), "tg" (B, N, code), "anchors" (N, code),
    "cw" (code)} from the config's seed: targets are zero off the positives, as the assigner leaves them"""
    rs = np.random.RandomState(int(cfg["seed"]))
    B, N, C, code, bins = (int(cfg[k]) for k in ("B", "N", "num_class", "code", "bins"))
    inp = {"cls": (rs.standard_normal((B, N, C)) * 3).astype(F), "box": (rs.standard_normal((B, N, code)) * 0.5).astype(F),
           "dir": (rs.standard_normal((B, N, bins)) * 2).astype(F) if bins else None}
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
    fixed = [n for n in cfg["specials"] if n not in WHOLE_SCENE]
    if fixed:
        labels[0, :40:3] = 1 + np.arange(len(labels[0, :40:3])) % int(cfg["label_max"])     # enough positives, at fixed places
        labels[0, 1:40:3] = 0
    tg = (rs.standard_normal((B, N, code)) * 0.5).astype(F)
    tg[..., 6] = rs.uniform(-np.pi, np.pi, size=(B, N)).astype(F)
    tg[labels <= 0] = 0
    anchors = np.zeros((N, code), dtype=F)
    anchors[:, :3] = (rs.uniform(-40, 40, size=(N, 3))).astype(F)
    anchors[:, 3:6] = F(1.6)
    anchors[:, 6] = np.where(np.arange(N) % 2 == 0, F(0), F(1.57))
    if cfg.get("layout"):      # (H, W): three anchor tensors (1, H, W, 1, 2, code), flattened as the reference's cat(dim=-3)
        H, W = cfg["layout"]
        assert N == H * W * 6
        grid = anchors.reshape(H, W, 3, 2, code)
        for a in range(3):
            grid[:, :, a, :, 3:6] = np.asarray(LAYOUT_SIZE[a], dtype=F)
            grid[:, :, a, :, 6] = np.asarray(LAYOUT_ROT[a], dtype=F)
    inp.update(labels=labels.astype(np.int64 if cfg["int64"] else np.int32), tg=tg, anchors=anchors,
               cw=np.asarray(cfg["code_weights"], dtype=F))
    if cfg["specials"]:
        rows = _first_positives(inp, 10 if fixed else 1)
        for name in cfg["specials"]:
            SPECIALS[name](inp, cfg, rows)
    return inp


def edge_scene_cfgs():
    """the second config set: what tools/make_golden_anchor_loss.py records into tests/golden/anchor_loss_edges.npz and
    tests/anchor_loss_cases.py runs as cases.  A direction scene records the scalars and grad_dir alone ("record")"""
    c, out = base_cfg, {}
    for bins, off in ((2, 0.78539), (3, 0.3), (4, 0.0), (8, 0.78539), (1, 0.0)):
        B, N = edge_shape(bins, off)
        out[f"dir_edges_b{bins}"] = c(B=B, N=N, num_class=1, bins=bins, dir_offset=off, samples=["all"] * B, seed=30 + bins,
                                      specials=["dir_edges"], record=["losses", "grad_dir"])
    out["dir_logits"] = c(B=1, N=70, seed=41, specials=["dir_logits"], record=["losses", "grad_dir"])
    out["nonfinite"] = c(B=1, N=70, seed=42, specials=["nonfinite_box", "nonfinite_cls"])
    out["nonfinite_inf"] = c(B=1, N=70, seed=43, specials=["inf_box"])
    out["nonfinite_l1"] = c(B=1, N=70, seed=44, beta=0.0, specials=["nonfinite_box"])
    out["extreme"] = c(B=1, N=70, seed=45, specials=["extreme"])
    out["layout"] = c(B=2, N=36, seed=46, pos=0.5, layout=[2, 3])
    # al_finish past its first row of 256 partials (257 of them), past it with one partial a sample (2049 samples of one
    # anchor, with and without a positive), and past its first batch of 8 rows inside a sample (9 samples of 229 workgroups:
    # 2061 partials, sample 1 holds partial 256 and sample 8 partial 2048).  Only the four scalars are recorded
    out["parts257"] = c(B=1, N=65537, seed=47, pos=0.01, record=["losses"])
    out["parts_b2049"] = c(B=2049, N=1, seed=48, pos=0.5, record=["losses"])
    out["parts2061"] = c(B=9, N=58369, seed=49, pos=0.002, record=["losses"])
    return out


# ---- the fixture -------------------------------------------------------------------------------------------------------------
def scenes(gold):
    """[(name, cfg)] of tests/golden/anchor_loss.npz"""
    return [(n, json.loads(str(gold[f"{n}/cfg"]))) for n in json.loads(str(gold["scenes"]))]


def recorded(gold, name):
    out = {k: gold[f"{name}/{k}"] for k in OUTPUTS if f"{name}/{k}" in gold}
    return out


def only(outputs, rec):
    """the outputs (restated, or exact()'s pairs) that a scene recorded"""
    return {k: v for k, v in outputs.items() if k in rec}


def anchor_tensors(cfg, flat, order=(0, 1, 2)):
    """the three (1, H, W, 1, 2, code) anchor tensors of a layout whose cat(dim=-3), in `order`, flattens to `flat`"""
    H, W = cfg["layout"]
    grid = np.asarray(flat).reshape(1, H, W, 3, 2, -1)
    return [np.ascontiguousarray(grid[:, :, :, a:a + 1]) for a in order]


# ---- a bare head: the attributes get_loss reads ---------------------------------------------------------------------------
class Cfg(dict):
    """a dict with attribute access (what the reference's EasyDict gives its classes)"""
    __getattr__ = dict.__getitem__


def loss_stub(name, **attrs):
    """an object whose class carries a reference loss class's name and the attributes get_loss reads from it"""
    return _with(type(name, (), {})(), attrs)


def _with(obj, attrs):
    for k, v in attrs.items():
        setattr(obj, k, v)
    return obj


def model_cfg(cfg, **kw):
    out = Cfg(LOSS_CONFIG=Cfg(LOSS_WEIGHTS=dict(cls_weight=cfg["cls_weight"], loc_weight=cfg["loc_weight"],
                                                dir_weight=cfg["dir_weight"], code_weights=list(cfg["code_weights"]))),
              DIR_OFFSET=cfg["dir_offset"], NUM_DIR_BINS=cfg["bins"], USE_MULTIHEAD=False)
    out.update(kw)
    return out


def bare_head(cfg, inp, device="cpu", head_class=None, requires_grad=True):
    """-> (head, preds): an object with model_cfg, num_class, num_anchors_per_location, anchors (a list of one
    (1, 1, N, 1, 1, code) tensor), the three loss objects and forward_ret_dict, as AnchorHeadTemplate holds them; preds the
    leaf tensors {"cls", "box", "dir"}"""
    import torch
    head = (head_class or type("Head", (), {}))()
    head.model_cfg = model_cfg(cfg)
    head.num_class, head.num_anchors_per_location, head.use_multihead = int(cfg["num_class"]), 1, False
    a = torch.from_numpy(inp["anchors"].copy()).to(device)
    head.anchors = [a.view(1, 1, -1, 1, 1, a.shape[-1])]
    shape = lambda k: inp[k].shape       # noqa: E731
    if cfg.get("layout"):
        H, W = cfg["layout"]
        head.num_anchors_per_location = 6
        head.anchors = [torch.from_numpy(t).to(device) for t in anchor_tensors(cfg, inp["anchors"])]
        shape = lambda k: (inp[k].shape[0], H, W, 6 * inp[k].shape[2])       # noqa: E731
    head.cls_loss_func = loss_stub("SigmoidFocalClassificationLoss", alpha=ALPHA, gamma=GAMMA)
    cw = torch.from_numpy(np.asarray(inp["cw"], dtype=F).copy()).to(device)
    if float(cfg["beta"]) == 0.0:
        head.reg_loss_func = loss_stub("WeightedL1Loss", code_weights=cw)
    else:
        head.reg_loss_func = loss_stub("WeightedSmoothL1Loss", beta=cfg["beta"], code_weights=cw)
    head.dir_loss_func = loss_stub("WeightedCrossEntropyLoss")
    preds = {k: torch.from_numpy(inp[k].copy().reshape(shape(k))).to(device).requires_grad_(requires_grad)
             for k in ("cls", "box", "dir") if inp[k] is not None}
    head.forward_ret_dict = dict(cls_preds=preds["cls"], box_preds=preds["box"],
                                 box_cls_labels=torch.from_numpy(inp["labels"].copy()).to(device),
                                 box_reg_targets=torch.from_numpy(inp["tg"].copy()).to(device))
    if "dir" in preds:
        head.forward_ret_dict["dir_cls_preds"] = preds["dir"]
    return head, preds
