"""numpy restatement of ``AxisAlignedTargetAssigner.assign_targets`` under the contract of DESIGN.md section 7i (not a
test module; tests/test_anchor_targets_cpu.py, tests/test_gpu_anchor_targets.py, tools/make_golden_anchor_targets.py
and tools/anchor_targets_bench.py import it).

All arithmetic float32 in the written order (numpy does not fuse); log / cos / sin are the double functions of the
float32 argument rounded once.  A config is a plain dict (what the fixture records as JSON):
    class_names, anchor_range [6], use_multihead, code_size (ResidualCoder's argument), sincos,
    classes: [{class_name, anchor_sizes, anchor_rotations, anchor_bottom_heights, align_center, matched_threshold,
               unmatched_threshold, grid_size [nx, ny]}]
"""
import json

import numpy as np

F = np.float32
PI32 = F(np.pi)
QUARTER = F(np.pi / 4)
TINY = F(1e-5)


# ---- configs as the reference's classes read them ---------------------------------------------------------------------
class Cfg(dict):
    """a dict with attribute access (what the reference's EasyDict gives its classes)"""
    __getattr__ = dict.__getitem__


def model_cfg(cfg, pos_fraction=-1.0, norm_by_num_examples=False, match_height=False):
    return Cfg(ANCHOR_GENERATOR_CONFIG=[Cfg(class_name=c["class_name"], anchor_sizes=c["anchor_sizes"],
                                            anchor_rotations=c["anchor_rotations"],
                                            anchor_bottom_heights=c["anchor_bottom_heights"],
                                            align_center=c["align_center"], matched_threshold=c["matched_threshold"],
                                            unmatched_threshold=c["unmatched_threshold"]) for c in cfg["classes"]],
               TARGET_ASSIGNER_CONFIG=Cfg(NAME="AxisAlignedTargetAssigner", POS_FRACTION=pos_fraction, SAMPLE_SIZE=512,
                                          NORM_BY_NUM_EXAMPLES=norm_by_num_examples, MATCH_HEIGHT=match_height),
               USE_MULTIHEAD=cfg["use_multihead"])


class Coder:
    """the two attributes of ResidualCoder the assigner reads"""

    def __init__(self, cfg):
        self.encode_angle_by_sincos = bool(cfg["sincos"])
        self.code_size = int(cfg["code_size"]) + int(self.encode_angle_by_sincos)


def make_anchors(cfg):
    """per class the (1, ny, nx, sizes, rotations, code) float32 anchors of AnchorGenerator.generate_anchors, padded with
    zero columns to the coder's code size as AnchorHeadTemplate.generate_anchors does.  The x / y shifts come from
    torch.arange on the CPU, as in the reference (tools/make_golden_anchor_targets.py asserts equal bits)."""
    import torch
    rng = cfg["anchor_range"]
    ndim = Coder(cfg).code_size
    out = []
    for c in cfg["classes"]:
        nx, ny = c["grid_size"]
        if c["align_center"]:
            xs, ys = (rng[3] - rng[0]) / nx, (rng[4] - rng[1]) / ny
            xo, yo = xs / 2, ys / 2
        else:
            xs, ys = (rng[3] - rng[0]) / (nx - 1), (rng[4] - rng[1]) / (ny - 1)
            xo, yo = 0, 0
        x = torch.arange(rng[0] + xo, rng[3] + 1e-5, step=xs, dtype=torch.float32).numpy()
        y = torch.arange(rng[1] + yo, rng[4] + 1e-5, step=ys, dtype=torch.float32).numpy()
        z = np.array(c["anchor_bottom_heights"], dtype=F)
        sizes = np.array(c["anchor_sizes"], dtype=F).reshape(-1, 3)
        rots = np.array(c["anchor_rotations"], dtype=F)
        a = np.zeros((len(z), len(y), len(x), len(sizes), len(rots), max(ndim, 7)), dtype=F)
        a[..., 0] = x[None, None, :, None, None]
        a[..., 1] = y[None, :, None, None, None]
        a[..., 3:6] = sizes[None, None, None, :, None, :]
        a[..., 2] = z[:, None, None, None, None] + a[..., 5] / F(2)
        a[..., 6] = rots[None, None, None, None, :]
        out.append(a)
    return out


# ---- the arithmetic ------------------------------------------------------------------------------------------------------
def nearest_bev(boxes):
    """(n, >= 7) float32 -> (n, 4) [x1, y1, x2, y2]"""
    b = np.asarray(boxes, dtype=F)
    r = b[:, 6]
    rot = np.abs(r - np.floor(r / PI32 + F(0.5)) * PI32)
    keep = rot < QUARTER
    dx, dy = np.where(keep, b[:, 3], b[:, 4]), np.where(keep, b[:, 4], b[:, 3])
    hx, hy = dx / F(2), dy / F(2)
    out = np.stack([b[:, 0] - hx, b[:, 1] - hy, b[:, 0] + hx, b[:, 1] + hy], axis=1)
    assert out.dtype == F
    return out


def rot_of(r):
    r = np.asarray(r, dtype=F)
    return np.abs(r - np.floor(r / PI32 + F(0.5)) * PI32)


def iou_matrix(ra, rb):
    """(n, 4), (m, 4) rectangles -> (n, m) float32"""
    xmin, xmax = np.maximum(ra[:, None, 0], rb[None, :, 0]), np.minimum(ra[:, None, 2], rb[None, :, 2])
    ymin, ymax = np.maximum(ra[:, None, 1], rb[None, :, 1]), np.minimum(ra[:, None, 3], rb[None, :, 3])
    xl, yl = np.maximum(xmax - xmin, F(0)), np.maximum(ymax - ymin, F(0))
    area_a = (ra[:, 2] - ra[:, 0]) * (ra[:, 3] - ra[:, 1])
    area_b = (rb[:, 2] - rb[:, 0]) * (rb[:, 3] - rb[:, 1])
    inter = xl * yl
    out = inter / np.maximum((area_a[:, None] + area_b[None, :]) - inter, F(1e-6))
    assert out.dtype == F
    return out


def kept_rows(gt_boxes):
    """(M, 7 + C) -> number of rows kept: up to the last row whose values do not sum to 0 (float32, left to right);
    row 0 always"""
    g = np.asarray(gt_boxes, dtype=F)
    if len(g) == 0:
        return 0
    s = np.zeros(len(g), dtype=F)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(g.shape[1]):
            s = s + g[:, k]
    live = np.flatnonzero(~(s == 0))
    return (int(live[-1]) if len(live) else 0) + 1


def class_rows(cids, class_names, anchor_name):
    """bool per kept row: class id c names class_names[c - 1] with Python's wrap; an id outside names nothing"""
    n = len(class_names)
    out = np.zeros(len(cids), dtype=bool)
    for j, c in enumerate(cids):
        k = int(c) - 1
        if k < 0:
            k += n
        out[j] = 0 <= k < n and class_names[k] == anchor_name
    return out


def f32_of_double(fn, x):
    return fn(np.asarray(x, dtype=F).astype(np.float64)).astype(F)


def encode(g, a, sincos):
    """ResidualCoder.encode_torch: g (n, 7 + Cg), a (n, 7 + Ca) float32 -> (n, 7 + sincos + min(Cg, Ca))"""
    g, a = np.array(g, dtype=F), np.array(a, dtype=F)
    a[:, 3:6] = np.maximum(a[:, 3:6], TINY)
    g[:, 3:6] = np.maximum(g[:, 3:6], TINY)
    diag = np.sqrt(a[:, 3] * a[:, 3] + a[:, 4] * a[:, 4])
    cols = [(g[:, 0] - a[:, 0]) / diag, (g[:, 1] - a[:, 1]) / diag, (g[:, 2] - a[:, 2]) / a[:, 5]]
    cols += [f32_of_double(np.log, g[:, k] / a[:, k]) for k in (3, 4, 5)]
    if sincos:
        cols += [f32_of_double(np.cos, g[:, 6]) - f32_of_double(np.cos, a[:, 6]),
                 f32_of_double(np.sin, g[:, 6]) - f32_of_double(np.sin, a[:, 6])]
    else:
        cols.append(g[:, 6] - a[:, 6])
    cols += [g[:, e] - a[:, e] for e in range(7, 7 + min(g.shape[1], a.shape[1]) - 7)]
    out = np.stack(cols, axis=1)
    assert out.dtype == F
    return out


def assign_single(anchors, gts, cids, matched, unmatched, sincos, code, detail=None):
    """anchors (n, 7 + Ca), gts (k, 7 + Cg) of this class in index order, cids (k,) int -> labels, targets, weights.
    detail (a dict) receives iou, colmax, rowmax, arg, forced."""
    n, k = len(anchors), len(gts)
    labels = np.zeros(n, dtype=np.int32)
    targets = np.zeros((n, code), dtype=F)
    if k and n:
        iou = iou_matrix(nearest_bev(anchors), nearest_bev(gts))
        arg = iou.argmax(axis=1)
        rowmax = iou[np.arange(n), arg]
        colmax = iou.max(axis=0)
        forced = ((iou == colmax[None, :]) & (colmax[None, :] != 0)).any(axis=1)
        cls = np.asarray(cids, dtype=np.int32)[arg]
        labels[:] = -1
        labels[rowmax >= F(matched)] = cls[rowmax >= F(matched)]
        labels[rowmax < F(unmatched)] = 0
        labels[forced] = cls[forced]
        fg = labels > 0
        targets[fg] = encode(gts[arg[fg]], anchors[fg], sincos)
        if detail is not None:
            detail.update(iou=iou, colmax=colmax, rowmax=rowmax, arg=arg, forced=forced)
    weights = (labels > 0).astype(F)
    return labels, targets, weights


def flatten(anchors, use_multihead):
    a = np.asarray(anchors, dtype=F)
    if use_multihead:
        a = a.transpose(3, 4, 0, 1, 2, 5)
    return np.ascontiguousarray(a).reshape(-1, a.shape[-1])


def assign(cfg, all_anchors, gt, details=None):
    """gt (B, M, 7 + Cg + 1) -> dict of box_cls_labels (B, N) int32, box_reg_targets (B, N, code) float32, reg_weights
    (B, N) float32.  details (a list) receives per sample a list of per-class dicts (anchors, rows, cids, iou, ...)."""
    gt = np.asarray(gt, dtype=F)
    sincos = bool(cfg["sincos"])
    names = list(cfg["class_names"])
    multi = bool(cfg["use_multihead"])
    flat = [flatten(a, multi) for a in all_anchors]
    code = 7 + int(sincos) + min(flat[0].shape[1] - 7, gt.shape[2] - 8)
    L, T, W = [], [], []
    for b in range(gt.shape[0]):
        kept = kept_rows(gt[b, :, :-1])
        boxes, cids = gt[b, :kept, :-1], gt[b, :kept, -1].astype(np.int32)
        per, info = [], []
        for c, a in zip(cfg["classes"], flat):
            rows = np.flatnonzero(class_rows(cids, names, c["class_name"]))
            d = dict(anchors=a, rows=rows, cids=cids[rows], matched=F(c["matched_threshold"]), unmatched=F(c["unmatched_threshold"]))
            per.append(assign_single(a, boxes[rows], cids[rows], c["matched_threshold"], c["unmatched_threshold"], sincos, code, d))
            info.append(d)
        if details is not None:
            details.append(info)
        if multi:
            lab, tar, wei = (np.concatenate([p[i] for p in per], axis=0) for i in range(3))
        else:
            fm = all_anchors[0].shape[:3]
            lab = np.concatenate([p[0].reshape(*fm, -1) for p in per], axis=-1).reshape(-1)
            tar = np.concatenate([p[1].reshape(*fm, -1, code) for p in per], axis=-2).reshape(-1, code)
            wei = np.concatenate([p[2].reshape(*fm, -1) for p in per], axis=-1).reshape(-1)
        L.append(lab), T.append(tar), W.append(wei)
    if not L:   # B = 0: the shapes without a sample
        n_out = sum(len(a) for a in flat)
        return {"box_cls_labels": np.zeros((0, n_out), dtype=np.int32), "box_reg_targets": np.zeros((0, n_out, code), dtype=F),
                "reg_weights": np.zeros((0, n_out), dtype=F)}
    return {"box_cls_labels": np.stack(L), "box_reg_targets": np.stack(T), "reg_weights": np.stack(W)}


# ---- the sincos columns against the reference ----------------------------------------------------
# |ours - reference| for the columns cos rg - cos ra and sin rg - sin ra.  Every function value lies in [-1, 1], where a
# float32 ulp is at most 2^-24 (below 1) -- the unit the accuracy statements are in.  Ours is the double function
# rounded once: within 0.5000001 ulp of the true value.  The reference's is torch's CPU kernel: SLEEF's u10 functions
# (documented maximum error 1.0 ulp) or the libm's cosf / sinf (glibc documents 1 ulp).  So one function value differs
# by at most 1.5 ulp <= 1.5 * 2^-24 between the two, the exact differences of two such values by at most 3 * 2^-24, and
# each side rounds its difference (magnitude <= 2, half an ulp there is 2^-24) once: 3 * 2^-24 + 2 * 2^-24.
SINCOS_BOUND = np.float64(5 * 2.0 ** -24)


# ---- comparison with a report ---------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def mismatches(got, ref, cfg=None, sincos_cols_bounded=False):
    """-> list of strings, empty if got == ref: labels and weights exactly, targets bit for bit (with
    sincos_cols_bounded the two sincos columns to SINCOS_BOUND instead)"""
    out = []
    gl, rl = np.asarray(got["box_cls_labels"]), np.asarray(ref["box_cls_labels"])
    gt_, rt = np.asarray(got["box_reg_targets"]), np.asarray(ref["box_reg_targets"])
    gw, rw = np.asarray(got["reg_weights"]), np.asarray(ref["reg_weights"])
    if gl.shape != rl.shape or gt_.shape != rt.shape or gw.shape != rw.shape:
        return [f"shapes {gl.shape} {gt_.shape} {gw.shape} against {rl.shape} {rt.shape} {rw.shape}"]
    if gl.dtype != np.int32 or gt_.dtype != F or gw.dtype != F:
        return [f"dtypes {gl.dtype} {gt_.dtype} {gw.dtype}"]
    bad = (gl != rl) | (bits(gw) != bits(rw))
    tb = bits(gt_) != bits(rt)
    if sincos_cols_bounded:
        close = np.abs(gt_[..., 6:8].astype(np.float64) - rt[..., 6:8].astype(np.float64)) <= SINCOS_BOUND
        tb[..., 6:8] &= ~close
    bad |= tb.any(axis=-1)
    for b, i in np.argwhere(bad)[:8]:
        out.append(f"sample {b} output row {i}: label {gl[b, i]} / {rl[b, i]}, weight {gw[b, i]} / {rw[b, i]}, "
                   f"targets {gt_[b, i].tolist()} / {rt[b, i].tolist()}")
    if out:
        out.insert(0, f"{int(bad.sum())} of {bad.size} rows differ")
    return out


def explain(cfg, all_anchors, gt, b, row):
    """(class, anchor within the class, the IoUs involved) of output row `row` of sample b, for a mismatch report"""
    details = []
    assign(cfg, all_anchors, gt[b:b + 1], details)
    multi = bool(cfg["use_multihead"])
    per = [int(np.prod(a.shape[:5])) for a in all_anchors]
    if multi:
        c = int(np.searchsorted(np.cumsum(per), row, side="right"))
        i = row - int(np.sum(per[:c]))
    else:
        k = [a.shape[3] * a.shape[4] for a in all_anchors]
        loc, j = divmod(row, int(sum(k)))
        c = int(np.searchsorted(np.cumsum(k), j, side="right"))
        i = loc * k[c] + j - int(np.sum(k[:c]))
    d = details[0][c]
    if "iou" not in d:
        return f"class {c} ({cfg['classes'][c]['class_name']}) anchor {i}: no gt of the class"
    pos = np.flatnonzero(d["iou"][i] > 0)
    return (f"class {c} ({cfg['classes'][c]['class_name']}) anchor {i}: gt rows {d['rows'][pos].tolist()} IoU "
            f"{d['iou'][i, pos].tolist()} column max {d['colmax'][pos].tolist()} row max {d['rowmax'][i]} arg row "
            f"{d['rows'][d['arg'][i]]} forced {bool(d['forced'][i])} thresholds {d['matched']} / {d['unmatched']}")


def report(got, ref, cfg, all_anchors, gt, sincos_cols_bounded=False):
    """'' if equal, else the mismatching rows with (sample, anchor, class) and the IoUs involved"""
    lines = mismatches(got, ref, cfg, sincos_cols_bounded)
    if not lines:
        return ""
    gl, rl = np.asarray(got["box_cls_labels"]), np.asarray(ref["box_cls_labels"])
    if gl.shape == rl.shape:
        tb = (bits(got["box_reg_targets"]) != bits(ref["box_reg_targets"])).any(axis=-1) | (gl != rl)
        for b, i in np.argwhere(tb)[:4]:
            lines.append(f"sample {b} row {i}: " + explain(cfg, all_anchors, np.asarray(gt), int(b), int(i)))
    return "\n".join(lines)


# ---- the fixture ---------------------------------------------------------------------------------------------------------
def scenes(rec):
    """[(name, cfg, gt)] of a loaded fixture"""
    names = json.loads(str(rec["scenes"]))
    return [(n, json.loads(str(rec[n + "_cfg"])), rec[n + "_gt"]) for n in names]


def recorded(rec, name):
    return {"box_cls_labels": rec[name + "_labels"], "box_reg_targets": rec[name + "_targets"], "reg_weights": rec[name + "_weights"]}


def fixture_cases(rec):
    """name -> bool for every case the fixture promises, read from its recorded arrays alone"""
    got = {}

    def hit(name, cond=True):
        got[name] = got.get(name, False) or bool(cond)

    keys = ["no gt: row 0 zero with class 0", "trailing zero rows trimmed", "zero row kept in the middle",
            "trailing row [1, -1, 0, ...] trimmed", "class id 0 lands in the last class", "class without anchors",
            "column max below unmatched, best anchors foreground", "two anchors tie for a column max",
            "gt with column max 0 forces nothing", "forced by j, argmax k != j, takes k's box",
            "same footprint, different z: the lower index wins", "IoU == matched", "IoU == matched, not forced",
            "IoU one float below matched", "IoU one float above matched", "IoU one float below unmatched",
            "IoU one float above unmatched", "IoU == unmatched", "rot one float below pi/4", "rot == pi/4", "rot one float above pi/4",
            "heading beyond +2 pi", "heading beyond -2 pi", "gt size below 1e-5", "three classes, different thresholds, single head",
            "three classes multihead, code 9 + sincos", "one class", "B = 1", "B = 2", "B = 3", "map 1 x 5 x 7", "map 1 x 33 x 40",
            "2 x 1 anchor under a concentric 4 x 1 gt gives 0.5", "a class with more than 256 gts",
            "a tie across 256 that the lower index wins", "forced from a later tile",
            "forced from tile 0, the argmax in a later tile", "k in {2, 4, 6} in one head",
            "multihead classes of different row counts", "a class without a gt next to a sample with more than 256"]
    for k in keys:
        got[k] = False
    for name, cfg, gt in scenes(rec):
        anchors = make_anchors(cfg)
        details = []
        out = assign(cfg, anchors, gt, details)
        labels = recorded(rec, name)["box_cls_labels"]
        hit("B = %d" % gt.shape[0])
        fm = anchors[0].shape[:3]
        hit("map 1 x 5 x 7", fm == (1, 5, 7) and all(int(np.prod(a.shape[:5])) == 70 for a in anchors))
        hit("map 1 x 33 x 40", fm == (1, 33, 40) and all(int(np.prod(a.shape[:5])) > 256 for a in anchors))
        thr = {(c["matched_threshold"], c["unmatched_threshold"]) for c in cfg["classes"]}
        three = len(cfg["classes"]) == 3 and len(thr) >= 2
        hit("three classes, different thresholds, single head", three and not cfg["use_multihead"])
        hit("three classes multihead, code 9 + sincos", three and cfg["use_multihead"] and cfg["code_size"] == 9 and cfg["sincos"]
            and gt.shape[2] == 10 and anchors[0].shape[-1] == 10)
        hit("one class", len(cfg["classes"]) == 1 and len(cfg["class_names"]) == 1)
        per_loc = sorted(a.shape[3] * a.shape[4] for a in anchors)
        hit("k in {2, 4, 6} in one head", not cfg["use_multihead"] and per_loc == [2, 4, 6])
        hit("multihead classes of different row counts", cfg["use_multihead"] and len({int(np.prod(a.shape[:5])) for a in anchors}) >= 3)
        for ci in range(len(anchors)):
            n_sel = [len(details[b][ci]["rows"]) for b in range(gt.shape[0])]
            hit("a class without a gt next to a sample with more than 256", min(n_sel) == 0 and max(n_sel) > 256)
        anchor_names = [c["class_name"] for c in cfg["classes"]]
        for b in range(gt.shape[0]):
            g = gt[b]
            kept = kept_rows(g[:, :-1])
            hit("no gt: row 0 zero with class 0", not g.any())
            zero = ~g[:, :-1].any(axis=1)
            hit("trailing zero rows trimmed", kept < len(g) and zero[kept:].all() and kept > 1)
            hit("zero row kept in the middle", zero[:kept - 1].any())
            hit("trailing row [1, -1, 0, ...] trimmed", any(np.array_equal(r[:7], np.array([1, -1, 0, 0, 0, 0, 0], dtype=F)) for r in g[kept:]))
            cids = g[:kept, -1].astype(np.int32)
            for j in range(kept):
                k = cids[j] - 1 + (len(cfg["class_names"]) if cids[j] - 1 < 0 else 0)
                if 0 <= k < len(cfg["class_names"]) and cfg["class_names"][k] not in anchor_names and g[j, :7].any():
                    hit("class without anchors")
            for ci, d in enumerate(details[b]):
                if "iou" not in d:
                    continue
                iou, colmax, rowmax, arg, forced, rows = d["iou"], d["colmax"], d["rowmax"], d["arg"], d["forced"], d["rows"]
                m, u = d["matched"], d["unmatched"]
                sel = g[rows]
                lab = assign_single(d["anchors"], sel[:, :-1], d["cids"], m, u, bool(cfg["sincos"]), out["box_reg_targets"].shape[-1])[0]
                is_max = (iou == colmax[None, :]) & (colmax[None, :] != 0)
                rect = nearest_bev(sel)
                hit("a class with more than 256 gts", len(rows) > 256)
                for j in range(len(rows)):
                    best = np.flatnonzero(is_max[:, j])
                    if d["cids"][j] == 0 and sel[j, :7].any() and colmax[j] > 0 and cfg["classes"][ci]["class_name"] == cfg["class_names"][-1]:
                        hit("class id 0 lands in the last class", (lab[best[arg[best] == j]] == 0).all())
                    hit("column max below unmatched, best anchors foreground", 0 < colmax[j] < u and len(best) and (lab[best] > 0).all())
                    hit("two anchors tie for a column max", len(best) >= 2)
                    hit("gt with column max 0 forces nothing", colmax[j] == 0 and sel[j, :7].any())
                    other = best[arg[best] != j]
                    hit("forced by j, argmax k != j, takes k's box",
                        len(other) and (rowmax[other] < m).any() and (lab[other] == d["cids"][arg[other]]).all() and (lab[other] > 0).any())
                    for key, mine, ok in (("forced from a later tile", other[arg[other] < 256], j >= 256),
                                          ("forced from tile 0, the argmax in a later tile", other[arg[other] >= 256], j < 256)):
                        only_j = [i for i in mine if is_max[i].sum() == 1]      # nothing but j forces the anchor
                        hit(key, ok and len(only_j) and (rowmax[only_j] < u).all() and (lab[only_j] > 0).all())
                    r = rot_of(sel[j, 6])
                    if sel[j, 3] != sel[j, 4] and colmax[j] > 0:
                        hit("rot one float below pi/4", r == np.nextafter(QUARTER, F(0)))
                        hit("rot == pi/4", r == QUARTER)
                        hit("rot one float above pi/4", r == np.nextafter(QUARTER, F(1)))
                    hit("heading beyond +2 pi", sel[j, 6] > 2 * np.pi and colmax[j] > 0)
                    hit("heading beyond -2 pi", sel[j, 6] < -2 * np.pi and colmax[j] > 0)
                    hit("gt size below 1e-5", (sel[j, 3:6] < TINY).any() and ((arg == j) & (lab > 0)).any())
                    for k2 in j + 1 + np.flatnonzero((bits(rect[j + 1:]) == bits(rect[j:j + 1])).all(axis=1)):
                        same = sel[j, 2] != sel[k2, 2]
                        fg = (lab > 0) & (iou[:, j] == rowmax) & (iou[:, k2] == rowmax)
                        hit("same footprint, different z: the lower index wins", same and fg.any() and (arg[fg] == j).all())
                        hit("a tie across 256 that the lower index wins", j < 256 <= k2 and same and fg.any() and (arg[fg] == j).all())
                free = ~forced
                hit("IoU == matched", (rowmax == m).any())
                hit("IoU == matched, not forced", (free & (rowmax == m) & (lab > 0)).any())
                hit("IoU one float below matched", (free & (rowmax == np.nextafter(m, F(0))) & (lab == -1)).any())
                hit("IoU one float above matched", (free & (rowmax == np.nextafter(m, F(1))) & (lab > 0)).any())
                hit("IoU one float below unmatched", (free & (rowmax == np.nextafter(u, F(0))) & (lab == 0)).any())
                hit("IoU == unmatched", (free & (rowmax == u) & (lab == -1)).any())
                hit("IoU one float above unmatched", (free & (rowmax == np.nextafter(u, F(1))) & (lab == -1)).any())
                a = d["anchors"]
                for j in range(len(rows)):
                    s = sel[j]
                    if s[3] == 4 and s[4] == 1 and rot_of(s[6]) < QUARTER:
                        under = (a[:, 0] == s[0]) & (a[:, 1] == s[1]) & (a[:, 3] == 2) & (a[:, 4] == 1) & (rot_of(a[:, 6]) < QUARTER)
                        hit("2 x 1 anchor under a concentric 4 x 1 gt gives 0.5", under.any() and (iou[under, j] == F(0.5)).all())
        assert labels.shape == out["box_cls_labels"].shape
    return got
