"""numpy restatement of modest_roi_targets_match / _sample and of the drop-in modest_amd.utils.roi_targets (DESIGN.md
section 7n): RoIHeadTemplate.assign_targets over ProposalTargetLayer.forward in the reference's float32 operations and
order.  The BEV overlap is oracle.labels.boxes_iou_bev(..., overlap_only=True, arith="f64"), the twin the device equals bit
for bit.  The draws are a callable, so a test can feed recorded picks or seeded generators; `reference_draws` makes the
reference's calls in the reference's order on numpy's and torch's CPU generators.

FAULTS names deliberately wrong variants; each must change the expected result of a named case of
tests/roi_targets_cases.py (tests/test_roi_targets_cpu.py holds them to that).
"""
import json

import numpy as np

from oracle import labels as ol

F = np.float32
LISTS = ("fg", "hard", "easy")
KEYS = ("rois", "gt_of_rois", "gt_iou_of_rois", "roi_scores", "roi_labels", "reg_valid_mask", "rcnn_cls_labels",
        "gt_of_rois_src")
TWO_PI, PI, HALF_PI, PI_3_2 = F(2 * np.pi), F(np.pi), F(np.pi * 0.5), F(np.pi * 1.5)

# fault -> the case of tests/roi_targets_cases.py whose expected result it changes
FAULTS = {
    "trim_first_zero": "gt_zero_between",      # trim stops at the first zero row instead of the last non-zero one
    "tie_highest": "duplicated_gts",           # equal maxima go to the highest gt row
    "hard_at_cls_fg": "cls_fg_below_reg_fg",   # hard is cut at CLS_FG_THRESH instead of REG_FG_THRESH
    "class_ignored": "labels_beyond",          # the class restriction is ignored
    "fg_strict": "thresh_at_fg",               # > where fg has >=
    "fold_no_first_remainder": "rois_1000",    # the heading fold lacks its first remainder
}
# The fold without its SECOND remainder is no fault: there h + pi lies in (3 pi / 2, 5 pi / 2), the step after it takes
# 2 pi off whatever exceeds pi, and both fmod(x, 2 pi) and x - 2 pi are exact for x in [2 pi, 4 pi), so every float32
# comes out the same.  EQUIVALENT names such variants; the CPU test holds them to changing nothing.
EQUIVALENT = {"fold_no_second_remainder": "rois_1000"}


def cfg_get(cfg, name, *default):
    if isinstance(cfg, dict):
        return cfg.get(name, *default) if default else cfg[name]
    return getattr(cfg, name, *default)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want, keys=KEYS):
    return all(np.asarray(got[k]).dtype == np.asarray(want[k]).dtype and np.asarray(got[k]).shape == np.asarray(want[k]).shape
               and np.array_equal(bits(got[k]), bits(want[k])) for k in keys)


def describe(got, want, keys=KEYS):
    out = []
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if g.dtype != w.dtype or g.shape != w.shape:
            out.append(f"{k}: {g.dtype}{g.shape} against {w.dtype}{w.shape}")
            continue
        bad = np.argwhere(bits(g) != bits(w))
        if len(bad):
            i = tuple(bad[0])
            out.append(f"{k}: {len(bad)} of {g.size} elements differ, first at {i}: {g[i]!r} against {w[i]!r}")
    return out


# ------------------------------------------------------------------------------------------------------------ the match call
def trim(gt, fault=None):
    """number of valid rows of one sample's (G, 7 + C + 1) gts: through the last row whose f32 sum in column order is not
    == 0, one row at the least"""
    gt = np.asarray(gt, F)
    if len(gt) == 0:
        return 1
    with np.errstate(all="ignore"):
        s = gt[:, 0].copy()
        for c in range(1, gt.shape[1]):
            s = s + gt[:, c]
    nz = np.flatnonzero(~(s == 0))
    if fault == "trim_first_zero":
        z = np.flatnonzero(s == 0)
        return max(1, int(z[0])) if len(z) else len(gt)
    return int(nz[-1]) + 1 if len(nz) else 1


def iou3d(a, b, arith="f64"):
    """boxes_iou3d_gpu (iou3d_nms_utils.py:57-81) of (n, 7) and (m, 7) in float32 -> (n, m)"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    with np.errstate(all="ignore"):
        bev = ol.boxes_iou_bev(a, b, overlap_only=True, arith=arith)
        two = F(2)
        a_top, a_bot = (a[:, 2] + a[:, 5] / two)[:, None], (a[:, 2] - a[:, 5] / two)[:, None]
        b_top, b_bot = (b[:, 2] + b[:, 5] / two)[None], (b[:, 2] - b[:, 5] / two)[None]
        d = np.minimum(a_top, b_top) - np.maximum(a_bot, b_bot)       # numpy's minimum / maximum hand a NaN on
        h = np.where(d < 0, F(0), d)
        o3 = bev * h
        va, vb = (a[:, 3] * a[:, 4] * a[:, 5])[:, None], (b[:, 3] * b[:, 4] * b[:, 5])[None]
        u = va + vb - o3
        return (o3 / np.where(u < F(1e-6), F(1e-6), u)).astype(F)


def match(rois, labels, gt, by_class, fault=None, arith="f64"):
    """one sample -> (max_iou (N,) float32, assignment (N,) int64, valid gts)"""
    rois, gt = np.asarray(rois, F), np.asarray(gt, F)
    n = trim(gt, fault)
    valid = gt[:n] if len(gt) else np.zeros((1, gt.shape[1]), F)
    iou = iou3d(rois[:, :7], valid[:, :7], arith)
    best, at, seen = np.zeros(len(rois), F), np.zeros(len(rois), np.int64), np.zeros(len(rois), bool)
    with np.errstate(all="ignore"):
        glab = valid[:, -1].astype(np.int64)
    for k in range(n):
        comp = np.ones(len(rois), bool)
        if by_class and fault != "class_ignored":
            comp = np.asarray(labels, np.int64) == glab[k]
        v = iou[:, k]
        with np.errstate(all="ignore"):
            more = (v >= best) if fault == "tie_highest" else (v > best)
        upd = comp & (~seen | more | (np.isnan(v) & ~np.isnan(best)))
        best[upd], at[upd] = v[upd], k
        seen |= comp
    return best, at, n


def lists(max_iou, cfg, fault=None):
    """-> [fg, hard, easy] roi rows, ascending"""
    reg_fg, cls_fg, lo = F(cfg_get(cfg, "REG_FG_THRESH")), F(cfg_get(cfg, "CLS_FG_THRESH")), F(cfg_get(cfg, "CLS_BG_THRESH_LO"))
    fg_t = min(reg_fg, cls_fg)
    with np.errstate(all="ignore"):
        fg = (max_iou > fg_t) if fault == "fg_strict" else (max_iou >= fg_t)
        hard = (max_iou < (cls_fg if fault == "hard_at_cls_fg" else reg_fg)) & (max_iou >= lo)
        easy = max_iou < lo
    return [np.flatnonzero(fg), np.flatnonzero(hard), np.flatnonzero(easy)]


def reference_draws(counts, cfg, np_random=None, generator=None, sample=0):
    """subsample_rois / sample_bg_inds (proposal_target_layer.py:117-192) on the list lengths alone
    -> (M, 2) int64 of (list, position)"""
    import torch
    npr = np.random if np_random is None else np_random
    M = int(cfg_get(cfg, "ROI_PER_IMAGE"))
    nf, nh, ne = (int(v) for v in counts)
    fg_per = int(np.round(cfg_get(cfg, "FG_RATIO") * M))
    picks = []

    def randint(lid, high, n):
        pos = torch.randint(low=0, high=high, size=(n,), generator=generator).long().numpy()
        picks.extend((lid, int(p)) for p in pos)

    def bg(n):
        if nh > 0 and ne > 0:
            hn = min(int(n * cfg_get(cfg, "HARD_BG_RATIO")), nh)
            randint(1, nh, hn)
            randint(2, ne, n - hn)
        elif nh > 0:
            randint(1, nh, n)
        else:
            randint(2, ne, n)

    if nf > 0 and nh + ne > 0:
        n_fg = min(fg_per, nf)
        picks.extend((0, int(p)) for p in npr.permutation(nf)[:n_fg])
        bg(M - n_fg)
    elif nf > 0:
        picks.extend((0, int(p)) for p in np.floor(npr.rand(M) * nf).astype(F).astype(np.int64))
    elif nh + ne > 0:
        bg(M)
    else:
        raise NotImplementedError(f"sample {sample}: FG={nf}, BG={nh + ne}")
    return np.asarray(picks, np.int64).reshape(-1, 2)


# ----------------------------------------------------------------------------------------------------------- the sample call
def rem(a, b):
    """torch's remainder of float32 by a float32 scalar: fmod, then the divisor's sign"""
    with np.errstate(all="ignore"):
        m = np.fmod(np.asarray(a, F), F(b))
        return np.where((m != 0) & ((F(b) < 0) != (m < 0)), m + F(b), m).astype(F)


def f32_trig(fn, v):
    with np.errstate(all="ignore"):
        return fn(np.asarray(v, F).astype(np.float64)).astype(F)


def canonical(rois, gt_src, fault=None):
    """roi_head_template.py:110-130 on (.., 7 + C) rois and their (.., 7 + C + 1) gts, in float32 steps"""
    rois, g = np.asarray(rois, F), np.array(gt_src, F)
    with np.errstate(all="ignore"):
        ry = rem(rois[..., 6], TWO_PI)
        x, y, z = g[..., 0] - rois[..., 0], g[..., 1] - rois[..., 1], g[..., 2] - rois[..., 2]
        c, s = f32_trig(np.cos, -ry), f32_trig(np.sin, -ry)
        zero, one = F(0), F(1)
        g[..., 0] = x * c + y * (-s) + z * zero          # (x, y, z) times [[c, s, 0], [-s, c, 0], [0, 0, 1]]
        g[..., 1] = x * s + y * c + z * zero
        g[..., 2] = x * zero + y * zero + z * one
        h = (g[..., 6] - ry) if fault == "fold_no_first_remainder" else rem(g[..., 6] - ry, TWO_PI)
        opp = (h > HALF_PI) & (h < PI_3_2)
        turned = h + PI if fault == "fold_no_second_remainder" else rem(h + PI, TWO_PI)
        h = np.where(opp, turned, h)
        h = np.where(h > PI, h - TWO_PI, h)
        h = np.where(h < -HALF_PI, -HALF_PI, h)
        h = np.where(h > HALF_PI, HALF_PI, h)
        g[..., 6] = h
    return g.astype(F)


def cls_labels(iou, cfg):
    kind = cfg_get(cfg, "CLS_SCORE_TYPE")
    fg, bg = cfg_get(cfg, "CLS_FG_THRESH"), cfg_get(cfg, "CLS_BG_THRESH")
    with np.errstate(all="ignore"):
        if kind == "cls":
            out = (iou > F(fg)).astype(np.int64)
            out[(iou > F(bg)) & (iou < F(fg))] = -1
            return out
        if kind == "roi_iou":
            is_fg, is_bg = iou > F(fg), iou < F(bg)
            out = is_fg.astype(F)
            mid = ~is_fg & ~is_bg
            out[mid] = (iou[mid] - F(bg)) / F(float(fg) - float(bg))
            return out
    raise NotImplementedError


def sample(picks, found, rois, scores, labels, gt, cfg, fault=None):
    """picks (B, M, 2); found: per sample (max_iou, assignment, lists) -> the eight outputs; a pick outside its list is a
    slot of zeros"""
    rois, gt = np.asarray(rois, F), np.asarray(gt, F)
    B, M, cols = len(rois), picks.shape[1], rois.shape[2]
    out = {"rois": np.zeros((B, M, cols), F), "gt_of_rois_src": np.zeros((B, M, cols + 1), F), "gt_iou_of_rois": np.zeros((B, M), F),
           "roi_scores": np.zeros((B, M), F), "roi_labels": np.zeros((B, M), np.int64)}
    ok = np.zeros((B, M), bool)
    for b in range(B):
        iou, at, ls = found[b]
        for m in range(M):
            lid, pos = int(picks[b, m, 0]), int(picks[b, m, 1])
            if not (0 <= lid < 3 and 0 <= pos < len(ls[lid])):
                continue
            r = ls[lid][pos]
            ok[b, m] = True
            out["rois"][b, m], out["roi_scores"][b, m], out["roi_labels"][b, m] = rois[b, r], np.asarray(scores, F)[b, r], labels[b][r]
            out["gt_iou_of_rois"][b, m] = iou[r]
            if gt.shape[1]:
                out["gt_of_rois_src"][b, m] = gt[b, at[r]]
    iou = out["gt_iou_of_rois"]
    with np.errstate(all="ignore"):
        out["reg_valid_mask"] = (iou > F(cfg_get(cfg, "REG_FG_THRESH"))).astype(np.int64)
    out["rcnn_cls_labels"] = cls_labels(iou, cfg)
    out["gt_of_rois"] = canonical(out["rois"], out["gt_of_rois_src"], fault)
    for k in ("gt_of_rois", "reg_valid_mask", "rcnn_cls_labels"):
        out[k][~ok] = 0
    return {k: out[k] for k in KEYS}


def assign_targets(rois, scores, labels, gt, cfg, draws=reference_draws, fault=None, details=None):
    """the drop-in on host arrays -> the reference's dict of eight; details (a dict) receives counts, found and picks"""
    rois, gt, labels = np.asarray(rois, F), np.asarray(gt, F), np.asarray(labels, np.int64)
    if cfg_get(cfg, "CLS_SCORE_TYPE") not in ("cls", "roi_iou"):
        raise NotImplementedError
    by_class = cfg_get(cfg, "SAMPLE_ROI_BY_EACH_CLASS", False)
    found = []
    for b in range(len(rois)):
        iou, at, _ = match(rois[b], labels[b], gt[b], by_class, fault)
        found.append((iou, at, lists(iou, cfg, fault)))
    counts = np.array([[len(l) for l in f[2]] for f in found], np.int32).reshape(len(rois), 3)
    picks = np.stack([np.asarray(draws(counts[b], cfg, sample=b), np.int64) for b in range(len(rois))]) if len(rois) else \
        np.zeros((0, int(cfg_get(cfg, "ROI_PER_IMAGE")), 2), np.int64)
    if details is not None:
        details.update(counts=counts, found=found, picks=picks)
    return sample(picks, found, rois, scores, labels, gt, cfg, fault)


def forward(rois, scores, labels, gt, cfg, draws=reference_draws):
    """ProposalTargetLayer.forward: seven keys, gt_of_rois not transformed"""
    out = assign_targets(rois, scores, labels, gt, cfg, draws)
    out["gt_of_rois"] = out.pop("gt_of_rois_src")
    return {k: out[k] for k in KEYS[:7]}


# ------------------------------------------------------------------------------------------------------------------ fixture
def scenes(rec):
    return json.loads(str(rec["scenes"]))


def scene_inputs(rec, name):
    """-> (cfg, (numpy seed, torch seed), rois, roi_scores, roi_labels, gt_boxes)"""
    cfg = json.loads(str(rec[name + "_cfg"]))
    return cfg, tuple(int(v) for v in rec[name + "_seeds"]), rec[name + "_in_rois"], rec[name + "_in_roi_scores"], \
        rec[name + "_in_roi_labels"], rec[name + "_gt_boxes"]


def recorded(rec, name):
    return {k: rec[name + "_" + k] for k in KEYS}
