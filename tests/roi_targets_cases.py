"""Small synthetic cases for modest_roi_targets_match / _sample and the drop-in: the smallest shapes
at which the kernels can go wrong.  Boxes are clustered as tests/iou3d_cases.py:proposals makes them: every roi is a moved
copy of one gt of its sample, aimed at one of the three lists and checked against the restatement.

case(name) -> dict(name, cfg, rois (B, N, 7 + C), roi_scores, roi_labels, gt_boxes (B, G, 7 + C + 1), seeds (numpy, torch),
finite, gt_view ("plain" | "strided"), raises, branches (per sample the lists the case claims non-empty, or None)).
T is the match kernel's gt tile and WG the rois a workgroup takes at a time, both from the Python module, so the registry
follows the kernel.  The class column is always a finite number.
"""
import functools

import numpy as np

import roi_targets_seq as seq
from modest_amd.utils import roi_targets as rt

F = np.float32
T, WG = rt.GT_TILE, rt.WORKGROUP
POINTRCNN = dict(ROI_PER_IMAGE=16, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True, CLS_SCORE_TYPE="cls", CLS_FG_THRESH=0.6,
                 CLS_BG_THRESH=0.45, CLS_BG_THRESH_LO=0.1, HARD_BG_RATIO=0.8, REG_FG_THRESH=0.55)
PVRCNN = dict(POINTRCNN, CLS_SCORE_TYPE="roi_iou", CLS_FG_THRESH=0.75, CLS_BG_THRESH=0.25)
SHIFT = {"fg": 0.08, "mid": 0.4, "hard": 0.55, "easy": 1.6}       # "mid": in fg and in hard at once (CLS_FG < REG_FG)
KINDS = ("fg", "hard", "easy")
HIT = {"fg": lambda ls: len(ls[0]) == 1 and len(ls[1]) == 0, "mid": lambda ls: len(ls[0]) == 1 and len(ls[1]) == 1,
       "hard": lambda ls: len(ls[1]) == 1 and len(ls[0]) == 0, "easy": lambda ls: len(ls[2]) == 1}


def objects(rng, n, C=0, classes=(1, 2, 3)):
    """n gts on a 9 m grid (no roi reaches two of them) -> (n, 7 + C + 1)"""
    i = np.arange(n)
    box = np.c_[9.0 * (i % 12) - 50, 9.0 * (i // 12) - 40, rng.uniform(-1.5, 0.5, n), rng.uniform(3.2, 4.8, n),
                rng.uniform(1.5, 2.0, n), rng.uniform(1.4, 1.7, n), rng.uniform(-3.2, 3.2, n)]
    return np.c_[box, rng.uniform(-1, 1, (n, C)), rng.choice(classes, n)].astype(F)


def moved(rng, obj, kind):
    b = obj[:7].astype(np.float64).copy()
    ang = rng.uniform(0, 2 * np.pi)
    b[:2] += SHIFT[kind] * rng.uniform(0.6, 1.4) * np.array([np.cos(ang), np.sin(ang)])
    b[2] += rng.normal(0, 0.03)
    b[3:6] *= rng.normal(1, 0.03, 3)
    b[6] += rng.normal(0, 0.05) + np.pi * (rng.random() < 0.3) + 2 * np.pi * rng.integers(-1, 2)
    return b.astype(F)


def sample(rng, cfg, gt, want, C=0):
    """rois of one sample whose maxima fall into the lists `want` (kind -> count) names, in random order"""
    by_class = cfg.get("SAMPLE_ROI_BY_EACH_CLASS", False)
    valid = gt[:seq.trim(gt)]
    live = np.flatnonzero(valid[:, 3] > 0) if (valid[:, 3] > 0).any() else np.arange(len(valid))
    rois, labels = [], []
    for kind, count in want.items():
        have = misses = 0
        while have < count:
            k = rng.choice(live)
            r = moved(rng, valid[k], kind if misses < 20 else str(rng.choice(list(SHIFT))))   # thresholds moved: any distance
            lab = np.int64(valid[k, -1])
            best, _, _ = seq.match(r[None], np.array([lab]), gt, by_class)
            ls = seq.lists(best, cfg)
            if not HIT[kind](ls):
                misses += 1
                continue
            rois.append(np.concatenate([r, rng.uniform(-1, 1, C).astype(F)]))
            labels.append(lab)
            have += 1
    perm = rng.permutation(len(rois))
    return np.stack(rois)[perm].astype(F), np.asarray(labels, np.int64)[perm]


def split(rng, n):
    """n rois over the three lists, each list non-empty where n allows"""
    if n < 3:
        return {"fg": n}
    c = rng.multinomial(n - 3, [0.35, 0.35, 0.3]) + 1
    return dict(zip(KINDS, (int(v) for v in c)))


def build(seed, B=2, N=24, valid=5, trailing=2, C=0, cfg=POINTRCNN, want=None, **more):
    """the generic case: B samples of N rois against `valid` gts and `trailing` zero rows"""
    rng = np.random.default_rng([2026, seed])
    cfg = dict(cfg)
    gts, rois, labels = [], [], []
    for b in range(B):
        g = np.zeros((valid + trailing, 8 + C), F)
        g[:valid] = objects(rng, valid, C)
        w = want[b] if isinstance(want, (list, tuple)) else want
        r, l = sample(rng, cfg, g, w or split(rng, N), C)
        gts.append(g), rois.append(r), labels.append(l)
    n = len(rois[0])
    return dict(cfg=cfg, rois=np.stack(rois), roi_scores=rng.random((B, n)).astype(F), roi_labels=np.stack(labels),
                gt_boxes=np.stack(gts), seeds=(1000 + seed, 2000 + seed), **dict(dict(finite=True, gt_view="plain", raises=None, branches=None), **more))


def _with(c, **kw):
    c.update(kw)
    return c


def _thresh_at(seed, key, kind, cfg=POINTRCNN):
    """`key` set to the float32 maximum of a roi of list `kind`, taken from the restatement"""
    c = build(seed, B=1, N=30, cfg=cfg)
    best, _, _ = seq.match(c["rois"][0], c["roi_labels"][0], c["gt_boxes"][0], True)
    r = seq.lists(best, c["cfg"])[KINDS.index(kind)][0]
    c["cfg"][key] = float(best[r])
    c["chosen"] = (int(r), float(best[r]))
    return c


def _gt_zero_between(seed):
    c = build(seed, B=2, N=24, valid=6, trailing=3)
    c["gt_boxes"][:, 2] = 0            # a zero row between valid rows stays; rois aimed at it now have maximum 0
    return c


def _duplicated(seed):
    c = build(seed, B=2, N=24, valid=4, trailing=1)
    g = c["gt_boxes"]
    c["gt_boxes"] = np.concatenate([g[:, :4], g[:, :4], g[:, 4:]], 1)      # every gt twice: equal maxima
    return c


def _labels_beyond(seed):
    c = build(seed, B=2, N=24)
    c["roi_labels"][:, ::3] = 9        # a class no gt has: maximum 0, assignment 0
    return c


def _nonfinite(seed):
    c = build(seed, B=2, N=40, valid=8, trailing=1)
    r, g = c["rois"], c["gt_boxes"]
    r[0, 0, 0], r[0, 1, 3], r[0, 2, 6], r[0, 3, 2] = np.nan, np.inf, -np.inf, np.nan
    r[0, 4, 3:6] = 0
    r[0, 5, 4] = -r[0, 5, 4]
    r[1, 0, 5], r[1, 1, 6] = np.inf, np.nan
    g[0, 1, 0], g[0, 2, 4], g[0, 3, 6] = np.nan, np.inf, np.nan
    g[0, 4, 3:6] = 0
    g[0, 5, 3] = -g[0, 5, 3]
    g[1, 7, 2] = -np.inf               # the last valid row: its sum is not a number, it stays
    c["finite"] = False
    return c


def _all_nan(seed):
    c = build(seed, B=2, N=8)
    c["rois"][1] = np.nan
    return _with(c, finite=False, raises=NotImplementedError)


def _one_member(seed, wants):
    c = build(seed, B=len(wants), N=0, want=wants)
    c["branches"] = [tuple(k for k in KINDS if w.get(k)) for w in wants]
    return c


BUILDERS = {}
for _n in (1, 63, 64, 65, WG - 1, WG, WG + 1, 1000):
    BUILDERS[f"rois_{_n}"] = functools.partial(build, 10 + len(BUILDERS), B=2 if _n < 1000 else 1, N=_n,
                                               cfg=dict(POINTRCNN, ROI_PER_IMAGE=128) if _n == 1000 else POINTRCNN)
BUILDERS["gts_zero_box"] = functools.partial(build, 30, valid=0, trailing=3, want={"easy": 12})
for _n in (1, T - 1, T, T + 1, 2 * T + 1):
    BUILDERS[f"gts_{_n}"] = functools.partial(build, 31 + len(BUILDERS), B=2, N=32, valid=_n, trailing=1)
for _n in (0, 1, 40):
    BUILDERS[f"gt_trailing_{_n}"] = functools.partial(build, 40 + _n, trailing=_n)
BUILDERS["gt_zero_between"] = functools.partial(_gt_zero_between, 45)
for _n in (1, 3, 300):
    BUILDERS[f"batch_{_n}"] = functools.partial(build, 50 + _n % 7, B=_n, N=8, valid=3)
BUILDERS["m_1"] = functools.partial(build, 60, cfg=dict(POINTRCNN, ROI_PER_IMAGE=1))
BUILDERS["m_128"] = functools.partial(build, 61, cfg=dict(POINTRCNN, ROI_PER_IMAGE=128))
BUILDERS["m_512"] = functools.partial(build, 62, N=100, cfg=dict(POINTRCNN, ROI_PER_IMAGE=512))
BUILDERS["one_fg"] = functools.partial(_one_member, 70, [dict(fg=1, hard=9, easy=6), dict(fg=1, hard=15), dict(fg=1, easy=15)])
BUILDERS["fg_only"] = functools.partial(_one_member, 71, [dict(fg=1), dict(fg=1)])
BUILDERS["one_hard"] = functools.partial(_one_member, 72, [dict(hard=1, easy=11), dict(fg=4, hard=1, easy=7)])
BUILDERS["one_easy"] = functools.partial(_one_member, 73, [dict(hard=11, easy=1), dict(fg=4, hard=7, easy=1)])
BUILDERS["fg_only_many"] = functools.partial(_one_member, 74, [dict(fg=20), dict(fg=20)])
BUILDERS["cls_fg_below_reg_fg"] = functools.partial(build, 80, cfg=dict(POINTRCNN, CLS_FG_THRESH=0.3, CLS_BG_THRESH=0.2),
                                                    want=dict(fg=8, mid=10, hard=10, easy=8))
BUILDERS["thresh_at_fg"] = functools.partial(_thresh_at, 81, "REG_FG_THRESH", "hard")
BUILDERS["thresh_at_reg_fg"] = functools.partial(_thresh_at, 82, "REG_FG_THRESH", "fg")
BUILDERS["thresh_at_cls_fg"] = functools.partial(_thresh_at, 83, "CLS_FG_THRESH", "fg")
BUILDERS["thresh_at_cls_bg"] = functools.partial(_thresh_at, 84, "CLS_BG_THRESH", "hard")
BUILDERS["thresh_at_cls_bg_roi_iou"] = functools.partial(_thresh_at, 85, "CLS_BG_THRESH", "hard", PVRCNN)
BUILDERS["thresh_at_lo"] = functools.partial(_thresh_at, 86, "CLS_BG_THRESH_LO", "hard")
BUILDERS["duplicated_gts"] = functools.partial(_duplicated, 90)
BUILDERS["nonfinite"] = functools.partial(_nonfinite, 91)
BUILDERS["all_nan"] = functools.partial(_all_nan, 92)
BUILDERS["c_2"] = functools.partial(build, 93, C=2)
BUILDERS["c_2_roi_iou"] = functools.partial(build, 94, C=2, cfg=dict(PVRCNN, ROI_PER_IMAGE=32))
BUILDERS["labels_beyond"] = functools.partial(_labels_beyond, 95)
BUILDERS["strided_gt"] = functools.partial(build, 96, gt_view="strided")
BUILDERS["by_class_off"] = functools.partial(build, 97, cfg=dict(POINTRCNN, SAMPLE_ROI_BY_EACH_CLASS=False))
BUILDERS["by_class_off_roi_iou"] = functools.partial(build, 98, cfg=dict(PVRCNN, SAMPLE_ROI_BY_EACH_CLASS=False))
BUILDERS["roi_iou"] = functools.partial(build, 99, N=40, cfg=PVRCNN)
NAMES = tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    c = BUILDERS[name]()
    c.setdefault("gt_view", "plain")
    c["name"] = name
    for k in ("rois", "roi_scores", "roi_labels", "gt_boxes"):
        c[k] = np.ascontiguousarray(c[k])
        c[k].setflags(write=False)
    return c


def seeded_draws(c):
    """the case's seeds put into numpy's and torch's global generators -> seq.reference_draws"""
    import torch
    np.random.seed(c["seeds"][0])
    torch.manual_seed(c["seeds"][1])
    return seq.reference_draws


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> (the restatement's eight outputs, details) under the case's seeds; computed once and shared"""
    c = case(name)
    details = {}
    out = seq.assign_targets(c["rois"], c["roi_scores"], c["roi_labels"], c["gt_boxes"], c["cfg"], seeded_draws(c), details=details)
    return out, details
