"""Cases of the post-processing op shared by tests/test_post_process_cpu.py and tests/test_gpu_post_process.py, built from
the clustered NMS proposals of tests/iou3d_cases.py (96 jittered copies of each of 48 objects).  Each is the smallest shape
at which the kernels of csrc/post_process.hip can still go wrong; `present(case, info)` asserts from the inputs and
the restatement that the edge the case is named after is there.

A case is a dict of the arguments of post_process_seq.post_process / modest_amd.ops.post_process -- box, cls (stacked (n, .)
with batch_index, or dense (B, N, .) with batch_index None), B, pre, post, nms_thresh, rotated, score_thresh, normalized,
output_raw_score, labels, gt_boxes, rois, recall_thresh -- and `present`.  want(case) is the restatement's result, computed
once per case and read-only.  info(case): per sample the passing rows, the candidates, the survivors and the chunked
walk's statistics.
"""
import functools

import numpy as np

import iou3d_cases as ic
import post_process_seq as seq
import proposals_seq as ps

F = np.float32
TILE = 64          # boxes of a list the recall kernel stages at a time: modest_post_process_tile() (a GPU test holds them equal)
LANES = 256        # four rounds of the 64 gts a recall workgroup takes at a time
BIG = 4096         # NMS_PRE_MAXSIZE of the reference's test configs
RECALL = (0.3, 0.5, 0.7)      # RECALL_THRESH_LIST of the reference's configs
PAYLOAD = 0x7FC12345          # a quiet NaN with a payload: extra box columns are copied, never computed with
ARGS = ("B", "pre", "post", "nms_thresh", "rotated", "score_thresh", "normalized", "output_raw_score", "labels", "batch_index",
        "gt_boxes", "rois", "recall_thresh")


def pool(offset=0.0):
    p, sc = ic.proposals(offset)
    return np.array(p), np.array(sc)


def objects(offset=0.0, n=48, rng=None, jitter=0.1):
    """n gts near the pool's objects: one pool row per object cluster found greedily, moved a little; (n, 8) with a class"""
    p, _ = pool(offset)
    rng = np.random.default_rng(21) if rng is None else rng
    take = p[rng.choice(len(p), n, replace=n > len(p))].copy()
    take[:, :2] += rng.normal(0, jitter, (n, 2)).astype(F)
    return np.concatenate([take, rng.integers(1, 4, (n, 1)).astype(F)], 1).astype(F)


def make(box, cls, B=1, bidx="zeros", **kw):
    box = np.ascontiguousarray(box, F)
    cls = np.ascontiguousarray(cls, F)
    if bidx is not None:
        cls = cls.reshape(len(box), -1)
        if isinstance(bidx, str):
            bidx = np.zeros(len(box), F)
        bidx = np.ascontiguousarray(bidx)
    c = dict(box=box, cls=cls, batch_index=bidx, B=B, pre=BIG, post=100, nms_thresh=0.7, rotated=True, score_thresh=0.1,
             normalized=True, output_raw_score=False, labels=None, gt_boxes=None, rois=None, recall_thresh=(),
             present=lambda c, info: True)
    c.update(kw)
    return c


def with_gts(c, n=6, seed=21):
    """a (B, n, 7 + C + 1) gt tensor near the pool's objects and the reference's three thresholds"""
    cols = c["box"].shape[-1]
    gt = np.zeros((c["B"], n, cols + 1), F)
    for b in range(c["B"]):
        o = objects(0.0, n, np.random.default_rng([seed, b]))
        gt[b, :, :7], gt[b, :, -1] = o[:, :7], o[:, 7]
    c.update(gt_boxes=gt, recall_thresh=RECALL)
    return c


def info(c):
    """per sample: passing rows, candidates, survivors, the chunked walk's statistics"""
    box, cls, per = ps._flat(c["box"], c["cls"], c["batch_index"])
    raw, _ = ps.score_label(cls)
    score = raw if c["normalized"] else seq.sigmoid(raw)
    smp = ps.sample_of(c["batch_index"], len(box), c["B"], per)
    out = []
    for b in range(c["B"]):
        rows = np.flatnonzero(smp == b)
        with np.errstate(invalid="ignore"):
            ok = np.ones(len(rows), bool) if c["score_thresh"] is None else score[rows] >= F(c["score_thresh"])
        rows = rows[ok]
        cand = rows[ps.candidates(score[rows], np.zeros(len(rows), np.int64), 1, c["pre"])[0]]
        one = dict(chunks=0, tests=0, last_in_chunk=None, left_behind=False)
        kept = ps.chunked_walk(box[cand], c["nms_thresh"], c["rotated"], c["post"], stats=one) if len(cand) else []
        one.update(passing=len(rows), candidates=len(cand), kept=len(kept), scores=score[cand])
        out.append(one)
    return out


# ------------------------------------------------------------------------------------------------ passing candidates
def passing(n, rotated=True, thr=0.1, normalized=True, gts=6):
    """n rows at or above the threshold among 200 below it, shuffled"""
    def build():
        p, sc = pool()
        x = sc if normalized else ((sc - F(0.5)) * F(8)).astype(F)      # logits in [-4, 4)
        s = x if normalized else seq.sigmoid(x)
        hi, lo = np.flatnonzero(s >= F(thr))[:n], np.flatnonzero(s < F(thr))[:200]
        rows = np.concatenate([hi, lo])[np.random.default_rng(31).permutation(n + 200)]
        c = make(p[rows], x[rows], rotated=rotated, score_thresh=thr, normalized=normalized,
                 present=lambda c, i: i[0]["passing"] == n == i[0]["candidates"] and (n == 0) == (i[0]["kept"] == 0)
                 and len(c["box"]) == n + 200)
        return with_gts(c, gts) if gts else c
    return build


def pre_after_threshold():
    """300 passing rows, 5 NaN scores and 200 failing ones, PRE 100: the NaNs would take five of the hundred places"""
    p, sc = pool()
    hi, lo = np.flatnonzero(sc >= F(0.1))[:300], np.flatnonzero(sc < F(0.1))[:205]
    s = sc.copy()
    s[lo[:5]] = np.nan
    rows = np.concatenate([hi, lo])[np.random.default_rng(32).permutation(505)]
    return with_gts(make(p[rows], s[rows], pre=100, post=100, nms_thresh=0.85,
                         present=lambda c, i: i[0]["passing"] == 300 and i[0]["candidates"] == 100
                         and int(np.isnan(c["cls"]).sum()) == 5))


def pre_cuts_a_tie():
    p, sc = pool()
    q = (np.floor(sc[:1000] * 50) / 50).astype(F)      # about 20 rows per score

    def present(c, i):
        s = i[0]["scores"]
        order = np.argsort(ps.descending_bits(q[q >= F(0.1)]), kind="stable")
        return len(s) == 200 and q[q >= F(0.1)][order[199]] == q[q >= F(0.1)][order[200]] and i[0]["passing"] > 800
    return make(p[:1000], q, pre=200, post=512, nms_thresh=0.85, present=present)


def post_inside_a_chunk():
    p, sc = pool()
    return with_gts(make(p, sc, post=100, nms_thresh=0.85,
                         present=lambda c, i: i[0]["kept"] == 100 and i[0]["left_behind"]
                         and 0 < i[0]["last_in_chunk"] < ps.CHUNK - 1 and 4000 < i[0]["passing"] < 4608), 48)


def post_never_reached():
    p, sc = pool()
    return make(p, sc, post=100, nms_thresh=0.01, present=lambda c, i: 20 <= i[0]["kept"] < 100 and i[0]["passing"] > 4000)


def score_thresh_of(thr, rotated=True):
    def build():
        p, sc = pool()
        return with_gts(make(p[:1000], sc[:1000], score_thresh=thr, rotated=rotated, post=200,
                             present=lambda c, i: i[0]["passing"] == int((sc[:1000] >= F(thr)).sum()) < 1000
                             and i[0]["kept"] >= 20), 12)
    return build


# ------------------------------------------------------------------------------------------------ scores
def score_equal_to_thresh():
    p, sc = pool()
    s = sc[:300].copy()
    s[[3, 50, 51, 299]] = F(0.1)
    s[[4, 52]] = np.nextafter(F(0.1), F(0))

    def present(c, i):
        sel = want(c)[0][0][1]
        return int((sel == F(0.1)).sum()) >= 1 and not (sel < F(0.1)).any() and float(F(0.1)) != 0.1
    return make(p[:300], s, post=300, nms_thresh=0.85, score_thresh=0.1, present=present)


def non_finite_scores(thr):
    def build():
        p, sc = pool()
        cls = np.stack([sc[:300], sc[300:600], sc[600:900]], 1).copy()
        cls[7, 1] = np.nan
        cls[200, 0] = cls[200, 2] = np.nan
        cls[11] = [np.inf, 0.1, np.inf]
        cls[12] = [-np.inf, -np.inf, -np.inf]
        cls[13] = [-0.0, -1.0, -2.0]
        cls[14] = [0.0, -0.0, -1.0]

        def present(c, i):
            boxes, scores, labels = want(c)[0][0]
            has = lambda r: bool((boxes.view(np.uint32) == c["box"][r].view(np.uint32)).all(1).any())      # noqa: E731
            if thr is None:      # NaN first, every row a candidate
                return np.isnan(scores[:2]).all() and labels[0] == 2 and np.isposinf(scores[2]) and i[0]["passing"] == 300
            zero_in = thr <= 0
            return (not np.isnan(scores).any() and np.isposinf(scores[0]) and labels[0] == 1 and not has(7) and not has(200)
                    and not has(12) and i[0]["passing"] < 300 and has(13) == zero_in and has(14) == zero_in)
        box = p[:300].copy()
        box[[7, 200, 11, 12, 13, 14], 0] += F(0.5)      # none of them an exact duplicate of another row
        # NMS at 0.99 keeps nearly every candidate, so membership shows what passed
        return make(box, cls, post=300, nms_thresh=0.99, score_thresh=thr, present=present)
    return build


SATURATED = np.array([18.0, 18.5, 40.0, 17.5, 16.0, -104.0, -110.0, -90.0, -88.5, -103.0, 15.5, 19.0], F)


def saturating_logits():
    """logits whose sigmoid rounds to 1 (ties, by ascending row), to 0 and to denormals; no threshold"""
    p, sc = pool()
    x = ((sc[:200] - F(0.5)) * F(8)).astype(F)
    x[:len(SATURATED)] = SATURATED

    def present(c, i):
        s = seq.sigmoid(SATURATED)
        boxes, scores, _ = want(c)[0][0]
        ones = np.flatnonzero(s == 1)
        at = [int(np.flatnonzero((boxes.view(np.uint32) == c["box"][r].view(np.uint32)).all(1))[0]) for r in ones]
        return (len(ones) >= 4 and at == sorted(at) and (s[[5, 6]] == 0).all() and ((s[[7, 8]] > 0) & (s[[7, 8]] < np.finfo(F).tiny)).all()
                and len(np.unique(SATURATED[ones])) == len(ones) and (np.diff(SATURATED[ones]) < 0).any() and i[0]["kept"] == 200)
    return make(p[:200], x, post=200, nms_thresh=2.0, score_thresh=None, normalized=False, present=present)


# ------------------------------------------------------------------------------------------------ classes and labels
def class_ties(K, C, normalized=True, raw_out=False):
    def build():
        p, sc = pool()
        n = 500
        s = sc[:n] if normalized else ((sc[:n] - F(0.5)) * F(8)).astype(F)
        if K == 3:
            cls = np.stack([s, s, s - F(0.5)], 1).copy()
            cls[::3, 2] = s[::3]
            cls[1::3, 0] = s[1::3] - F(1)
        else:
            cls = s[:, None].copy()
        box = np.concatenate([p[:n], np.random.default_rng(5).random((n, C)).astype(F)], 1) if C else p[:n]

        def present(c, i):
            _, scores, labels = want(c)[0][0]
            neg = (scores < 0).any()
            return (c["box"].shape[1] == 7 + C and set(labels) == ({1, 2} if K == 3 else {1}) and i[0]["kept"] >= 20
                    and neg == (raw_out and not normalized))
        return with_gts(make(box, cls, post=500, normalized=normalized, output_raw_score=raw_out, present=present))
    return build


def given_labels(shape3):
    """dense, B = 2, K = 1, labels 1 .. 3 given as (B, N) or (B, N, 1)"""
    def build():
        p0, s0 = pool()
        p1, s1 = pool(60.0)
        n = 300
        box, cls = np.stack([p0[:n], p1[:n]]), np.stack([s0[:n], s1[:n]])[..., None]
        labels = np.random.default_rng(41).integers(1, 4, (2, n, 1) if shape3 else (2, n)).astype(np.int64)

        def present(c, i):
            got = want(c)[0]
            return all(set(g[2]) == {1, 2, 3} for g in got) and c["labels"].ndim == (3 if shape3 else 2)
        return with_gts(make(box, cls, B=2, bidx=None, labels=labels, present=present))
    return build


# ------------------------------------------------------------------------------------------------ batch forms
def three_samples():
    """stacked: 1 000 / 300 / 0 rows, interleaved, float32 batch_index, six strays that would win every sample"""
    p0, s0 = pool()
    p1, s1 = pool(60.0)
    box = np.concatenate([p0[:1000], p1[:300], p1[1000:1006]])
    cls = np.concatenate([s0[:1000], s1[:300], np.full(6, 2.0, F)])
    bidx = np.concatenate([np.zeros(1000, F), np.ones(300, F), np.array([3, -1, 0.5, np.nan, 2.5, 1e9], F)])
    perm = np.random.default_rng(6).permutation(len(box))

    def present(c, i):
        return ([o["passing"] > 0 for o in i] == [True, True, False] and i[0]["kept"] != i[1]["kept"] and i[2]["kept"] == 0
                and not any((g[1] == 2).any() for g in want(c)[0]))
    return with_gts(make(box[perm], cls[perm], B=3, bidx=bidx[perm], post=300, present=present))


def dense(rotated=True, raw=False):
    """B = 3 samples of 600 rows, K = 3, C = 2; the extra column carries a NaN payload"""
    def build():
        p0, s0 = pool()
        p1, s1 = pool(60.0)
        rng = np.random.default_rng(8)
        n = 600
        box = np.stack([p0[:n], p1[:n], p0[1000:1000 + n]])
        extra = rng.random((3, n, 2)).astype(F)
        extra[..., 0] = np.array([PAYLOAD], np.uint32).view(F)[0]
        box = np.concatenate([box, extra], 2)
        cls = np.stack([np.stack([s0[:n], s0[1000:1000 + n], s0[2000:2000 + n]], 1), np.stack([s1[:n], s1[1000:1000 + n], s1[2000:2000 + n]], 1),
                        np.stack([s0[3000:3000 + n], s1[3000:3000 + n], s1[2000:2000 + n]], 1)])
        if raw:
            cls = ((cls - F(0.5)) * F(8)).astype(F)

        def present(c, i):
            got = want(c)[0]
            return all((g[0][:, 7].view(np.uint32) == PAYLOAD).all() and len(g[0]) >= 20 for g in got) and c["box"].shape == (3, n, 9)
        return with_gts(make(box, cls, B=3, bidx=None, rotated=rotated, normalized=not raw, present=present))
    return build


# ------------------------------------------------------------------------------------------------ recall
def gts_of(n, zeros_after=0, nan_row=None, all_zero=False, thresholds=RECALL):
    """1 000 rows; n gts (then `zeros_after` rows of zeros), recall from the final boxes"""
    def build():
        p, sc = pool()
        c = make(p[:1000], sc[:1000], post=200)
        gt = np.zeros((1, n + zeros_after, 8), F)
        if n and not all_zero:
            gt[0, :n] = objects(0.0, n, np.random.default_rng([22, n]), jitter=0.4)
        if nan_row is not None:
            gt[0, nan_row, 0] = np.nan
        c.update(gt_boxes=gt, recall_thresh=thresholds)

        def present(c, i):
            r = want(c)[1]
            valid = 1 if all_zero and n + zeros_after else n
            ok = r["gt"] == valid and not any(r["roi"]) and len(r["rcnn"]) == len(thresholds) and (n > 0 or not any(r["rcnn"]))
            if valid > 8 and thresholds:
                ok = ok and r["rcnn"][0] > r["rcnn"][-1] > 0
            return ok and c["gt_boxes"].shape[1] == n + zeros_after
        c["present"] = present
        return c
    return build


def zero_between():
    """gts with a row of zeros in the middle and two behind: the last non-zero row ends the list, the zero row counts"""
    c = gts_of(10, zeros_after=2)()
    gt = c["gt_boxes"].copy()
    gt[0, 4] = 0
    c["gt_boxes"] = gt
    c["present"] = lambda c, i: want(c)[1]["gt"] == 10 and not c["gt_boxes"][0, 4].any() and c["gt_boxes"].shape[1] == 12
    return c


def nan_gt():
    c = gts_of(10, nan_row=3)()
    inner = c["present"]
    c["present"] = lambda c, i: inner(c, i) and want(c)[1]["rcnn"][0] <= 9 and np.isnan(c["gt_boxes"][0, 3, 0])
    return c


def rois_present(n_rois=100, n_gt=30):
    """dense, B = 2, 300 rows and n_rois rois a sample: "rcnn" counts over ALL rows, "roi" over the rois"""
    def build():
        c = given_labels(False)()
        rois = np.stack([pool()[0][2000:2000 + n_rois], pool(60.0)[0][2000:2000 + n_rois]])
        c = with_gts(c, n_gt, seed=23)
        c.update(rois=np.ascontiguousarray(rois, F), score_thresh=0.7, post=50)

        def present(c, i):
            r = want(c)[1]
            final = seq.post_process(c["box"], c["cls"], **{k: c[k] for k in ARGS}, fault="recall_from_final")[1]
            return r["gt"] == 2 * n_gt and any(r["roi"]) and r["roi"] != r["rcnn"] and final["rcnn"] != r["rcnn"] and c["rois"].shape[1] == n_rois
        c["present"] = present
        return c
    return build


def recall_tie():
    """a threshold that equals one gt's maximum exactly: > does not count it"""
    c = gts_of(12)()
    preds, _ = seq.post_process(c["box"], c["cls"], **{k: c[k] for k in ARGS})
    best = seq.max_iou(preds[0][0], c["gt_boxes"][0, :, :7])
    tie = float(np.sort(best)[len(best) // 2])
    c["recall_thresh"] = (0.3, tie, 0.7)
    c["tie"] = tie

    def present(c, i):
        return F(tie) == tie and int((best == F(tie)).sum()) >= 1 and 0 < tie < 1
    c["present"] = present
    return c


# ------------------------------------------------------------------------------------------------ limits
def post_full():
    p, sc = pool()
    return make(p, sc, post=seq.POST_MAX, nms_thresh=0.9, score_thresh=0.01,
                present=lambda c, i: i[0]["kept"] == 1024 == seq.POST_MAX and i[0]["chunks"] >= 17)


def many_samples():
    """B = 65535 dense samples of 2 rows, the second below the threshold in every other sample; two gts a sample"""
    B = seq.BATCH_MAX
    p, sc = pool()
    s = np.arange(B)
    i, j = s % 4608, (s * 7 + 1 + s // 4608) % 4608
    box = np.stack([p[i], p[j]], 1)
    cls = np.stack([sc[i] * F(0.5) + F(0.5), np.where(s % 2 == 0, F(0.05), sc[j] * F(0.25) + F(0.125))], 1)[..., None]
    gt = np.zeros((B, 2, 8), F)
    gt[:, 0, :7], gt[:, 0, 7] = p[i], 1

    def present(c, inf):
        preds, r = want(c)
        n = np.array([len(g[0]) for g in preds])
        return c["B"] == B == 65535 and set(n) == {1, 2} and r["gt"] == B and r["rcnn"] == [B, B, B]
    c = make(box, cls, B=B, bidx=None, post=2, present=present)
    c.update(gt_boxes=gt, recall_thresh=RECALL)
    return c


def wide(box_cols=7, cls_cols=1):
    """130 rows, one of the two widths at its limit of 4096"""
    def build():
        p, sc = pool()
        n = 130
        rng = np.random.default_rng(10)
        box = np.concatenate([p[:n], rng.random((n, box_cols - 7)).astype(F)], 1)
        cls = rng.random((n, cls_cols)).astype(F) * F(0.05)
        r = np.arange(n)
        top = (sc[:n] * F(0.5) + F(0.5)).astype(F)
        if cls_cols > 1:
            cls[r[0::3], 4000 + r[0::3] % 96] = top[0::3]
            cls[1::3, 0] = top[1::3]
            cls[2::3, 5] = cls[2::3, 4095] = top[2::3]
        else:
            cls[:, 0] = top

        def present(c, i):
            boxes, _, labels = want(c)[0][0]
            lab = set(labels)
            return (c["box"].shape[1] == box_cols and c["cls"].shape[1] == cls_cols and 4096 in (box_cols, cls_cols) and len(boxes) >= 20
                    and boxes[:, -1].all() and (cls_cols == 1 or (1 in lab and 6 in lab and 4096 not in lab and max(lab) > 4000)))
        return with_gts(make(box, cls, post=70, nms_thresh=0.85, present=present))
    return build


def sixteen_thresholds():
    c = gts_of(40, thresholds=tuple(round(0.05 * k, 2) for k in range(1, 17)))()
    inner = c["present"]
    c["present"] = lambda c, i: inner(c, i) and len(c["recall_thresh"]) == seq.THRESH_MAX == 16 and len(set(want(c)[1]["rcnn"])) >= 4
    return c


CASES = {
    "pass 0": passing(0), "pass 1": passing(1), "pass 63": passing(63), "pass 64": passing(64), "pass 65": passing(65),
    "pass 129": passing(129), "pass 65 axis-aligned": passing(65, rotated=False), "pass 129 logits": passing(129, normalized=False),
    "pass 64 logits, threshold 0.7": passing(64, thr=0.7, normalized=False),
    "PRE cuts after the threshold": pre_after_threshold, "PRE cuts a tie": pre_cuts_a_tie,
    "POST inside a chunk": post_inside_a_chunk, "POST never reached": post_never_reached,
    "threshold 0.01": score_thresh_of(0.01), "threshold 0.1": score_thresh_of(0.1), "threshold 0.7": score_thresh_of(0.7),
    "threshold 0.1 axis-aligned": score_thresh_of(0.1, False), "threshold 0.7 axis-aligned": score_thresh_of(0.7, False),
    "score equal to SCORE_THRESH": score_equal_to_thresh, "non-finite scores": non_finite_scores(0.1),
    "non-finite scores, threshold 0": non_finite_scores(0.0), "no threshold": non_finite_scores(None),
    "saturating logits": saturating_logits,
    "K 1": class_ties(1, 0), "K 3 with equal maxima, C 2": class_ties(3, 2), "K 3 logits": class_ties(3, 0, normalized=False),
    "OUTPUT_RAW_SCORE": class_ties(3, 0, normalized=False, raw_out=True),
    "OUTPUT_RAW_SCORE normalised": class_ties(1, 0, raw_out=True),
    "given labels": given_labels(False), "given labels (B, N, 1)": given_labels(True),
    "3 samples and strays": three_samples, "dense": dense(), "dense axis-aligned logits": dense(False, True),
    "gt 0": gts_of(0), "gt 1": gts_of(1), "gt 63": gts_of(TILE - 1), "gt 64": gts_of(TILE), "gt 65": gts_of(TILE + 1),
    "gt 255": gts_of(LANES - 1), "gt 257": gts_of(LANES + 1),
    "trailing zero rows": gts_of(10, zeros_after=5), "zero row between": zero_between, "all-zero gts": gts_of(0, zeros_after=5, all_zero=True),
    "empty threshold list": gts_of(10, thresholds=()), "NaN gt": nan_gt, "rois present": rois_present(),
    "rois 65, gts 65": rois_present(TILE + 1, TILE + 1), "recall tie": recall_tie,
    "POST 1024 full": post_full, "B 65535": many_samples, "4096 box columns": wide(box_cols=4096),
    "4096 class columns": wide(cls_cols=4096), "16 thresholds": sixteen_thresholds,
}
assert set(seq.FAULTS.values()) <= set(CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    for k in ("box", "cls", "batch_index", "labels", "gt_boxes", "rois"):
        if c[k] is not None:
            c[k].setflags(write=False)
    c["name"] = name
    return c


def args(c):
    return {k: c[k] for k in ARGS}


_WANT = {}


def want(c, **kw):
    """the restatement's (preds, recall), computed once per case"""
    key = c.get("name", id(c))
    if kw:
        return seq.post_process(c["box"], c["cls"], **args(c), **kw)
    if key not in _WANT:
        _WANT[key] = seq.post_process(c["box"], c["cls"], **args(c))
        for g in _WANT[key][0]:
            for a in g:
                a.setflags(write=False)
    return _WANT[key]


def is_distinct(c):
    """no order is open: normalised scores pairwise distinct within every sample, class values pairwise distinct within
    every row, no NaN"""
    box, cls, per = ps._flat(c["box"], c["cls"], c["batch_index"])
    raw, _ = ps.score_label(cls)
    score = raw if c["normalized"] else seq.sigmoid(raw)
    smp = ps.sample_of(c["batch_index"], len(box), c["B"], per)
    if np.isnan(cls).any():
        return False
    if cls.shape[1] > 1 and (np.diff(np.sort(cls, 1), axis=1) == 0).any():
        return False
    return all(len(np.unique(score[smp == s])) == int((smp == s).sum()) for s in range(c["B"]))
