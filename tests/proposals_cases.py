"""Cases of the RoI proposal layer shared by tests/test_proposals_cpu.py and tests/test_gpu_proposals.py, built from the
clustered NMS proposals of tests/iou3d_cases.py (96 jittered copies of each of 48 objects, exact duplicates among them).
Each is the smallest shape at which the walk of csrc/proposals.hip can still go wrong; `present(case, stats)` asserts from
the inputs and the restatement that the edge the case is named after is there.

CASES are the shapes of the workloads; EDGE_CASES (below them) the inputs of a diverged or untrained detector and the
kernel's limits themselves.

A case is a dict: box, cls (numpy, stacked (n, .) or dense (B, N, .)), batch_index (None: dense), B, pre, post, thresh,
rotated, present.  want(case) is the restatement's result, computed once per case and read-only.
"""
import functools

import numpy as np

import iou3d_cases as ic
import proposals_seq as seq

F = np.float32
CHUNK, WAVES = seq.CHUNK, seq.WAVES
BIG = 9000     # NMS_PRE_MAXSIZE of the reference's configs


def pool(offset=0.0):
    p, sc = ic.proposals(offset)
    return np.array(p), np.array(sc)


def stacked(box, cls, B=1, bidx=None, **kw):
    box, cls = np.ascontiguousarray(box, F), np.ascontiguousarray(cls, F).reshape(len(box), -1)
    if bidx is None:
        bidx = np.zeros(len(box), F)
    c = dict(box=box, cls=cls, batch_index=np.ascontiguousarray(bidx), B=B, pre=BIG, post=100, thresh=0.7, rotated=True,
             present=lambda c, st: True)
    c.update(kw)
    return c


def stats_of(c, rows_of=None):
    """per sample: the chunked walk's statistics (proposals_seq.chunked_walk), its candidates and survivors; rows_of (a
    list) receives each sample's surviving rows"""
    box, cls, n_per = seq._flat(c["box"], c["cls"], c["batch_index"])
    score, _ = seq.score_label(cls)
    smp = seq.sample_of(c["batch_index"], len(box), c["B"], n_per)
    per = []
    for cand in seq.candidates(score, smp, c["B"], c["pre"]):
        one = dict(chunks=0, tests=0, last_in_chunk=None, left_behind=False)
        kept = seq.chunked_walk(box[cand], c["thresh"], c["rotated"], c["post"], stats=one) if len(cand) else []
        one.update(candidates=len(cand), kept=len(kept))
        per.append(one)
        if rows_of is not None:
            rows_of.append(cand[kept] if len(cand) else cand)
    return per


def n_rows(n, rotated=True):
    def make():
        p, sc = pool()
        return stacked(p[:n], sc[:n], rotated=rotated, present=lambda c, st: st[0]["candidates"] == n and 1 <= st[0]["kept"] <= n)
    return make


def post_of(post, thresh=0.85, rotated=True):
    def make():
        p, sc = pool()
        return stacked(p[:1000], sc[:1000], post=post, thresh=thresh, rotated=rotated,
                       present=lambda c, st: st[0]["kept"] == post)
    return make


def post_mid_chunk():
    p, sc = pool()
    # the 100th survivor lies inside a chunk and live candidates follow it there
    return stacked(p, sc, post=100, thresh=0.85,
                   present=lambda c, st: st[0]["kept"] == 100 and st[0]["left_behind"] and 0 < st[0]["last_in_chunk"] < CHUNK - 1)


def fewer_than_post():
    p, sc = pool()
    return stacked(p, sc, post=100, thresh=0.01, present=lambda c, st: st[0]["kept"] == 44 and st[0]["candidates"] == 4608)


def thresh_of(thresh, rotated=True):
    def make():
        p, sc = pool()
        return stacked(p, sc, post=512, thresh=thresh, rotated=rotated,
                       present=lambda c, st: st[0]["candidates"] == 4608 and st[0]["kept"] >= 20)
    return make


def pre_of(pre):
    def make():
        p, sc = pool()
        return stacked(p[:1000], sc[:1000], pre=pre, post=512, thresh=0.85,
                       present=lambda c, st: st[0]["candidates"] == min(pre, 1000))
    return make


def pre_cuts_a_tie():
    p, sc = pool()
    q = (np.floor(sc[:1000] * 50) / 50).astype(F)      # about 20 rows per score

    def present(c, st):
        order = np.argsort(seq.descending_bits(q), kind="stable")
        return q[order[199]] == q[order[200]] and st[0]["candidates"] == 200
    return stacked(p[:1000], q, pre=200, post=512, thresh=0.85, present=present)


def duplicates():
    p, sc = pool()
    box = np.concatenate([p[:150], p[:150]])[np.random.default_rng(3).permutation(300)]
    return stacked(box, np.random.default_rng(4).random(300).astype(F), thresh=0.7,
                   present=lambda c, st: len(np.unique(c["box"], axis=0)) <= 150 and st[0]["kept"] >= 20)


def equal_scores(rotated=True):
    def make():
        p, _ = pool()
        return stacked(p[:1000], np.full(1000, 0.5, F), thresh=0.7, post=64, rotated=rotated,
                       present=lambda c, st: st[0]["kept"] == 64)
    return make


def nan_scores():
    p, sc = pool()
    cls = np.stack([sc[:300], sc[300:600], sc[600:900]], 1).copy()
    cls[7, 1] = np.nan          # a NaN beside larger and smaller numbers: the row's score is the NaN, its label 2
    cls[200, 0] = cls[200, 2] = np.nan
    cls[11] = [np.inf, 0.1, np.inf]
    cls[12] = [-np.inf, -np.inf, -np.inf]
    cls[13] = [-0.0, 0.0, -1.0]

    def present(c, st):
        rois, scores, labels = want(c)
        return (np.isnan(scores[0, :2]).all() and labels[0, 0] == 2 and labels[0, 1] == 1 and np.isposinf(scores[0, 2])
                and labels[0, 2] == 1 and np.array_equal(rois[0, 0], c["box"][7]) and np.array_equal(rois[0, 1], c["box"][200]))
    return stacked(p[:300], cls, post=300, thresh=0.85, present=present)


def class_ties(C=2):
    def make():
        p, sc = pool()
        n = 500
        cls = np.stack([sc[:n], sc[:n], (sc[:n] * F(0.5))], 1).copy()     # columns 0 and 1 tie everywhere
        cls[::3, 2] = sc[:n][::3]                                         # ... and all three on every third row
        cls[1::3, 0] = 0                                                  # column 1 alone on others
        box = np.concatenate([p[:n], np.random.default_rng(5).random((n, C)).astype(F)], 1) if C else p[:n]

        def present(c, st):
            labels = want(c)[2][0]
            return c["box"].shape[1] == 7 + C and set(labels[:st[0]["kept"]]) == {1, 2}
        return stacked(box, cls, thresh=0.7, present=present)
    return make


def three_samples(post=512, thresh=0.85, rotated=True, strays=False):
    """stacked: 4 608 / 1 000 / 0 rows, interleaved, batch_index float32"""
    def make():
        p0, s0 = pool()
        p1, s1 = pool(60.0)
        box = np.concatenate([p0, p1[:1000]])
        cls = np.concatenate([s0, s1[:1000]])
        bidx = np.concatenate([np.zeros(4608, F), np.ones(1000, F)])
        if strays:
            box = np.concatenate([box, p1[1000:1006]])
            cls = np.concatenate([cls, np.full(6, 2.0, F)])                  # they would win every sample
            bidx = np.concatenate([bidx, np.array([3, -1, 0.5, np.nan, 2.5, 1e9], F)])
        perm = np.random.default_rng(6).permutation(len(box))

        def present(c, st):
            k = c["batch_index"]
            runs = int((np.diff(k[np.isfinite(k)]) != 0).sum())
            return ([s["candidates"] for s in st] == [4608, 1000, 0] and st[0]["kept"] == post and st[2]["kept"] == 0
                    and runs > 1000 and k.dtype == F)
        return stacked(box[perm], cls[perm], B=3, bidx=bidx[perm], post=post, thresh=thresh, rotated=rotated, present=present)
    return make


def dense(as_stacked=False, rotated=True):
    """B = 3 samples of 1 000 rows, K = 3, C = 2; the same rows in the stacked form give the same result"""
    def make():
        p0, s0 = pool()
        p1, s1 = pool(60.0)
        rng = np.random.default_rng(8)
        box = np.stack([p0[:1000], p1[:1000], p0[1000:2000]])
        box = np.concatenate([box, rng.random((3, 1000, 2)).astype(F)], 2)
        cls = np.stack([np.stack([s0[:1000], s0[1000:2000], s0[2000:3000]], 1), np.stack([s1[:1000], s1[1000:2000], s1[2000:3000]], 1),
                        np.stack([s0[3000:4000], s1[3000:4000], s1[2000:3000]], 1)])
        c = dict(box=np.ascontiguousarray(box, F), cls=np.ascontiguousarray(cls, F), batch_index=None, B=3, pre=BIG, post=100,
                 thresh=0.7, rotated=rotated, present=lambda c, st: [s["candidates"] for s in st] == [1000] * 3)
        if as_stacked:
            c.update(box=c["box"].reshape(-1, 9), cls=c["cls"].reshape(-1, 3),
                     batch_index=np.repeat(np.arange(3), 1000).astype(np.int64))
        return c
    return make


def past_every_capacity():
    """two samples that reach POST = 512 side by side and an empty one: every wavefront's share of the kept list longer
    than a chunk, more chunks than wavefronts, more than one sample bit in the key"""
    c = three_samples(post=512, thresh=0.85)()
    inner = c["present"]
    c["present"] = lambda c, st: inner(c, st) and st[0]["kept"] > CHUNK * WAVES and st[0]["chunks"] > WAVES and c["B"] > 2
    return c


CASES = {
    "1 row": n_rows(1), "63 rows": n_rows(63), "64 rows": n_rows(64), "65 rows": n_rows(65), "129 rows": n_rows(129),
    "1000 rows": n_rows(1000), "65 rows axis-aligned": n_rows(65, False), "1000 rows axis-aligned": n_rows(1000, False),
    "POST 1": post_of(1), "POST 64": post_of(64), "POST 65": post_of(65), "POST 100": post_of(100), "POST 512": post_of(512, 0.95),
    "POST 65 axis-aligned": post_of(65, rotated=False),
    "POST inside a chunk": post_mid_chunk, "fewer than POST": fewer_than_post,
    "PRE above": pre_of(BIG), "PRE equal": pre_of(1000), "PRE below": pre_of(200), "PRE cuts a tie": pre_cuts_a_tie,
    "thresh 0.01": thresh_of(0.01), "thresh 0.7": thresh_of(0.7), "thresh 0.85": thresh_of(0.85),
    "thresh 0.7 axis-aligned": thresh_of(0.7, False),
    "exact duplicates": duplicates, "equal scores": equal_scores(), "equal scores axis-aligned": equal_scores(False),
    "NaN scores": nan_scores, "K 3 with equal maxima, C 2": class_ties(2), "K 3 with equal maxima, C 0": class_ties(0),
    "3 samples": three_samples(post=100, thresh=0.7), "3 samples and strays": three_samples(post=100, thresh=0.7, strays=True),
    "3 samples axis-aligned": three_samples(post=100, thresh=0.7, rotated=False),
    "dense": dense(), "dense rows stacked": dense(True), "dense axis-aligned": dense(rotated=False),
    "past every capacity": past_every_capacity,
}


# ------------------------------------------------------------------------------------------------ the edges
# A second registry, kept apart because the CPU test bounds CASES (rows, B, POST): scores as the detectors hand them over
# (raw logits, mostly negative), boxes of a diverged detector, and every limit of csrc/proposals.hip run, not only refused.
# Scores that must stay pairwise distinct are moved by exact maps only: the pool's lie on the 2^-24 grid of [0, 1), and
# sc - 0.5 and sc - 1 are exact there.
HALF = F(0.5)
LOGIT = F(0.625)          # sc - 0.5 leaves 79 negative scores among the 512 kept of "logits", sc - 0.625 (as exact) 172
PAYLOAD = 0x7FC12345      # a quiet NaN with a payload: extra box columns are copied, never computed with


def logits(rotated=True):
    def make():
        p, sc = pool()
        s = (sc - LOGIT)[:1000]

        def present(c, st):
            kept = want(c)[1][0, :st[0]["kept"]]
            return (st[0]["kept"] == 512 and int((kept < 0).sum()) >= 100 and int((kept > 0).sum()) >= 100
                    and len(np.unique(s)) == 1000 and is_distinct(c))
        return stacked(p[:1000], s, post=512, thresh=0.85, rotated=rotated, present=present)
    return make


def logits_k3():
    p, sc = pool()
    three = np.stack([sc[:1000], sc[1000:2000], sc[2000:3000]], 1)
    cls = three - F(0.875)      # mixed sign, the maximum negative on two rows in three
    cls[::2] = three[::2] - F(1)      # every other row: all negative

    def present(c, st):
        k = st[0]["kept"]
        _, scores, labels = want(c)
        return ((c["cls"][::2] < 0).all() and (c["cls"][1::2] > 0).any() and (c["cls"][1::2] < 0).any()
                and set(labels[0, :k]) == {1, 2, 3} and (scores[0, :k] < 0).any() and (scores[0, :k] > 0).any() and is_distinct(c))
    return stacked(p[:1000], cls, post=512, thresh=0.85, present=present)


EIGHT = np.array([1e-45, -1e-45, 0.0, -0.0, 1e-39, -1e-39, -0.0, 0.0], F)      # the scores of rows 0 .. 7
EIGHT_ORDER = [4, 0, 2, 3, 6, 7, 1, 5]      # 1e-39, 1e-45, the four zeros by ascending row, -1e-45, -1e-39


def zeros_and_denormals():
    p, sc = pool()
    s = (sc - HALF)[:300].copy()
    s[:8] = EIGHT

    def present(c, st):
        rois, scores, _ = want(c)
        at = [int(np.flatnonzero((rois[0] == c["box"][r]).all(1) & (scores[0].view(np.uint32) == EIGHT[r:r + 1].view(np.uint32)))[0])
              for r in EIGHT_ORDER]
        return (st[0]["kept"] == 300 and at == sorted(at) and (EIGHT[[0, 1, 4, 5]] != 0).all()
                and (np.abs(EIGHT) < np.finfo(F).tiny).all() and len(np.unique(c["box"][:8], axis=0)) == 8)
    return stacked(p[:300], s, post=300, thresh=np.inf, present=present)


POISON = (np.nan, np.inf, -np.inf)
ROTATED_COLUMNS = range(7)      # the columns poisoned in the rotated non-finite case


def poisoned_rows():
    """60 of the first 400 pool rows, each given NaN / +inf / -inf (cycled) in one of the columns 0 .. 6 (cycled), and
    five degenerate ones: -> (rows, column or -1, boxes)"""
    p, _ = pool()
    box = p[:400].copy()
    rows = np.sort(np.random.default_rng(1).choice(400, 65, replace=False))
    col = np.full(65, -1)
    for k, r in enumerate(rows[:60]):
        col[k] = k % 7
        box[r, col[k]] = POISON[k % 3]
    a, b, c, d, e = rows[60:]
    box[a, 3] = 0
    box[b, 3:5] = 0
    box[c, 3] = -1
    box[d, 6] = 1e30
    box[e, 0] = 3e38
    return rows, col, box


def non_finite(rotated=True, columns=range(7)):
    def make():
        _, sc = pool()
        rows, col, box = poisoned_rows()
        take = np.ones(400, bool)
        take[rows[:60][~np.isin(col[:60], list(columns))]] = False      # a poisoned column that is left out: the row goes
        extra = np.random.default_rng(2).random((400, 2)).astype(F)
        extra[:, 0] = np.array([PAYLOAD], np.uint32).view(F)[0]
        box, s, bad = np.concatenate([box, extra], 1)[take], sc[:400][take], np.isin(np.arange(400), rows)[take]

        def present(c, st):
            rois = want(c)[0][0, :st[0]["kept"]]
            got = (c["box"][bad][:, None, :7].view(np.uint32) == rois[None, :, :7].view(np.uint32)).all(2).any(1)
            clean = seq.survivors(c["box"][~bad], c["cls"][~bad], 1, c["pre"], c["post"], c["thresh"], c["rotated"],
                                  c["batch_index"][~bad])[0]
            return (not np.isfinite(c["box"][bad][:, :7]).all(1).all() and got.any() and not got.all()
                    and len(clean) != st[0]["kept"] and (rois[:, 7].view(np.uint32) == PAYLOAD).all() and len(rois) > 100)
        return stacked(box, s, post=400, thresh=0.7, rotated=rotated, present=present)
    return make


def post_full():
    p, sc = pool()
    return stacked(p, sc, post=seq.POST_MAX, thresh=0.9,
                   present=lambda c, st: st[0]["kept"] == 1024 == seq.POST_MAX and st[0]["chunks"] >= 17 and is_distinct(c))


def edge_pre(pre):
    def make():
        c = pre_of(pre)()
        inner = c["present"]
        c["present"] = lambda c, st: (inner(c, st) and st[0]["kept"] <= pre and (pre > 0 or not want(c)[0].any()) and is_distinct(c))
        return c
    return make


def edge_thresh(thresh, rotated=True):
    """300 rows, POST 300: at or below 0 every later box is suppressed by an overlapping earlier one (below 0 by the
    first, so every chunk is dead before it is read); at 1 and above, NaN included, nothing is (up to an IoU that rounds
    above 1), and the kept list grows by whole chunks"""
    def make():
        p, sc = pool()
        t = F(thresh)

        def present(c, st):
            k, n = st[0]["kept"], 300
            return (st[0]["candidates"] == n and (k == 1 if t < 0 else 1 < k < 100 if t == 0 else n - 5 <= k <= n if t == 1 else k == n)
                    and is_distinct(c))
        return stacked(p[:300], sc[:300], post=300, thresh=thresh, rotated=rotated, present=present)
    return make


STRAY_Z = F(777)      # the strays' z: no row of a sample has it
STRAYS_F32 = np.array([65535, 65536, -1, 0.5, np.nan, 1e9], F)
STRAYS_I64 = np.array([65535, 65536, -1, 2 ** 32, -2 ** 63, 10 ** 9], np.int64)      # 2^32: sample 0 if cut to 32 bits


def many_samples(form):
    """B = 65535 samples of 2 rows: a pool row and, in every third sample, the same box moved by 0.25 m (the pair
    overlaps: 1 kept), else another pool row.  form: "f32" / "i64" (stacked, interleaved by a permutation, 6 strays with
    score 2.0) or "dense" ((65535, 2, 7))"""
    def make():
        B = seq.BATCH_MAX
        p, sc = pool()
        s = np.arange(B)
        i, j = s % 4608, (s * 7 + 1 + s // 4608) % 4608
        box = np.stack([p[i], p[j]], 1)
        near = s % 3 == 0
        box[near, 1] = box[near, 0]
        box[near, 1, 0] += F(0.25)
        cls = np.stack([sc[i] - HALF, sc[j] - F(1)], 1)[..., None]

        def present(c, st):
            rois, scores, _ = want(c)
            kept = np.array([o["kept"] for o in st])
            return (c["B"] == B == 65535 and all(o["candidates"] == 2 for o in st) and (kept == 1).any() and (kept == 2).any()
                    and set(kept) == {1, 2} and not (rois[..., 2] == STRAY_Z).any() and not (scores == 2).any()
                    and c["box"].size // 7 == (2 * B if form == "dense" else 131076))
        if form == "dense":
            return dict(box=np.ascontiguousarray(box, F), cls=np.ascontiguousarray(cls, F), batch_index=None, B=B, pre=BIG, post=2,
                        thresh=0.7, rotated=True, present=present)
        stray = p[:6].copy()
        stray[:, 2] = STRAY_Z
        box, cls = np.concatenate([box.reshape(-1, 7), stray]), np.concatenate([cls.reshape(-1), np.full(6, 2.0, F)])
        bidx = np.concatenate([np.repeat(s, 2).astype(F), STRAYS_F32]) if form == "f32" else np.concatenate([np.repeat(s, 2), STRAYS_I64])
        perm = np.random.default_rng(9).permutation(len(box))
        return stacked(box[perm], cls[perm], B=B, bidx=bidx[perm], post=2, thresh=0.7, present=present)
    return make


def wide(box_cols=7, cls_cols=1):
    """130 rows, POST 70, one of the two widths at its limit of 4096"""
    def make():
        p, sc = pool()
        n = 130
        rng = np.random.default_rng(10)
        box = np.concatenate([p[:n], rng.random((n, box_cols - 7)).astype(F)], 1)
        cls = (rng.random((n, cls_cols)).astype(F) * HALF - F(1))      # below every maximum set here
        r = np.arange(n)
        top = (sc[:n] - HALF).astype(F)
        if cls_cols > 1:
            cls[r[0::3], 4000 + r[0::3] % 96] = top[0::3]      # the maximum far out
            cls[1::3, 0] = top[1::3]                           # ... in column 0
            cls[2::3, 5] = cls[2::3, 4095] = top[2::3]         # ... twice: the lower column takes it
        else:
            cls[:, 0] = top

        def present(c, st):
            k = st[0]["kept"]
            rois, _, labels = want(c)
            lab = set(labels[0, :k])
            return (k == 70 and c["box"].shape[1] == box_cols and c["cls"].shape[1] == cls_cols and 4096 in (box_cols, cls_cols)
                    and rois[0, :k, -1].all()
                    and (cls_cols == 1 or (1 in lab and 6 in lab and 4096 not in lab and max(lab) > 4000 and lab - {1, 6} != set())))
        return stacked(box, cls, post=70, thresh=0.85, present=present)
    return make


EDGE_CASES = {
    "logits": logits(), "logits axis-aligned": logits(False), "logits K 3": logits_k3, "zeros and denormals": zeros_and_denormals,
    "non-finite boxes": non_finite(True, ROTATED_COLUMNS), "non-finite boxes axis-aligned": non_finite(False),
    "POST 1024 full": post_full,
    "PRE 0": edge_pre(0), "PRE 1": edge_pre(1), "PRE 64": edge_pre(64), "PRE 65": edge_pre(65),
    "thresh -1": edge_thresh(-1.0), "thresh 0": edge_thresh(0.0), "thresh 1": edge_thresh(1.0), "thresh NaN": edge_thresh(np.nan),
    "thresh +inf": edge_thresh(np.inf), "thresh -1 axis-aligned": edge_thresh(-1.0, False),
    "thresh +inf axis-aligned": edge_thresh(np.inf, False),
    "B 65535 stacked": many_samples("f32"), "B 65535 stacked int64": many_samples("i64"), "B 65535 dense": many_samples("dense"),
    "4096 box columns": wide(box_cols=4096), "4096 class columns": wide(cls_cols=4096),
}
assert not set(EDGE_CASES) & set(CASES)
# no order is open on these (is_distinct, asserted by each): the reference's own path must give the same bits.  The
# B 65535 cases are distinct too but stay out: that path is a Python loop over the samples
EDGE_DISTINCT = ["logits", "logits axis-aligned", "logits K 3", "POST 1024 full", "PRE 0", "PRE 1", "PRE 64", "PRE 65",
                 "thresh -1", "thresh 0", "thresh 1", "thresh -1 axis-aligned"]


@functools.lru_cache(maxsize=None)
def case(name):
    c = (CASES[name] if name in CASES else EDGE_CASES[name])()
    for k in ("box", "cls", "batch_index"):
        if c[k] is not None:
            c[k].setflags(write=False)
    c["name"] = name
    return c


_WANT = {}


def want(c):
    """the restatement's three outputs, computed once per case"""
    key = c.get("name", id(c))
    if key not in _WANT:
        out = seq.proposals(c["box"], c["cls"], c["B"], c["pre"], c["post"], c["thresh"], c["rotated"], c["batch_index"])
        for a in out:
            a.setflags(write=False)
        _WANT[key] = out
    return _WANT[key]


def is_distinct(c):
    """scores pairwise distinct within every sample and class values pairwise distinct within every row: no order is
    open, the reference's own path must give the same bits"""
    box, cls, per = seq._flat(c["box"], c["cls"], c["batch_index"])
    score, _ = seq.score_label(cls)
    smp = seq.sample_of(c["batch_index"], len(box), c["B"], per)
    if np.isnan(cls).any():
        return False
    if cls.shape[1] > 1 and (np.diff(np.sort(cls, 1), axis=1) == 0).any():
        return False
    return all(len(np.unique(score[smp == s])) == int((smp == s).sum()) for s in range(c["B"]))
