"""Cases of the RoI proposal layer shared by tests/test_proposals_cpu.py and tests/test_gpu_proposals.py, built from the
clustered NMS proposals of tests/iou3d_cases.py (96 jittered copies of each of 48 objects, exact duplicates among them).
Each is the smallest shape at which the walk of csrc/proposals.hip can still go wrong; `present(case, stats)` asserts from
the inputs and the restatement that the edge the case is named after is there.

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


def stats_of(c):
    """per sample: the chunked walk's statistics (proposals_seq.chunked_walk), its candidates and survivors"""
    box, cls, n_per = seq._flat(c["box"], c["cls"], c["batch_index"])
    score, _ = seq.score_label(cls)
    smp = seq.sample_of(c["batch_index"], len(box), c["B"], n_per)
    per = []
    for cand in seq.candidates(score, smp, c["B"], c["pre"]):
        one = dict(chunks=0, tests=0, last_in_chunk=None, left_behind=False)
        kept = seq.chunked_walk(box[cand], c["thresh"], c["rotated"], c["post"], stats=one) if len(cand) else []
        one.update(candidates=len(cand), kept=len(kept))
        per.append(one)
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
@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
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
