"""numpy restatement of the RoI proposal layer (modest_amd.ops.proposals, csrc/proposals.hip):
RoIHeadTemplate.proposal_layer over class_agnostic_nms with MULTI_CLASSES_NMS off, with the order the library fixes where
the reference leaves it open (equal scores by ascending row, the lowest class among equal maxima, NaN above every number,
-0 == +0).

  proposals(...)           score / label, a stable order by (sample, descending score, row), the cut at PRE, the greedy
                           walk of the oracle (oracle.labels.nms: the f64 twin for rotated boxes, the glibc build for
                           axis-aligned ones, as tests/test_gpu_iou3d.py:_nms_expect), the cut at POST, the padding
  proposals_chunked(...)   the same results by the kernel's own walk: chunks of CHUNK candidates against a kept list dealt
                           round-robin to WAVES wavefronts, then among themselves, resolved in order, stopping at the
                           POST-th survivor inside a chunk; `fault` breaks it in one named way (FAULTS)
  proposals(key_fault=..)  the first restatement over one named wrong sort key (KEY_FAULTS)
  parent_walk(...)         the keep list of one sample, for the tools and tests that need the positions

Boxes are (n, 7 + C) float32, class values (n, K) float32.  `batch_index` None means the dense form ((B, N, .) inputs).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import labels as ol  # noqa: E402

F = np.float32
CHUNK, WAVES, POST_MAX, BATCH_MAX = 64, 4, 1024, 65535      # csrc/proposals.hip
FAULTS = ("first wavefront's share only", "chunk not tested against itself", "suppressed candidates still suppress",
          "kept list restarts per chunk")
KEY_FAULTS = ("negatives not inverted", "-0 below +0", "denormals are zero", "NaN last")      # wrong sort keys


def score_label(cls):
    """max over the columns and its column: the lowest column among equal maxima, the first NaN above every number"""
    cls = np.asarray(cls, F)
    best, at = cls[:, 0].copy(), np.zeros(len(cls), np.int64)
    for j in range(1, cls.shape[1]):
        v = cls[:, j]
        with np.errstate(invalid="ignore"):
            take = (v > best) | (np.isnan(v) & ~np.isnan(best))
        best, at = np.where(take, v, best), np.where(take, j, at)
    return best.astype(F), at


def descending_bits(s, fault=None):
    """uint32 whose ascending order is the descending order of the scores: NaN first, -0 == +0; `fault` builds one
    named wrong key instead (KEY_FAULTS)"""
    assert fault is None or fault in KEY_FAULTS, fault
    s = np.asarray(s, F).copy()
    if fault != "-0 below +0":
        s[s == 0] = 0
    if fault == "denormals are zero":
        s[np.abs(s) < np.finfo(F).tiny] = 0
    u = s.view(np.uint32).astype(np.uint64)
    neg = (u ^ 0x80000000) if fault == "negatives not inverted" else (~u & 0xFFFFFFFF)
    asc = np.where(u & 0x80000000, neg, u | 0x80000000)
    out = (~asc) & 0xFFFFFFFF
    out[np.isnan(s)] = 0xFFFFFFFF if fault == "NaN last" else 0
    return out.astype(np.uint64)


def sample_of(batch_index, n, B, rows_per_sample=None):
    """the sample of every row, B where it names none"""
    if batch_index is None:
        return np.arange(n, dtype=np.int64) // max(int(rows_per_sample), 1)
    b = np.asarray(batch_index).reshape(-1)
    with np.errstate(invalid="ignore"):
        ok = (b >= 0) & (b < B) & (b == np.floor(b))
    return np.where(ok, np.nan_to_num(b, nan=0.0, posinf=0.0, neginf=0.0), B).astype(np.int64)


def candidates(score, sample, B, pre, key_fault=None):
    """per sample the rows of its min(pre, rows) highest scores, in walk order"""
    key = (sample.astype(np.uint64) << np.uint64(32)) | descending_bits(score, key_fault)
    order = np.argsort(key, kind="stable")
    cut = np.searchsorted(sample[order], np.arange(B + 1))      # the stable order is grouped by sample
    return [order[cut[s]:min(cut[s + 1], cut[s] + pre)] for s in range(B)]


def iou_normal(a, b, nan_propagates=False):
    """iou_normal of csrc/iou_bev.h for all pairs, float32 in the written order -> (na, nb).  fmaxf / fminf return the
    other operand when one is a NaN, as np.fmax / np.fmin do; np.maximum / np.minimum (nan_propagates, kept to show the
    difference) hand the NaN on"""
    a, b = np.asarray(a, F)[:, None, :], np.asarray(b, F)[None, :, :]
    two = F(2)
    hi, lo = (np.maximum, np.minimum) if nan_propagates else (np.fmax, np.fmin)
    with np.errstate(all="ignore"):
        left = hi(a[..., 0] - a[..., 3] / two, b[..., 0] - b[..., 3] / two)
        right = lo(a[..., 0] + a[..., 3] / two, b[..., 0] + b[..., 3] / two)
        top = hi(a[..., 1] - a[..., 4] / two, b[..., 1] - b[..., 4] / two)
        bottom = lo(a[..., 1] + a[..., 4] / two, b[..., 1] + b[..., 4] / two)
        w, h = hi(right - left, F(0)), hi(bottom - top, F(0))
        inter = w * h
        sa, sb = a[..., 3] * a[..., 4], b[..., 3] * b[..., 4]
        return (inter / hi(sa + sb - inter, F(1e-8))).astype(F)


def pair_iou(a, b, rotated):
    """iou(a[i], b[j]) as the kernels evaluate it (the earlier box first)"""
    if len(a) == 0 or len(b) == 0:
        return np.zeros((len(a), len(b)), F)
    a, b = np.ascontiguousarray(a[:, :7], F), np.ascontiguousarray(b[:, :7], F)
    return ol.boxes_iou_bev(a, b, arith="f64") if rotated else iou_normal(a, b)


def parent_walk(boxes_sorted, thresh, rotated, post):
    """positions of the first `post` survivors of the greedy walk over score-sorted boxes"""
    if len(boxes_sorted) == 0:
        return np.zeros(0, np.int64)
    keep = ol.nms(np.ascontiguousarray(boxes_sorted[:, :7], F), F(thresh), rotated=rotated, arith="f64" if rotated else "glibc")
    return keep[:post]


def chunked_walk(boxes_sorted, thresh, rotated, post, fault=None, stats=None):
    """the same positions by the kernel's walk.  stats (a dict) receives: chunks walked, pair tests made, the position in
    its chunk of the last survivor, whether live candidates were left behind it in that chunk"""
    thresh = F(thresh)
    kept = []
    tests = chunks = 0
    last_in_chunk, left_behind = None, False
    for c0 in range(0, len(boxes_sorted), CHUNK):
        if len(kept) >= post:
            break
        chunks += 1
        cand = boxes_sorted[c0:c0 + CHUNK]
        m = len(cand)
        # (A) against the kept list, dealt round-robin to the wavefronts
        dead = np.zeros(m, bool)
        base = [] if fault == "kept list restarts per chunk" else kept
        for w in range(1 if fault == "first wavefront's share only" else WAVES):
            share = base[w::WAVES]
            if share:
                hit = pair_iou(boxes_sorted[share], cand, rotated) > thresh
                tests += hit.size
                dead |= hit.any(0)
        # (B) the live candidates among themselves: row i, bit j > i
        alive = ~dead
        mat = np.zeros((m, m), bool)
        idx = np.flatnonzero(alive)
        if len(idx) and fault != "chunk not tested against itself":
            mat[np.ix_(idx, idx)] = np.triu(pair_iou(cand[idx], cand[idx], rotated) > thresh, 1)
            tests += len(idx) * (len(idx) - 1) // 2
        # (C) in order, up to the POST-th survivor
        for i in range(m):
            if not alive[i]:
                if fault == "suppressed candidates still suppress" and not dead[i]:
                    alive = alive & ~mat[i]
                continue
            if len(kept) >= post:
                left_behind = True
                break
            kept.append(c0 + i)
            last_in_chunk = i
            alive = alive & ~mat[i]
            alive[i] = False
    if stats is not None:
        stats.update(chunks=chunks, tests=tests, last_in_chunk=last_in_chunk, left_behind=left_behind)
    return np.asarray(kept, np.int64)


def _assemble(box, cls, B, post, rows_of):
    cols = box.shape[1]
    score, label = score_label(cls)
    rois = np.zeros((B, post, cols), F)
    scores = np.zeros((B, post), F)
    labels = np.ones((B, post), np.int64)
    for s, rows in enumerate(rows_of):
        rows = rows[:post]
        rois[s, :len(rows)] = box[rows]
        scores[s, :len(rows)] = score[rows]
        labels[s, :len(rows)] = label[rows] + 1
    return rois, scores, labels


def _flat(box, cls, batch_index):
    box, cls = np.asarray(box, F), np.asarray(cls, F)
    per = None
    if batch_index is None:
        assert box.ndim == 3 and cls.ndim == 3
        per = box.shape[1]
        box, cls = box.reshape(-1, box.shape[-1]), cls.reshape(-1, cls.shape[-1])
    return box, cls, per


def survivors(box, cls, B, pre, post, thresh, rotated=True, batch_index=None, walk=parent_walk, key_fault=None, **kw):
    """per sample the rows of the survivors, in order"""
    box, cls, per = _flat(box, cls, batch_index)
    score, _ = score_label(cls)
    sample = sample_of(batch_index, len(box), B, per)
    out = []
    for rows in candidates(score, sample, B, pre, key_fault):
        out.append(rows[walk(box[rows], thresh, rotated, post, **kw)] if len(rows) else rows)
    return out


def proposals(box, cls, B, pre, post, thresh, rotated=True, batch_index=None, key_fault=None):
    """-> rois (B, post, 7 + C) float32, roi_scores (B, post) float32, roi_labels (B, post) int64"""
    rows_of = survivors(box, cls, B, pre, post, thresh, rotated, batch_index, key_fault=key_fault)
    box, cls, _ = _flat(box, cls, batch_index)
    return _assemble(box, cls, B, post, rows_of)


def proposals_chunked(box, cls, B, pre, post, thresh, rotated=True, batch_index=None, fault=None):
    rows_of = survivors(box, cls, B, pre, post, thresh, rotated, batch_index, walk=chunked_walk, fault=fault)
    box, cls, _ = _flat(box, cls, batch_index)
    return _assemble(box, cls, B, post, rows_of)


def same(got, want):
    """the three outputs bit for bit (a NaN equal to a NaN of the same bits)"""
    return all(np.asarray(g).dtype == np.asarray(w).dtype and np.asarray(g).shape == np.asarray(w).shape
               and np.asarray(g).tobytes() == np.asarray(w).tobytes() for g, w in zip(got, want))


def describe(got, want):
    out = []
    for name, g, w in zip(("rois", "roi_scores", "roi_labels"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        if g.shape != w.shape or g.dtype != w.dtype:
            out.append(f"{name}: {g.dtype}{g.shape} against {w.dtype}{w.shape}")
            continue
        bad = ~((g == w) | ((g != g) & (w != w)))
        if bad.any():
            at = np.argwhere(bad)[0]
            out.append(f"{name}: {int(bad.sum())} differ, first at {tuple(int(v) for v in at)}: {g[tuple(at)]!r} against {w[tuple(at)]!r}")
    return out


# ------------------------------------------------------------------------------------------------ the recorded fixture
def scenes(rec):
    import json
    return json.loads(str(rec["scenes"]))


def scene_inputs(rec, name):
    import json
    cfg = json.loads(str(rec[name + "_cfg"]))
    bidx = rec[name + "_batch_index"] if name + "_batch_index" in rec else None
    return cfg, rec[name + "_box"], rec[name + "_cls"], bidx


def recorded(rec, name):
    return rec[name + "_rois"], rec[name + "_roi_scores"], rec[name + "_roi_labels"]
