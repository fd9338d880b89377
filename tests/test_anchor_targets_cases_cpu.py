"""CPU: the cases of tests/anchor_targets_cases.py hold the edges they are named after, and they have teeth: eight
deliberately wrong variants of the numpy restatement -- the mistakes the structure of csrc/anchor_targets.hip makes
possible -- each differ from the true restatement on the case named for it in CAUGHT_BY."""
import numpy as np
import pytest

import anchor_targets_cases as cases
import anchor_targets_seq as seq
from modest_amd.utils import target_assigner as ta

F = np.float32
CHUNK, TILE, BLOCK = cases.CHUNK, cases.TILE, cases.BLOCK
SENTINEL = 0x5A5A5A5A


@pytest.mark.parametrize("name", cases.names())
def test_case_holds_its_edge(name):
    case = cases.by_name(name)
    assert case["gt"].dtype == F and case["gt"].ndim == 3
    case["present"](case)


def test_every_family_and_constant_is_there():
    fam = {c["family"] for c in cases.cases()}
    assert fam == {"rows", "select", "tiles", "layouts", "columns", "zero"}
    assert {c["M"] for c in cases.cases() if c["family"] == "rows"} >= {0, 1, 63, 64, 65, 127, 128, 129, 300}
    assert {c["cols"] for c in cases.cases() if c["family"] == "columns"} == {(7, 8), (7, 10), (9, 10), (10, 10)}
    assert {c["BM"] for c in cases.cases() if c["family"] == "zero"} == {(0, 5), (2, 0), (0, 0)}
    assert (CHUNK, TILE, BLOCK) == (64, 256, 256)
    assert max(c["gt"].shape[1] for c in cases.cases()) <= 700 and max(len(seq.flatten(a, False)) for c in cases.cases()
                                                                       for a in cases.reference(c)["anchors"]) <= 2000


# ---- the wrong variants -------------------------------------------------------------------------------------------------
TRUE = dict(kept_rows=seq.kept_rows, class_rows=seq.class_rows, assign_single=seq.assign_single)


def finish(anchors, gts, cids, matched, unmatched, sincos, code, arg, rowmax, forced):
    """the label rule and the encoding of assign_single for a given (arg, rowmax, forced)"""
    n = len(anchors)
    labels = np.full(n, -1, dtype=np.int32)
    targets = np.zeros((n, code), dtype=F)
    c = np.asarray(cids, dtype=np.int32)[arg]
    labels[rowmax >= F(matched)] = c[rowmax >= F(matched)]
    labels[rowmax < F(unmatched)] = 0
    labels[forced] = c[forced]
    fg = labels > 0
    targets[fg] = seq.encode(gts[arg[fg]], anchors[fg], sincos)
    return labels, targets, (labels > 0).astype(F)


def with_parts(fn):
    """an assign_single that hands the true (iou, colmax, rowmax, arg, forced) to fn, which returns (arg, rowmax, forced)"""
    def single(anchors, gts, cids, matched, unmatched, sincos, code, detail=None):
        d = {}
        true = TRUE["assign_single"](anchors, gts, cids, matched, unmatched, sincos, code, d)
        if "iou" not in d:
            return true
        if detail is not None:
            detail.update(d)
        return finish(anchors, gts, cids, matched, unmatched, sincos, code, *fn(d))
    return single


def kept_from_the_first_chunk(g):
    return TRUE["kept_rows"](np.asarray(g)[:CHUNK])


def cursor_restarts_per_chunk(cids, class_names, anchor_name):
    """the cursor restarts at every chunk and the count is the last chunk's: what is read back is the last chunk's rows"""
    mine = TRUE["class_rows"](cids, class_names, anchor_name)
    if len(mine):
        mine[:(len(mine) - 1) // CHUNK * CHUNK] = False
    return mine


def highest_index_on_a_tie(d):
    iou = d["iou"]
    arg = iou.shape[1] - 1 - iou[:, ::-1].argmax(axis=1)
    return arg, iou[np.arange(len(iou)), arg], d["forced"]


def last_tile_wins(d):
    """arg, row maximum and forced start again at every tile of 256 gts"""
    t0 = (d["iou"].shape[1] - 1) // TILE * TILE
    iou = d["iou"][:, t0:]
    arg = iou.argmax(axis=1)
    forced = ((iou == d["colmax"][None, t0:]) & (d["colmax"][None, t0:] != 0)).any(axis=1)
    return arg + t0, iou[np.arange(len(iou)), arg], forced


def forced_from_the_first_tile_only(d):
    forced = ((d["iou"] == d["colmax"][None, :]) & (d["colmax"][None, :] != 0))[:, :TILE].any(axis=1)
    return d["arg"], d["rowmax"], forced


def column_maxima_per_block(d):
    """every workgroup of 256 anchors compares with its own column maxima"""
    forced = np.zeros(len(d["iou"]), dtype=bool)
    for i0 in range(0, len(forced), BLOCK):
        iou = d["iou"][i0:i0 + BLOCK]
        col = iou.max(axis=0)
        forced[i0:i0 + BLOCK] = ((iou == col[None, :]) & (col[None, :] != 0)).any(axis=1)
    return d["arg"], d["rowmax"], forced


def stored(case, table_of):
    """the restatement's per-class results put through the device's store map (row i of a class -> output row
    (i // k) * stride + offset + i % k) into sentinel-filled outputs, with the class table changed by table_of"""
    cfg, gt = case["cfg"], case["gt"]
    anchors = cases.reference(case)["anchors"]
    per = []

    def recording(*a, **k):
        per.append(TRUE["assign_single"](*a, **k))
        return per[-1]
    saved = seq.assign_single
    seq.assign_single = recording
    try:
        true = seq.assign(cfg, anchors, gt)
    finally:
        seq.assign_single = saved
    rows, table, n_out = ta.output_layout([a.shape for a in anchors], cfg["use_multihead"])
    B, code = gt.shape[0], true["box_reg_targets"].shape[-1]
    lab = np.full((B, n_out), SENTINEL, dtype=np.int32)
    tar = np.full((B, n_out, code), SENTINEL, dtype=np.uint32).view(F)
    wei = np.full((B, n_out), SENTINEL, dtype=np.uint32).view(F)
    n_cls = len(anchors)
    for b in range(B):
        for ci, (first, n, k, stride, off) in enumerate(table_of(table)):
            i = np.arange(n)
            o = (i // k) * stride + off + i % k
            ok = o < n_out      # a wrong table may point past the end: such a row is dropped here
            lab[b, o[ok]], tar[b, o[ok]], wei[b, o[ok]] = (per[b * n_cls + ci][x][:n][ok] for x in range(3))
    return {"box_cls_labels": lab, "box_reg_targets": tar, "reg_weights": wei}, true


def k_of_the_first_class(table):
    return [(first, n, table[0][2], stride, off) for first, n, k, stride, off in table]


def longest_cut_to_the_shortest(table):
    ns = [t[1] for t in table]
    return [(first, min(ns) if n == max(ns) else n, k, stride, off) for first, n, k, stride, off in table]


VARIANTS = {
    "kept-row count from the first 64 rows": dict(kept_rows=kept_from_the_first_chunk),
    "compaction cursor restarted at each 64-row chunk": dict(class_rows=cursor_restarts_per_chunk),
    "arg takes the highest index on a tie": dict(assign_single=with_parts(highest_index_on_a_tie)),
    "arg and forced per 256-gt tile, the last tile wins": dict(assign_single=with_parts(last_tile_wins)),
    "forced ignores gts past 256": dict(assign_single=with_parts(forced_from_the_first_tile_only)),
    "column maxima per 256-anchor block, never merged": dict(assign_single=with_parts(column_maxima_per_block)),
    "every class stored with the k of the first class": dict(store=k_of_the_first_class),
    "the longest class cut to the shortest's row count": dict(store=longest_cut_to_the_shortest),
}

# variant -> the cases that must catch it (each is asserted; other cases may catch it too)
CAUGHT_BY = {
    "kept-row count from the first 64 rows": ["rows M=65: the last live row at [0, 62, 63, 64], chunks [0, 1]",
                                              "rows M=200: chunk 1 all zero between live chunks 0 and 2"],
    "compaction cursor restarted at each 64-row chunk": ["select M=330: n_sel 0, 1, 63, 64, 65, 255, 256, 257 in one batch"],
    "arg takes the highest index on a tie": ["tiles 64: one footprint at positions either side of the boundary, the lower index wins",
                                             "tiles 256: one footprint at positions either side of the boundary, the lower index wins"],
    "arg and forced per 256-gt tile, the last tile wins": ["tiles 512: an argmax in the third tile",
                                                           "tiles 256: one footprint at positions either side of the boundary, the lower index wins"],
    "forced ignores gts past 256": ["tiles 256: forced from past the boundary with the argmax before it, the mirror image, a zero column maximum late"],
    "column maxima per 256-anchor block, never merged": ["tiles: a column maximum with equal bits in two workgroups, and one that only the merge decides"],
    "every class stored with the k of the first class": ["layouts single head: k = 2, 6, 4, two heights",
                                                         "layouts single head: k = 2, 6, 4, two heights, align_center"],
    "the longest class cut to the shortest's row count": ["layouts multihead: 70, 35, 1248 and 1000 rows on grids of their own"],
}


def wrong(case, patch, monkeypatch):
    if "store" in patch:
        return stored(case, patch["store"])[0]
    with monkeypatch.context() as m:
        for k, v in patch.items():
            m.setattr(seq, k, v)
        return seq.assign(case["cfg"], cases.reference(case)["anchors"], case["gt"])


def test_the_store_map_reproduces_the_restatement():
    """unchanged, the table of output_layout puts every class's rows where the reference's concatenation puts them, on
    every case (unequal k, two heights, classes of different lengths), and leaves no sentinel"""
    for case in cases.cases():
        got, true = stored(case, lambda t: t)
        assert not seq.mismatches(got, true), case["name"]
        assert not (got["box_cls_labels"] == SENTINEL).any() and not (seq.bits(got["box_reg_targets"]) == SENTINEL).any()


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_wrong_variant_is_caught(variant, monkeypatch):
    assert sorted(VARIANTS) == sorted(CAUGHT_BY)
    caught = []
    for case in cases.cases():
        got = wrong(case, VARIANTS[variant], monkeypatch)
        if seq.mismatches(got, cases.reference(case)["out"]):
            caught.append(case["name"])
    assert seq.kept_rows is TRUE["kept_rows"] and seq.class_rows is TRUE["class_rows"] and seq.assign_single is TRUE["assign_single"]
    print(variant, "-> caught by", caught)
    missing = [n for n in CAUGHT_BY[variant] if n not in caught]
    assert not missing, f"{variant}: not caught by {missing}; caught by {caught}"
    families = {cases.by_name(n)["family"] for n in caught}
    assert families <= {"rows", "select", "tiles", "layouts", "columns"} and "zero" not in families
