"""Cases for the anchor target assigner past the constants of csrc/anchor_targets.hip (not a test module;
tests/test_anchor_targets_cases_cpu.py, tests/test_gpu_anchor_targets.py and tools/make_golden_anchor_targets.py import it).

The constants crossed: CHUNK = 64 (at_select walks a sample's gt rows 64 at a time by ballot and carries the kept-row
count and the compaction cursor from chunk to chunk), TILE = 256 (at_colmax / at_assign stage a class's selected gts
through LDS 256 at a time and carry row maximum, argmax and the forced flag from tile to tile), BLOCK = 256 (anchors per
workgroup: column maxima are merged across workgroups, and the grid is sized by the longest class).

A case is a dict: name, family, cfg (anchor_targets_seq's config dict), gt (B, M, cols) float32 and present(case), which
asserts FROM THE INPUTS (through the numpy restatement's details) that the edge the case is named after is there.
"position" below is the index of a gt among the selected gts of its class (its place in details[b][c]["rows"]).
"""
import numpy as np

import anchor_targets_seq as seq

F = np.float32
CHUNK, TILE, BLOCK = 64, 256, 256
FAR = 1000.0


def cls(name, sizes, rots, zs, m, u, grid, align=False):
    return dict(class_name=name, anchor_sizes=[list(s) for s in sizes], anchor_rotations=list(rots), anchor_bottom_heights=list(zs),
                align_center=align, matched_threshold=m, unmatched_threshold=u, grid_size=list(grid))


def reference(case):
    """anchors, restatement outputs and details of a case, computed once and left unchanged"""
    if "_ref" not in case:
        anchors = seq.make_anchors(case["cfg"])
        details = []
        out = seq.assign(case["cfg"], anchors, case["gt"], details)
        for v in out.values():
            v.setflags(write=False)
        case["_ref"] = dict(anchors=anchors, out=out, details=details)
    return case["_ref"]


def class_labels(d, cfg, code):
    """labels of one class's anchors from its details entry"""
    n = len(d["anchors"])
    if "iou" not in d:
        return np.zeros(n, dtype=np.int32)
    lab = np.full(n, -1, dtype=np.int32)
    cid = d["cids"][d["arg"]]
    lab[d["rowmax"] >= d["matched"]] = cid[d["rowmax"] >= d["matched"]]
    lab[d["rowmax"] < d["unmatched"]] = 0
    lab[d["forced"]] = cid[d["forced"]]
    return lab


def position(d, row):
    """position of gt row `row` among the class's selected gts"""
    at = np.flatnonzero(d["rows"] == row)
    assert len(at) == 1, (row, d["rows"])
    return int(at[0])


def near(rs, flat, cid, cols, far=False):
    """a gt near a random anchor of `flat`, always overlapping it"""
    a = flat[rs.randint(len(flat))]
    size = a[3:6] * rs.uniform(0.8, 1.25, 3)
    off = np.clip(rs.normal(0, 0.3, 2), -0.6, 0.6) * min(a[3], a[4])
    row = [a[0] + off[0], a[1] + off[1], a[2] + rs.normal(0, 0.2), *size,
           a[6] + rs.normal(0, 0.25) + np.pi * rs.randint(-3, 4)]
    row += list(rs.normal(0, 2, cols - 8)) + [cid]
    if far:
        row[0] += FAR
    return np.array(row, dtype=F)


# ================================================================================================ rows: the kept-row count
def rows_cfg():
    """one class, 6 x 8 locations 4 m apart, 96 anchors of 2 x 1"""
    return dict(anchor_range=[0, -10, -3, 28, 10, 1], use_multihead=False, code_size=7, sincos=False, class_names=["Car"],
                classes=[cls("Car", [[2.0, 1.0, 1.5]], [0, 1.57], [-1.0], 0.6, 0.45, (8, 6))])


def rows_sample(rs, flat, M, last, mark=0):
    """M rows: random cars (one in ten a zero row) before row `last`, row `last` exactly an anchor's box at z = 0.25 (IoU
    1 with it, which no random row reaches: trimming it changes the outputs), zero rows after it"""
    g = np.zeros((M, 8), dtype=F)
    for j in range(last):
        if rs.randint(10):
            g[j] = near(rs, flat, 1, 8)
    a = flat[(2 * (7 + 3 * mark)) % len(flat)]
    g[last] = [a[0], a[1], 0.25, a[3], a[4], a[5], 0, 1]
    return g


def rows_present(case):
    ref = reference(case)
    gt = case["gt"]
    assert gt.shape[1] == case["M"]
    for b in range(gt.shape[0]):
        s = np.zeros(gt.shape[1], dtype=F)
        for k in range(gt.shape[2] - 1):
            s = s + gt[b, :, k]
        live = np.flatnonzero(s != 0)
        want = case["kept"][b]
        assert seq.kept_rows(gt[b, :, :-1]) == want, (case["name"], b)
        last = case["last"][b]
        if last is None:
            continue
        assert len(live) and live[-1] == last and want == last + 1, (case["name"], b, live[-1:])
        assert last // CHUNK == case["chunks"][b], (case["name"], b)
        d = ref["details"][b][0]
        p = position(d, last)
        lab = class_labels(d, case["cfg"], 7)
        assert ((d["arg"] == p) & (lab > 0) & (d["rowmax"] == 1)).any(), (case["name"], b, "the last live row decides no anchor")
    case.get("more", lambda c: None)(case)


def rows_cases():
    cfg = rows_cfg()
    flat = seq.flatten(seq.make_anchors(cfg)[0], False)
    rs = np.random.RandomState(6401)
    out = []

    def add(name, gt, kept, last, **kw):
        gt = np.asarray(gt, dtype=F)
        out.append(dict(name=name, family="rows", cfg=cfg, gt=gt, M=gt.shape[1], kept=kept, last=last,
                        chunks=[None if v is None else v // CHUNK for v in last], present=rows_present, **kw))

    add("rows M=0", np.zeros((2, 0, 8), dtype=F), [0, 0], [None, None])
    add("rows M=1: a live row and a zero row", [rows_sample(rs, flat, 1, 0), np.zeros((1, 8), dtype=F)], [1, 1], [0, None])
    for M in (63, 64, 65, 127, 128, 129, 300):
        lasts = [v for v in (0, 62, 63, 64, 127, 128) if v < M - 1] + [M - 1]
        gt = [rows_sample(rs, flat, M, v, i) for i, v in enumerate(lasts)]
        add("rows M=%d: the last live row at %s, chunks %s" % (M, lasts, sorted({v // CHUNK for v in lasts})), gt,
            [v + 1 for v in lasts], lasts)
    # a whole chunk of zero rows between two live chunks stays kept
    g = rows_sample(rs, flat, 200, 150)
    g[64:128] = 0

    def zero_chunk(case):
        assert not case["gt"][0, 64:128].any() and case["gt"][0, :64, :7].any(axis=1).sum() > 32 and case["kept"] == [151]
    add("rows M=200: chunk 1 all zero between live chunks 0 and 2", [g], [151], [150], more=zero_chunk)
    # all chunks after the first zero
    g = rows_sample(rs, flat, 300, 40)

    def first_only(case):
        assert not case["gt"][0, 64:].any() and case["M"] > 4 * CHUNK
    add("rows M=300: every chunk after the first is zero", [g], [41], [40], more=first_only)
    # a trailing row that sums to 0 alone in the last chunk: trimmed.  Sample 0 the row [1, -1, 0, ...], sample 1 a row with
    # an anchor's footprint (4 - 2 - 1.5 + 2 + 1 - 3.5 + 0 = 0 exactly in every order), which would change the outputs if kept
    g0, g1 = rows_sample(rs, flat, 130, 100), rows_sample(rs, flat, 130, 127, 1)
    g0[129] = [1, -1, 0, 0, 0, 0, 0, 1]
    g1[129] = [4, -2, -1.5, 2, 1, -3.5, 0, 1]

    def trailing(case):
        gt = case["gt"]
        for b in range(2):
            assert not gt[b, 128].any() and gt[b, 129, :7].any() and gt[b, 129, :7].sum() == 0
            assert not gt[b, case["kept"][b]:128].any()
        a = flat[(flat[:, 0] == 4) & (flat[:, 1] == -2) & (flat[:, 6] == 0)]
        assert len(a) == 1 and a[0, 3] == 2 and a[0, 4] == 1     # kept, that row would have IoU 1 with this anchor
    add("rows M=130: a trailing row summing to 0 alone in chunk 2 is trimmed", [g0, g1], [101, 128], [100, 127], more=trailing)
    # a sample of zero rows only: row 0 kept, its id 0 names the last class, which has anchors: n_sel = 1, every IoU 0
    g0 = rows_sample(rs, flat, 130, 129)

    def all_zero(case):
        ref = reference(case)
        d = ref["details"][1][0]
        assert not case["gt"][1].any() and case["cfg"]["class_names"][-1] == case["cfg"]["classes"][-1]["class_name"]
        assert len(d["rows"]) == 1 and d["rows"][0] == 0 and not d["iou"].any()
        assert not ref["out"]["box_cls_labels"][1].any()
    add("rows M=130: a sample of zero rows only keeps row 0 for the last class", [g0, np.zeros((130, 8), dtype=F)], [130, 1],
        [129, None], more=all_zero)
    return out


# ================================================================================================ select: the compaction
def select_cfg():
    """three anchor classes and a name without anchors, 24 x 20 locations: 960 anchors per class"""
    return dict(anchor_range=[0, 0, -3, 76, 92, 1], use_multihead=False, code_size=7, sincos=False,
                class_names=["Car", "Pedestrian", "Cyclist", "Van"],
                classes=[cls("Car", [[3.9, 1.6, 1.56]], [0, 1.57], [-1.78], 0.6, 0.45, (20, 24)),
                         cls("Pedestrian", [[0.8, 0.6, 1.73]], [0, 1.57], [-0.6], 0.5, 0.35, (20, 24)),
                         cls("Cyclist", [[1.76, 0.6, 1.73]], [0, 1.57], [-0.6], 0.5, 0.35, (20, 24))])


def select_ids(rs, M, counts, all_chunk=None, none_chunk=None):
    """a kind per row: 1..3 a gt of that class, -1..-3 one of that class 1000 m away, 0 a live row with id 0, 4 the name
    without anchors, 9 a zero row.  Every chunk but `all_chunk` = (chunk, class) gets one far row, one id 0, one of the
    anchor-less name and one zero row; `none_chunk` = (chunk, class) gets no row of that class; the rest is shuffled."""
    counts = dict(counts)
    ids = [None] * M
    n_chunks = (M + CHUNK - 1) // CHUNK
    other = M - sum(counts.values())
    if all_chunk:
        k, c = all_chunk
        ids[k * CHUNK:(k + 1) * CHUNK] = [c] * CHUNK
        counts[c] -= CHUNK
        assert counts[c] >= 0
    for k in range(n_chunks):
        if all_chunk and k == all_chunk[0]:
            continue
        free = [j for j in range(k * CHUNK, min(M, (k + 1) * CHUNK))]
        at = rs.choice(free[:-1], 4, replace=False)      # not the chunk's last row: the sample's last row stays a gt
        ok = [c for c in counts if counts[c] > 0 and not (none_chunk and none_chunk == (k, c))]
        c = ok[rs.randint(len(ok))]
        ids[at[0]] = -c
        counts[c] -= 1
        ids[at[1]], ids[at[2]], ids[at[3]] = 0, 4, 9
        other -= 3
    assert other >= 0
    pool = [c for c, n in counts.items() for _ in range(n)] + [(0, 4, 9)[i % 3] for i in range(other)]
    pool = [pool[i] for i in rs.permutation(len(pool))]
    if none_chunk:
        k, c = none_chunk
        for j in range(k * CHUNK, (k + 1) * CHUNK):
            if ids[j] is None:
                i = next(i for i, v in enumerate(pool) if v != c)
                ids[j] = pool.pop(i)
    for j in range(M):
        if ids[j] is None:
            ids[j] = pool.pop()
    assert not pool
    if ids[-1] not in (1, 2, 3):       # the last row a gt near the anchors, so that nothing is trimmed
        lo = max(k for k in range(n_chunks) if not (all_chunk and k == all_chunk[0]) and not (none_chunk and k == none_chunk[0])
                 and k < n_chunks - 1)
        j = next(j for j in range(lo * CHUNK, (lo + 1) * CHUNK) if ids[j] in (1, 2, 3)
                 and not (none_chunk and none_chunk[0] == n_chunks - 1 and ids[j] == none_chunk[1]))
        ids[-1], ids[j] = ids[j], ids[-1]
    return ids


def select_gt(rs, cfg, samples, M):
    flats = [seq.flatten(a, False) for a in seq.make_anchors(cfg)]
    gt = np.zeros((len(samples), M, 8), dtype=F)
    for b, s in enumerate(samples):
        for j, kind in enumerate(select_ids(rs, M, s["counts"], s.get("all"), s.get("none"))):
            if kind == 9:
                continue
            c = abs(kind) if kind in (1, 2, 3, -1, -2, -3) else 1 + rs.randint(3)
            gt[b, j] = near(rs, flats[c - 1], kind if kind in (0, 4) else c, 8, far=kind < 0)
    return gt


def select_present(case):
    ref = reference(case)
    cfg, gt = case["cfg"], case["gt"]
    names = cfg["class_names"]
    M = gt.shape[1]
    seen = set()
    for b, s in enumerate(case["samples"]):
        assert seq.kept_rows(gt[b, :, :-1]) == M
        cids = gt[b, :, -1].astype(np.int32)
        member = [seq.class_rows(cids, names, c["class_name"]) for c in cfg["classes"]]
        for ci in range(3):
            n = int(member[ci].sum())
            assert n == s["counts"][ci + 1] == len(ref["details"][b][ci]["rows"]), (case["name"], b, ci, n)
            seen.add(n)
        zero = ~gt[b, :, :-1].any(axis=1)
        far = gt[b, :, 0] > FAR / 2
        van = (cids == 4) & ~zero
        id0 = (cids == 0) & ~zero
        full = [k for k in range(M // CHUNK)]
        for k in range((M + CHUNK - 1) // CHUNK):
            sl = slice(k * CHUNK, min(M, (k + 1) * CHUNK))
            if s.get("all") and s["all"][0] == k:
                assert member[s["all"][1] - 1][sl].all() and k in full, (case["name"], b, "the chunk of one class")
                continue
            if s.get("none") and s["none"][0] == k:
                assert not member[s["none"][1] - 1][sl].any() and member[s["none"][1] - 1].any(), (case["name"], b)
            assert zero[sl].any() and far[sl].any() and van[sl].any() and id0[sl].any(), (case["name"], b, k)
            big = [ci for ci in range(3) if s["counts"][ci + 1] >= 2 * CHUNK and not (s.get("none") == (k, ci + 1))]
            if k in full:
                assert all(member[ci][sl].any() and not member[ci][sl].all() for ci in big), (case["name"], b, k, "not interleaved")
        for ci in range(3):
            d = ref["details"][b][ci]
            if "colmax" in d:
                assert ((d["colmax"] == 0) == (gt[b, d["rows"], 0] > FAR / 2)).all()
    assert set(case["need"]) <= seen or any(n >= 513 for n in seen) and case["need"] == ["513+"], (case["name"], seen)
    assert (ref["out"]["box_cls_labels"] > 0).any(axis=1).all()


def select_cases():
    cfg = select_cfg()
    rs = np.random.RandomState(25601)
    a = [dict(counts={1: 0, 2: 256, 3: 1}, all=(2, 2)),
         dict(counts={1: 257, 2: 0, 3: 1}, all=(0, 1)),
         dict(counts={1: 63, 2: 64, 3: 65}, all=(3, 3), none=(1, 1)),
         dict(counts={1: 255, 2: 1, 3: 0}, all=(4, 1))]
    b = [dict(counts={1: 513, 2: 20, 3: 0}, all=(7, 1), none=(3, 2)),
         dict(counts={1: 0, 2: 300, 3: 257}, all=(1, 3), none=(8, 3))]
    return [dict(name="select M=330: n_sel 0, 1, 63, 64, 65, 255, 256, 257 in one batch", family="select", cfg=cfg, samples=a,
                 gt=select_gt(rs, cfg, a, 330), need=[0, 1, 63, 64, 65, 255, 256, 257], present=select_present),
            dict(name="select M=600: n_sel 513 next to a sample without a gt of the class", family="select", cfg=cfg, samples=b,
                 gt=select_gt(rs, cfg, b, 600), need=["513+"], present=select_present)]


# ================================================================================================ tiles: ties and forcing
NX, NY = 20, 24


def tiles_cfg():
    """one class, 24 x 20 locations 4 m apart, 960 anchors of 2 x 1 in four workgroups; location (ix, iy) holds anchors
    2 (iy NX + ix) (rotation 0) and + 1 (rotation 1.57)"""
    return dict(anchor_range=[0, 0, -3, 76, 92, 1], use_multihead=False, code_size=7, sincos=False, class_names=["Car"],
                classes=[cls("Car", [[2.0, 1.0, 1.5]], [0, 1.57], [-1.0], 0.6, 0.45, (NX, NY))])


def anchor_at(ix, iy, r=0):
    return 2 * (iy * NX + ix) + r


def twin(ix, iy, z, sx=4.0, sy=4.0, x0=0.0, y0=0.0, a=(2.0, 1.0), cid=1):
    """a gt of 1.125 x 1.25 times the anchor a centred on location (ix, iy): IoU 1 / 1.40625 with its rotation-0 anchor"""
    return [x0 + sx * ix, y0 + sy * iy, z, a[0] * 1.125, a[1] * 1.25, 1.5, 0, cid]


def forcer(ix, iy, sx=4.0, sy=4.0, x0=0.0, y0=0.0, a=(2.0, 1.0), cid=1, k_at=1.125, k_len=2.0):
    """(j, k): j (0.75 x 1 anchors, off the corner) has its column maximum, far below `matched`, at a rotation-0 anchor
    of (ix, iy); that anchor overlaps k (k_len anchors long, k_at anchors along x, its best anchor one of (ix + 1, iy))
    more: forced by j, it takes k's box"""
    x, y = x0 + sx * ix, y0 + sy * iy
    j = [x + 0.75 * a[0], y + 0.75 * a[1], -0.2, 0.75 * a[0], a[1], 1.5, 0, cid]
    k = [x + k_at * a[0], y, -0.1, k_len * a[0], a[1], 1.6, 0, cid]
    return j, k


def between(ix, iy, dx=0.0, w=3.0):
    """a gt w x 3 centred dx off the middle between locations (ix, iy) and (ix + 1, iy)"""
    return [4 * ix + 2 + dx, 4 * iy, -0.4, w, 3, 1.5, 0, 1]


def tiles_gt(rs, n, specials, taken):
    """n rows of one class: `specials` {position: row}, every other position a small square on a location of its own (IoU
    1/8 with both its anchors) or, one in four and once the locations run out, a gt 1000 m away"""
    free = [(ix, iy) for iy in range(NY) for ix in range(NX) if (ix, iy) not in taken]
    free = [free[i] for i in rs.permutation(len(free))]
    g = np.zeros((n, 8), dtype=F)
    for p in range(n):
        if p in specials:
            g[p] = specials[p]
        elif free and rs.randint(4):
            ix, iy = free.pop()
            g[p] = [4 * ix, 4 * iy, rs.uniform(-1, 0), 0.5, 0.5, 1.5, 0, 1]
        else:
            g[p] = [FAR + rs.uniform(0, 50), rs.uniform(0, 50), -0.5, 2, 1, 1.5, 0, 1]
    return g


def tiles_present(case):
    ref = reference(case)
    for b in range(case["gt"].shape[0]):
        d = ref["details"][b][0]
        assert np.array_equal(d["rows"], np.arange(case["gt"].shape[1]))     # one class: position == row
    case["check"](case, ref)


def tiles_cases():
    cfg = tiles_cfg()
    rs = np.random.RandomState(51201)
    out = []

    def add(name, gt, check):
        out.append(dict(name=name, family="tiles", cfg=cfg, gt=np.asarray(gt, dtype=F), present=tiles_present, check=check))

    for bd in (CHUNK, TILE):
        n = bd + 40
        # ---- the lowest index wins across the boundary: (p, q) = (bd - 1, bd) and (3, bd + 5)
        pairs = [(bd - 1, bd, (3, 2)), (3, bd + 5, (9, 15))]
        sp = {}
        for p, q, (ix, iy) in pairs:
            sp[p], sp[q] = twin(ix, iy, -0.25), twin(ix, iy, 0.5)

        def lowest(case, ref, pairs=pairs, bd=bd):
            d = ref["details"][0][0]
            lab = class_labels(d, case["cfg"], 7)
            for p, q, (ix, iy) in pairs:
                assert p < bd <= q
                i = anchor_at(ix, iy)
                tie = np.flatnonzero((d["iou"][:, p] == d["rowmax"]) & (d["iou"][:, q] == d["rowmax"]) & (lab > 0))
                assert i in tie and (d["arg"][tie] == p).all() and case["gt"][0, p, 2] != case["gt"][0, q, 2]
                assert np.array_equal(seq.bits(d["iou"][:, p]), seq.bits(d["iou"][:, q]))
        add("tiles %d: one footprint at positions either side of the boundary, the lower index wins" % bd,
            [tiles_gt(rs, n, sp, {(3, 2), (9, 15)})], lowest)
        # ---- forced from a later tile, taking an earlier tile's box; the mirror image; a zero column maximum late
        j1, k1 = forcer(5, 5)
        j2, k2 = forcer(12, 18)
        sp = {7: k1, bd + 3: j1, 11: j2, bd + 9: k2, bd + 1: [FAR, 8, -0.5, 2, 1, 1.5, 0, 1]}
        spots = [((5, 5), bd + 3, 7), ((12, 18), 11, bd + 9)]

        def forced(case, ref, spots=spots, bd=bd):
            d = ref["details"][0][0]
            lab = class_labels(d, case["cfg"], 7)
            for (ix, iy), j, k in spots:
                i = anchor_at(ix, iy)
                assert (j < bd) != (k < bd)
                assert 0 < d["colmax"][j] < d["unmatched"] and d["iou"][i, j] == d["colmax"][j]
                assert np.flatnonzero(d["iou"][:, j] == d["colmax"][j]).tolist() == [i]
                assert d["arg"][i] == k and d["rowmax"][i] < d["unmatched"] and d["forced"][i] and lab[i] == 1
                assert d["iou"][i, k] < d["colmax"][k]                   # nothing but j forces the anchor
                rest = np.arange(len(d["colmax"])) != j
                assert ((d["iou"][i] != d["colmax"]) | (d["colmax"] == 0))[rest].all()
            z = bd + 1
            assert d["colmax"][z] == 0 and case["gt"][0, z, :7].any() and not (d["iou"][:, z] != 0).any()
            # late forcing only: the forced set of the first `bd` gts alone is another one
            early = []
            seq.assign(case["cfg"], ref["anchors"], case["gt"][:, :bd], early)
            assert early[0][0]["forced"][anchor_at(5, 5)] != d["forced"][anchor_at(5, 5)]
            assert (early[0][0]["forced"] != d["forced"]).any()
        add("tiles %d: forced from past the boundary with the argmax before it, the mirror image, a zero column maximum late" % bd,
            [tiles_gt(rs, n, sp, {(5, 5), (6, 5), (12, 18), (13, 18)})], forced)

    # ---- the argmax in tile 2, every tile with work
    def third(case, ref):
        d = ref["details"][0][0]
        lab = class_labels(d, case["cfg"], 7)
        assert len(d["rows"]) > 2 * TILE and ((d["arg"] >= 2 * TILE) & (lab > 0)).any()
        for t in range(3):
            assert ((d["arg"] // TILE == t) & (lab > 0)).any() and (d["colmax"][t * TILE:(t + 1) * TILE] == 0).any()
        i = anchor_at(10, 10)
        assert d["arg"][i] == 2 * TILE + 8 and d["rowmax"][i] >= d["matched"]
    add("tiles 512: an argmax in the third tile", [tiles_gt(rs, 2 * TILE + 30, {2 * TILE + 8: twin(10, 10, -0.3)}, {(10, 10)})], third)

    # ---- a column maximum reached with identical bits in two workgroups; one whose IoUs differ between two workgroups
    sp = {20: between(7, 6), TILE + 20: between(15, 12), 30: between(3, 19, dx=-0.5, w=4.0)}

    def across(case, ref):
        d = ref["details"][0][0]
        for p, (ix, iy) in ((20, (7, 6)), (TILE + 20, (15, 12))):
            i, k = anchor_at(ix, iy), anchor_at(ix + 1, iy)
            assert i // BLOCK != k // BLOCK and d["colmax"][p] > 0
            assert np.flatnonzero(d["iou"][:, p] == d["colmax"][p]).tolist() == [i, k]
            assert d["forced"][i] and d["forced"][k] and d["arg"][i] == p and d["arg"][k] == p
        i, k = anchor_at(3, 19, 1), anchor_at(4, 19)
        assert i // BLOCK != k // BLOCK and d["iou"][i, 30] == d["colmax"][30] > d["iou"][k, 30] > 0
        assert d["forced"][i] and not d["forced"][k]
        assert (np.delete(d["iou"][k], 30) == 0).all()
    add("tiles: a column maximum with equal bits in two workgroups, and one that only the merge decides",
        [tiles_gt(rs, TILE + 40, sp, {(7, 6), (8, 6), (15, 12), (16, 12), (3, 19), (4, 19)})], across)
    return out


# ================================================================================================ layouts: unequal classes
def single_cfg(align=False, grid=(10, 8)):
    """2, 6 and 4 anchors per location and two bottom heights: the largest class is not the first"""
    nx, ny = grid
    return dict(anchor_range=[0, -14, -3, 36, 14, 1], use_multihead=False, code_size=7, sincos=False,
                class_names=["Car", "Pedestrian", "Cyclist"],
                classes=[cls("Car", [[3.9, 1.6, 1.56]], [0, 1.57], [-1.78, -1.0], 0.6, 0.45, grid, align),
                         cls("Pedestrian", [[0.8, 0.6, 1.73], [1.0, 0.8, 1.8]], [0, 0.78, 1.57], [-0.6, -0.3], 0.5, 0.35, grid, align),
                         cls("Cyclist", [[1.76, 0.6, 1.73], [2.0, 0.8, 1.6]], [0, 1.57], [-0.6, -0.3], 0.5, 0.35, grid, align)])


def multi_cfg():
    """classes on grids of their own: 70, 35, 1 248 and 1 000 rows, the longest in the middle, 9 columns + sincos"""
    return dict(anchor_range=[0, -20, -3, 48, 20, 1], use_multihead=True, code_size=9, sincos=True,
                class_names=["Car", "Pedestrian", "Cyclist", "Truck"],
                classes=[cls("Car", [[3.9, 1.6, 1.56]], [0, 1.57], [-1.78], 0.6, 0.45, (7, 5)),
                         cls("Pedestrian", [[0.8, 0.6, 1.73]], [0], [-0.6], 0.5, 0.35, (7, 5)),
                         cls("Cyclist", [[1.76, 0.6, 1.73]], [0, 1.57], [-0.6], 0.5, 0.35, (26, 24)),
                         cls("Truck", [[6.0, 2.5, 2.8]], [0, 1.57], [-1.5], 0.55, 0.4, (25, 20))])


def layout_gt(rs, cfg, per_class=(0, 1, 80), pad=3):
    anchors = seq.make_anchors(cfg)
    flats = [seq.flatten(a, cfg["use_multihead"]) for a in anchors]
    cols = 8 + (2 if cfg["code_size"] == 9 else 0)
    n = len(flats)
    counts = [[per_class[(ci + b) % 3] for ci in range(n)] for b in range(3)]
    gt = np.zeros((3, max(sum(c) for c in counts) + pad, cols), dtype=F)
    for b in range(3):
        kinds = [ci for ci in range(n) for _ in range(counts[b][ci])]
        for j, i in enumerate(rs.permutation(len(kinds))):
            gt[b, j] = near(rs, flats[kinds[i]], kinds[i] + 1, cols, far=rs.randint(12) == 0 and counts[b][kinds[i]] > 1)
    return gt, counts


def layout_present(case):
    ref = reference(case)
    cfg = case["cfg"]
    rows = [int(np.prod(a.shape[:5])) for a in ref["anchors"]]
    ks = [a.shape[3] * a.shape[4] for a in ref["anchors"]]
    assert rows == case["rows"] and ks == case["k"], (rows, ks)
    if cfg["use_multihead"]:
        assert min(rows) < 64 and any(r % BLOCK for r in rows) and max(rows) >= min(rows) + 4 * BLOCK
        assert 0 < rows.index(max(rows)) < len(rows) - 1 and 35 in rows and 70 in rows and 1000 in rows
        assert len({tuple(c["grid_size"]) for c in cfg["classes"]}) >= 3
    else:
        assert sorted(ks) == [2, 4, 6] and ks[0] != max(ks) and all(a.shape[0] == 2 for a in ref["anchors"])
        assert all(c["align_center"] == case["align"] for c in cfg["classes"])
    first = np.cumsum([0] + rows)
    stride = sum(ks)
    lab = ref["out"]["box_cls_labels"]
    for ci in range(len(rows)):
        got = sorted(len(ref["details"][b][ci]["rows"]) for b in range(3))
        assert got[0] == 0 and got[1] == 1 and got[2] >= 70, (case["name"], ci, got)
        if cfg["use_multihead"]:
            mine = lab[:, first[ci]:first[ci + 1]]
        else:
            off = sum(ks[:ci])
            mine = lab.reshape(3, -1, stride)[:, :, off:off + ks[ci]]
        assert (mine == ci + 1).any() and not ((mine > 0) & (mine != ci + 1)).any(), (case["name"], ci)


def layout_cases():
    rs = np.random.RandomState(24601)
    out = []
    for align in (False, True):
        cfg = single_cfg(align)
        gt, _ = layout_gt(rs, cfg)
        out.append(dict(name="layouts single head: k = 2, 6, 4, two heights" + (", align_center" if align else ""), family="layouts",
                        cfg=cfg, gt=gt, rows=[320, 960, 640], k=[2, 6, 4], align=align, present=layout_present))
    cfg = multi_cfg()
    gt, _ = layout_gt(rs, cfg)
    out.append(dict(name="layouts multihead: 70, 35, 1248 and 1000 rows on grids of their own", family="layouts", cfg=cfg, gt=gt,
                    rows=[70, 35, 1248, 1000], k=[2, 1, 2, 2], present=layout_present))
    return out


# ================================================================================================ columns
def columns_cfg(code_size, sincos):
    return dict(anchor_range=[0, -8, -3, 24, 8, 1], use_multihead=False, code_size=code_size, sincos=sincos, class_names=["Car", "Cyclist"],
                classes=[cls("Car", [[2.0, 1.0, 1.5]], [0, 1.57], [-1.0], 0.5, 0.25, (7, 5)),
                         cls("Cyclist", [[1.75, 0.5, 1.75]], [0, 1.57], [-0.6], 0.45, 0.3, (7, 5))])


def columns_present(case):
    ref = reference(case)
    cfg, gt = case["cfg"], case["gt"]
    a_cols = ref["anchors"][0].shape[-1]
    assert (a_cols, gt.shape[2]) == case["cols"]
    code = ref["out"]["box_reg_targets"].shape[-1]
    assert code == 7 + int(cfg["sincos"]) + min(a_cols - 7, gt.shape[2] - 8) == case["code"]
    row = gt[0, 8]
    assert row[:7].any() and row[:7].sum() == 0 and not gt[0, 9:].any()
    if gt.shape[2] == 10:      # the velocities keep the row, which then owns the anchor under it
        assert row[7:9].sum() != 0 and seq.kept_rows(gt[0, :, :-1]) == 9
        d = ref["details"][0][0]
        p = position(d, 8)
        assert ((d["arg"] == p) & (d["rowmax"] == 1)).any()
    else:
        assert seq.kept_rows(gt[0, :, :-1]) == 8
    fg = ref["out"]["box_cls_labels"] > 0
    assert fg.any()
    if code > 7 + int(cfg["sincos"]):
        assert ref["out"]["box_reg_targets"][fg][:, -2:].any()


def columns_cases():
    rs = np.random.RandomState(71001)
    out = []
    for (a_cols, g_cols, code_size, sincos) in ((7, 8, 7, False), (7, 10, 7, False), (9, 10, 9, False), (10, 10, 9, True)):
        cfg = columns_cfg(code_size, sincos)
        flats = [seq.flatten(a, False) for a in seq.make_anchors(cfg)]
        gt = np.zeros((2, 12, g_cols), dtype=F)
        for b in range(2):
            for j in range(8 - 3 * b):
                gt[b, j] = near(rs, flats[j % 2], 1 + j % 2, g_cols)
        # the seven box values sum to 0 exactly, the velocities (where the gt has them) do not
        gt[0, 8, :7] = [4, -4, -1.5, 2, 1, -1.5, 0]
        gt[0, 8, 7:-1] = [0.5, 0.25][:g_cols - 8]
        gt[0, 8, -1] = 1
        code = 7 + int(sincos) + min(a_cols - 7, g_cols - 8)
        out.append(dict(name="columns: anchors %d, gt %d%s" % (a_cols, g_cols, ", sincos" if sincos else ""), family="columns", cfg=cfg,
                        gt=gt, cols=(a_cols, g_cols), code=code, present=columns_present))
    return out


# ================================================================================================ zero sizes
def zero_present(case):
    ref = reference(case)
    B, M = case["gt"].shape[:2]
    assert (B == 0 or M == 0) and (B, M) == case["BM"]
    n = sum(int(np.prod(a.shape[:5])) for a in ref["anchors"])
    out = ref["out"]
    assert out["box_cls_labels"].shape == (B, n) and out["box_reg_targets"].shape == (B, n, 7) and out["reg_weights"].shape == (B, n)
    assert not any(v.any() for v in out.values())


def zero_cases():
    cfg = columns_cfg(7, False)
    return [dict(name="zero sizes: B = %d, M = %d" % (B, M), family="zero", cfg=cfg, gt=np.zeros((B, M, 8), dtype=F), BM=(B, M),
                 present=zero_present) for B, M in ((0, 5), (2, 0), (0, 0))]


_CASES = []


def cases():
    """every case, built once"""
    if not _CASES:
        _CASES.extend(rows_cases() + select_cases() + tiles_cases() + layout_cases() + columns_cases() + zero_cases())
        for c in _CASES:
            c["gt"].setflags(write=False)
        assert len({c["name"] for c in _CASES}) == len(_CASES)
    return _CASES


def names():
    return [c["name"] for c in cases()]


def by_name(name):
    return next(c for c in cases() if c["name"] == name)
