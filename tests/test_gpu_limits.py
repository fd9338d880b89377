"""GPU: stages 2 + 3 at the sizes the product runs and past every fixed capacity of their kernels -- mask / seed chains
longer than one MAD launch (MAD_SETS = 16 sets: 8 scans) and than the staging slots (MODEST_STAGE_SLOTS = 8), clusters
and cluster counts past the LDS sizes of the statistics kernels (CS_LDS_KEYS = CS_GROUP_MAXC = 8 192), more boxes than
one lowest-point launch has tickets for (MODEST_ZW_TICKETS = 4 096), a PP block of 64 scans (b4_deal's table at
G = 64) and NMS on more boxes than one pinned chunk of the host walk holds (32 MB: 16 256 rows at cb = 258).

Bars: integer / index / label outputs, order statistics and thresholds bit exact against a plain NumPy statement of the
same operation; plane distances to a few ulp (fma chain against NumPy's dot product); box rows 1e-9 against the oracle."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _calib(tmp_path):
    from modest_amd import synth
    from modest_amd.utils import kitti_util
    open(tmp_path / "c.txt", "w").write(synth.CALIB_TXT)
    return kitti_util.Calibration(str(tmp_path / "c.txt"))


# --------------------------------------------------------------------------- 1. MAD thresholds, mask / seed chains
def _mad_ref(z):
    z = np.asarray(z, dtype=np.float32)
    med = np.median(z)
    assert med.dtype == np.float32
    return np.median(np.abs(z - med))


def test_mad_threshold_batch_past_one_launch(gpu):
    """ops.mad_threshold_batch with 1, 15, 16, 17 and 33 sets (a launch holds MAD_SETS = 16): every threshold equals
    np.median(|z - median(z)|) in float32, bit for bit -- sets of one and two candidates, ties, and sets of more than
    32 768 candidates (past the keys kept in registers: the KeysGlobal passes)."""
    import torch
    from modest_amd import ops
    rng = np.random.default_rng(21)
    sizes = [1, 2, 3, 1023, 1024, 1025, 32767, 32768, 32769, 45000, 70001, 5000, 400, 12000, 301, 299, 2048]
    for count in (1, 15, 16, 17, 33):
        cands, refs = [], []
        for k in range(count):
            n = sizes[(k * 7 + count) % len(sizes)]
            z = rng.normal(-1.7, 0.05, n).astype(np.float32)
            if k % 3 == 1:
                z = np.round(z * 50).astype(np.float32) / np.float32(50)   # heavy ties
            if k % 5 == 2:
                z[: n // 2] = np.float32(-1.7)                            # half of the set one value
            xyz = np.c_[rng.uniform(-20, 20, (n, 2)), z].astype(np.float32)
            cands.append(torch.from_numpy(xyz).to(gpu))
            refs.append(_mad_ref(z))
        got = ops.mad_threshold_batch(cands)
        assert got.dtype == np.float32 and got.shape == (count,)
        for k in range(count):
            assert got[k] == refs[k], (count, k, cands[k].shape[0], got[k], refs[k])
    assert max(sizes) > 32768 and 32769 in sizes


def _chain_scans(gpu, n, seed, tiny):
    """n synthetic scans of 2 000 .. 30 000 points (400 at the indices `tiny`: candidate sets of <= 300 points, which
    the library hands back to the host statement)"""
    import torch
    from modest_amd import synth
    rng = np.random.default_rng(seed)
    scans = []
    for k in range(n):
        n_live = 400 if k in tiny else int(rng.choice([2000, 5000, 9000, 14000, 21000, 30000]))
        raw = np.ascontiguousarray(synth.make_scan(seed * 1000 + k, n_live=n_live, n_trav=2, n_frames=1).live_raw)
        pp = np.clip(0.5 + 0.5 * np.sin(raw[:, 0] * 0.3 + k) + rng.normal(0, 0.03, len(raw)), 0, 1).astype(np.float32)
        scans.append((raw, pp, torch.from_numpy(raw).to(gpu), torch.from_numpy(pp).to(gpu)))
    return scans


def test_mask_and_seed_chains_of_production_length(gpu, tmp_path, monkeypatch):
    """Chains of 9, 16, 17, 32 and 64 scans (configs/generate_mask.yaml: 16, bench.py: 32, the library's limit: 64) through
    both chain paths -- modest_mask_stage_batch + separate box calls (ONE_CALL_CHAIN False) and modest_seed_chain (True) -- and
    gen_label_chain: labels, box rows, plane, kept rows, generator state, IoU matrices and label text equal those of
    generate_mask_scan / gen_label_scan run one scan at a time, with scans the library hands back at index 8, 15, 16 and
    the last; two scans of the longest chain (one of index >= 8) against the oracle."""
    from modest_amd import config, generate_mask as gm, ops
    from modest_amd.gen_label_files import gen_label_chain, gen_label_scan
    from oracle import labels as ol
    from oracle import mask as om
    calib = _calib(tmp_path)
    margs = config.compose("generate_mask", ["data_root=/unused"])
    largs = config.compose("generate_label_files", ["data_root=/unused"])
    tiny = (8, 15, 16, 31, 63)
    scans = _chain_scans(gpu, 64, 41, tiny)
    pe = margs.plane_estimate
    for k in tiny:   # handed back: fewer than 301 ground candidates for the first fit
        assert om.plane_candidate_mask(scans[k][0], pe.max_hs, pe.range).sum() <= 300, k
    single = []
    for k, (raw, pp, rd, pd) in enumerate(scans):
        rs = np.random.RandomState(500 + k)
        labels, rows, info = gm.generate_mask_scan(raw, pp, calib, margs, random_state=rs, ptc_dev=rd, pp_dev=pd, as_rows=True)
        text, kept = gen_label_scan(rows, calib, largs)
        single.append((labels, rows, info, rs.get_state(), text, kept))
    assert sum(len(s[1]) for s in single) >= 100 and sum(len(s[4].splitlines()) for s in single) >= 30

    def run(idx, one_call):
        monkeypatch.setattr(gm, "ONE_CALL_CHAIN", one_call)
        rss = [np.random.RandomState(500 + k) for k in idx]
        res = gm.generate_mask_chain([dict(ptc=scans[k][0], pp_score=scans[k][1], random_state=rs, ptc_dev=scans[k][2],
                                           pp_dev=scans[k][3]) for k, rs in zip(idx, rss)], calib, margs, as_rows=True, with_iou=True)
        lab = gen_label_chain([r[1] for r in res], calib, largs, ious=[r[3] for r in res])
        return res, lab, [rs.get_state() for rs in rss]

    for L in (9, 16, 17, 32, 64):
        idx = list(range(L))
        assert idx[-1] in tiny and any(k in tiny for k in idx[8:])
        for one_call in (False, True):
            res, lab, st = run(idx, one_call)
            n_iou = 0
            for k, (labels, rows, info, iou), (text, kept), s in zip(idx, res, lab, st):
                ref = single[k]
                assert np.array_equal(labels, ref[0]) and np.array_equal(rows, ref[1]), (L, one_call, k)
                assert np.array_equal(info["plane"], ref[2]["plane"]) and info["n_kept"] == ref[2]["n_kept"], (L, one_call, k)
                assert s[2] == ref[3][2] and np.array_equal(s[1], ref[3][1]), (L, one_call, k)
                assert text == ref[4] and np.array_equal(kept, ref[5]), (L, one_call, k)
                if iou is not None and len(rows):
                    assert np.array_equal(iou, ops.objs_iou(rows)), (L, k)
                    n_iou += 1
            assert n_iou >= (L // 3 if one_call else 0), (L, one_call, n_iou)
    # the oracle on two scans of the chain of 64, one of the first eight and one behind them: those with the most boxes
    # among the scans of up to 14 000 points (the oracle's sklearn graph is the slow part)
    pick = [max((k for k in part if len(scans[k][0]) <= 14000), key=lambda k: len(single[k][1])) for part in (range(8), range(8, 64))]
    for k in pick:
        raw, pp = scans[k][0], scans[k][1]
        ref = om.generate_mask_scan(raw, pp, calib, random_state=np.random.RandomState(500 + k), n_jobs=1)
        assert np.array_equal(single[k][0], ref["labels"]), k
        got = single[k][1]
        want = np.array([[*o.t, o.l, o.w, o.h, o.ry, o.volume] for o in ref["objs"]], dtype=np.float64).reshape(-1, 8)
        assert got.shape == want.shape and len(got) >= 2, k
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-9)
        assert single[k][4] == ol.gen_label_scan(ref["objs"], calib)[0], k


# --------------------------------------------------------------------------- 2. cluster statistics
def stats_reference(pts, pp, labels, C, plane, q):
    """ops.cluster_stats restated in NumPy: per cluster (count, min / max signed plane distance in float64, the order
    statistics a <= b that numpy's 'linear' percentile interpolates between, gamma).  The kernel's virtual index is the
    float32 one numpy uses for float32 data: vi = float32(n - 1) * float32(q), gamma = vi - floor(vi) in float32."""
    plane = np.asarray(plane, dtype=np.float64)
    dist = (pts[:, :3] @ plane[:3] + plane[3]) / np.sqrt((plane[:3] ** 2).sum())
    out = np.zeros((C, 6), dtype=np.float64)
    order = np.argsort(labels, kind="stable")
    cuts = np.searchsorted(labels[order], np.arange(C + 1))
    qf = np.float32(q)
    for c in range(C):
        m = order[cuts[c]:cuts[c + 1]]
        n = len(m)
        out[c, 0] = n
        if n == 0:
            continue
        out[c, 1], out[c, 2] = dist[m].min(), dist[m].max()
        vi = np.float32(n - 1) * qf
        fl = np.floor(vi)
        prev, nxt = int(fl), int(fl) + 1
        if vi >= np.float32(n - 1):
            prev = nxt = n - 1
        nxt = min(nxt, n - 1)
        part = np.partition(pp[m], [prev, nxt])
        out[c, 3], out[c, 4], out[c, 5] = part[prev], part[nxt], np.float32(vi - fl)
    return out


def stats_case(rng, sizes, n_noise, pp_kind):
    """points (n,4) float32 with labels: cluster c has sizes[c] members (0 = an empty label), n_noise points of -1,
    everything shuffled; PP values of the given kind"""
    labels = np.concatenate([np.full(s, c, dtype=np.int32) for c, s in enumerate(sizes)] + [np.full(n_noise, -1, dtype=np.int32)])
    rng.shuffle(labels)
    n = len(labels)
    centre = rng.uniform(-30, 30, (len(sizes) + 1, 3)) * np.array([1.0, 1.0, 0.05])
    pts = (centre[labels] + rng.normal(0, 1.5, (n, 3))).astype(np.float32)
    pts = np.c_[pts, rng.uniform(0, 1, n)].astype(np.float32)
    if pp_kind == "ties":
        pp = (rng.integers(0, 6, n) / 5).astype(np.float32)
    elif pp_kind == "equal":
        pp = np.full(n, 0.35, dtype=np.float32)
    elif pp_kind == "signed_zero":
        pp = np.where(rng.uniform(size=n) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
        pp[rng.uniform(size=n) < 0.1] = np.float32(0.25)
    else:
        pp = rng.uniform(0, 1, n).astype(np.float32)
    return np.ascontiguousarray(pts), pp, labels


QUANTILES = (0.0, float(np.float32(10) / np.float32(100)), 0.2, 0.5, 1.0)


def _check_stats(got, ref, pp, labels, q, tag):
    from modest_amd.utils.clustering_utils import percentile_from_order_stats
    assert got.shape == ref.shape, tag
    assert np.array_equal(got[:, 0], ref[:, 0]), tag
    full = ref[:, 0] > 0
    # plane distance: an fma chain on the device against NumPy's dot product -- a few ulp of the terms' magnitude
    scale = np.max(np.abs(ref[full, 1:3])) + 10.0
    assert np.max(np.abs(got[full, 1:3] - ref[full, 1:3])) <= 8 * np.finfo(np.float64).eps * scale, tag
    # order statistics and gamma exact; compared as values (-0.0 == 0.0)
    assert np.all(got[full, 3] == ref[full, 3]) and np.all(got[full, 4] == ref[full, 4]), tag
    assert np.array_equal(got[full, 5], ref[full, 5]), tag
    pct = percentile_from_order_stats(got[:, 3], got[:, 4], got[:, 5])
    order = np.argsort(labels, kind="stable")
    cuts = np.searchsorted(labels[order], np.arange(len(ref) + 1))
    for c in np.flatnonzero(full)[:40]:
        assert pct[c] == np.quantile(pp[order[cuts[c]:cuts[c + 1]]], np.float32(q)), (tag, c)


def _stats_paths(gpu, monkeypatch, pts, pp, labels, C, plane, q):
    """the statistics of one case by the default path and with MODEST_CS_GROUPED=1 (read at every call)"""
    import torch
    from modest_amd import ops
    dp, dpp, dl = (torch.from_numpy(x).to(gpu) for x in (pts, pp, labels))
    out = []
    for grouped in (False, True):
        if grouped:
            monkeypatch.setenv("MODEST_CS_GROUPED", "1")
        else:
            monkeypatch.delenv("MODEST_CS_GROUPED", raising=False)
        out.append(ops.cluster_stats(dp, dpp, dl, C, plane, q))
    monkeypatch.delenv("MODEST_CS_GROUPED", raising=False)
    return out


PLANE = np.array([0.012, -0.021, 0.9996, 1.71], dtype=np.float64)


@pytest.mark.parametrize("pp_kind", ["uniform", "ties", "equal", "signed_zero"])
def test_cluster_stats_large_clusters_every_path(gpu, monkeypatch, pp_kind):
    """Clusters of 1, 2, 3, 8 191 and 8 192 members (the one-launch path: members and keys in LDS) and, in a second call,
    8 193, 20 000 and 100 000 members (cs_stats_direct overflows, the grouped path re-runs with the uncached two-select
    branch), with noise labels and an empty label -- by the default path and with MODEST_CS_GROUPED=1, for every quantile,
    against stats_reference; percentiles equal np.quantile."""
    rng = np.random.default_rng({"uniform": 1, "ties": 2, "equal": 3, "signed_zero": 4}[pp_kind])
    for sizes in ([1, 2, 3, 8191, 0, 8192, 17], [8193, 2, 20000, 0, 100000, 1, 8192]):
        pts, pp, labels = stats_case(rng, sizes, 3000, pp_kind)
        for q in QUANTILES:
            ref = stats_reference(pts, pp, labels, len(sizes), PLANE, q)
            for path, got in zip(("default", "grouped"), _stats_paths(gpu, monkeypatch, pts, pp, labels, len(sizes), PLANE, q)):
                _check_stats(got, ref, pp, labels, q, (pp_kind, max(sizes), q, path))
    # (n - 1) * q is an integer in float32 but not in float64: 10 * float32(0.1) = 1 in float32, 1 + 1.5e-8 in float64
    q = float(np.float32(0.1))
    assert np.float32(10) * np.float32(q) == np.float32(1) and 10 * q != 1.0
    pts, pp, labels = stats_case(rng, [11, 11, 9001, 3], 50, "uniform")
    ref = stats_reference(pts, pp, labels, 4, PLANE, q)
    assert ref[0, 5] == 0.0 and ref[0, 3] < ref[0, 4]   # gamma 0: the percentile is the order statistic of rank 1 itself
    for path, got in zip(("default", "grouped"), _stats_paths(gpu, monkeypatch, pts, pp, labels, 4, PLANE, q)):
        _check_stats(got, ref, pp, labels, q, ("float32 index", path))


@pytest.mark.parametrize("n_clusters", [8192, 8193, 20000])
def test_cluster_stats_many_clusters(gpu, monkeypatch, n_clusters):
    """8 192 clusters (the one-workgroup grouping pass) and 8 193 / 20 000 (cs_count, cs_scan, cs_scatter), with and without a
    cluster of 9 000 members (the default path overflows into the grouped one), by both paths, against stats_reference."""
    rng = np.random.default_rng(n_clusters)
    for big in (False, True):
        sizes = rng.integers(1, 9, n_clusters)
        sizes[rng.integers(0, n_clusters, 20)] = 0
        if big:
            sizes[n_clusters // 2] = 9000
        pts, pp, labels = stats_case(rng, list(sizes), 5000, "ties" if big else "uniform")
        for q in (QUANTILES[1], 0.5):
            ref = stats_reference(pts, pp, labels, n_clusters, PLANE, q)
            for path, got in zip(("default", "grouped"), _stats_paths(gpu, monkeypatch, pts, pp, labels, n_clusters, PLANE, q)):
                _check_stats(got, ref, pp, labels, q, (n_clusters, big, q, path))


def test_chain_statistics_fallback_for_a_cluster_past_the_lds(gpu, tmp_path):
    """A dense wall of 12 000 points with one PP value (40 m long, 0.1 m thick, 0.6 m high: a box of 2.4 m^3 the volume gate
    keeps) spliced into one scan of a chain of 10: DBSCAN returns a cluster of 12 000 points, the chain's statistics launch
    (csb_stats) overflows for that scan and modest_cluster_stats takes it on its own.  The chain (both paths), the per-scan call
    and the oracle's generate_mask_scan (filter_labels) agree."""
    import torch
    from modest_amd import config, generate_mask as gm
    from oracle import mask as om
    calib = _calib(tmp_path)
    margs = config.compose("generate_mask", ["data_root=/unused"])
    scans = _chain_scans(gpu, 10, 43, (9,))
    rng = np.random.default_rng(5)
    raw = scans[4][0]
    blk = np.c_[rng.uniform(5.0, 45.0, 12000), rng.uniform(6.0, 6.1, 12000), rng.uniform(-1.3, -0.7, 12000),
                rng.uniform(0, 1, 12000)].astype(np.float32)
    keep = ~((raw[:, 0] > 4.0) & (raw[:, 0] < 46.0) & (raw[:, 1] > 5.0) & (raw[:, 1] < 7.1))
    raw = np.ascontiguousarray(np.r_[raw[keep], blk])
    pp = np.r_[scans[4][1][keep], np.full(12000, 0.2, dtype=np.float32)].astype(np.float32)
    scans[4] = (raw, pp, torch.from_numpy(raw).to(gpu), torch.from_numpy(pp).to(gpu))
    ref = om.generate_mask_scan(raw, pp, calib, random_state=np.random.RandomState(904), n_jobs=1)
    db = ref["dbscan"]
    assert np.bincount(db[db >= 0]).max() > 8192          # the branch: a DBSCAN cluster past CS_LDS_KEYS
    assert np.bincount(ref["labels"])[1:].max() > 8192    # ... which filter_labels and the volume gate keep
    single = gm.generate_mask_scan(raw, pp, calib, margs, random_state=np.random.RandomState(904), ptc_dev=scans[4][2],
                                   pp_dev=scans[4][3], as_rows=True)
    assert np.array_equal(single[0], ref["labels"])
    want = np.array([[*o.t, o.l, o.w, o.h, o.ry, o.volume] for o in ref["objs"]], dtype=np.float64).reshape(-1, 8)
    np.testing.assert_allclose(single[1], want, rtol=1e-9, atol=1e-9)
    for one_call in (False, True):
        gm.ONE_CALL_CHAIN = one_call
        try:
            res = gm.generate_mask_chain([dict(ptc=s[0], pp_score=s[1], random_state=np.random.RandomState(900 + k), ptc_dev=s[2],
                                               pp_dev=s[3]) for k, s in enumerate(scans)], calib, margs, as_rows=True)
        finally:
            gm.ONE_CALL_CHAIN = True
        assert np.array_equal(res[4][0], single[0]) and np.array_equal(res[4][1], single[1]), one_call
        for k in (0, 9):
            s = scans[k]
            one = gm.generate_mask_scan(s[0], s[1], calib, margs, random_state=np.random.RandomState(900 + k), ptc_dev=s[2],
                                        pp_dev=s[3], as_rows=True)
            assert np.array_equal(res[k][0], one[0]) and np.array_equal(res[k][1], one[1]), (one_call, k)


# --------------------------------------------------------------------------- 3. lowest point inside a box
def _lowest_ref(pts, boxes):
    """oracle.mask.get_lowest_point_rect per box (float64 NumPy); -inf where no point is inside (numpy raises there)"""
    from oracle import mask as om
    out = np.empty(len(boxes), dtype=np.float64)
    for i, (cx, cz, l, w, ry) in enumerate(boxes):
        try:
            out[i] = om.get_lowest_point_rect(pts, np.array([cx, cz]), l, w, ry)
        except ValueError:
            out[i] = -np.inf
    return out


def _boxes6(boxes):
    b = np.asarray(boxes, dtype=np.float64)
    return np.c_[b[:, 0], b[:, 1], b[:, 2], b[:, 3], np.cos(b[:, 4]), np.sin(b[:, 4])]


def test_lowest_point_many_boxes_edges_and_empty_boxes(gpu):
    """ops.lowest_point against get_lowest_point_rect: 4 097 and 9 000 boxes (more than one launch of MODEST_ZW_TICKETS =
    4 096 ticket words), a cluster of 50 000 points (every one of the LOW_SPLIT = 8 slices holds the maximum of some box),
    empty boxes (-inf), points exactly on the +-l/2 and +-w/2 edges (outside: the inequalities are strict) at headings 0,
    +-pi/2 and pi."""
    import torch
    from modest_amd import ops
    rng = np.random.default_rng(17)
    for n_pts, n_boxes in ((6000, 4097), (3000, 9000), (50000, 96)):
        pts = np.c_[rng.uniform(-30, 30, n_pts), rng.normal(1.0, 0.5, n_pts), rng.uniform(0, 60, n_pts)]
        boxes = np.c_[rng.uniform(-35, 35, n_boxes), rng.uniform(-5, 65, n_boxes), rng.uniform(0.5, 6, n_boxes),
                      rng.uniform(0.5, 3, n_boxes), rng.uniform(-np.pi, np.pi, n_boxes)]
        boxes[::7, 0] += 200.0   # nothing there: -inf
        got = ops.lowest_point(torch.from_numpy(pts).to(gpu), _boxes6(boxes))
        ref = _lowest_ref(pts, boxes)
        assert np.array_equal(got, ref), (n_pts, n_boxes, np.flatnonzero(got != ref)[:5])
        assert np.isinf(ref).sum() >= n_boxes // 7 and np.isfinite(ref).sum() >= n_boxes // 2
        if n_boxes > 4096:
            assert np.isfinite(ref[4096:]).sum() > 0
        else:   # which slice (point index mod 8 * 1024) holds each box's maximum
            arg = [np.flatnonzero(pts[:, 1] == r)[0] for r in ref if np.isfinite(r)]
            assert len({(i // 1024) % 8 for i in arg}) == 8
    # edges: for every heading a box with points on the midpoints of its four edges (high: outside, they would win) and
    # lower points inside; dyadic centres and extents, so that the rotated coordinates of the edge points are exact
    heads = (0.0, np.pi / 2, -np.pi / 2, np.pi)
    pts, boxes, want = [], [], []
    for h, (cx, cz) in zip(heads, ((2.5, 10.25), (-6.0, 20.5), (8.75, 31.0), (-12.5, 44.0))):
        l, w = 4.5, 1.75
        c, s = np.cos(h), np.sin(h)
        for u, v in ((l / 2, 0.0), (-l / 2, 0.0), (0.0, w / 2), (0.0, -w / 2)):
            # box frame (u, v) -> scan offset (dx, dz) of an axis point: exact when one of them is zero
            dx, dz = (u, v) if h == 0.0 else ((-u, -v) if h == np.pi else ((v, -u) if h > 0 else (-v, u)))
            pts.append([cx + dx, 9.0, cz + dz])
        inner = rng.uniform(-0.45, 0.45, (40, 2)) * [l, w]
        ys = rng.normal(1.0, 0.3, 40)
        for (u, v), y in zip(inner, ys):
            pts.append([cx + u * c + v * s, y, cz - u * s + v * c])
        boxes.append([cx, cz, l, w, h])
        want.append(ys.max())
    pts, boxes = np.array(pts, dtype=np.float64), np.array(boxes)
    got = ops.lowest_point(torch.from_numpy(pts).to(gpu), _boxes6(boxes))
    assert np.array_equal(got, _lowest_ref(pts, boxes))
    assert np.array_equal(got, np.array(want)), (got, want)   # no edge point (y = 9) counted


# --------------------------------------------------------------------------- 4. PP block of 64 scans
@pytest.mark.parametrize("num_cus", [None, "8", "15"])
def test_pp_block_of_64_scans(gpu, monkeypatch, num_cus):
    """A PP block of 64 scans (the most modest_pp_score_block takes) kept whole, at the device's CU count and with
    MODEST_NUM_CUS = 8 and 15 (a fresh context: G = 64 join rows of at least two workgroups, NW = 128 >
    4 * num_cus -- b4_deal's table is sized from NW): equal to the per-scan chain; the first and last scans to the oracle."""
    import torch
    from modest_amd import _lib, synth
    from modest_amd.frame_store import FrameStore
    from oracle import pp_score as opp
    monkeypatch.setenv("MODEST_PP4_CHECK", "1")
    if num_cus is None:
        monkeypatch.delenv("MODEST_NUM_CUS", raising=False)
    else:
        monkeypatch.setenv("MODEST_NUM_CUS", num_cus)
    S = 64
    sh = synth.make_shard(S, n_live=1500, n_trav=2, n_frames=40, n_per_frame=1200, seed=47, frame_gap=0.4)
    store = FrameStore(gpu, 0.3, ctx=_lib.Context(torch.cuda.current_device()))
    items, ids = [], {}
    for t, tr in enumerate(sh.tracks):
        for j, (raw, W) in enumerate(tr):
            ids[(t, j)] = len(ids)
            items.append((ids[(t, j)], torch.from_numpy(raw).to(gpu), W))
    lives = []
    for sc in sh.scans:
        lives.append(100000 + sc.index)
        items.append((lives[-1], torch.from_numpy(sc.live_raw).to(gpu), sc.live_W))
    store.insert_many(items)
    descs = [store.describe(lives[i], sc.live_rel, [ids[h] for h in sc.hist], [t for t, _ in sc.hist], sc.rels, sh.nusc)
             for i, sc in enumerate(sh.scans)]
    ref = store.pp_score_batch(lives, descs, 2, return_counts=True, block=False)[1]
    Hb, cb = store.pp_score_batch(lives, descs, 2, return_counts=True, block=True)
    assert getattr(store, "block_calls", 0) == 1   # one block of all 64 scans
    for i in range(S):
        assert torch.equal(cb[i], ref[i]), (num_cus, i)
    for i in (0, S - 1):
        lv, hist = sh.stacked(i)
        Href, cref = opp.pp_score(lv, hist, 0.3, workers=min(16, os.cpu_count() or 1))
        assert np.array_equal(cb[i].cpu().numpy().astype(np.int64), cref), (num_cus, i)
        assert np.max(np.abs(Hb[i].cpu().numpy().astype(np.float64) - Href)) <= 1e-6
    assert int(sum(int(c.sum()) for c in cb)) > 0


# --------------------------------------------------------------------------- 5. NMS and 3-D IoU
def test_nms_past_the_first_chunk_of_the_host_walk(gpu):
    """nms_gpu / nms_normal_gpu on 16 500 boxes: cb = 258 words per row, 16 256 rows per 32 MB chunk of the host walk -- the
    walk crosses into a second chunk, where boxes are kept and suppressed (scores fall with x: the last boxes in score order
    lie side by side).  Keep equals order[oracle nms] in score order."""
    import torch
    from modest_amd.utils.iou3d_nms import iou3d_nms_utils as iu
    from oracle import labels as ol
    n = 16500
    rng = np.random.default_rng(12)
    x = rng.uniform(-100, 100, n)
    big = np.c_[x, rng.uniform(-100, 100, n), rng.uniform(-1, 1, n), rng.uniform(1, 5, (n, 2)), rng.uniform(1, 2, n),
                rng.uniform(-3.2, 3.2, n)].astype(np.float32)
    scores = ((x + 100) / 200 + rng.normal(0, 0.02, n)).astype(np.float32)
    order = np.argsort(-scores, kind="stable")
    rows_per_chunk = (32 << 20) // (((n + 63) // 64) * 8)
    assert rows_per_chunk == 16256 < n
    sc = torch.from_numpy(scores).to(gpu)
    for rotated, fn in ((True, iu.nms_gpu), (False, iu.nms_normal_gpu)):
        pos = ol.nms(big[order], 0.1, rotated=rotated)
        late = pos[pos >= rows_per_chunk]
        assert len(late) >= 20 and n - rows_per_chunk - len(late) >= 20, (rotated, len(late))   # kept and suppressed there
        keep, _ = fn(torch.from_numpy(big).to(gpu), sc, 0.1)
        assert np.array_equal(keep.cpu().numpy(), order[pos]), rotated


def test_boxes_iou3d_off_the_diagonal(gpu):
    """boxes_iou3d_gpu between two different box sets against the float64 statement of iou3d_nms_utils.py:54-87: BEV
    overlap (the oracle's C restatement) x height overlap / (volume a + volume b - intersection)."""
    import torch
    from modest_amd.utils.iou3d_nms import iou3d_nms_utils as iu
    from oracle import labels as ol
    rng = np.random.default_rng(13)

    def boxes(k):
        return np.c_[rng.uniform(-6, 6, (k, 2)), rng.uniform(-1, 1, k), rng.uniform(1, 5, (k, 2)), rng.uniform(0.5, 2.5, k),
                     rng.uniform(-3.2, 3.2, k)].astype(np.float32)

    a, b = boxes(70), boxes(45)
    b[:5] = a[:5]   # identical pairs
    got = iu.boxes_iou3d_gpu(torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu)).cpu().numpy()
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    top = np.minimum((a64[:, 2] + a64[:, 5] / 2)[:, None], (b64[:, 2] + b64[:, 5] / 2)[None, :])
    bot = np.maximum((a64[:, 2] - a64[:, 5] / 2)[:, None], (b64[:, 2] - b64[:, 5] / 2)[None, :])
    inter = ol.boxes_iou_bev(a, b, overlap_only=True).astype(np.float64) * np.clip(top - bot, 0, None)
    vol = a64[:, 3:6].prod(1)[:, None] + b64[:, 3:6].prod(1)[None, :]
    want = inter / np.maximum(vol - inter, 1e-6)
    assert got.shape == want.shape == (70, 45)
    assert np.max(np.abs(got - want)) <= 2e-5
    assert (want > 0.01).sum() >= 200 and np.all(np.abs(np.diag(got[:5, :5]) - 1) < 1e-4)
