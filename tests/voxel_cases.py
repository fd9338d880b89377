"""Edge families of the point-to-voxel grouping, shared by tests/test_voxelize_cpu.py (host path, cloud by cloud) and
tests/test_gpu_voxelize.py (device path, the clouds of a case as one batch).  Not a test module.

A case is a dict: name, clouds (list of (N, C) float32), voxel_size, point_cloud_range, P (max_num_points), M (max_voxels),
and `present`: a function of the case that asserts FROM THE INPUTS that the edge the case is named after is there.
The smallest shapes at which the kernels can still go wrong: the device sort works in tiles of 2048 rows, sub-blocks of
64 and scan blocks of 1024, a voxel row is filled by 64 lanes.
"""
import functools

import numpy as np

import voxel_seq as seq

PP_RANGE = [0, -39.68, -3, 89.6, 39.68, 1]       # tools/cfgs/lyft_models/pointpillar_dynamic_obj.yaml
PP_VOXEL = [0.16, 0.16, 4]
PP_GRID = [560, 496, 1]
KITTI_RANGE = [0, -40, -3, 70.4, 40, 1]
FINE_VOXEL = [0.05, 0.05, 0.1]
FINE_GRID = [1408, 1600, 40]
F = np.float32


def centre(cx, cy, width=4, rng=None, jitter=0.0):
    """points inside PointPillars cells (cx, cy): cell centres, optionally jittered by +-jitter cells"""
    cx, cy = np.asarray(cx, dtype=np.float64), np.asarray(cy, dtype=np.float64)
    out = np.zeros((len(cx), width), dtype=F)
    jx = jy = 0.0
    if rng is not None and jitter:
        jx, jy = rng.uniform(-jitter, jitter, len(cx)), rng.uniform(-jitter, jitter, len(cx))
    out[:, 0] = ((cx + 0.5 + jx) * 0.16).astype(F)
    out[:, 1] = (-39.68 + (cy + 0.5 + jy) * 0.16).astype(F)
    out[:, 2] = F(-1.0)
    if rng is not None:
        out[:, 3:] = rng.uniform(0, 1, (len(cx), width - 3)).astype(F)
    else:
        out[:, 3:] = (np.arange(len(cx), dtype=F)[:, None] + 1) / 64
    return out


def scatter_cloud(seed, n, width=4, spread=1.1):
    """uniform over a box a little larger than the range (some points outside), plus a dense patch (shared cells)"""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, width), dtype=F)
    k = n // 2
    out[:k, 0] = rng.uniform(-0.05 * 89.6, spread * 89.6, k)
    out[:k, 1] = rng.uniform(-spread * 39.68, spread * 39.68, k)
    out[:k, 2] = rng.uniform(-3.5, 1.5, k)
    out[k:, 0] = rng.uniform(10.0, 12.0, n - k)
    out[k:, 1] = rng.uniform(-1.0, 1.0, n - k)
    out[k:, 2] = rng.uniform(-2.0, 0.0, n - k)
    out[:, 3:] = rng.uniform(0, 1, (n, width - 3))
    return out[rng.permutation(n)]


def case(name, clouds, present, P=32, M=16000, voxel_size=PP_VOXEL, point_cloud_range=PP_RANGE):
    clouds = [np.ascontiguousarray(c, dtype=F) for c in clouds]
    assert len({c.shape[1] for c in clouds}) == 1
    return dict(name=name, clouds=clouds, present=present, P=P, M=M, voxel_size=voxel_size,
                point_cloud_range=point_cloud_range)


def cell_ids(c, cloud):
    """per point: the cell number, -1 for a dropped point"""
    cf, kept = seq.cells(cloud, c["point_cloud_range"], c["voxel_size"])
    g = seq.grid_size(c["point_cloud_range"], c["voxel_size"])
    ci = np.where(kept[:, None], cf, 0).astype(np.int64)
    return np.where(kept, (ci[:, 2] * g[1] + ci[:, 1]) * g[0] + ci[:, 0], -1)


def occupancy(c, cloud):
    ids = cell_ids(c, cloud)
    return np.unique(ids[ids >= 0], return_counts=True)[1]


# ------------------------------------------------------------------------------------------------ the families
def sizes():
    out = []
    for n in (0, 1, 63, 64, 65, 5003):
        def present(c, n=n):
            assert len(c["clouds"][0]) == n and (n % 64 or n in (0, 64))
            if n > 1000:
                ids = cell_ids(c, c["clouds"][0])
                assert (ids < 0).any() and occupancy(c, c["clouds"][0]).max() > 1 and n > 2 * 2048 and n % 64
        out.append(case(f"n{n}", [scatter_cloud(100 + n, n)], present))
    return out


def batches():
    a, b, d = scatter_cloud(1, 700), scatter_cloud(2, 2300), scatter_cloud(3, 129)
    empty = np.zeros((0, 4), dtype=F)

    def has(k, empty_at=None):
        def present(c):
            assert len(c["clouds"]) == k
            if empty_at is not None:
                assert len(c["clouds"][empty_at]) == 0 and all(len(x) for i, x in enumerate(c["clouds"]) if i != empty_at)
        return present
    return [case("batch1", [a], has(1)), case("batch2", [a, b], has(2)), case("batch3", [a, b, d], has(3)),
            case("batch_empty_middle", [a, empty, b], has(3, 1)), case("batch_empty_last", [a, b, empty], has(3, 2)),
            # M applies per cloud: the second cloud alone has more cells than M, the first fewer
            case("batch_cap_per_cloud", [d, b, a], has(3), M=300)]


def occupancies():
    rng = np.random.default_rng(7)
    P = 5
    small = centre([3] * 3 + [9] * 5 + [20] * 6, [4] * 3 + [8] * 5 + [30] * 6, rng=rng, jitter=0.4)
    n = 7001
    big = scatter_cloud(8, n)
    at = np.unique(np.linspace(0, n - 1, 3000).astype(np.int64))   # one cell's points over the whole index range
    big[at] = centre([100] * len(at), [200] * len(at), rng=rng, jitter=0.45)

    def present_small(c):
        assert sorted(occupancy(c, c["clouds"][0]).tolist()) == [3, 5, 6] and c["P"] == 5

    def present_big(c):
        ids = cell_ids(c, c["clouds"][1])
        where = np.nonzero(ids == 200 * 560 + 100)[0]
        assert len(where) >= 2990 and where[0] == 0 and where[-1] == n - 1 and len(where) > 100 * c["P"]
        assert np.all(np.diff(where) <= 3)   # every 64-row sub-block, 1024-row block and 2048-row tile holds some
    return [case("occupancy_small", [small[np.random.default_rng(1).permutation(len(small))]], present_small, P=P),
            case("occupancy_one_cell_3000", [small, big], present_big, P=P)]


def slot_counts():
    rng = np.random.default_rng(11)
    cloud = np.concatenate([scatter_cloud(11, 1300), centre([50] * 120 + [51] * 80, [60] * 200, rng=rng, jitter=0.45)])
    cloud = cloud[rng.permutation(len(cloud))]

    def present(c):
        occ = occupancy(c, c["clouds"][0])
        assert (occ > c["P"]).any() and (occ <= c["P"]).any()
    return [case(f"P{p}", [cloud], present, P=p) for p in (1, 2, 5, 32)] + \
        [case("P70", [centre([5] * 150 + [6] * 70 + [7] * 3, [5] * 223)], lambda c: None, P=70)]   # a voxel row wider than a wavefront


def voxel_caps():
    M, out = 7, []
    for k in (M - 1, M, M + 1):
        cx = np.repeat(np.arange(k) * 3 + 1, 2)

        def present(c, k=k):
            assert len(occupancy(c, c["clouds"][0])) == k and c["M"] == M
        out.append(case(f"cells{k}_cap{M}", [centre(cx, cx % 5)[np.random.default_rng(k).permutation(2 * k)]], present, M=M))
    # 7 cells open, then new cells (rejected) interleaved with returns to open cells (must enter), in two clouds
    order = [0, 1, 2, 3, 4, 5, 6, 7, 2, 8, 0, 7, 6, 9, 1, 1, 8, 3]
    cloud = centre(np.asarray(order) * 2, np.asarray(order) + 10)

    def present_returns(c):
        for cl in c["clouds"]:
            ids = cell_ids(c, cl)
            first = [i for i in range(len(ids)) if ids[i] not in ids[:i]]
            assert len(first) > M
            full_at = first[M - 1]
            opened = set(ids[first[:M]].tolist())
            after = ids[full_at + 1:]
            assert any(v in opened for v in after) and any(v not in opened for v in after)
            late = [i for i in range(first[M], len(ids)) if ids[i] in opened]
            assert late, "a point returns to an open cell after the first rejected one"
    out.append(case("cap_returns", [cloud, cloud[::-1].copy()], present_returns, M=M, P=3))
    return out


@functools.lru_cache(maxsize=None)
def reciprocal_differs(count=6):
    """float32 x in the range on which floorf(d / vs) and floorf(d * (1 / vs)) differ (about 6 per million)"""
    rng, found = np.random.default_rng(2024), []
    vs, inv = F(0.16), F(1) / F(0.16)
    for _ in range(40):
        x = rng.uniform(0, 89.6, 1 << 20).astype(F)
        d = x - F(0)
        bad = np.floor(d / vs) != np.floor(d * inv)
        found.extend(x[bad].tolist())
        if len(found) >= count:
            break
    return np.asarray(found[:count], dtype=F)


def arithmetic():
    lo, hi = np.asarray(PP_RANGE[:3], dtype=F), np.asarray(PP_RANGE[3:], dtype=F)
    inside = np.asarray([10.0, 1.0, -1.0], dtype=F)

    def rows(vals, axis):
        out = np.tile(np.concatenate([inside, [F(0.5)]]).astype(F), (len(vals), 1))
        out[:, axis] = vals
        return out
    below = np.nextafter(hi, F(-np.inf)).astype(F)
    corners = np.concatenate([rows([lo[j], hi[j], below[j]], j) for j in range(3)])

    def present_corners(c):
        cl = c["clouds"][0]
        cf, kept = seq.cells(cl, PP_RANGE, PP_VOXEL)
        assert cl[0, 0] == lo[0] and cl[3, 1] == lo[1] and cl[6, 2] == lo[2] and kept[[0, 3, 6]].all()
        assert cl[1, 0] == hi[0] and cl[4, 1] == hi[1] and cl[7, 2] == hi[2] and not kept[[1, 4, 7]].any()
        # the largest float32 below hi: inside the range on every axis, but on y it floors to 496 == grid_y
        assert cl[5, 1] < hi[1] and cf[5, 1] == 496 and not kept[5]
        assert cl[2, 0] < hi[0] and cf[2, 0] == 559 and kept[2]

    kx = (np.arange(561, dtype=F) * F(0.16)).astype(F)
    ky = (lo[1] + np.arange(497, dtype=F) * F(0.16)).astype(F)
    bounds = np.concatenate([rows(kx, 0), rows(ky, 1)])

    def present_bounds(c):
        cf, _ = seq.cells(c["clouds"][0][:561], PP_RANGE, PP_VOXEL)
        assert int((cf[:560, 0] != np.arange(560)).sum()) == 43

    recip = rows(reciprocal_differs(), 0)

    def present_recip(c):
        d = c["clouds"][0][:, 0] - F(0)
        a, b = np.floor(d / F(0.16)), np.floor(d * (F(1) / F(0.16)))
        assert len(d) >= 4 and (a != b).all()

    specials = np.concatenate([rows([F(-0.0), F(np.nan), F(np.inf), F(-np.inf)], j) for j in range(3)] + [rows([10.0], 0)])

    def present_specials(c):
        cl = c["clouds"][0]
        cf, kept = seq.cells(cl, PP_RANGE, PP_VOXEL)
        for j in range(3):
            r = cl[4 * j:4 * j + 4, j]
            assert r[0] == 0 and np.signbit(r[0]) and np.isnan(r[1]) and r[2] == np.inf and r[3] == -np.inf
            assert not kept[4 * j + 1:4 * j + 4].any()
        assert np.signbit(cf[0, 0]) and cf[0, 0] == 0 and kept[0]   # -0.0 on x (lo_x = 0) is cell 0 through a float -0.0
        assert kept[4] and kept[8]   # -0.0 is an ordinary inside value on y and z

    nanfeat = centre([1, 2, 1], [1, 2, 1], width=5)
    nanfeat.view(np.uint32)[0, 3] = 0x7FC12345   # payloads survive
    nanfeat.view(np.uint32)[2, 4] = 0xFFA00001   # a signalling NaN with the sign set

    def present_nanfeat(c):
        cl = c["clouds"][0]
        assert np.isnan(cl[0, 3]) and np.isnan(cl[2, 4]) and seq.cells(cl, PP_RANGE, PP_VOXEL)[1].all()
    return [case("corners", [corners], present_corners), case("cell_boundaries", [bounds], present_bounds),
            case("reciprocal_differs", [recip], present_recip), case("specials", [specials], present_specials),
            case("nan_feature", [nanfeat], present_nanfeat),
            case("arithmetic_batched", [corners, specials, recip], lambda c: None)]


def features():
    def width_is(w):
        def present(c):
            assert all(x.shape[1] == w for x in c["clouds"])
        return present
    return [case(f"C{w}", [scatter_cloud(20 + w, 333, width=w), scatter_cloud(30 + w, 65, width=w)], width_is(w), P=5)
            for w in (3, 4, 5)]


def duplicates():
    base = scatter_cloud(40, 50)
    cloud = np.concatenate([base, base[:20], base, base[::-1]])

    def present(c):
        assert len(np.unique(c["clouds"][0], axis=0)) < len(c["clouds"][0]) / 2
    return [case("duplicates", [cloud], present, P=3)]


def orders():
    cloud = scatter_cloud(50, 2500)
    probe = dict(point_cloud_range=PP_RANGE, voxel_size=PP_VOXEL)
    ids = cell_ids(probe, cloud)
    asc = cloud[np.argsort(ids, kind="stable")]

    def present(c):
        a, d, s = (cell_ids(c, x) for x in c["clouds"])
        assert np.all(np.diff(a) >= 0) and np.all(np.diff(d) <= 0) and (np.diff(s) < 0).any() and (np.diff(s) > 0).any()
    return [case("orders", [asc, asc[::-1].copy(), cloud], present, P=4, M=900)]


def fine_grid():
    rng = np.random.default_rng(60)
    n = 3001
    cloud = np.zeros((n, 4), dtype=F)
    cloud[:, 0] = rng.uniform(-1, 72, n)
    cloud[:, 1] = rng.uniform(-41, 41, n)
    cloud[:, 2] = rng.uniform(-3.2, 1.2, n)
    cloud[:, 3] = rng.uniform(0, 1, n)
    cloud[1000:1400, :3] = cloud[1000, :3] + rng.uniform(0, 0.04, (400, 3)).astype(F)   # shared cells, several z

    def present(c):
        assert seq.grid_size(c["point_cloud_range"], c["voxel_size"]).tolist() == FINE_GRID
        cf, kept = seq.cells(c["clouds"][0], c["point_cloud_range"], c["voxel_size"])
        assert len(np.unique(cf[kept, 2])) > 20 and occupancy(c, c["clouds"][0]).max() > 5
    return [case("fine_grid", [cloud, cloud[::3].copy()], present, P=5, M=2500, voxel_size=FINE_VOXEL,
                 point_cloud_range=KITTI_RANGE)]


@functools.lru_cache(maxsize=None)
def all_cases():
    out = []
    for fam in (sizes, batches, occupancies, slot_counts, voxel_caps, arithmetic, features, duplicates, orders, fine_grid):
        out.extend(fam())
    assert len({c["name"] for c in out}) == len(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected(name):
    """per-cloud voxel_seq results of a case, computed once and shared"""
    c = next(x for x in all_cases() if x["name"] == name)
    return tuple(seq.voxelize(cl, c["voxel_size"], c["point_cloud_range"], c["P"], c["M"]) for cl in c["clouds"])
