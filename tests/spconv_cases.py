"""Edge families of the sparse 3-D convolutions, shared by tests/test_spconv_cpu.py (the restatement against a dense
oracle) and tests/test_gpu_spconv.py (the device against the restatement).  Not a test module.

A case is a dict: name, indices (N, 4) int32 [b, z, y, x], batch_size, shape [D, H, W], kernel, stride, padding, subm,
cin, cout, bias (bool), seed, dense (small enough to densify), and `present`: a function of the case that asserts FROM
THE INPUTS that the edge the case is named after is there.  The smallest shapes at which the kernels can still go wrong:
a convolution workgroup owns 64 output rows, the sort works in tiles of 2048 keys and sub-blocks of 64, the scans in
blocks of 1024, the weight gradient in segments of 1024 rows and chunks of 32 -- and, past 32 768 rows, in 32 longer
segments, which only that many rows can reach (the segments family).
"""
import functools

import numpy as np

import spconv_seq as seq

F = np.float32
GEOMETRIES = {   # the four layer geometries of VoxelBackBone8x: kernel, stride, padding, subm
    "subm": (3, 1, 0, True),
    "s2p1": (3, 2, 1, False),
    "s2p011": (3, 2, (0, 1, 1), False),
    "k311": ((3, 1, 1), (2, 1, 1), 0, False),
}


def random_sites(seed, n, batch_size, shape, clouds=None):
    """n unique sites, uniformly over the clouds in `clouds` (default: all), in random row order"""
    rng = np.random.default_rng(seed)
    clouds = list(range(batch_size)) if clouds is None else clouds
    cells = int(np.prod(shape))
    flat = rng.choice(cells * len(clouds), size=n, replace=False) if n else np.zeros(0, dtype=np.int64)
    b = np.asarray(clouds, dtype=np.int64)[flat // cells] if n else flat
    c = flat % cells
    return np.stack([b, c // (shape[1] * shape[2]), (c // shape[2]) % shape[1], c % shape[2]], axis=1).astype(np.int32)


def case(name, indices, batch_size, shape, geometry, present, cin=4, cout=16, bias=True, seed=0, dense=True):
    kernel, stride, padding, subm = GEOMETRIES[geometry]
    return dict(name=name, indices=np.ascontiguousarray(indices, dtype=np.int32).reshape(-1, 4), batch_size=batch_size,
                shape=list(shape), kernel=kernel, stride=stride, padding=padding, subm=subm, geometry=geometry, cin=cin,
                cout=cout, bias=bias, seed=seed, dense=dense, present=present)


def tensors(c):
    """features (N, Cin), weight (K, Cin, Cout), bias (Cout,) | None, dy (N_out, Cout): float32, fixed by the case"""
    rng = np.random.default_rng(1000 + c["seed"])
    K = int(np.prod(seq.triple(c["kernel"])))
    n_out = len(expected(c["name"])[0])
    x = rng.standard_normal((len(c["indices"]), c["cin"])).astype(F)
    w = rng.uniform(-0.5, 0.5, (K, c["cin"], c["cout"])).astype(F)
    b = rng.uniform(-1, 1, (c["cout"],)).astype(F) if c["bias"] else None
    dy = rng.standard_normal((n_out, c["cout"])).astype(F)
    if c.get("special"):
        x[0, :] = 0
        x[1, 0] = F(-0.0)
        x[2, :] = F(-0.0)
        w[0, 0, 0] = F(-0.0)
        dy[0, :] = F(-0.0)
    return x, w, b, dy


def site_set(c):
    return set(map(tuple, c["indices"].tolist()))


# ------------------------------------------------------------------------------------------------ the families
def sizes():
    out = []
    for n in (0, 1, 63, 64, 65, 3001):
        for geo in ("subm", "s2p1"):
            def present(c, n=n):
                assert len(c["indices"]) == n and (n % 64 or n in (0, 64))
                if n > 3000:
                    assert n > 2048 and n * 27 > 2048 * 8   # several sort tiles, scan blocks and gradient segments
            out.append(case(f"n{n}_{geo}", random_sites(10 + n, n, 1, [11, 30, 34]), 1, [11, 30, 34], geo, present, seed=n))
    return out


def batches():
    shape = [8, 10, 12]
    out = []

    def has(k, empty_at=()):
        def present(c):
            per = np.bincount(c["indices"][:, 0], minlength=k)
            assert c["batch_size"] == k and len(per) == k
            assert all((per[b] == 0) == (b in empty_at) for b in range(k))
        return present
    for geo in ("subm", "s2p1"):
        out += [case(f"batch1_{geo}", random_sites(1, 150, 1, shape), 1, shape, geo, has(1), seed=1),
                case(f"batch2_{geo}", random_sites(2, 300, 2, shape), 2, shape, geo, has(2), seed=2),
                case(f"batch3_{geo}", random_sites(3, 450, 3, shape), 3, shape, geo, has(3), seed=3),
                case(f"batch_empty_middle_{geo}", random_sites(4, 300, 3, shape, [0, 2]), 3, shape, geo, has(3, (1,)), seed=4),
                case(f"batch_empty_last_{geo}", random_sites(5, 300, 3, shape, [0, 1]), 3, shape, geo, has(3, (2,)), seed=5)]
        one = random_sites(6, 120, 1, shape)
        two = np.concatenate([one, one[::-1] + np.asarray([[1, 0, 0, 0]], dtype=np.int32)])

        def present_twins(c):
            a, b = (set(map(tuple, c["indices"][c["indices"][:, 0] == k][:, 1:].tolist())) for k in (0, 1))
            assert a == b and len(a) == 120
        out.append(case(f"same_sites_two_clouds_{geo}", two, 2, shape, geo, present_twins, seed=6))
    return out


def borders():
    """sites on index 0 and on the last index of every axis, and an occupied site exactly where a key that wrapped
    across a border would land: the end of a row and the start of the next, of a slab, of a cloud"""
    D, H, W = shape = [6, 7, 9]
    rows = []
    for b in (0, 1):
        rows += [(b, 0, 0, 0), (b, D - 1, H - 1, W - 1),            # the first and the last cell of the cloud
                 (b, 2, 3, W - 1), (b, 2, 4, 0),                       # end of a row, start of the next
                 (b, 2, H - 1, W - 1), (b, 3, 0, 0),                   # end of a slab, start of the next
                 (b, 0, 3, 4), (b, D - 1, 3, 4), (b, 3, 0, 4), (b, 3, H - 1, 4), (b, 3, 3, 0), (b, 3, 3, W - 1),
                 (b, 4, 5, W - 2), (b, 4, 5, W - 1), (b, 4, 6, 0), (b, 4, 6, 1)]
    rows = np.asarray(sorted(set(rows)), dtype=np.int32)
    rows = rows[np.random.default_rng(3).permutation(len(rows))]

    def present(c):
        s = site_set(c)
        D, H, W = c["shape"]
        assert {(0, D - 1, H - 1, W - 1), (1, 0, 0, 0)} <= s          # one key apart, in different clouds
        assert {(0, 2, 3, W - 1), (0, 2, 4, 0)} <= s and {(0, 2, H - 1, W - 1), (0, 3, 0, 0)} <= s
        for j, ext in enumerate(c["shape"]):
            assert {r[1 + j] for r in s} >= {0, ext - 1}
        # linear keys of the pairs differ by one: a lookup that formed the key first would find them as x-neighbours
        key = lambda r: ((r[0] * D + r[1]) * H + r[2]) * W + r[3]
        assert key((0, 2, 4, 0)) - key((0, 2, 3, W - 1)) == 1 and key((1, 0, 0, 0)) - key((0, D - 1, H - 1, W - 1)) == 1
    return [case(f"borders_{geo}", rows, 2, shape, geo, present, seed=20 + i, cin=3, cout=5)
            for i, geo in enumerate(GEOMETRIES)]


def occupancy():
    shape = [7, 8, 9]
    z, y, x = np.meshgrid(np.arange(1, 6), np.arange(2, 7), np.arange(3, 8), indexing="ij")
    block = np.stack([np.zeros(125, dtype=np.int64), z.ravel(), y.ravel(), x.ravel()], axis=1)
    block = block[np.random.default_rng(5).permutation(125)]

    def present_block(c):
        nbr = expected(c["name"])[2]
        assert len(c["indices"]) == 125 and ((nbr >= 0).sum(0) == nbr.shape[0]).any()   # a row with every offset present
        assert all((nbr[k] >= 0).any() for k in range(nbr.shape[0]))
    g = np.arange(0, 9, 3)
    iso = np.asarray([(b, zz, yy, xx) for b in (0, 1) for zz in g[:2] for yy in g for xx in g], dtype=np.int32)

    def present_isolated(c):
        nbr = expected(c["name"])[2]
        assert ((nbr >= 0).sum(0) == 1).all() and (nbr[13] == np.arange(len(c["indices"]))).all()
    return [case("full_block_subm", block, 1, shape, "subm", present_block, seed=30),
            case("full_block_s2p1", block, 1, shape, "s2p1", lambda c: None, seed=31),
            case("isolated_subm", iso, 2, [7, 9, 9], "subm", present_isolated, seed=32)]


def backbone_layers():
    """the four layer geometries on the extents D = 41 runs through: 41 -> 21 -> 11 -> 5 -> 2 (odd and even extents)"""
    steps = [("vb_conv2", [41, 16, 18], "s2p1", [21, 8, 9]), ("vb_conv3", [21, 8, 9], "s2p1", [11, 4, 5]),
             ("vb_conv4", [11, 4, 5], "s2p011", [5, 2, 3]), ("vb_conv_out", [5, 2, 3], "k311", [2, 2, 3]),
             ("vb_subm1", [41, 16, 18], "subm", [41, 16, 18])]
    out = []
    for i, (name, shape, geo, want) in enumerate(steps):
        def present(c, want=want):
            assert seq.out_shape(c["shape"], c["kernel"], c["stride"], c["padding"], c["subm"]) == want
            assert any(e % 2 for e in c["shape"]) and any(e % 2 == 0 for e in c["shape"])
        n = min(400, int(np.prod(shape)) * 2 // 3)
        out.append(case(name, random_sites(40 + i, n, 2, shape), 2, shape, geo, present, seed=40 + i))
    return out


def huge():
    """batch_size * D * H * W > 2^32 with a handful of sites: keys must be 64 bits wide and no table spans the grid"""
    D, H, W = shape = [1000, 2000, 2200]
    rows = [(0, 0, 0, 0), (0, 0, 0, 1), (0, D - 1, H - 1, W - 1), (1, 0, 0, 0), (1, D - 1, H - 1, W - 1), (1, D - 1, H - 1, W - 2),
            (0, 500, 1000, W - 1), (0, 500, 1001, 0), (1, 999, 1999, 0), (1, 700, 1500, 1100), (1, 701, 1501, 1101),
            (1, 700, 1500, 1101), (0, 976, 257, 1897), (1, 488, 976, 1074)]

    def present(c):
        D, H, W = c["shape"]
        assert c["batch_size"] * D * H * W > 2 ** 32 and D * H * W > 2 ** 32
        key = lambda r: ((r[0] * D + r[1]) * H + r[2]) * W + r[3]
        assert max(key(r) for r in site_set(c)) > 2 ** 32
        # two sites whose keys agree in their low 32 bits: a truncated key would make them one
        assert key((0, 976, 257, 1897)) - key((0, 0, 0, 1)) == 2 ** 32 and {(0, 976, 257, 1897), (0, 0, 0, 1)} <= site_set(c)
    return [case(f"huge_{geo}", np.asarray(rows, dtype=np.int32), 2, shape, geo, present, seed=50 + i, dense=False)
            for i, geo in enumerate(("subm", "s2p1"))]


def passes(sentinel):
    """8-bit passes of the radix sort over the bits of a sentinel key (sort64_bit_length, 8 bits per pass)"""
    return -(-int(sentinel).bit_length() // 8)


def huge_many():
    """the shape of huge() with 3 001 sites: keys past 32 bits in sorts that cross tiles (2 048 keys) and sub-blocks (64).
    A 5-pass sort with the payload is the input sort of every case; a 5-pass keys-only sort is the candidate sort of a
    strided case whose OUTPUT grid has more than 2^32 cells, which at stride 2 takes B = 8."""
    D, H, W = shape = [1000, 2000, 2200]

    def sites(seed, batch_size):
        """3 001 unique sites drawn coordinate by coordinate (a choice over the 8.8e9 cells would permute them all): 26
        clusters of 12 in a 3 x 3 x 3 neighbourhood, one of them past key 2^32 in cloud 0, the rest uniform"""
        rng = np.random.default_rng(seed)
        centres = np.stack([rng.integers(0, batch_size, 26), rng.integers(1, D - 1, 26), rng.integers(1, H - 1, 26),
                            rng.integers(1, W - 1, 26)], axis=1)
        centres[0] = (0, D - 3, H // 2, W // 2)
        centres[1] = (batch_size - 1, D - 5, H // 3, W // 3)
        planted = centres[:, None, :].repeat(12, axis=1)
        planted[:, :, 1:] += rng.integers(-1, 2, (26, 12, 3))
        planted = planted.reshape(-1, 4)
        rows = np.concatenate([planted, np.stack([rng.integers(0, batch_size, 4000), rng.integers(0, D, 4000),
                                                  rng.integers(0, H, 4000), rng.integers(0, W, 4000)], axis=1)])
        _, first = np.unique(rows, axis=0, return_index=True)
        rows = rows[np.sort(first)][:3001]
        return rows[rng.permutation(len(rows))].astype(np.int32)

    def present(c):
        D, H, W = c["shape"]
        B, n, K = c["batch_size"], len(c["indices"]), int(np.prod(seq.triple(c["kernel"])))
        assert n == 3001 and n > 2048 and n * K > 2048 * 8 and len(site_set(c)) == n
        key = ((c["indices"][:, 0].astype(np.int64) * D + c["indices"][:, 1]) * H + c["indices"][:, 2]) * W + c["indices"][:, 3]
        for b in (0, B - 1):   # keys above 2^32 in the first and in the last cloud
            assert (key[c["indices"][:, 0] == b] > 2 ** 32).any()
        # the input sentinel B D H W: 8.8e9 at B = 2 is 34 bits, 3.52e10 at B = 8 is 36 bits; ceil(34 / 8) = ceil(36 / 8) = 5
        cells_in = B * D * H * W
        assert cells_in.bit_length() == {2: 34, 8: 36}[B] and passes(cells_in) == 5
        out_idx, oshape, nbr, nbr_t = expected(c["name"])
        cells_out = B * int(np.prod(oshape))
        if c["subm"]:
            assert cells_out == cells_in
        elif B == 2:
            # the output sentinel 2 * 500 * 1000 * 1100 = 1.1e9 is 31 bits: the keys-only sort of this case has 4 passes
            assert oshape == [500, 1000, 1100] and cells_out.bit_length() == 31 and passes(cells_out) == 4
        else:
            # 8 * 500 * 1000 * 1100 = 4.4e9 is 33 bits, ceil(33 / 8) = 5: a 5-pass keys-only sort of n K = 81 027 keys
            assert oshape == [500, 1000, 1100] and cells_out.bit_length() == 33 and passes(cells_out) == 5
            okey = ((out_idx[:, 0].astype(np.int64) * oshape[0] + out_idx[:, 1]) * oshape[1] + out_idx[:, 2]) * oshape[2] + out_idx[:, 3]
            assert (okey > 2 ** 32).any() and len(out_idx) > 2048
        # the clusters make the maps more than the centre (submanifold) or one input per output (strided)
        assert ((nbr >= 0).sum(0) > 1).sum() > 100
    return [case("huge_many_subm", sites(80, 2), 2, shape, "subm", present, seed=80, dense=False),
            case("huge_many_s2p1", sites(81, 2), 2, shape, "s2p1", present, seed=81, dense=False, bias=False),
            case("huge_many_b8_s2p1", sites(82, 8), 8, shape, "s2p1", present, seed=82, dense=False, cin=3, cout=5)]


def segments():
    """row counts around the weight gradient's segmentation (seq.wgrad_segments): one full segment, the first seam, a
    seg_rows that is no multiple of the 32-row chunk, exactly at the cap of 32 segments and past it, where seg_rows
    exceeds 1024"""
    small, big = [11, 30, 34], [21, 120, 128]

    def has(n_out, segs, seg_rows, at_least=False):
        def present(c):
            out_idx, oshape, nbr, nbr_t = expected(c["name"])
            n = len(out_idx)
            assert n > n_out if at_least else n == n_out
            assert not c["subm"] or n == len(c["indices"])
            s, rows = seq.wgrad_segments(n)
            assert s == segs and (at_least or rows == seg_rows)
            assert s == max(1, min(32, -(-n // 1024))) and rows == -(-n // s) and (s - 1) * rows < n <= s * rows
            if n > 32768:
                assert rows > 1024 and -(-n // 1024) > 32   # the cap binds: the 1024-row rule alone would cut more segments
            if s > 1:   # the first and the last row of every segment contribute at some offset
                for q in range(s):
                    for o in (q * rows, min((q + 1) * rows, n) - 1):
                        assert (nbr[:, o] >= 0).any(), (c["name"], q, o)
                # ... and some seam has rows on both of its sides that contribute at the same offset
                seams = np.arange(1, s) * rows
                assert ((nbr[:, seams - 1] >= 0) & (nbr[:, seams] >= 0)).any()
        return present
    out = []
    for i, (n, segs, rows, shape, cin, cout, bias) in enumerate(((1024, 1, 1024, small, 4, 16, True), (1025, 2, 513, small, 3, 5, False),
                                                                 (2048, 2, 1024, small, 4, 5, True), (32768, 32, 1024, big, 3, 16, False),
                                                                 (32769, 32, 1025, big, 4, 16, True), (33797, 32, 1057, big, 3, 5, True))):
        out.append(case(f"seg{n}_subm", random_sites(90 + i, n, 1, shape), 1, shape, "subm", has(n, segs, rows), cin=cin, cout=cout,
                        bias=bias, seed=90 + i, dense=False))
    assert -(-33797 // 1024) == 34 and 32769 - 31 * 1025 == 994
    out.append(case("seg_many_s2p1", random_sites(97, 30000, 1, big), 1, big, "s2p1", has(32768, 32, None, at_least=True), cin=4, cout=5,
                    bias=False, seed=97, dense=False))
    return out


def channels():
    pairs =[(1, 4), (3, 16), (4, 16), (5, 32), (16, 3), (32, 64), (64, 128), (128, 5), (128, 128), (16, 16), (64, 64), (33, 65)]
    out = []
    for i, (cin, cout) in enumerate(pairs):
        geo = "s2p1" if i % 3 == 1 else "subm"

        def present(c, cin=cin, cout=cout):
            assert (c["cin"], c["cout"]) == (cin, cout) and len(c["indices"]) > 128   # more than one workgroup of rows
        out.append(case(f"c{cin}_{cout}_{geo}", random_sites(60 + i, 200, 2, [6, 10, 12]), 2, [6, 10, 12], geo, present,
                        cin=cin, cout=cout, bias=bool(i % 2), seed=60 + i))
    assert any(c["cin"] % 4 for c in out) and any(c["cout"] % 4 for c in out)
    assert {(4, 16), (64, 128)} <= {(c["cin"], c["cout"]) for c in out}
    assert any(c["bias"] for c in out) and any(not c["bias"] for c in out)
    return out


def values():
    def present(c):
        x, w, b, dy = tensors(c)
        assert not x[0].any() and not np.signbit(x[0]).any()          # a row of +0.0
        assert np.signbit(x[1, 0]) and x[1, 0] == 0 and np.signbit(x[2]).all() and np.signbit(w[0, 0, 0])
    out = []
    for geo, bias in (("subm", True), ("s2p1", False)):
        c = case(f"signed_zeros_{geo}", random_sites(70, 100, 1, [5, 6, 7]), 1, [5, 6, 7], geo, present, bias=bias, seed=70)
        c["special"] = True
        out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    out = []
    for fam in (sizes, batches, borders, occupancy, backbone_layers, huge, channels, values, huge_many, segments):
        out.extend(fam())
    assert len({c["name"] for c in out}) == len(out)
    return tuple(out)


def get(name):
    return next(c for c in all_cases() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(out_indices, out_shape, nbr, nbr_t) of the restatement, computed once and shared"""
    c = get(name)
    return seq.rulebook(c["indices"], c["batch_size"], c["shape"], c["kernel"], c["stride"], c["padding"], c["subm"])


@functools.lru_cache(maxsize=None)
def expected_values(name):
    """(forward32, input_grad32) of the restatement on tensors(case), computed once and shared"""
    c = get(name)
    x, w, b, dy = tensors(c)
    _, _, nbr, nbr_t = expected(name)
    return seq.forward32(x, w, b, nbr), seq.input_grad32(dy, w, nbr_t)


@functools.lru_cache(maxsize=None)
def expected_grads(name):
    """(weight_grad32, bias_grad32) of the restatement on tensors(case), computed once and shared"""
    x, w, b, dy = tensors(get(name))
    return seq.weight_grad32(x, dy, expected(name)[2]), seq.bias_grad32(dy)
