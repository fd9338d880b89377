"""Edge families of the inverse sparse convolution, shared by tests/test_spconv_inverse_cpu.py (the restatement against
a dense oracle) and tests/test_gpu_spconv_inverse.py (the device against the restatement).  Not a test module.

A case is a dict: name, indices (N, 4) int32 [b, z, y, x] -- the FINE sites, the input of the strided convolution whose
rulebook is inverted --, batch_size, shape, kernel, stride, padding, cin (the channels on the coarse side), cout (on the
fine side), bias (bool), seed, and `present`: a function of the case that asserts FROM THE INPUTS that the edge the case
is named after is there.  The smallest shapes at which the kernels can still go wrong: a workgroup owns 64 positions of
the class order inside one class, the grid is N / 64 + C workgroups, channels go through LDS in chunks of 32, the class
tiles apply for 2 .. 64 classes.
"""
import functools

import numpy as np

import spconv_cases as sc
import spconv_inverse_seq as inv
import spconv_seq as seq

F = np.float32
GEOMETRIES = {   # kernel, stride, padding
    "s2p1": sc.GEOMETRIES["s2p1"][:3],
    "s2p011": sc.GEOMETRIES["s2p011"][:3],
    "k311": sc.GEOMETRIES["k311"][:3],
    "s2p0": (3, 2, 0),         # fine rows at the far border that no output reads
    "s3": (3, 3, 0),           # 27 classes, one offset per row
    "s1": (3, 1, 1),           # a strided rulebook with stride 1: one class, the rows of nbr_t
    "k5s5": (5, 5, 0),         # 125 classes: past the 64 of the class tiles, the rows of nbr_t
}


def case(name, indices, batch_size, shape, geometry, present, cin=4, cout=16, bias=True, seed=0):
    kernel, stride, padding = GEOMETRIES[geometry]
    return dict(name=name, indices=np.ascontiguousarray(indices, dtype=np.int32).reshape(-1, 4), batch_size=batch_size,
                shape=list(shape), kernel=kernel, stride=stride, padding=padding, geometry=geometry, cin=cin, cout=cout,
                bias=bias, seed=seed, present=present)


def class_counts(c):
    return np.bincount(inv.row_classes(c["indices"], c["stride"], c["padding"]), minlength=inv.classes(c["stride"]))


def geometries():
    out = []
    for i, (geo, shape, n) in enumerate((("s2p1", [11, 16, 18], 600), ("s2p011", [11, 16, 18], 600), ("k311", [11, 6, 7], 300),
                                         ("s2p0", [6, 6, 6], 150), ("s3", [9, 10, 11], 400), ("s1", [5, 6, 7], 150),
                                         ("k5s5", [10, 11, 12], 1500))):
        def present(c, geo=geo):
            C, counts = inv.classes(c["stride"]), class_counts(c)
            assert C == {"s2p1": 8, "s2p011": 8, "k311": 2, "s2p0": 8, "s3": 27, "s1": 1, "k5s5": 125}[geo]
            assert (counts > 0).all() and len(c["indices"]) > 64
            table = expected(c["name"])[2]
            if geo == "s2p0":   # rows that nothing reads: every coordinate 5 lies past the last window
                unread = (table < 0).all(0)
                assert unread.any() and (c["indices"][unread, 1:] == 5).any(1).all() and not unread.all()
            if geo == "s3":
                assert ((table >= 0).sum(0) <= 1).all() and all(len(inv.admitted(k, 3, 3)) == 1 for k in range(27))
            if geo in ("s1", "k5s5"):
                assert not 2 <= C <= 64
        out.append(case(f"geo_{geo}", sc.random_sites(100 + i, n, 2, shape), 2, shape, geo, present, seed=100 + i,
                        bias=bool(i % 2)))
    return out


def sizes():
    out = []
    for n in (0, 1, 63, 64, 65, 3001):
        def present(c, n=n):
            assert len(c["indices"]) == n and (n % 64 or n in (0, 64))
            if n > 3000:
                assert n > 2048 and (class_counts(c) > 128).all()   # two sort tiles, several tiles in every class
                coarse = len(expected(c["name"])[0])   # the weight gradient walks the coarse rows: a seam, off the 32-row chunks
                assert coarse > 1024 and seq.wgrad_segments(coarse)[0] == 2 and seq.wgrad_segments(coarse)[1] % 32
        out.append(case(f"n{n}", sc.random_sites(10 + n, n, 1, [11, 30, 34]), 1, [11, 30, 34], "s2p1", present, seed=n))
    return out


def batches():
    shape = [8, 10, 12]

    def has(k, empty_at):
        def present(c):
            per = np.bincount(c["indices"][:, 0], minlength=k)
            assert c["batch_size"] == k and all((per[b] == 0) == (b in empty_at) for b in range(k))
        return present
    return [case("batch_empty_middle", sc.random_sites(4, 300, 3, shape, [0, 2]), 3, shape, "s2p1", has(3, (1,)), seed=4),
            case("batch_empty_last", sc.random_sites(5, 300, 3, shape, [0, 1]), 3, shape, "s2p011", has(3, (2,)), seed=5)]


def cells_of_parity(shape, parity, seed):
    """the cells of `shape` with (z, y, x) % 2 == parity, in a seeded random order"""
    z, y, x = np.meshgrid(*(np.arange(parity[j], shape[j], 2) for j in range(3)), indexing="ij")
    cells = np.stack([np.zeros(z.size, dtype=np.int64), z.ravel(), y.ravel(), x.ravel()], axis=1)
    return cells[np.random.default_rng(seed).permutation(len(cells))]


def occupancy():
    shape = [8, 16, 16]
    even = cells_of_parity(shape, (0, 0, 0), 1)[:200]

    def present_even(c):
        counts = class_counts(c)
        assert not (c["indices"][:, 1:] % 2).any() and (counts > 0).sum() == 1 and counts[7] == 200   # seven empty classes
    edge = np.concatenate([cells_of_parity(shape, (0, 0, 0), 2)[:64], cells_of_parity(shape, (1, 0, 0), 3)[:65],
                           cells_of_parity(shape, (0, 1, 1), 4)[:30]])
    edge = edge[np.random.default_rng(5).permutation(len(edge))]

    def present_edge(c):
        counts = sorted(class_counts(c).tolist())
        assert counts == [0, 0, 0, 0, 0, 30, 64, 65]   # a class that fills its tile exactly and one that needs a second
    one = np.asarray([(0, 2 + (q >> 2 & 1), 4 + (q >> 1 & 1), 6 + (q & 1)) for q in (5, 0, 3, 6, 1, 7, 2, 4)], dtype=np.int32)

    def present_one(c):
        counts, n = class_counts(c), len(c["indices"])
        assert n == 8 and (counts == 1).all()
        assert -(-n // 64) < 8 <= n // 64 + 8   # eight tiles: ceil(N / 64) workgroups would be too few, N / 64 + C are enough
    return [case("all_even", even, 1, shape, "s2p1", present_even, seed=30),
            case("tile_edge_in_class", edge, 1, shape, "s2p1", present_edge, seed=31, cin=5, cout=7),
            case("one_row_per_class", one, 1, shape, "s2p1", present_one, seed=32)]


def channels():
    pairs = [(64, 64), (64, 32), (32, 16), (128, 5), (3, 128), (1, 1)]
    out = []
    for i, (cin, cout) in enumerate(pairs):
        for bias in (False, True):
            def present(c, cin=cin, cout=cout, bias=bias):
                assert (c["cin"], c["cout"], c["bias"]) == (cin, cout, bias) and len(c["indices"]) > 128
            out.append(case(f"c{cin}_{cout}_{'bias' if bias else 'nobias'}", sc.random_sites(60 + i, 200, 2, [6, 10, 12]), 2,
                            [6, 10, 12], "s2p1" if i % 2 == 0 else "s2p011", present, cin=cin, cout=cout, bias=bias,
                            seed=60 + 2 * i + bias))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    out = []
    for fam in (geometries, sizes, batches, occupancy, channels):
        out.extend(fam())
    assert len({c["name"] for c in out}) == len(out)
    return tuple(out)


def get(name):
    return next(c for c in all_cases() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(coarse indices, coarse shape, pairs (K, N_fine), perm, class_start) of the restatements, computed once and shared"""
    c = get(name)
    coarse, oshape, _, _ = seq.rulebook(c["indices"], c["batch_size"], c["shape"], c["kernel"], c["stride"], c["padding"], False)
    table = inv.pairs(c["indices"], coarse, c["shape"], c["kernel"], c["stride"], c["padding"])
    perm, class_start = inv.class_order(c["indices"], c["stride"], c["padding"])
    return coarse, oshape, table, perm, class_start


def tensors(c):
    """x (N_coarse, Cin), weight (K, Cin, Cout), bias (Cout,) | None, dy (N_fine, Cout): float32, fixed by the case"""
    rng = np.random.default_rng(2000 + c["seed"])
    K = int(np.prod(seq.triple(c["kernel"])))
    n_coarse = len(expected(c["name"])[0])
    x = rng.standard_normal((n_coarse, c["cin"])).astype(F)
    w = rng.uniform(-0.5, 0.5, (K, c["cin"], c["cout"])).astype(F)
    b = rng.uniform(-1, 1, (c["cout"],)).astype(F) if c["bias"] else None
    dy = rng.standard_normal((len(c["indices"]), c["cout"])).astype(F)
    return x, w, b, dy


@functools.lru_cache(maxsize=None)
def expected_values(name):
    """(forward32, input_grad32) of the restatement on tensors(case), computed once and shared"""
    c = get(name)
    x, w, b, dy = tensors(c)
    coarse, _, table, _, _ = expected(name)
    return inv.forward32(x, w, b, table), inv.input_grad32(dy, w, table, len(coarse))


@functools.lru_cache(maxsize=None)
def expected_weight_grad(name):
    """The weight gradient in the order the device adds in: the sums of spconv_seq.weight_grad32 over the COARSE rows --
    segments of them in ascending order, coarse row o reading fine row nbr[k, o], the inverse of the pairs table -- with
    the two sides exchanged, (K, Cout, Cin), transposed.  -> dw (K, Cin, Cout) float32"""
    x, w, b, dy = tensors(get(name))
    coarse, _, table, _, _ = expected(name)
    nbr = np.full((table.shape[0], len(coarse)), -1, dtype=np.int32)
    k, fine = np.nonzero(table >= 0)
    nbr[k, table[k, fine]] = fine
    assert (nbr >= 0).sum() == (table >= 0).sum()   # a coarse row writes one fine site per offset
    return np.ascontiguousarray(seq.weight_grad32(dy, x, nbr).transpose(0, 2, 1))
