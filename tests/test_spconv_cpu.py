"""CPU: the sequential restatement of the sparse convolutions (tests/spconv_seq.py) against an
independent dense oracle -- torch.nn.functional.conv3d in float64 on the densified input --, the module API of
modest_amd.utils.spconv without touching the GPU, and the opt-in binding of pcdet_bind.install(sparse_conv=True)."""
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spconv_cases as sc  # noqa: E402
import spconv_seq as seq  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENSE = [c["name"] for c in sc.all_cases() if c["dense"]]
ORACLE_ERR = 2.0 ** -45   # the float64 oracle's own rounding, relative to S (thousands of terms at 2^-53 each)


def test_every_case_has_its_edge():
    for c in sc.all_cases():
        c["present"](c)
    names = [c["name"] for c in sc.all_cases()]
    assert len(names) >= 50 and not all(c["dense"] for c in sc.all_cases())


def densify(c, values):
    """(N, C) at the case's input sites -> (B, C, D, H, W) float64"""
    idx = torch.from_numpy(c["indices"].astype(np.int64))
    out = torch.zeros([c["batch_size"], *c["shape"], values.shape[1]], dtype=torch.float64)
    out[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]] = torch.from_numpy(np.asarray(values, dtype=np.float64))
    return out.permute(0, 4, 1, 2, 3).contiguous()


def oracle(c, x, w, b, dy):
    """-> out sites (M, 4) sorted, out values / S at them, dx / S at the input sites; all from conv3d in float64"""
    import torch.nn.functional as Fn
    k = seq.triple(c["kernel"])
    stride, pad = ((1, 1, 1), tuple(a // 2 for a in k)) if c["subm"] else (seq.triple(c["stride"]), seq.triple(c["padding"]))
    w5 = torch.from_numpy(np.asarray(w, dtype=np.float64).reshape(*k, c["cin"], c["cout"])).permute(4, 3, 0, 1, 2).contiguous()
    b1 = torch.from_numpy(np.asarray(b, dtype=np.float64)) if b is not None else None
    occ = densify(c, np.ones((len(c["indices"]), 1)))
    hit = Fn.conv3d(occ, torch.ones((1, 1, *k), dtype=torch.float64), stride=stride, padding=pad)[:, 0] > 0
    if c["subm"]:
        sites = torch.from_numpy(c["indices"].astype(np.int64))   # read at the input sites, in input order
    else:
        sites = torch.nonzero(hit)   # row-major: ascending in (b, z, y, x)
    at = (sites[:, 0], slice(None), sites[:, 1], sites[:, 2], sites[:, 3])
    xin = densify(c, x).requires_grad_(True)
    out = Fn.conv3d(xin, w5, b1, stride=stride, padding=pad)
    vals = out[at]
    S = Fn.conv3d(densify(c, np.abs(x)), w5.abs(), b1.abs() if b1 is not None else None, stride=stride, padding=pad)[at]
    ins = torch.from_numpy(c["indices"].astype(np.int64))
    at_in = (ins[:, 0], slice(None), ins[:, 1], ins[:, 2], ins[:, 3])
    dx = dS = np.zeros((len(ins), c["cin"]))
    if len(sites) == len(dy) and len(dy):
        g = torch.from_numpy(np.asarray(dy, dtype=np.float64))
        (dxd,) = torch.autograd.grad((vals * g).sum(), xin)
        dx = dxd[at_in].numpy()
        xa = densify(c, np.abs(x)).requires_grad_(True)
        (dSd,) = torch.autograd.grad((Fn.conv3d(xa, w5.abs(), None, stride=stride, padding=pad)[at] * g.abs()).sum(), xa)
        dS = dSd[at_in].numpy()
    return sites.numpy(), vals.detach().numpy(), S.numpy(), dx, dS


@pytest.mark.parametrize("name", DENSE)
def test_restatement_against_dense_conv3d(name):
    c = sc.get(name)
    x, w, b, dy = sc.tensors(c)
    out_idx, out_shape, nbr, nbr_t = sc.expected(name)
    got, got_dx = sc.expected_values(name)
    sites, vals, S, dx, dS = oracle(c, x, w, b, dy)
    # the sites agree exactly, in order
    assert out_idx.shape == sites.shape and (out_idx.astype(np.int64) == sites).all(), name
    assert out_shape == seq.out_shape(c["shape"], c["kernel"], c["stride"], c["padding"], c["subm"])
    K = nbr.shape[0]
    # |got - exact| <= gamma_n S, n = terms + 1 (K Cin products and sums, the bias); no element excluded
    bound = seq.gamma(K * c["cin"] + 1) * S + ORACLE_ERR * S
    err = np.abs(got.astype(np.float64) - vals)
    assert got.dtype == np.float32 and got.shape == vals.shape and (err <= bound).all(), (name, float((err - bound).max()))
    bound = seq.gamma(K * c["cout"] + 1) * dS + ORACLE_ERR * dS
    err = np.abs(got_dx.astype(np.float64) - dx)
    assert got_dx.shape == dx.shape and (err <= bound).all(), (name, float((err - bound).max()))
    # the float64 restatement is the same sum
    f64, S64, n64 = seq.forward64(x, w, b, nbr)
    assert np.allclose(f64, vals, rtol=0, atol=1e-9) and (n64 <= K * c["cin"] + 1).all()
    assert (np.abs(got - f64) <= seq.gamma(n64) * S64).all()
    d64, dS64, dn64 = seq.input_grad64(dy, w, nbr_t)
    assert np.allclose(d64, dx, rtol=0, atol=1e-9) and (np.abs(got_dx - d64) <= seq.gamma(dn64) * dS64).all()


def test_restatement_rejects_bad_rows_and_the_huge_shape_is_cheap():
    with pytest.raises(ValueError, match="duplicate"):
        seq.rulebook([[0, 1, 1, 1], [0, 1, 1, 1]], 1, [3, 3, 3], 3, 1, 0, True)
    with pytest.raises(ValueError, match="outside"):
        seq.rulebook([[0, 1, 1, 3]], 1, [3, 3, 3], 3, 1, 0, True)
    with pytest.raises(ValueError, match="outside"):
        seq.rulebook([[1, 1, 1, 1]], 1, [3, 3, 3], 3, 1, 0, True)
    out_idx, out_shape, nbr, nbr_t = sc.expected("huge_subm")
    # (0,0,0,0)-(0,0,0,1) are neighbours; the pairs across a row end and across the clouds are not
    rows = {tuple(r): i for i, r in enumerate(sc.get("huge_subm")["indices"].tolist())}
    a, b = rows[(0, 0, 0, 0)], rows[(0, 0, 0, 1)]
    assert nbr[14, a] == b and nbr[12, b] == a
    for p, q in (((0, 500, 1000, 2199), (0, 500, 1001, 0)), ((0, 999, 1999, 2199), (1, 0, 0, 0)), ((0, 0, 0, 1), (0, 976, 257, 1897))):
        assert not (nbr[:, rows[p]] == rows[q]).any() and not (nbr[:, rows[q]] == rows[p]).any()


# ------------------------------------------------------------------------------------------------ weight and bias gradients
def test_wgrad_segments():
    want = {0: (1, 0), 1: (1, 1), 1024: (1, 1024), 1025: (2, 513), 32768: (32, 1024), 32769: (32, 1025), 100000: (32, 3125)}
    for n, pair in want.items():
        assert seq.wgrad_segments(n) == pair, n
    for n in (1, 513, 1024, 1025, 2049, 31745, 32768, 32769, 33797, 100000):   # the segments cover the rows, none is empty
        s, rows = seq.wgrad_segments(n)
        assert (s - 1) * rows < n <= s * rows


@pytest.mark.parametrize("name", [c["name"] for c in sc.all_cases()])
def test_gradient_restatement_inside_the_bound(name):
    """weight_grad32 / bias_grad32 are sums of n - 1 terms in some order: inside gamma_n S of the float64 sums"""
    c = sc.get(name)
    x, w, b, dy = sc.tensors(c)
    nbr = sc.expected(name)[2]
    dw, db = sc.expected_grads(name)
    (dw64, Sw, nw), (db64, Sb, nb) = seq.weight_grad64(x, dy, nbr)
    assert dw.dtype == np.float32 and dw.shape == dw64.shape and db.dtype == np.float32 and db.shape == db64.shape
    err = np.abs(dw.astype(np.float64) - dw64)
    assert (err <= seq.gamma(nw) * Sw).all(), (name, "dw", float((err - seq.gamma(nw) * Sw).max()))
    err = np.abs(db.astype(np.float64) - db64)
    assert (err <= seq.gamma(nb) * Sb).all(), (name, "db", float((err - seq.gamma(nb) * Sb).max()))
    if len(dy) > 64:
        assert dw.any() and db.any()


def scalar_gradients(x, dy, nbr):
    """DESIGN.md section 7g's order of the weight and bias gradients as a literal loop over scalars, written apart from
    tests/spconv_seq.py: nothing vectorised, every product and every sum one float32 operation"""
    F = np.float32
    K, n_out = len(nbr), len(dy)
    cin, cout = x.shape[1], dy.shape[1]
    segments = (n_out + 1023) // 1024
    segments = 1 if segments < 1 else (32 if segments > 32 else segments)
    seg_rows = (n_out + segments - 1) // segments
    nbr = [list(map(int, row)) for row in nbr]
    dw, db = np.empty((K, cin, cout), dtype=F), np.empty((cout,), dtype=F)
    for k in range(K):
        for ci in range(cin):
            for co in range(cout):
                total = F(0.0)
                for s in range(segments):
                    acc = F(0.0)
                    for o in range(s * seg_rows, min((s + 1) * seg_rows, n_out)):
                        i = nbr[k][o]
                        if i < 0:
                            continue
                        product = F(x[i, ci] * dy[o, co])
                        acc = F(acc + product)
                    total = F(total + acc)
                dw[k, ci, co] = total
    for co in range(cout):
        total = F(0.0)
        for s in range(segments):
            acc = F(0.0)
            for o in range(s * seg_rows, min((s + 1) * seg_rows, n_out)):
                acc = F(acc + dy[o, co])
            total = F(total + acc)
        db[co] = total
    return dw, db


def seam_inputs():
    """3 offsets over 2 049 rows -- 3 segments of 683 rows, 683 = 21 * 32 + 11 --, half of the entries absent, the rows on
    both sides of either seam present at offset 0, and -0.0 on either side"""
    rng = np.random.default_rng(7)
    n_in, n_out = 500, 2049
    nbr = rng.integers(0, n_in, (3, n_out)).astype(np.int32)
    nbr[rng.random((3, n_out)) < 0.5] = -1
    nbr[0, [0, 682, 683, 1365, 1366, 2048]] = [5, 6, 7, 8, 9, 10]
    nbr[2, :683] = -1   # an offset with a segment in which nothing contributes
    x = rng.standard_normal((n_in, 2)).astype(np.float32)
    dy = rng.standard_normal((n_out, 3)).astype(np.float32)
    x[5], dy[683], dy[2048, 1] = np.float32(-0.0), np.float32(-0.0), np.float32(-0.0)
    return x, dy, nbr


@pytest.mark.parametrize("name", ["seg1025_subm", "seam2049", "signed_zeros_subm", "signed_zeros_s2p1"])
def test_gradient_restatement_is_the_scalar_loop(name):
    if name == "seam2049":
        x, dy, nbr = seam_inputs()
        assert seq.wgrad_segments(len(dy)) == (3, 683) and 683 % 32
    else:
        c = sc.get(name)
        c["present"](c)
        x, w, b, dy = sc.tensors(c)
        nbr = sc.expected(name)[2]
        if name == "seg1025_subm":
            assert seq.wgrad_segments(len(dy)) == (2, 513) and 513 % 32
        else:
            assert np.signbit(x[x == 0]).any() and np.signbit(dy[0]).all()
    want_dw, want_db = scalar_gradients(x, dy, nbr)
    dw, db = seq.weight_grad32(x, dy, nbr), seq.bias_grad32(dy)
    assert seq.same_bits(dw, want_dw), (name, int((dw.view(np.int32) != want_dw.view(np.int32)).sum()))
    assert seq.same_bits(db, want_db), (name, int((db.view(np.int32) != want_db.view(np.int32)).sum()))
    assert not np.signbit(dw[dw == 0]).any() and not np.signbit(db[db == 0]).any()   # a sum from +0 is never -0


# ------------------------------------------------------------------------------------------------ the module API
def test_shape_arithmetic():
    from modest_amd import ops
    from modest_amd.utils import spconv
    shape = [41, 1600, 1808]
    for conv, want in ((spconv.SparseConv3d(16, 32, 3, stride=2, padding=1, bias=False), [21, 800, 904]),
                       (spconv.SubMConv3d(16, 16, 3, padding=1, bias=False), shape),
                       (spconv.SubMConv3d(16, 16, 3, stride=2, padding=7), shape),   # accepted and ignored
                       (spconv.SparseConv3d(64, 64, 3, stride=2, padding=(0, 1, 1)), [20, 800, 904]),
                       (spconv.SparseConv3d(64, 128, (3, 1, 1), stride=(2, 1, 1), padding=0), [20, 1600, 1808])):
        assert conv.output_shape(shape) == want
    d = [41]
    for geo in ("s2p1", "s2p1", "s2p011", "k311"):
        k, s, p, subm = sc.GEOMETRIES[geo]
        d.append(ops.spconv_out_shape([d[-1], 8, 8], k, s, p, subm)[0])
    assert d == [41, 21, 11, 5, 2]
    with pytest.raises(ValueError, match="output shape"):
        spconv.SparseConv3d(4, 4, 3, stride=1, padding=0).output_shape([2, 10, 10])
    with pytest.raises(ValueError, match="output shape"):
        ops.spconv_out_shape([5, 5, 5], (7, 1, 1), 1, 0)
    with pytest.raises(ValueError, match="odd"):
        spconv.SubMConv3d(4, 4, 2)
    for bad in (dict(dilation=2), dict(groups=2)):
        with pytest.raises(NotImplementedError):
            spconv.SparseConv3d(4, 4, 3, **bad)
    with pytest.raises(NotImplementedError):
        spconv.SparseConvolution(3, 4, 4, 3, transposed=True)
    with pytest.raises(NotImplementedError):
        spconv.SparseConvolution(3, 4, 4, 3, inverse=True)


def test_parameters_and_state_dict():
    from modest_amd.utils import spconv
    torch.manual_seed(0)
    conv = spconv.SparseConv3d(16, 32, (3, 1, 1), stride=(2, 1, 1))
    assert tuple(conv.weight.shape) == (3, 1, 1, 16, 32) and tuple(conv.bias.shape) == (32,)
    assert sorted(conv.state_dict()) == ["bias", "weight"]
    nob = spconv.SubMConv3d(4, 16, 3, padding=1, bias=False, indice_key="subm1")
    assert tuple(nob.weight.shape) == (3, 3, 3, 4, 16) and nob.bias is None and sorted(nob.state_dict()) == ["weight"]
    bound = 1 / np.sqrt(27 * 4)   # kaiming_uniform_(a=sqrt(5)) with fan-in K * Cin
    top = float(nob.weight.detach().abs().max())
    assert 0.9 * bound < top <= bound
    other = spconv.SparseConv3d(16, 32, (3, 1, 1), stride=(2, 1, 1))
    other.load_state_dict(conv.state_dict())
    assert torch.equal(other.weight, conv.weight) and torch.equal(other.bias, conv.bias)
    assert isinstance(conv, spconv.SparseModule) and isinstance(conv, torch.nn.Module)


class Recorder(torch.nn.Module):
    def __init__(self, log, tag):
        super().__init__()
        self.log, self.tag = log, tag

    def forward(self, x):
        self.log.append((self.tag, type(x).__name__))
        return x + 1 if isinstance(x, torch.Tensor) else x


def test_sparse_sequential_constructors_and_dispatch():
    from modest_amd.utils import spconv

    class SparseRecorder(Recorder, spconv.SparseModule):
        pass
    log = []
    a, b, c = SparseRecorder(log, "a"), Recorder(log, "b"), Recorder(log, "c")
    positional = spconv.SparseSequential(a, b, c)
    ordered = spconv.SparseSequential(OrderedDict([("first", a), ("second", b)]))
    keyword = spconv.SparseSequential(conv=a, bn=b)
    assert len(positional) == 3 and positional[0] is a and positional[2] is c and positional[-1] is c
    assert list(ordered._modules) == ["first", "second"] and list(keyword._modules) == ["conv", "bn"]
    with pytest.raises(IndexError):
        positional[3]
    grown = spconv.SparseSequential().add(a).add(b, "named")
    assert len(grown) == 2 and list(grown._modules) == ["0", "named"]
    t = spconv.SparseConvTensor(torch.zeros((2, 3)), torch.zeros((2, 4), dtype=torch.int32), [4, 4, 4], 1)
    out = positional(t)
    # the SparseModule child was handed the tensor, the others its features
    assert out is t and log == [("a", "SparseConvTensor"), ("b", "Tensor"), ("c", "Tensor")] and torch.all(t.features == 2)
    del log[:]
    plain = positional(torch.zeros(3))
    assert log == [("a", "Tensor"), ("b", "Tensor"), ("c", "Tensor")] and torch.all(plain == 3)


def test_sparse_conv_tensor_and_dense_on_the_cpu():
    from modest_amd.utils import spconv
    idx = torch.tensor([[0, 0, 1, 2], [1, 3, 0, 0], [1, 3, 4, 5]], dtype=torch.int32)
    feats = torch.arange(6, dtype=torch.float32).reshape(3, 2).requires_grad_(True)
    t = spconv.SparseConvTensor(feats, idx, [4, 5, 6], 2)
    assert t.spatial_size == 120 and t.spatial_shape == [4, 5, 6] and t.batch_size == 2 and t.indice_dict == {}
    assert t.find_indice_pair("subm1") is None and t.find_indice_pair(None) is None
    t.indice_dict["subm1"] = "rulebook"
    assert t.find_indice_pair("subm1") == "rulebook"
    first, last = t.dense(), t.dense(channels_first=False)
    assert tuple(first.shape) == (2, 2, 4, 5, 6) and tuple(last.shape) == (2, 4, 5, 6, 2)
    assert torch.equal(first.permute(0, 2, 3, 4, 1), last) and float(last.detach().abs().sum()) == 15
    assert last[1, 3, 4, 5].tolist() == [4, 5] and last[0, 0, 1, 2].tolist() == [0, 1]
    (first * 2).sum().backward()
    assert torch.all(feats.grad == 2)
    t.features = feats.detach() * 3   # assignable
    assert float(t.dense().sum()) == 45


def test_cpu_tensors_raise_and_nothing_opens_the_gpu():
    from modest_amd import ops
    from modest_amd.utils import spconv
    idx = torch.zeros((1, 4), dtype=torch.int32)
    with pytest.raises(ValueError, match="device tensor"):
        ops.spconv_rulebook(idx, 1, [3, 3, 3], 3, 1, 0, True)
    conv = spconv.SubMConv3d(4, 4, 3)
    with pytest.raises(ValueError, match="device tensor"):
        conv(spconv.SparseConvTensor(torch.zeros((1, 4)), idx, [3, 3, 3], 1))


def test_names_that_are_not_provided():
    from modest_amd.utils import spconv
    for name in ("SparseInverseConv3d", "SparseConvTranspose3d", "SparseMaxPool3d", "ToDense", "SomethingElse"):
        cls = getattr(spconv, name)
        assert isinstance(cls, type) and getattr(spconv, name) is cls

        class Sub(cls):   # can be subclassed at import time
            pass
        with pytest.raises(NotImplementedError, match="not provided"):
            cls(1, 2)
    from modest_amd.utils import spconv_utils
    assert spconv.utils is spconv_utils


def test_entry_points_are_declared_and_mirrored():
    from modest_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "modest_hip.h")).read()
    for name, res, nargs in (("modest_spconv_rulebook_workspace_bytes", "int64_t", 3), ("modest_spconv_rulebook_plan", "int", 12),
                             ("modest_spconv_rulebook_fill", "int", 15), ("modest_spconv_gather_gemm", "int", 13),
                             ("modest_spconv_wgrad_workspace_bytes", "int64_t", 4), ("modest_spconv_wgrad", "int", 13)):
        assert f"{res} {name}(" in hdr
        decl = hdr[hdr.rindex(f"{res} {name}("):]
        assert decl[:decl.index(";")].count(",") + 1 == nargs == len(_lib.SIGNATURES[name][1])
        assert hasattr(_lib.load(), name)


def test_workspace_does_not_depend_on_the_grid_and_kernels_use_no_scratch():
    import json
    from modest_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    # a function of the rows and the kernel volume: 160 000 sites of the Lyft grid need what 160 000 sites of any grid need
    sub, full = (int(lib.modest_spconv_rulebook_workspace_bytes(160_000, 27, s)) for s in (1, 0))
    assert 0 < sub <= 64 * 160_000 + (1 << 16) and sub < full <= 32 * 27 * 160_000 + (1 << 20)
    assert int(lib.modest_spconv_rulebook_workspace_bytes(0, 27, 0)) >= 0
    res = json.load(open(os.path.join(os.path.dirname(build.LIB), "kernel_resources.json")))
    mine = {k: v for k, v in res.items() if v.get("file") in ("spconv.hip", "sort64.hip")}
    assert sum(v["file"] == "spconv.hip" for v in mine.values()) == 18 and sum(v["file"] == "sort64.hip" for v in mine.values()) == 4
    assert sum("sp_gather_gemm" in k for k in mine) == 4 and sum("sp_wgrad_partial" in k for k in mine) == 3
    assert all(v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 for v in mine.values()), mine


# ------------------------------------------------------------------------------------------------ the binding
def test_binding_is_opt_in():
    import types
    from modest_amd.utils import pcdet_bind, spconv_utils
    from modest_amd.utils import spconv as ours
    names = list(pcdet_bind.SHIMS) + list(pcdet_bind.STAND_INS) + ["spconv.utils"]
    saved = {k: sys.modules.get(k) for k in names}
    try:
        for k in names:
            sys.modules.pop(k, None)
        keys = sorted(list(pcdet_bind.SHIMS) + list(pcdet_bind.STAND_INS))
        # the default call: a stand-in, as before
        bound = pcdet_bind.install()
        assert sorted(bound) == keys and isinstance(sys.modules["spconv"], pcdet_bind.StandIn)
        assert sys.modules["spconv.utils"] is spconv_utils
        with pytest.raises(NotImplementedError, match="not provided"):
            sys.modules["spconv"].SparseConvTensor(1, 2, 3, 4)
        # opt in: the package replaces the stand-in, spconv.utils stays what it was, the other stand-in stays one
        bound = pcdet_bind.install(sparse_conv=True)
        import spconv
        from spconv.utils import VoxelGeneratorV2
        assert sorted(bound) == keys and bound["spconv"] is ours and spconv is ours and sys.modules["spconv"] is ours
        assert spconv.utils is spconv_utils and sys.modules["spconv.utils"] is spconv_utils
        assert VoxelGeneratorV2 is spconv_utils.VoxelGeneratorV2
        assert isinstance(sys.modules[pcdet_bind.STAND_INS[0]], pcdet_bind.StandIn)
        assert issubclass(spconv.SubMConv3d, spconv.SparseModule) and spconv.SparseConvTensor is ours.SparseConvTensor
        with pytest.raises(NotImplementedError, match="not provided"):
            spconv.SparseInverseConv3d(1, 2, 3)
        # idempotent, and a later default call leaves the package bound
        again = pcdet_bind.install(sparse_conv=True)
        assert all(again[k] is bound[k] for k in bound) and sys.modules["spconv"] is ours
        assert pcdet_bind.install()["spconv"] is ours and sys.modules["spconv.utils"] is spconv_utils
        # from nothing, with and without the stand-ins
        for k in list(pcdet_bind.STAND_INS) + ["spconv.utils"]:
            sys.modules.pop(k, None)
        bound = pcdet_bind.install(stand_ins=False, sparse_conv=True)
        assert sorted(bound) == sorted(list(pcdet_bind.SHIMS) + ["spconv"]) and sys.modules["spconv"] is ours
        assert pcdet_bind.STAND_INS[0] not in sys.modules and sys.modules["spconv.utils"] is spconv_utils
        # an spconv that is neither (an installed one) is left alone either way
        for k in list(pcdet_bind.STAND_INS) + ["spconv.utils"]:
            sys.modules.pop(k, None)
        real = sys.modules["spconv"] = types.ModuleType("spconv")
        pcdet_bind.install(sparse_conv=True)
        assert sys.modules["spconv"] is real and not hasattr(real, "utils") and "spconv.utils" not in sys.modules
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_the_benchmark_yardstick_computes_the_same_sums():
    """tools/spconv_bench.py's composition of stock operators (index_select -> mm -> index_add per offset), on the CPU,
    against the float64 restatement: inside gamma_n S whatever order it adds in."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("spconv_bench", os.path.join(ROOT, "tools", "spconv_bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    for name in ("batch3_s2p1", "c33_65_subm", "vb_conv4"):
        c = sc.get(name)
        x, w, b, dy = sc.tensors(c)
        out_idx, out_shape, nbr, nbr_t = sc.expected(name)
        pairs = bench.compose_pairs(torch.from_numpy(nbr))
        got = bench.compose_forward(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b) if b is not None else None,
                                    pairs, len(out_idx)).numpy()
        f64, S, n = seq.forward64(x, w, b, nbr)
        assert got.dtype == np.float32 and (np.abs(got - f64) <= seq.gamma(n) * S).all(), name
    assert [l[1:3] for l in bench.LAYERS] == [(4, 16), (16, 16), (16, 32), (32, 32), (32, 32), (32, 64), (64, 64), (64, 64),
                                              (64, 64), (64, 64), (64, 64), (64, 128)]
