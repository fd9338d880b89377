"""CPU: the sequential restatement of the inverse sparse convolution (tests/spconv_inverse_seq.py)
against the forward restatement on nbr_t and against an independent dense oracle -- conv_transpose3d in float64 on the
densified coarse tensor --, the class order against hand cases, the module API of modest_amd.utils.spconv_inverse
without touching the GPU, and the opt-in binding of pcdet_bind.install(sparse_inverse=True)."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spconv_inverse_cases as ic  # noqa: E402
import spconv_inverse_seq as inv  # noqa: E402
import spconv_seq as seq  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c["name"] for c in ic.all_cases()]
ORACLE_ERR = 2.0 ** -45   # the float64 oracle's own rounding, relative to S (thousands of terms at 2^-53 each)


def test_every_case_has_its_edge():
    for c in ic.all_cases():
        c["present"](c)
    geos = {c["geometry"] for c in ic.all_cases()}
    assert geos == set(ic.GEOMETRIES) and {len(c["indices"]) for c in ic.all_cases()} >= {0, 1, 63, 64, 65, 3001}
    assert {(c["cin"], c["cout"]) for c in ic.all_cases()} >= {(64, 64), (64, 32), (32, 16), (128, 5), (3, 128), (1, 1)}


@pytest.mark.parametrize("name", NAMES)
def test_restatement_is_the_forward_restatement_on_nbr_t(name):
    """the table written from the coordinates is nbr_t, the sums are spconv_seq's on it, and a row is only ever read at
    the offsets its class admits"""
    c = ic.get(name)
    x, w, b, dy = ic.tensors(c)
    coarse, oshape, table, perm, class_start = ic.expected(name)
    out_idx, out_shape, nbr, nbr_t = seq.rulebook(c["indices"], c["batch_size"], c["shape"], c["kernel"], c["stride"],
                                                  c["padding"], False)
    assert seq.same_bits(table, nbr_t) and seq.same_bits(coarse, out_idx)
    got, got_dx = ic.expected_values(name)
    assert seq.same_bits(got, seq.forward32(x, w, b, nbr_t))
    # the feature gradient is the forward restatement with the transposed weights on nbr
    assert seq.same_bits(got_dx, seq.forward32(dy, np.ascontiguousarray(w.transpose(0, 2, 1)), None, nbr))
    # the weight gradient in the device's order: spconv_seq's segmented sums over the coarse rows on the rulebook's nbr, the
    # two sides exchanged, transposed; inside gamma_n S of the float64 sums
    got_dw = ic.expected_weight_grad(name)
    assert seq.same_bits(got_dw, np.ascontiguousarray(seq.weight_grad32(dy, x, nbr).transpose(0, 2, 1)))
    (dw64, Sw, nw), _ = inv.weight_grad64(x, dy, table)
    err = np.abs(got_dw.astype(np.float64) - dw64)
    assert got_dw.shape == w.shape and (err <= seq.gamma(nw) * Sw).all(), (name, "dw", float((err - seq.gamma(nw) * Sw).max()))
    cls = inv.row_classes(c["indices"], c["stride"], c["padding"])
    for k_cls in np.unique(cls):
        used = np.nonzero((table[:, cls == k_cls] >= 0).any(1))[0].tolist()
        assert set(used) <= set(inv.admitted(int(k_cls), c["kernel"], c["stride"])), (name, int(k_cls))
    assert len(inv.admitted(0, 3, 2)) == 8 and inv.admitted(7, 3, 2) == [13] and inv.admitted(0, 3, 2)[:3] == [0, 2, 6]


def densify(indices, batch_size, shape, values):
    idx = torch.from_numpy(np.asarray(indices, dtype=np.int64).reshape(-1, 4))
    out = torch.zeros([batch_size, *shape, values.shape[1]], dtype=torch.float64)
    out[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]] = torch.from_numpy(np.asarray(values, dtype=np.float64))
    return out.permute(0, 4, 1, 2, 3).contiguous()


def transpose_conv(c, oshape, dense, w5):
    """conv_transpose3d onto exactly the fine shape: output_padding restores the last indices that the strided
    convolution's floor dropped, a crop removes what lies past the shape"""
    import torch.nn.functional as Fn
    k, s, p = seq.triple(c["kernel"]), seq.triple(c["stride"]), seq.triple(c["padding"])
    short = [c["shape"][j] - ((oshape[j] - 1) * s[j] - 2 * p[j] + k[j]) for j in range(3)]
    opad = [min(max(v, 0), s[j] - 1) for j, v in enumerate(short)]
    out = Fn.conv_transpose3d(dense, w5, stride=s, padding=p, output_padding=opad)
    out = out[:, :, :c["shape"][0], :c["shape"][1], :c["shape"][2]]
    full = out.new_zeros((*out.shape[:2], *c["shape"]))   # (rows past what even the output padding reaches are read by nothing)
    full[:, :, :out.shape[2], :out.shape[3], :out.shape[4]] = out
    return full


@pytest.mark.parametrize("name", NAMES)
def test_restatement_against_dense_conv_transpose3d(name):
    c = ic.get(name)
    x, w, b, dy = ic.tensors(c)
    coarse, oshape, table, _, _ = ic.expected(name)
    got, got_dx = ic.expected_values(name)
    k = seq.triple(c["kernel"])
    K = k[0] * k[1] * k[2]
    w5 = torch.from_numpy(np.asarray(w, dtype=np.float64).reshape(*k, c["cin"], c["cout"])).permute(3, 4, 0, 1, 2).contiguous()
    fine = torch.from_numpy(c["indices"].astype(np.int64))
    at = (fine[:, 0], slice(None), fine[:, 1], fine[:, 2], fine[:, 3])
    co = torch.from_numpy(coarse.astype(np.int64))
    at_co = (co[:, 0], slice(None), co[:, 1], co[:, 2], co[:, 3])
    xd = densify(coarse, c["batch_size"], oshape, x).requires_grad_(True)
    wv = w5.clone().requires_grad_(True)
    vals = transpose_conv(c, oshape, xd, wv)[at]
    S = transpose_conv(c, oshape, densify(coarse, c["batch_size"], oshape, np.abs(x)), w5.abs())[at].numpy()
    want = vals.detach().numpy()
    if b is not None:
        want, S = want + b.astype(np.float64)[None, :], S + np.abs(b.astype(np.float64))[None, :]
    bound = seq.gamma(K * c["cin"] + 1) * S + ORACLE_ERR * S
    err = np.abs(got.astype(np.float64) - want)
    print(f"{name}: forward max error {float(err.max()) if err.size else 0.0:.3g}")
    assert got.dtype == np.float32 and got.shape == want.shape and (err <= bound).all(), (name, float((err - bound).max()))
    f64, S64, n64 = inv.forward64(x, w, b, table)
    assert np.allclose(f64, want, rtol=0, atol=1e-9) and (np.abs(got - f64) <= seq.gamma(n64) * S64).all()
    if not len(fine) or not len(coarse):
        return
    # gradients: the oracle's autograd, the same bound
    g = torch.from_numpy(dy.astype(np.float64))
    dxd, dwd = torch.autograd.grad((vals * g).sum(), [xd, wv])
    xa = densify(coarse, c["batch_size"], oshape, np.abs(x)).requires_grad_(True)
    wa = w5.abs().requires_grad_(True)
    dSx, dSw = torch.autograd.grad((transpose_conv(c, oshape, xa, wa)[at] * g.abs()).sum(), [xa, wa])
    dx, dS = dxd[at_co].numpy(), dSx[at_co].numpy()
    bound = seq.gamma(K * c["cout"] + 1) * dS + ORACLE_ERR * dS
    err = np.abs(got_dx.astype(np.float64) - dx)
    assert got_dx.shape == dx.shape and (err <= bound).all(), (name, "dx", float((err - bound).max()))
    (dw64, Sw, nw), (db64, Sb, nb) = inv.weight_grad64(x, dy, table)
    dw_oracle = dwd.permute(2, 3, 4, 0, 1).reshape(K, c["cin"], c["cout"]).numpy()
    Sw_oracle = dSw.permute(2, 3, 4, 0, 1).reshape(K, c["cin"], c["cout"]).numpy()
    assert (np.abs(dw64 - dw_oracle) <= ORACLE_ERR * Sw_oracle + 1e-300).all() and np.allclose(Sw, Sw_oracle, rtol=1e-12, atol=0)
    assert (nw.ravel() - 1 == (table >= 0).sum(1)).all() and np.allclose(db64, dy.astype(np.float64).sum(0))


def test_class_order_against_hand_cases():
    rows = np.asarray([[0, 0, 0, 0], [0, 1, 0, 0], [1, 0, 0, 1], [0, 0, 0, 2], [0, 1, 1, 1], [1, 1, 0, 0]], dtype=np.int32)
    # stride 2, padding 0: the class is (z % 2) * 4 + (y % 2) * 2 + x % 2 = 0 4 1 0 7 4
    assert inv.row_classes(rows, 2, 0).tolist() == [0, 4, 1, 0, 7, 4]
    perm, start = inv.class_order(rows, 2, 0)
    assert perm.tolist() == [0, 3, 2, 1, 5, 4] and start.tolist() == [0, 2, 3, 3, 3, 5, 5, 5, 6]
    # padding 1 shifts every residue: 7 3 6 7 0 3, equal classes keep their row order
    assert inv.row_classes(rows, 2, 1).tolist() == [7, 3, 6, 7, 0, 3]
    perm, start = inv.class_order(rows, 2, 1)
    assert perm.tolist() == [4, 1, 5, 2, 0, 3] and start.tolist() == [0, 1, 1, 1, 3, 3, 3, 4, 6]
    # mixed strides and padding (2, 1, 3), (0, 0, 1): z % 2 * 3 + (x + 1) % 3
    assert inv.row_classes(rows, (2, 1, 3), (0, 0, 1)).tolist() == [1, 4, 2, 0, 5, 4] and inv.classes((2, 1, 3)) == 6
    perm, start = inv.class_order(rows, (2, 1, 3), (0, 0, 1))
    assert perm.tolist() == [3, 0, 2, 1, 5, 4] and start.tolist() == [0, 1, 2, 3, 3, 5, 6]
    perm, start = inv.class_order(rows[:0], 2, 1)
    assert perm.shape == (0,) and start.tolist() == [0] * 9 and perm.dtype == start.dtype == np.int32
    perm, start = inv.class_order(rows, 1, 1)
    assert perm.tolist() == [0, 1, 2, 3, 4, 5] and start.tolist() == [0, 6]


# ------------------------------------------------------------------------------------------------ the module API
def fake_rulebook(**kw):
    from modest_amd import ops
    rb = ops.SpconvRulebook()
    rb.subm, rb.batch_size, rb.in_shape, rb.out_shape = False, 2, [8, 10, 12], [4, 5, 6]
    rb.kernel, rb.stride, rb.padding, rb.kvol, rb.n_in, rb.n_out = (3, 3, 3), (2, 2, 2), (1, 1, 1), 27, 9, 5
    rb.indices = torch.zeros((9, 4), dtype=torch.int32)
    for k, v in kw.items():
        setattr(rb, k, v)
    return rb


def coarse_tensor(spconv, rb, rows=5, shape=(4, 5, 6), batch_size=2, key="down"):
    t = spconv.SparseConvTensor(torch.zeros((rows, 4)), torch.zeros((rows, 4), dtype=torch.int32), list(shape), batch_size)
    if rb is not None:
        t.indice_dict[key] = rb
    return t


def test_constructor_state_dict_and_subclassing():
    from modest_amd.utils import spconv, spconv_inverse
    torch.manual_seed(0)
    conv = spconv_inverse.SparseInverseConv3d(16, 32, (3, 1, 1), indice_key="spconv_down2")
    assert tuple(conv.weight.shape) == (3, 1, 1, 16, 32) and tuple(conv.bias.shape) == (32,)
    assert sorted(conv.state_dict()) == ["bias", "weight"] and conv.indice_key == "spconv_down2" and conv.kernel_size == [3, 1, 1]
    nob = spconv_inverse.SparseInverseConv3d(64, 32, 3, "spconv3", False)   # spconv 1.2's positional order
    assert tuple(nob.weight.shape) == (3, 3, 3, 64, 32) and nob.bias is None and sorted(nob.state_dict()) == ["weight"]
    assert nob.indice_key == "spconv3"
    bound = 1 / np.sqrt(27 * 64)   # as SparseConvolution: kaiming_uniform_(a=sqrt(5)) with fan-in K * Cin
    assert 0.9 * bound < float(nob.weight.detach().abs().max()) <= bound
    other = spconv_inverse.SparseInverseConv3d(16, 32, (3, 1, 1), indice_key="x", use_hash=True, algo=None)
    other.load_state_dict(conv.state_dict())
    assert torch.equal(other.weight, conv.weight) and torch.equal(other.bias, conv.bias)
    assert isinstance(conv, spconv.SparseModule) and isinstance(conv, torch.nn.Module)
    for bad in (dict(in_channels=0, out_channels=4, kernel_size=3), dict(in_channels=4, out_channels=129, kernel_size=3),
                dict(in_channels=4, out_channels=4, kernel_size=8), dict(in_channels=4, out_channels=4, kernel_size=(3, 0, 3))):
        with pytest.raises(ValueError):
            spconv_inverse.SparseInverseConv3d(**bad)

    class Sub(spconv_inverse.SparseInverseConv3d):
        pass
    assert isinstance(Sub(4, 4, 3, indice_key="k"), spconv.SparseModule)
    # the same class objects under both names; what neither provides still imports and fails when called
    for name in ("SparseConvTensor", "SparseModule", "SparseSequential", "SparseConvolution", "SparseConv3d", "SubMConv3d", "utils"):
        assert getattr(spconv_inverse, name) is getattr(spconv, name)
    for name in ("SparseConvTranspose3d", "SparseMaxPool3d", "SomethingElse"):
        assert getattr(spconv_inverse, name) is getattr(spconv, name)
        with pytest.raises(NotImplementedError, match="not provided"):
            getattr(spconv_inverse, name)(1, 2)
    # modest_amd.utils.spconv itself is what it was
    with pytest.raises(NotImplementedError, match="not provided"):
        spconv.SparseInverseConv3d(1, 2, 3)
    with pytest.raises(NotImplementedError):
        spconv.SparseConvolution(3, 4, 4, 3, inverse=True)


def test_value_errors_are_raised_before_anything_touches_a_device(monkeypatch):
    from modest_amd import ops
    from modest_amd.utils import spconv_inverse as spconv
    launched = []

    def no_load():
        launched.append("load")
        raise AssertionError("a check that should have come first let the call reach the library")
    monkeypatch.setattr(ops, "load", no_load)
    conv = spconv.SparseInverseConv3d(4, 4, 3, indice_key="down")
    good = fake_rulebook()
    assert conv.rulebook_of(coarse_tensor(spconv, good)) is good
    calls = dict(ops.SPCONV_INVERSE_CALLS)
    for layer, t, match in (
            (spconv.SparseInverseConv3d(4, 4, 3), coarse_tensor(spconv, good), "needs the indice_key"),
            (spconv.SparseInverseConv3d(4, 4, 3, indice_key="other"), coarse_tensor(spconv, good), "names no rulebook"),
            (conv, coarse_tensor(spconv, None), "names no rulebook"),
            (conv, coarse_tensor(spconv, fake_rulebook(subm=True)), "submanifold"),
            (spconv.SparseInverseConv3d(4, 4, (3, 1, 1), indice_key="down"), coarse_tensor(spconv, good), "kernel"),
            (conv, coarse_tensor(spconv, good, rows=9), "rows"),
            (conv, coarse_tensor(spconv, good, rows=4), "rows"),
            (conv, coarse_tensor(spconv, good, shape=(8, 10, 12)), "spatial shape"),
            (conv, coarse_tensor(spconv, good, shape=(4, 5, 7)), "spatial shape"),
            (conv, coarse_tensor(spconv, good, batch_size=3), "batch size")):
        with pytest.raises(ValueError, match=match):
            layer(t)
    assert not launched and ops.SPCONV_INVERSE_CALLS == calls


def test_cpu_tensors_raise():
    from modest_amd import ops
    from modest_amd.utils import spconv_inverse as spconv
    rb = fake_rulebook()
    with pytest.raises(ValueError, match="device tensor"):
        spconv.SparseInverseConv3d(4, 4, 3, indice_key="down")(coarse_tensor(spconv, rb))
    with pytest.raises(ValueError, match="device tensor"):
        ops.spconv_inverse_forward(torch.zeros((5, 4)), torch.zeros((27, 4, 4)), None, rb)
    with pytest.raises(ValueError, match="device tensor"):
        ops.spconv_inverse_backward(torch.zeros((5, 4)), torch.zeros((27, 4, 4)), torch.zeros((9, 4)), rb)
    with pytest.raises(ValueError, match="device tensor"):
        ops.spconv_class_order(rb)
    with pytest.raises(ValueError, match="submanifold"):
        ops.spconv_class_order(fake_rulebook(subm=True))
    with pytest.raises(ValueError, match="order"):
        ops.spconv_inverse_forward(torch.zeros((5, 4)), torch.zeros((27, 4, 4)), None, rb, order="tiles")
    assert sorted(ops.SPCONV_INVERSE_CALLS) == ["class_order", "forward", "input_grad", "weight_grad"]
    assert sorted(ops.SPCONV_CALLS) == ["forward", "input_grad", "rulebook", "weight_grad"]
    assert ops.SPCONV_INVERSE_ORDER in ("classes", "rows") and ops.spconv_classes(rb) == 8


# ------------------------------------------------------------------------------------------------ the library
def test_entry_points_are_declared_and_mirrored():
    from modest_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "modest_hip.h")).read()
    for name, res, nargs in (("modest_spconv_class_order_workspace_bytes", "int64_t", 2), ("modest_spconv_class_order", "int", 9),
                             ("modest_spconv_gather_gemm_classes", "int", 14)):
        assert f"{res} {name}(" in hdr
        decl = hdr[hdr.rindex(f"{res} {name}("):]
        assert decl[:decl.index(";")].count(",") + 1 == nargs == len(_lib.SIGNATURES[name][1])
        assert hasattr(_lib.load(), name)


def test_new_kernels_use_no_scratch_and_the_old_files_keep_their_kernels():
    from modest_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    res = json.load(open(os.path.join(os.path.dirname(build.LIB), "kernel_resources.json")))
    mine = {k: v for k, v in res.items() if v.get("file") == "spconv_inverse.hip"}
    assert len(mine) == 6 and sum("spi_class_gemm" in k for k in mine) == 4 and not any("sp_gather_gemm" in k for k in mine)
    assert all(v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 for v in mine.values()), mine
    assert sum(v.get("file") == "spconv.hip" for v in res.values()) == 18 and sum(v.get("file") == "sort64.hip" for v in res.values()) == 4
    # the workspace is a function of the rows alone, and small
    a, b = (int(lib.modest_spconv_class_order_workspace_bytes(160_000, c)) for c in (8, 27))
    # two (key, row) buffers of 8 + 4 bytes a row and the sort's table of 256 words per 2048 rows: 24.5 bytes a row
    assert a == b and 0 < a <= 25 * 160_000
    assert int(lib.modest_spconv_class_order_workspace_bytes(0, 8)) >= 0
    assert int(lib.modest_spconv_class_order_workspace_bytes(-1, 8)) < 0 and int(lib.modest_spconv_class_order_workspace_bytes(10, 0)) < 0


# ------------------------------------------------------------------------------------------------ the binding
def test_binding_is_opt_in():
    from modest_amd.utils import pcdet_bind, spconv_utils
    from modest_amd.utils import spconv as base
    from modest_amd.utils import spconv_inverse as ours
    names = list(pcdet_bind.SHIMS) + list(pcdet_bind.STAND_INS) + ["spconv.utils", pcdet_bind.ANCHOR_TARGETS_NAME]
    saved = {k: sys.modules.get(k) for k in names}

    def clear():
        for k in list(pcdet_bind.STAND_INS) + ["spconv.utils"]:
            sys.modules.pop(k, None)
    try:
        for k in names:
            sys.modules.pop(k, None)
        keys = sorted(list(pcdet_bind.SHIMS) + list(pcdet_bind.STAND_INS))
        # the default call and sparse_conv=True: as before
        bound = pcdet_bind.install()
        assert sorted(bound) == keys and isinstance(sys.modules["spconv"], pcdet_bind.StandIn)
        bound = pcdet_bind.install(sparse_conv=True)
        assert sorted(bound) == keys and sys.modules["spconv"] is base
        # opt in: the package replaces modest_amd.utils.spconv, spconv.utils stays what it was
        bound = pcdet_bind.install(sparse_inverse=True)
        import spconv
        from spconv.utils import VoxelGeneratorV2
        assert sorted(bound) == keys and bound["spconv"] is ours and spconv is ours and sys.modules["spconv"] is ours
        assert spconv.utils is spconv_utils and sys.modules["spconv.utils"] is spconv_utils
        assert VoxelGeneratorV2 is spconv_utils.VoxelGeneratorV2
        assert isinstance(sys.modules[pcdet_bind.STAND_INS[0]], pcdet_bind.StandIn)
        assert issubclass(spconv.SparseInverseConv3d, spconv.SparseModule) and spconv.SubMConv3d is base.SubMConv3d
        assert isinstance(spconv.SparseInverseConv3d(64, 32, 3, indice_key="spconv3", bias=False), torch.nn.Module)
        # idempotent; later calls without the flag, or with sparse_conv, leave the package bound
        again = pcdet_bind.install(sparse_inverse=True)
        assert all(again[k] is bound[k] for k in bound) and sys.modules["spconv"] is ours
        assert pcdet_bind.install()["spconv"] is ours and pcdet_bind.install(sparse_conv=True)["spconv"] is ours
        assert sys.modules["spconv"] is ours and sys.modules["spconv.utils"] is spconv_utils
        # over the stand-in, and from nothing with and without the stand-ins
        clear()
        pcdet_bind.install()
        assert isinstance(sys.modules["spconv"], pcdet_bind.StandIn)
        assert pcdet_bind.install(sparse_inverse=True)["spconv"] is ours and sys.modules["spconv"] is ours
        clear()
        bound = pcdet_bind.install(stand_ins=False, sparse_inverse=True)
        assert sorted(bound) == sorted(list(pcdet_bind.SHIMS) + ["spconv"]) and sys.modules["spconv"] is ours
        assert pcdet_bind.STAND_INS[0] not in sys.modules and sys.modules["spconv.utils"] is spconv_utils
        clear()
        assert pcdet_bind.install(sparse_conv=True, sparse_inverse=True, roiaware_pool=True, anchor_targets=True)["spconv"] is ours
        # a foreign spconv is left alone
        clear()
        real = sys.modules["spconv"] = types.ModuleType("spconv")
        pcdet_bind.install(sparse_inverse=True)
        assert sys.modules["spconv"] is real and not hasattr(real, "utils") and "spconv.utils" not in sys.modules
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_the_benchmark_yardstick_computes_the_same_sums():
    """tools/spconv_inverse_bench.py's composition of stock operators (index_select -> mm -> index_add_ per offset), on
    the CPU, against the float64 restatement: inside gamma_n S whatever order it adds in."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("spconv_inverse_bench", os.path.join(ROOT, "tools", "spconv_inverse_bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    for name in ("geo_s2p1", "geo_s2p0", "c64_32_bias"):
        c = ic.get(name)
        x, w, b, dy = ic.tensors(c)
        table = ic.expected(name)[2]
        pairs = bench.compose_pairs(torch.from_numpy(table))
        got = bench.compose_forward(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b) if b is not None else None,
                                    pairs, len(c["indices"])).numpy()
        f64, S, n = inv.forward64(x, w, b, table)
        assert got.dtype == np.float32 and (np.abs(got - f64) <= seq.gamma(n) * S).all(), name
    assert [l[1:3] for l in bench.LAYERS] == [(64, 64), (64, 32), (32, 16)]
