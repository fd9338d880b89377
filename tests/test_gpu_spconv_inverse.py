"""GPU: the inverse sparse convolution (modest_amd/csrc/spconv_inverse.hip through modest_amd.ops.spconv_inverse_* and
modest_amd.utils.spconv_inverse) against the sequential restatement (tests/spconv_inverse_seq.py):
the edge families of tests/spconv_inverse_cases.py -- class order, forward on the class tiles and on the rows, feature
gradient bit for bit with no element excluded, into sentinel-filled outputs, twice; weight and bias gradients inside
gamma_n * S of the float64 sums, the weight gradient also bit for bit in the stated order over the coarse rows --,
what is launched and what is not, and an encoder-decoder chain of the layer kinds of UNetV2 against conv3d / conv_transpose3d in float64 on the CPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spconv_cases as sc  # noqa: E402
import spconv_inverse_cases as ic  # noqa: E402
import spconv_inverse_seq as inv  # noqa: E402
import spconv_seq as seq  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = 0x5A5A5A5A   # as int32 and as the float32 with these bits
U = 2.0 ** -24


@pytest.fixture(autouse=True)
def device(gpu):
    """every test here needs the device (tests/conftest.py: fails under -m gpu without one, skips on a GPU-less host)"""
    return gpu


def sentinel(shape, dtype=torch.float32):
    t = torch.full(tuple(shape), SENTINEL, dtype=torch.int32, device=DEV)
    return t if dtype == torch.int32 else t.view(torch.float32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rulebook(c):
    from modest_amd import ops
    return ops.spconv_rulebook(dev(c["indices"]), c["batch_size"], c["shape"], c["kernel"], c["stride"], c["padding"], False)


def run(c):
    """class order, forward both ways, backward on the device into sentinel-filled outputs -> dict of numpy arrays"""
    from modest_amd import ops
    x, w, b, dy = ic.tensors(c)
    rb = rulebook(c)
    xd, wd, bd, dyd = dev(x), dev(w), (dev(b) if b is not None else None), dev(dy)
    perm, class_start = ops.spconv_class_order(rb)
    outs = {}
    for order in ("classes", "rows"):
        out = sentinel((rb.n_in, c["cout"]))
        got = ops.spconv_inverse_forward(xd, wd, bd, rb, out=out, order=order)
        assert got.data_ptr() == out.data_ptr()
        outs[order] = got.cpu().numpy()
    gx = sentinel((rb.n_out, c["cin"]))
    dx, dw, db = ops.spconv_inverse_backward(xd, wd, dyd, rb, grad_input=gx)
    assert dx.data_ptr() == gx.data_ptr() and tuple(dw.shape) == tuple(wd.shape) and tuple(db.shape) == (c["cout"],)
    return dict(nbr_t=rb.nbr_t.cpu().numpy(), coarse=rb.out_indices.cpu().numpy(), perm=perm.cpu().numpy(),
                class_start=class_start.cpu().numpy(), classes=outs["classes"], rows=outs["rows"], dx=dx.cpu().numpy(),
                dw=dw.cpu().numpy(), db=db.cpu().numpy())


@pytest.mark.parametrize("name", [c["name"] for c in ic.all_cases()])
def test_device_is_the_restatement(name):
    from modest_amd import ops
    c = ic.get(name)
    c["present"](c)
    x, w, b, dy = ic.tensors(c)
    coarse, oshape, table, perm, class_start = ic.expected(name)
    want_out, want_dx = ic.expected_values(name)
    before = dict(ops.SPCONV_CALLS)
    first = run(c)
    assert ops.SPCONV_CALLS == dict(before, rulebook=before["rulebook"] + 1)   # inverse calls are counted on their own
    # the table written from the coordinates is the map the device gathers through; the class order exactly
    for key, want in (("nbr_t", table), ("coarse", coarse), ("perm", perm), ("class_start", class_start)):
        assert seq.same_bits(first[key], want), (name, key)
    # forward on the class tiles and on the rows, and the feature gradient: bit for bit, no element excluded
    for key, want in (("classes", want_out), ("rows", want_out), ("dx", want_dx)):
        assert seq.same_bits(first[key], want), (name, key, int((first[key].view(np.int32) != want.view(np.int32)).sum()))
    assert first["classes"].tobytes() == first["rows"].tobytes()
    # weight and bias gradients: inside gamma_n S of the float64 sums, n = contributing rows + 1
    (dw64, Sw, nw), (db64, Sb, nb) = inv.weight_grad64(x, dy, table)
    err = np.abs(first["dw"].astype(np.float64) - dw64)
    assert (err <= seq.gamma(nw) * Sw).all(), (name, "dw", float((err - seq.gamma(nw) * Sw).max()))
    err = np.abs(first["db"].astype(np.float64) - db64)
    assert (err <= seq.gamma(nb) * Sb).all(), (name, "db", float((err - seq.gamma(nb) * Sb).max()))
    # ... and the weight gradient bit for bit in the stated order over the coarse rows (the bias gradient is torch's sum)
    want_dw = ic.expected_weight_grad(name)
    assert seq.same_bits(first["dw"], want_dw), (name, "dw", int((first["dw"].view(np.int32) != want_dw.view(np.int32)).sum()))
    # a second run gives identical bytes for every output
    again = run(c)
    for key in first:
        assert seq.same_bits(first[key], again[key]), (name, key, "second run")


def coarse_input(c, rb, requires_grad=False, key="down"):
    from modest_amd.utils import spconv_inverse as spconv
    x = dev(ic.tensors(c)[0]).requires_grad_(requires_grad)
    t = spconv.SparseConvTensor(x, rb.out_indices, rb.out_shape, c["batch_size"])
    t.indice_dict[key] = rb
    return t


def test_what_is_launched_and_what_is_not(monkeypatch):
    from modest_amd import ops
    from modest_amd.utils import spconv_inverse as spconv
    monkeypatch.setattr(ops, "SPCONV_INVERSE_ORDER", "classes")   # the module on the class tiles, whatever the default is
    c = ic.get("c3_128_bias")
    x, w, b, dy = ic.tensors(c)
    want_out, want_dx = ic.expected_values(c["name"])
    rb = rulebook(c)
    fine = rb.indices
    conv = spconv.SparseInverseConv3d(c["cin"], c["cout"], c["kernel"], indice_key="down", bias=True).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(dev(w).view_as(conv.weight))
        conv.bias.copy_(dev(b))
    fwd, inverse = dict(ops.SPCONV_CALLS), dict(ops.SPCONV_INVERSE_CALLS)
    # the input needs no gradient: no feature-gradient launch, None handed back; the first use builds the class order
    t = coarse_input(c, rb)
    out = conv(t)
    assert out.indices is fine and out.spatial_shape == c["shape"] and out.batch_size == c["batch_size"]
    assert out.indice_dict is t.indice_dict and seq.same_bits(out.features.detach().cpu().numpy(), want_out)
    (out.features * dev(dy)).sum().backward()
    assert ops.SPCONV_INVERSE_CALLS == dict(class_order=inverse["class_order"] + 1, forward=inverse["forward"] + 1,
                                            input_grad=inverse["input_grad"], weight_grad=inverse["weight_grad"] + 1)
    assert t.features.grad is None and tuple(conv.weight.grad.shape) == tuple(conv.weight.shape)
    gw, gb = conv.weight.grad.clone(), conv.bias.grad.clone()
    direct = ops.spconv_inverse_backward(t.features, conv.weight.detach(), dev(dy), rb, need_input_grad=False)
    assert direct[0] is None and ops.SPCONV_INVERSE_CALLS["input_grad"] == inverse["input_grad"]
    assert torch.equal(direct[1], gw) and torch.equal(direct[2], gb)
    # a second inverse convolution on the rulebook, and a second pass: no class-order call; with a feature gradient now
    conv.zero_grad()
    other = spconv.SparseInverseConv3d(c["cin"], 8, c["kernel"], indice_key="down", bias=False).to(DEV)
    t = coarse_input(c, rb, requires_grad=True)
    other(t)
    out = conv(t)
    (out.features * dev(dy)).sum().backward()
    assert ops.SPCONV_INVERSE_CALLS["class_order"] == inverse["class_order"] + 1
    assert ops.SPCONV_INVERSE_CALLS["input_grad"] == inverse["input_grad"] + 1
    assert seq.same_bits(t.features.grad.cpu().numpy(), want_dx) and torch.equal(conv.weight.grad, gw)
    # none of it is a call of the forward convolutions, none builds a rulebook
    assert ops.SPCONV_CALLS == fwd
    # the errors launch nothing
    inverse = dict(ops.SPCONV_INVERSE_CALLS)
    sub = ops.spconv_rulebook(rb.out_indices, c["batch_size"], rb.out_shape, 3, 1, 0, True)
    fwd = dict(ops.SPCONV_CALLS)
    bad = coarse_input(c, rb)
    bad.indice_dict["subm"] = sub
    short = spconv.SparseConvTensor(t.features.detach()[:-1].contiguous(), rb.out_indices[:-1].contiguous(), rb.out_shape, c["batch_size"])
    short.indice_dict = bad.indice_dict
    shaped = spconv.SparseConvTensor(t.features.detach(), rb.out_indices, c["shape"], c["batch_size"])
    shaped.indice_dict = bad.indice_dict
    batched = spconv.SparseConvTensor(t.features.detach(), rb.out_indices, rb.out_shape, c["batch_size"] + 1)
    batched.indice_dict = bad.indice_dict
    for layer, tensor, match in ((spconv.SparseInverseConv3d(3, 8, 3), bad, "needs the indice_key"),
                                 (spconv.SparseInverseConv3d(3, 8, 3, indice_key="up"), bad, "names no rulebook"),
                                 (spconv.SparseInverseConv3d(3, 8, 3, indice_key="subm"), bad, "submanifold"),
                                 (spconv.SparseInverseConv3d(3, 8, (3, 3, 1), indice_key="down"), bad, "kernel"),
                                 (conv, short, "rows"), (conv, shaped, "spatial shape"), (conv, batched, "batch size")):
        with pytest.raises(ValueError, match=match):
            layer.to(DEV)(tensor)
    with pytest.raises(ValueError, match="expected"):
        ops.spconv_inverse_forward(dev(x)[:, :2].contiguous(), dev(w), None, rb)
    with pytest.raises(ValueError, match="submanifold"):
        ops.spconv_inverse_forward(dev(x), dev(w), None, sub)
    with pytest.raises(ValueError, match="device tensor"):
        ops.spconv_inverse_forward(torch.from_numpy(x), dev(w), None, rb)
    assert ops.SPCONV_INVERSE_CALLS == inverse and ops.SPCONV_CALLS == fwd


# ------------------------------------------------------------------------------------------------ the chain
CHAIN_SHAPE = [11, 16, 18]
# (kind, cin, cout, geometry, key): two levels down and up again, the layer kinds of UNetV2
CHAIN = [("subm", 4, 16, "subm", "subm1"), ("conv", 16, 32, "s2p1", "A"), ("subm", 32, 32, "subm", "subm2"),
         ("conv", 32, 64, "s2p011", "B"), ("subm", 64, 64, "subm", "subm3"), ("inv", 64, 32, "s2p011", "B"),
         ("subm", 64, 32, "subm", "subm2"), ("inv", 32, 16, "s2p1", "A")]
# unit roundoffs of an eval-mode BatchNorm element (tests/test_gpu_spconv.py): 9 u counted, 16 leaves the order free
BN_C = 16


def build_chain(spconv):
    """the eight convolutions and their BatchNorms from `import spconv` names alone, on the CPU"""
    torch.manual_seed(0)
    convs, bns = [], []
    for kind, cin, cout, geo, key in CHAIN:
        k, s, p, _ = sc.GEOMETRIES[geo]
        if kind == "subm":
            conv = spconv.SubMConv3d(cin, cout, k, padding=1, bias=False, indice_key=key)
        elif kind == "conv":
            conv = spconv.SparseConv3d(cin, cout, k, stride=s, padding=p, bias=False, indice_key=key)
        else:
            conv = spconv.SparseInverseConv3d(cin, cout, k, indice_key=key, bias=False)
        with torch.no_grad():
            # mostly positive weights on non-negative activations keep sum |w| |a| near |sum w a|, so that the propagated
            # worst-case bound stays a statement (tests/test_gpu_spconv.py); an inverse convolution sees at most 8 offsets
            taps = 4 if kind == "inv" else 6
            conv.weight.uniform_(-0.2, 1.0).mul_(1.0 / (0.4 * cin * taps))
        bn = torch.nn.BatchNorm1d(cout, eps=1e-3, momentum=0.01)
        with torch.no_grad():
            bn.running_mean.uniform_(0.0, 0.4)
            bn.running_var.uniform_(0.5, 1.5)
            bn.weight.uniform_(0.8, 1.2)
            bn.bias.uniform_(-0.1, 0.3)
        convs.append(conv)
        bns.append(bn)
    return torch.nn.ModuleList(convs), torch.nn.ModuleList(bns)


def run_chain(spconv, convs, bns, t):
    """subm -> strided A -> subm -> strided B -> subm (+= identity, as SparseBasicBlock) -> inverse(B) -> concatenate with
    the lateral features -> subm -> inverse(A); eval-mode BatchNorm and ReLU after every convolution"""
    def block(i, x):
        return spconv.SparseSequential(convs[i], bns[i], torch.nn.ReLU())(x)
    a2 = block(2, block(1, block(0, t)))
    a3 = block(3, a2)
    out = convs[4](a3)
    out.features = bns[4](out.features)
    out.features += a3.features
    out.features = torch.relu(out.features)
    a5 = block(5, out)
    assert a5.indices is a2.indices and a5.spatial_shape == a2.spatial_shape
    a5.features = torch.cat((a2.features, a5.features), dim=1)
    return block(7, block(6, a5))


def vjp(f, inputs, upstream):
    inputs = [t.detach().clone().requires_grad_(True) for t in inputs]
    return torch.autograd.grad((f(*inputs) * upstream).sum(), inputs)


def acc(D1, f1, D2, f2):
    """two gradients that autograd adds: one more rounding"""
    return D1 + D2, f1 + f2 + U * ((D1 + D2).abs() + f1 + f2)


class Twin:
    """the chain in float64 on dense tensors with the active-site masks carried, and the bound of
    test_voxel_backbone_chain_against_dense_float64 propagated forwards and backwards; an inverse convolution is
    conv_transpose3d onto its rulebook's input shape, masked to its input sites"""

    def __init__(self, convs, bns):
        self.convs, self.bns, self.steps = convs, bns, {}

    def block(self, i, A, e, imask, omask_of, residual=None):
        import torch.nn.functional as Fn
        kind, cin, cout, geo, key = CHAIN[i]
        conv, bn = self.convs[i], self.bns[i]
        k3 = seq.triple(sc.GEOMETRIES[geo][0])
        f64 = torch.float64
        if kind == "subm":
            stride, pad = (1, 1, 1), tuple(a // 2 for a in k3)
        else:
            stride, pad = seq.triple(sc.GEOMETRIES[geo][1]), seq.triple(sc.GEOMETRIES[geo][2])
        if kind == "inv":
            W = conv.weight.detach().cpu().double().permute(3, 4, 0, 1, 2).contiguous()
            target = omask_of.shape[2:]
            opad = [target[j] - ((A.shape[2 + j] - 1) * stride[j] - 2 * pad[j] + k3[j]) for j in range(3)]
            assert all(0 <= opad[j] < stride[j] for j in range(3))
            lin = lambda t, w: Fn.conv_transpose3d(t, w, stride=stride, padding=pad, output_padding=opad)
            omask = omask_of
        else:
            W = conv.weight.detach().cpu().double().permute(4, 3, 0, 1, 2).contiguous()
            lin = lambda t, w: Fn.conv3d(t, w, stride=stride, padding=pad)
            omask = imask if kind == "subm" else (Fn.conv3d(imask, torch.ones((1, 1, *k3), dtype=f64), stride=stride, padding=pad) > 0).double()
        f, fabs = (lambda t: lin(t, W)), (lambda t: lin(t, W.abs()))
        n = k3[0] * k3[1] * k3[2] * cin + 1
        Y = f(A) * omask
        ey = fabs(e + float(seq.gamma(n)) * (A.abs() + e)) * omask
        sc_ = (bn.weight.detach().cpu().double() / torch.sqrt(bn.running_var.cpu().double() + bn.eps)).view(1, -1, 1, 1, 1)
        mean, beta = bn.running_mean.cpu().double().view(1, -1, 1, 1, 1), bn.bias.detach().cpu().double().view(1, -1, 1, 1, 1)
        Z = ((Y - mean) * sc_ + beta) * omask
        ez = (sc_.abs() * ey + BN_C * U * (sc_.abs() * (Y.abs() + ey + mean.abs()) + beta.abs())) * omask
        if residual is not None:   # features += identity: one more rounding
            I, eI = residual
            Z, ez = Z + I, ez + eI + U * ((Z + I).abs() + ez + eI)
        self.steps[i] = dict(A=A, e=e, Y=Y, ey=ey, Z=Z, ez=ez, W=W, lin=lin, f=f, fabs=fabs, omask=omask, imask=imask, sc=sc_,
                             mean=mean, kvol=k3[0] * k3[1] * k3[2], cin=cin, cout=cout, residual=residual is not None)
        return torch.relu(Z), ez, omask

    def forward(self, A, mask):
        e = torch.zeros_like(A)
        a0, e0, m0 = self.block(0, A, e, mask, None)
        a1, e1, m1 = self.block(1, a0, e0, m0, None)
        a2, e2, _ = self.block(2, a1, e1, m1, None)
        a3, e3, m3 = self.block(3, a2, e2, m1, None)
        a4, e4, _ = self.block(4, a3, e3, m3, None, residual=(a3, e3))
        a5, e5, _ = self.block(5, a4, e4, m3, m1)
        a6, e6, _ = self.block(6, torch.cat((a2, a5), 1), torch.cat((e2, e5), 1), m1, None)
        return self.block(7, a6, e6, m1, m0)

    def back(self, i, D, fb, check):
        """the gradient D (bound fb) at block i's output -> at its input, and at its identity; `check` is handed every
        parameter gradient with its float64 twin and bound"""
        step, conv, bn = self.steps[i], self.convs[i], self.bns[i]
        sure = (step["Z"].abs() > step["ez"]).double()
        on = (step["Z"] > 0).double()
        fb = sure * on * fb + (1 - sure) * (D.abs() + fb)
        D = D * on
        res = (D, fb) if step["residual"] else None
        rows_out = float(step["omask"].sum())
        gamma_w = bn.weight.detach().cpu().double().view(1, -1, 1, 1, 1)
        Xn = (step["Y"] - step["mean"]) * (step["sc"] / gamma_w) * step["omask"]
        inv_ = (step["sc"] / gamma_w).abs()
        exn = (inv_ * step["ey"] + BN_C * U * inv_ * (step["Y"].abs() + step["ey"] + step["mean"].abs())) * step["omask"]
        red = lambda t: t.sum(dim=(0, 2, 3, 4))
        gn = seq.gamma(rows_out + BN_C)
        check(f"bn{i}.bias", bn.bias.grad, red(D), red(fb) + gn * red(D.abs() + fb))
        check(f"bn{i}.weight", bn.weight.grad, red(D * Xn),
              red(Xn.abs() * fb + exn * D.abs() + exn * fb) + gn * red((Xn.abs() + exn) * (D.abs() + fb)))
        fb = (step["sc"].abs() * fb + 2 * U * step["sc"].abs() * (D.abs() + fb)) * step["omask"]
        D = D * step["sc"] * step["omask"]
        # the weight gradient: at an offset the pairs are one to one, so at most min(input rows, output rows) terms
        rows = min(float(step["imask"].sum()), rows_out)
        wshape = step["W"].shape
        bil = lambda a, d: vjp(lambda w: step["lin"](a, w), [torch.zeros(wshape, dtype=torch.float64)], d)[0]
        want = bil(step["A"], D)
        bound = bil(step["A"].abs(), fb) + bil(step["e"], D.abs() + fb) + \
            float(seq.gamma(rows + 1)) * bil(step["A"].abs() + step["e"], D.abs() + fb)
        gw = conv.weight.grad.cpu().double()
        gw = gw.permute(3, 4, 0, 1, 2) if CHAIN[i][0] == "inv" else gw.permute(4, 3, 0, 1, 2)
        check(f"conv{i}.weight", gw, want, bound, says_something=True)
        n = step["kvol"] * step["cout"] + 1
        zero = torch.zeros_like(step["A"])
        Dn = vjp(step["f"], [zero], D)[0] * step["imask"]
        fb = vjp(step["fabs"], [zero], fb + float(seq.gamma(n)) * (D.abs() + fb))[0] * step["imask"]
        return Dn, fb, res

    def backward(self, D, fb, check):
        D, fb, _ = self.back(7, D, fb, check)
        D, fb, _ = self.back(6, D, fb, check)
        (Dl, D), (fl, fb) = (D[:, :32], D[:, 32:]), (fb[:, :32], fb[:, 32:])
        D, fb, _ = self.back(5, D, fb, check)
        D, fb, (Dr, fr) = self.back(4, D, fb, check)
        D, fb = acc(D, fb, Dr, fr)
        D, fb, _ = self.back(3, D, fb, check)
        D, fb = acc(D, fb, Dl, fl)
        D, fb, _ = self.back(2, D, fb, check)
        D, fb, _ = self.back(1, D, fb, check)
        self.back(0, D, fb, check)


def chain_inputs():
    idx = sc.random_sites(7, 600, 2, CHAIN_SHAPE)
    feats = np.random.default_rng(8).uniform(0.0, 1.0, (len(idx), 4)).astype(np.float32)
    G = np.random.default_rng(9).standard_normal((2, 16, *CHAIN_SHAPE)).astype(np.float32)
    return idx, feats, G


def dense_inputs(idx, feats):
    i = torch.from_numpy(idx.astype(np.int64))
    A = torch.zeros([2, *CHAIN_SHAPE, 4], dtype=torch.float64)
    A[i[:, 0], i[:, 1], i[:, 2], i[:, 3]] = torch.from_numpy(feats).double()
    mask = torch.zeros([2, 1, *CHAIN_SHAPE], dtype=torch.float64)
    mask[i[:, 0], 0, i[:, 1], i[:, 2], i[:, 3]] = 1
    return A.permute(0, 4, 1, 2, 3).contiguous(), mask


def test_encoder_decoder_chain_against_dense_float64():
    """Two levels down and up again on ~600 voxels, built from `import spconv` names after install(sparse_inverse=True).
    The tolerance is the per-layer bound of test_voxel_backbone_chain_against_dense_float64 propagated through the
    graph: an inverse convolution is bounded like a convolution (n = K Cin + 1 forwards, K Cout + 1 backwards, at most
    min(input rows, output rows) + 1 terms in a weight gradient element); `features += identity` and every sum of two
    gradients that autograd forms add one rounding, u (|sum| + both bounds); the concatenation is exact."""
    from modest_amd import ops
    from modest_amd.utils import pcdet_bind
    from modest_amd.utils import spconv_inverse as ours
    names = list(pcdet_bind.SHIMS) + list(pcdet_bind.STAND_INS) + ["spconv.utils"]
    saved = {k: sys.modules.get(k) for k in names}
    try:
        pcdet_bind.install(sparse_inverse=True)
        import spconv
        assert spconv is ours
        convs, bns = build_chain(spconv)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    idx, feats, G = chain_inputs()
    convs, bns = convs.to(DEV).eval(), bns.to(DEV).eval()
    t = spconv.SparseConvTensor(dev(feats), dev(idx), CHAIN_SHAPE, 2)
    fwd, inverse = dict(ops.SPCONV_CALLS), dict(ops.SPCONV_INVERSE_CALLS)
    out = run_chain(spconv, convs, bns, t)
    # it ends on the first level's sites: the very tensor the input carried
    assert out.indices is t.indices and out.spatial_shape == CHAIN_SHAPE and out.indice_dict is t.indice_dict
    assert sorted(t.indice_dict) == ["A", "B", "subm1", "subm2", "subm3"]
    assert ops.SPCONV_CALLS["rulebook"] == fwd["rulebook"] + 5 and ops.SPCONV_CALLS["forward"] == fwd["forward"] + 6
    assert ops.SPCONV_INVERSE_CALLS["forward"] == inverse["forward"] + 2
    assert ops.SPCONV_INVERSE_CALLS["class_order"] == inverse["class_order"] + (2 if ops.SPCONV_INVERSE_ORDER == "classes" else 0)
    dense = out.dense()
    (dense * dev(G)).sum().backward()
    assert ops.SPCONV_INVERSE_CALLS["input_grad"] == inverse["input_grad"] + 2 and ops.SPCONV_CALLS["input_grad"] == fwd["input_grad"] + 5

    convs, bns = convs.cpu(), bns.cpu()
    twin = Twin(convs, bns)
    A0, mask = dense_inputs(idx, feats)
    A, e, omask = twin.forward(A0, mask)
    assert torch.equal(omask, mask)
    got = dense.detach().cpu().double()
    err = (got - A).abs()
    print(f"chain forward: max |dense| {float(A.abs().max()):.4g}, max error {float(err.max()):.3g}, max bound {float(e.max()):.3g}")
    assert got.shape == A.shape and (err <= e).all(), ("forward", float((err - e).max()))
    assert float(e.max()) < 0.05 * float(A.abs().max()) and float(A.abs().max()) > 0.1   # the bound says something
    assert int((got != 0).sum()) > 100

    def check(name, grad, want, bound, says_something=False):
        err = (grad.cpu().double() - want).abs()
        print(f"chain {name}: max |gradient| {float(want.abs().max()):.4g}, max error {float(err.max()):.3g}, max bound {float(bound.max()):.3g}")
        assert (err <= bound).all(), (name, float((err - bound).max()))
        if says_something:
            assert float(bound.max()) < 0.05 * float(want.abs().max()), name
    twin.backward(torch.from_numpy(G).double() * mask, torch.zeros_like(A), check)
    assert t.features.grad is None
