"""GPU: the sparse 3-D convolutions (modest_amd/csrc/spconv.hip through modest_amd.ops.spconv_* and the modules of
modest_amd.utils.spconv) against the sequential restatement (tests/spconv_seq.py): the edge
families of tests/spconv_cases.py, rulebook and forward and feature gradient bit for bit with no element excluded, into
sentinel-filled outputs, twice; the weight and bias gradients inside gamma_n * S of the float64 sums and bit for bit in
the stated order of segments and rows, up to and past the cap of 32 segments; and the layer
sequence of VoxelBackBone8x against torch.nn.Conv3d in float64 on the CPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spconv_cases as sc  # noqa: E402
import spconv_seq as seq  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = 0x5A5A5A5A   # as int32 and as the float32 with these bits
U = 2.0 ** -24


@pytest.fixture(autouse=True)
def device(gpu):
    """every test here needs the device (tests/conftest.py: fails under -m gpu without one, skips on a GPU-less host)"""
    return gpu


def sentinel(shape):
    return torch.full(tuple(shape), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(c):
    """rulebook, forward, backward on the device into sentinel-filled outputs -> dict of numpy arrays"""
    from modest_amd import ops
    x, w, b, dy = sc.tensors(c)
    rb = ops.spconv_rulebook(dev(c["indices"]), c["batch_size"], c["shape"], c["kernel"], c["stride"], c["padding"], c["subm"])
    K = rb.kvol
    xd, wd, bd, dyd = dev(x), dev(w), (dev(b) if b is not None else None), dev(dy)
    out = sentinel((rb.n_out, c["cout"]))
    got = ops.spconv_forward(xd, wd, bd, rb, out=out)
    assert got.data_ptr() == out.data_ptr()
    gx, gw, gb = sentinel((rb.n_in, c["cin"])), sentinel((K, c["cin"], c["cout"])), sentinel((c["cout"],))
    dx, dw, db = ops.spconv_backward(xd, wd, dyd, rb, grad_input=gx, grad_weight=gw, grad_bias=gb)
    assert dx.data_ptr() == gx.data_ptr() and dw.data_ptr() == gw.data_ptr() and db.data_ptr() == gb.data_ptr()
    return dict(out_indices=rb.out_indices.cpu().numpy(), out_shape=np.asarray(rb.out_shape), nbr=rb.nbr.cpu().numpy(),
                nbr_t=rb.nbr_t.cpu().numpy(), out=got.cpu().numpy(), dx=dx.cpu().numpy(), dw=dw.cpu().numpy(), db=db.cpu().numpy())


@pytest.mark.parametrize("name", [c["name"] for c in sc.all_cases()])
def test_device_is_the_restatement(name):
    c = sc.get(name)
    c["present"](c)
    x, w, b, dy = sc.tensors(c)
    out_idx, out_shape, nbr, nbr_t = sc.expected(name)
    want_out, want_dx = sc.expected_values(name)
    first = run(c)
    # output sites, output shape and both maps: exactly and in order
    assert first["out_shape"].tolist() == out_shape
    for key, want in (("out_indices", out_idx), ("nbr", nbr), ("nbr_t", nbr_t)):
        assert seq.same_bits(first[key], want), (name, key)
    # forward and feature gradient: bit for bit, no element excluded
    assert seq.same_bits(first["out"], want_out), (name, "forward", int((first["out"].view(np.int32) != want_out.view(np.int32)).sum()))
    assert seq.same_bits(first["dx"], want_dx), (name, "dx", int((first["dx"].view(np.int32) != want_dx.view(np.int32)).sum()))
    # weight and bias gradients: inside gamma_n S of the float64 sums, n = contributing rows + 1
    (dw64, Sw, nw), (db64, Sb, nb) = seq.weight_grad64(x, dy, nbr)
    err = np.abs(first["dw"].astype(np.float64) - dw64)
    assert (err <= seq.gamma(nw) * Sw).all(), (name, "dw", float((err - seq.gamma(nw) * Sw).max()))
    err = np.abs(first["db"].astype(np.float64) - db64)
    assert (err <= seq.gamma(nb) * Sb).all(), (name, "db", float((err - seq.gamma(nb) * Sb).max()))
    # ... and bit for bit in the stated order of segments and rows, no element excluded
    want_dw, want_db = sc.expected_grads(name)
    assert seq.same_bits(first["dw"], want_dw), (name, "dw", int((first["dw"].view(np.int32) != want_dw.view(np.int32)).sum()))
    assert seq.same_bits(first["db"], want_db), (name, "db", int((first["db"].view(np.int32) != want_db.view(np.int32)).sum()))
    # a second run gives identical bytes for every output
    again = run(c)
    for key in first:
        assert seq.same_bits(first[key], again[key]), (name, key, "second run")


def test_bad_rows_raise_and_produce_nothing():
    from modest_amd import ops
    c = sc.get("batch2_s2p1")
    good = c["indices"]
    calls = dict(ops.SPCONV_CALLS)
    for bad, match in ((np.concatenate([good, good[7:8]]), "duplicate"),
                       (np.concatenate([good[:5], good[:1], good[5:]]), "duplicate"),
                       (np.concatenate([good, [[2, 0, 0, 0]]]).astype(np.int32), "outside"),
                       (np.concatenate([good, [[0, c["shape"][0], 0, 0]]]).astype(np.int32), "outside"),
                       (np.concatenate([good, [[0, 0, 0, c["shape"][2]]]]).astype(np.int32), "outside"),
                       (np.concatenate([[[0, 0, -1, 0]], good]).astype(np.int32), "outside")):
        for subm in (False, True):
            with pytest.raises(Exception, match=match):
                ops.spconv_rulebook(dev(bad), c["batch_size"], c["shape"], 3, 2, 1, subm)
    assert ops.SPCONV_CALLS["rulebook"] == calls["rulebook"] + 12 and ops.SPCONV_CALLS["forward"] == calls["forward"]
    # ... and a good call works afterwards
    rb = ops.spconv_rulebook(dev(good), c["batch_size"], c["shape"], c["kernel"], c["stride"], c["padding"], c["subm"])
    assert seq.same_bits(rb.out_indices.cpu().numpy(), sc.expected(c["name"])[0])
    with pytest.raises(ValueError, match="output shape"):
        ops.spconv_rulebook(dev(good[:0]), 1, [2, 10, 12], 3, 1, 0, False)
    with pytest.raises(ValueError):
        ops.spconv_rulebook(dev(good)[:, :3].contiguous(), 2, c["shape"], 3, 1, 0, True)
    with pytest.raises(TypeError):
        ops.spconv_rulebook(dev(good).long(), 2, c["shape"], 3, 1, 0, True)


def sparse_input(c, requires_grad=False):
    from modest_amd.utils import spconv
    x = dev(sc.tensors(c)[0]).requires_grad_(requires_grad)
    return spconv.SparseConvTensor(x, dev(c["indices"]), c["shape"], c["batch_size"])


def test_rulebook_is_shared_under_an_indice_key(monkeypatch):
    from modest_amd import ops
    from modest_amd.utils import spconv
    c = sc.get("batch3_subm")
    built = []
    real = ops.spconv_rulebook
    monkeypatch.setattr(ops, "spconv_rulebook", lambda *a, **k: built.append(a) or real(*a, **k))
    torch.manual_seed(1)
    net = spconv.SparseSequential(spconv.SubMConv3d(4, 16, 3, padding=1, bias=False, indice_key="subm1"), torch.nn.ReLU(),
                                  spconv.SubMConv3d(16, 16, 3, padding=1, bias=False, indice_key="subm1"),
                                  spconv.SparseConv3d(16, 8, 3, stride=2, padding=1, indice_key="spconv2"),
                                  spconv.SubMConv3d(8, 8, 3, indice_key="subm2"), spconv.SubMConv3d(8, 8, 3, indice_key="subm2")).to(DEV)
    t = sparse_input(c)
    out = net(t)
    assert len(built) == 3 and sorted(t.indice_dict) == ["spconv2", "subm1", "subm2"] and out.indice_dict is t.indice_dict
    assert out.find_indice_pair("subm1").out_indices is t.indices      # a submanifold result carries the same indices tensor
    assert out.indices is t.find_indice_pair("spconv2").out_indices and out.spatial_shape == [4, 5, 6]
    # a convolution that finds its rulebook makes no rulebook call (and with it no synchronise)
    before = ops.SPCONV_CALLS["rulebook"]
    spconv.SubMConv3d(4, 4, 3, indice_key="subm1").to(DEV)(t)
    assert ops.SPCONV_CALLS["rulebook"] == before and len(built) == 3
    # a key reused with another geometry raises
    for other in (spconv.SubMConv3d(4, 4, (3, 1, 1), indice_key="subm1"), spconv.SparseConv3d(4, 4, 3, stride=2, padding=1, indice_key="subm1"),
                  spconv.SparseConv3d(16, 4, 3, stride=2, padding=0, indice_key="spconv2"),
                  spconv.SparseConv3d(16, 4, 3, stride=1, padding=1, indice_key="spconv2")):
        with pytest.raises(ValueError, match="indice_key"):
            other.to(DEV)(with_dict(t, other.in_channels))
    # ... and so does the same key on another input shape
    small = spconv.SparseConvTensor(t.features, t.indices, [9, 10, 12], t.batch_size)
    small.indice_dict = t.indice_dict
    with pytest.raises(ValueError, match="indice_key"):
        net[0](small)


def with_dict(t, channels):
    from modest_amd.utils import spconv
    s = spconv.SparseConvTensor(t.features.new_zeros((len(t.indices), channels)), t.indices, t.spatial_shape, t.batch_size)
    s.indice_dict = t.indice_dict
    return s


def test_module_gradients_and_no_feature_gradient_when_not_needed():
    from modest_amd import ops
    from modest_amd.utils import spconv
    c = sc.get("c3_16_s2p1")
    x, w, b, dy = sc.tensors(c)
    out_idx, out_shape, nbr, nbr_t = sc.expected(c["name"])
    want_out, want_dx = sc.expected_values(c["name"])
    conv = spconv.SparseConv3d(c["cin"], c["cout"], c["kernel"], stride=c["stride"], padding=c["padding"], bias=c["bias"],
                             indice_key="down").to(DEV)
    with torch.no_grad():
        conv.weight.copy_(dev(w).view_as(conv.weight))
        if c["bias"]:
            conv.bias.copy_(dev(b))
    # the input does not require grad (the first layer's voxel features): no feature-gradient launch, None handed back
    before = dict(ops.SPCONV_CALLS)
    t = sparse_input(c, requires_grad=False)
    out = conv(t)
    (out.features * dev(dy)).sum().backward()
    assert ops.SPCONV_CALLS["input_grad"] == before["input_grad"] and ops.SPCONV_CALLS["weight_grad"] == before["weight_grad"] + 1
    assert t.features.grad is None and seq.same_bits(out.features.detach().cpu().numpy(), want_out)
    direct = ops.spconv_backward(t.features, conv.weight.detach(), dev(dy), out.find_indice_pair("down"), need_input_grad=False)
    assert direct[0] is None and ops.SPCONV_CALLS["input_grad"] == before["input_grad"]
    gw = conv.weight.grad.clone()
    assert tuple(gw.shape) == tuple(conv.weight.shape) and torch.equal(gw, direct[1])
    want_dw, want_db = sc.expected_grads(c["name"])
    assert seq.same_bits(gw.cpu().numpy(), want_dw.reshape(tuple(conv.weight.shape)))   # the module's gradient is the restatement's
    if c["bias"]:
        assert seq.same_bits(conv.bias.grad.cpu().numpy(), want_db)
    # with a feature gradient: through dense(), which autograd differentiates
    conv.zero_grad()
    t = sparse_input(c, requires_grad=True)
    out = conv(t)
    dense = out.dense()
    assert tuple(dense.shape) == (c["batch_size"], c["cout"], *out_shape)
    g = torch.zeros_like(dense)
    idx = torch.from_numpy(out_idx.astype(np.int64)).to(DEV)
    g[idx[:, 0], :, idx[:, 1], idx[:, 2], idx[:, 3]] = dev(dy)
    (dense * g).sum().backward()
    assert ops.SPCONV_CALLS["input_grad"] == before["input_grad"] + 1
    assert seq.same_bits(t.features.grad.cpu().numpy(), want_dx) and torch.equal(conv.weight.grad, gw)
    last = out.dense(channels_first=False)
    assert torch.equal(last.permute(0, 4, 1, 2, 3), dense) and int((dense != 0).sum()) <= out_idx.shape[0] * c["cout"]


# ------------------------------------------------------------------------------------------------ the chain
CHAIN_SHAPE = [41, 64, 72]
CHAIN_RANGE = [0, -1.6, -3, 3.6, 1.6, 1.1]
CHAIN_VOXEL = [0.05, 0.05, 0.1]
# (kind, cin, cout, kernel, stride, padding, key): the layer sequence of VoxelBackBone8x
CHAIN = [("subm", 4, 16, 3, 1, 1, "subm1"), ("subm", 16, 16, 3, 1, 1, "subm1"),
         ("conv", 16, 32, 3, 2, 1, "spconv2"), ("subm", 32, 32, 3, 1, 1, "subm2"), ("subm", 32, 32, 3, 1, 1, "subm2"),
         ("conv", 32, 64, 3, 2, 1, "spconv3"), ("subm", 64, 64, 3, 1, 1, "subm3"), ("subm", 64, 64, 3, 1, 1, "subm3"),
         ("conv", 64, 64, 3, 2, (0, 1, 1), "spconv4"), ("subm", 64, 64, 3, 1, 1, "subm4"), ("subm", 64, 64, 3, 1, 1, "subm4"),
         ("conv", 64, 128, (3, 1, 1), (2, 1, 1), 0, "spconv_down2")]
# unit roundoffs of an eval-mode BatchNorm element: var + eps, a reciprocal square root (<= 2 ulp = 4 u), x - mean, the products with
# it and with the weight, the sum with the bias: 9 u; 16 leaves the library its choice of the order of these steps
BN_C = 16


def chain_cloud(seed, n_ground, n_wall):
    rng = np.random.default_rng(seed)
    g = np.stack([rng.uniform(0, 3.6, n_ground), rng.uniform(-1.6, 1.6, n_ground), -1.5 + 0.05 * rng.standard_normal(n_ground)], 1)
    wl = np.stack([1.8 + 0.03 * rng.standard_normal(n_wall), rng.uniform(-1.0, 1.0, n_wall), rng.uniform(-1.5, 0.9, n_wall)], 1)
    pts = np.concatenate([g, wl])
    return np.concatenate([pts, rng.uniform(0, 1, (len(pts), 1))], 1).astype(np.float32)[rng.permutation(len(pts))]


def vjp(f, inputs, upstream):
    """gradients of sum(f(*inputs) * upstream) w.r.t. the inputs (float64, CPU)"""
    inputs = [t.detach().clone().requires_grad_(True) for t in inputs]
    return torch.autograd.grad((f(*inputs) * upstream).sum(), inputs)


def test_voxel_backbone_chain_against_dense_float64():
    """The layer sequence of VoxelBackBone8x on ~4 000 voxels, BatchNorm1d (eval mode, fixed statistics) and ReLU between
    the convolutions, dense() at the end and a linear loss; against the same chain of torch.nn.functional.conv3d in float64
    on the CPU with the active-site masks carried layer by layer.

    The tolerance is the per-layer bound propagated.  Write a for a device value, A for its float64 twin and e >= |a - A|.
      convolution  y = sum w a in the contract's order: |y - Y| <= sum |w| e + gamma_n sum |w| (|A| + e), n = K Cin + 1
      BatchNorm    y = s a + t with s = g / sqrt(var + eps), t = b - mean s (fixed): |y - Y| <= |s| e + BN_C u (|s| (|A| + e + |mean|) + |b|)
      ReLU, masks, dense(): 1-Lipschitz or exact, e passes through.
    Backwards, with upstream gradient d (float64 twin D, bound f):
      feature gradient: the same as the convolution with the transposed weights, n = K Cout + 1
      weight gradient  sum a d: sum (|A| f + e |D| + e f) + gamma_(rows + 1) sum (|A| + e) (|D| + f)
      BatchNorm        dx = s d: |s| f + 2 u |s| (|D| + f); its own gradients are sums over the rows of d and of d xn, bounded
                       like the weight gradient with n = rows + BN_C
      ReLU             passes d where the pre-activation is positive; where |pre-activation| <= e the two sides may
                       disagree about the sign and the bound becomes |D| + f.
    """
    import torch.nn.functional as Fn
    from modest_amd import ops
    from modest_amd.utils import spconv
    pts = [chain_cloud(1, 1700, 600), chain_cloud(2, 1400, 850)]
    stacked = np.concatenate([np.concatenate([np.full((len(p), 1), b, np.float32), p], 1) for b, p in enumerate(pts)])
    vox, coords, num, _, counts = ops.voxelize(dev(stacked), CHAIN_VOXEL, CHAIN_RANGE, 5, 16000, batch_size=2)
    assert 3000 <= len(coords) <= 5000 and (counts > 1000).all(), counts
    feats = (vox.sum(1) / num.float()[:, None]).contiguous()   # MeanVFE
    torch.manual_seed(0)
    layers, bns = [], []
    for kind, cin, cout, k, s, p, key in CHAIN:
        cls = spconv.SubMConv3d if kind == "subm" else spconv.SparseConv3d
        conv = cls(cin, cout, k, stride=s, padding=p, bias=False, indice_key=key)
        with torch.no_grad():
            # Mostly positive weights on non-negative activations: sum |w| |a| stays within 1.1 of |sum w a|, so the
            # propagated worst-case bound grows by that factor per layer, not by the sqrt(K Cin) ~ 40 of centred weights
            # (1.4e9 after twelve layers: a bound that says nothing).  Scaled to keep the activations near 1.
            conv.weight.uniform_(-0.2, 1.0).mul_(1.0 / (0.4 * cin * min(conv.weight[..., 0, 0].numel(), 6)))
        bn = torch.nn.BatchNorm1d(cout, eps=1e-3, momentum=0.01)
        with torch.no_grad():
            bn.running_mean.uniform_(0.0, 0.4)
            bn.running_var.uniform_(0.5, 1.5)
            bn.weight.uniform_(0.8, 1.2)
            bn.bias.uniform_(-0.1, 0.3)
        layers.append(conv)
        bns.append(bn)
    net = spconv.SparseSequential(*[spconv.SparseSequential(c, b, torch.nn.ReLU()) for c, b in zip(layers, bns)]).to(DEV).eval()
    before = dict(ops.SPCONV_CALLS)
    out = net(spconv.SparseConvTensor(feats, coords, CHAIN_SHAPE, 2))
    assert out.spatial_shape == [2, 8, 9] and ops.SPCONV_CALLS["rulebook"] == before["rulebook"] + 8
    dense = out.dense()
    G = torch.from_numpy(np.random.default_rng(3).standard_normal(tuple(dense.shape)).astype(np.float32))
    (dense * G.to(DEV)).sum().backward()
    assert ops.SPCONV_CALLS["input_grad"] == before["input_grad"] + 11   # not for the first layer

    # ---- the float64 twin with its error bounds, layer by layer
    f64 = torch.float64
    idx = coords.long().cpu()
    A = torch.zeros([2, *CHAIN_SHAPE, 4], dtype=f64)
    A[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]] = feats.cpu().double()
    A = A.permute(0, 4, 1, 2, 3).contiguous()
    mask = torch.zeros([2, 1, *CHAIN_SHAPE], dtype=f64)
    mask[idx[:, 0], 0, idx[:, 1], idx[:, 2], idx[:, 3]] = 1
    e = torch.zeros_like(A)
    tape = []
    for (kind, cin, cout, k, s, p, key), conv, bn in zip(CHAIN, layers, bns):
        k3 = seq.triple(k)
        stride, pad = ((1, 1, 1), tuple(a // 2 for a in k3)) if kind == "subm" else (seq.triple(s), seq.triple(p))
        W = conv.weight.detach().cpu().double().permute(4, 3, 0, 1, 2).contiguous()
        f = lambda t, w=W, stride=stride, pad=pad: Fn.conv3d(t, w, stride=stride, padding=pad)
        fabs = lambda t, w=W.abs(), stride=stride, pad=pad: Fn.conv3d(t, w, stride=stride, padding=pad)
        omask = mask if kind == "subm" else (Fn.conv3d(mask, torch.ones((1, 1, *k3), dtype=f64), stride=stride, padding=pad) > 0).double()
        n = k3[0] * k3[1] * k3[2] * cin + 1
        Y = f(A) * omask
        ey = fabs(e + float(seq.gamma(n)) * (A.abs() + e)) * omask   # (one convolution: the bound is linear in its inputs)
        sc_ = (bn.weight.detach().cpu().double() / torch.sqrt(bn.running_var.cpu().double() + bn.eps)).view(1, -1, 1, 1, 1)
        mean, beta = bn.running_mean.cpu().double().view(1, -1, 1, 1, 1), bn.bias.detach().cpu().double().view(1, -1, 1, 1, 1)
        Z = ((Y - mean) * sc_ + beta) * omask
        ez = (sc_.abs() * ey + BN_C * U * (sc_.abs() * (Y.abs() + ey + mean.abs()) + beta.abs())) * omask
        tape.append(dict(A=A, e=e, Y=Y, ey=ey, Z=Z, ez=ez, W=W, f=f, fabs=fabs, omask=omask, imask=mask, sc=sc_, mean=mean, kdims=k3,
                         stride=stride, pad=pad, cin=cin, cout=cout))
        A, e, mask = torch.relu(Z), ez, omask
    got = dense.detach().cpu().double()
    assert got.shape == A.shape
    err = (got - A).abs()
    print(f"chain forward: max |dense| {float(A.abs().max()):.4g}, max error {float(err.max()):.3g}, max bound {float(e.max()):.3g}")
    assert (err <= e).all(), ("forward", float((err - e).max()))
    assert float(e.max()) < 0.05 * float(A.abs().max()) and float(A.abs().max()) > 0.1   # the bound says something
    assert int((got != 0).sum()) > 100

    D, fb = G.double() * mask, torch.zeros_like(A)
    for step, conv, bn in zip(tape[::-1], layers[::-1], bns[::-1]):
        # ReLU
        sure = (step["Z"].abs() > step["ez"]).double()
        on = (step["Z"] > 0).double()
        fb = sure * on * fb + (1 - sure) * (D.abs() + fb)
        D = D * on
        # BatchNorm (eval): its own gradients, then dx = s d
        rows = float(step["omask"].sum())
        Xn = (step["Y"] - step["mean"]) * (step["sc"] / bn.weight.detach().cpu().double().view(1, -1, 1, 1, 1)) * step["omask"]
        inv = (step["sc"] / bn.weight.detach().cpu().double().view(1, -1, 1, 1, 1)).abs()
        exn = (inv * step["ey"] + BN_C * U * inv * (step["Y"].abs() + step["ey"] + step["mean"].abs())) * step["omask"]
        red = lambda t: t.sum(dim=(0, 2, 3, 4))
        gn = seq.gamma(rows + BN_C)
        for name, want, bound in (("bias", red(D), red(fb) + gn * red(D.abs() + fb)),
                                  ("weight", red(D * Xn), red(Xn.abs() * fb + exn * D.abs() + exn * fb) + gn * red((Xn.abs() + exn) * (D.abs() + fb)))):
            err = (getattr(bn, name).grad.cpu().double() - want).abs()
            assert (err <= bound).all(), ("BatchNorm", name, step["cout"], float((err - bound).max()))
        fb = (step["sc"].abs() * fb + 2 * U * step["sc"].abs() * (D.abs() + fb)) * step["omask"]
        D = D * step["sc"] * step["omask"]
        # the convolution's weight gradient
        wshape = step["W"].shape
        bil = lambda a, d: vjp(lambda w: Fn.conv3d(a, w, stride=step["stride"], padding=step["pad"]), [torch.zeros(wshape, dtype=f64)], d)[0]
        want = bil(step["A"], D)
        bound = bil(step["A"].abs(), fb) + bil(step["e"], D.abs() + fb) + \
            float(seq.gamma(rows + 1)) * bil(step["A"].abs() + step["e"], D.abs() + fb)
        gw = conv.weight.grad.cpu().double().permute(4, 3, 0, 1, 2)
        err = (gw - want).abs()
        print(f"chain weight gradient {step['cin']}->{step['cout']}: max |dw| {float(want.abs().max()):.4g}, max error {float(err.max()):.3g}, "
              f"max bound {float(bound.max()):.3g}")
        assert (err <= bound).all(), ("weight gradient", step["cin"], step["cout"], float((err - bound).max()))
        assert float(bound.max()) < 0.05 * float(want.abs().max())
        # the feature gradient
        n = step["kdims"][0] * step["kdims"][1] * step["kdims"][2] * step["cout"] + 1
        zero = torch.zeros_like(step["A"])
        Dn = vjp(step["f"], [zero], D)[0] * step["imask"]
        fb = vjp(step["fabs"], [zero], fb + float(seq.gamma(n)) * (D.abs() + fb))[0] * step["imask"]
        D = Dn
    assert layers[0].weight.grad is not None and feats.grad is None
