"""GPU: the PillarVFE and BEV scatter kernels (csrc/pillar_vfe.hip) against the numpy restatement
tests/pillar_vfe_seq.py BIT FOR BIT -- every element of out, the winners, the float64 sums, mean32 / invstd32, the running
buffers, dW, dgamma, dbeta, the canvas and the features' gradient -- on the recorded scenes (tests/golden/pillar_vfe.npz) and
the named cases (tests/pillar_vfe_cases.py), through the ops into sentinel-filled outputs and through the two drop-in forward
methods on minimal stand-in modules with autograd; inputs unchanged, the same bits on a second call, eval mode changes no buffer,
rows of the scatter out of range by one on each side inside a padded sentinel buffer, no host synchronisation, one mid-size run,
and the refusals of the modules, the ops and the library, one step past each limit.  A mismatch reports the element."""
import os
import warnings

import numpy as np
import pytest
import torch

import pillar_vfe_seq as seq
from pillar_vfe_cases import CASES, mid, out_of_range_coords
from modest_amd import ops

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pillar_vfe.npz")
F = np.float32
SENTINEL = 0x5A5A5A5A
_restated = {}


@pytest.fixture(scope="module")
def gold():
    return {name: (case, rec) for name, case, rec in seq.scenes(dict(np.load(GOLD)))}


def restated(key, case):
    """the restatement of a case -- the last forward of its steps, its backward, the canvas and the features' gradient --
    computed once and left unchanged"""
    if key not in _restated:
        fwd = seq.restate_steps(case)
        res = dict(fwd)
        if case["training"]:
            res["dW"], res["dgamma"], res["dbeta"] = seq.restate_backward(case, fwd, case["grad"])
        res["canvas"] = seq.scatter(fwd["out"], case["coords"], case["batch_size"], case["ny"], case["nx"])
        _restated[key] = res
    return _restated[key]


def filled(shape, dtype, gpu):
    """a tensor of the shape and dtype whose every 32-bit word is the sentinel"""
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    raw = torch.full(((nbytes + 7) // 8 * 2,), SENTINEL, dtype=torch.int32, device=gpu)
    return raw.view(torch.uint8)[:nbytes].view(dtype).view(shape)


def to(a, gpu):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def geometry(case):
    return dict(voxel_size=case["voxel_size"], offsets=case["offsets"], parts=case["parts"])


def through_ops(case, gpu, sentinel=True):
    """the steps of a case through ops.pillar_vfe (+ backward, scatter, scatter backward) -> dict of numpy results"""
    P, S, Cp = case["voxels"].shape
    C, K = case["W"].shape
    Q = 2 * C + K * C + K
    train = case["training"]
    ins = [to(case[k], gpu) for k in ("voxels", "num", "coords", "W", "gamma", "beta")]
    rm, rv = to(case["running_mean"], gpu), to(case["running_var"], gpu)
    tracked = torch.tensor(int(case.get("tracked", 0)), dtype=torch.int64, device=gpu)
    before = [t.clone() for t in ins]
    for _ in range(case["steps"]):
        out = None
        if sentinel:
            out = (filled((P, C), torch.float32, gpu), filled((P, C), torch.uint8, gpu) if train else None,
                   filled((Q,), torch.float64, gpu) if train else None, filled((2, C), torch.float32, gpu) if train else None)
        feat, winner, sums, stat = ops.pillar_vfe(*ins, rm, rv, tracked, eps=case["eps"], momentum=case["momentum"], training=train,
                                                  out=out, **geometry(case))
        assert out is None or feat is out[0]
    res = dict(out=feat, winner=winner, sums=sums, stat=stat, running_mean=rm, running_var=rv)
    if train:
        grad = to(case["grad"], gpu)
        gout = (filled((C, K), torch.float32, gpu), filled((C,), torch.float32, gpu), filled((C,), torch.float32, gpu)) if sentinel else None
        res["dW"], res["dgamma"], res["dbeta"] = ops.pillar_vfe_backward(*ins[:5], feat, winner, grad, sums, stat, out=gout, **geometry(case))
    B, ny, nx = case["batch_size"], case["ny"], case["nx"]
    res["canvas"] = ops.pillar_scatter(feat, ins[2], B, ny, nx, out=filled((B, C, ny, nx), torch.float32, gpu) if sentinel else None)
    G = to(seq.grad_canvas_of(case), gpu)
    res["grad_feat"] = ops.pillar_scatter_backward(G, ins[2], out=filled((P, C), torch.float32, gpu) if sentinel else None)
    for a, b in zip(ins, before):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))          # inputs are left untouched
    res = {k: None if v is None else v.cpu().numpy() for k, v in res.items()}
    res["tracked"] = int(tracked.item())
    return res


def through_modules(case, gpu):
    """the steps of a case through the two bound forward methods and autograd -> dict of numpy results"""
    vfe, sc, batch = seq.bare_modules(case, gpu)
    pfn = vfe.pfn_layers[0]
    keys = sorted(vfe.state_dict())
    train = case["training"]
    with torch.enable_grad() if train else torch.no_grad():
        for _ in range(case["steps"]):
            bd = vfe(dict(batch))
        feats = bd["pillar_features"]
        assert tuple(feats.shape) == (case["voxels"].shape[0], case["W"].shape[0]) and feats.requires_grad == train
        if train:
            feats.retain_grad()
        canvas = sc(bd)["spatial_features"]
        res = dict(out=feats, canvas=canvas, running_mean=pfn.norm.running_mean, running_var=pfn.norm.running_var)
        if train:
            (canvas * to(seq.grad_canvas_of(case), gpu)).sum().backward()
            res.update(dW=pfn.linear.weight.grad, dgamma=pfn.norm.weight.grad, dbeta=pfn.norm.bias.grad, grad_feat=feats.grad)
    assert sorted(vfe.state_dict()) == keys                                    # the module's parameters and buffers are its own
    res = {k: v.detach().cpu().numpy() for k, v in res.items()}
    res["tracked"] = int(pfn.norm.num_batches_tracked.item())
    return res


def compare(got, want, case, how, every=True):
    names = ["out", "running_mean", "running_var", "canvas"] + (["dW", "dgamma", "dbeta"] if case["training"] else [])
    if every and case["training"]:
        names += ["winner", "sums", "stat"]
    for k in names:
        why = seq.report(got[k], want[k], f"{how}: {k}:")
        assert not why, why
    assert got["tracked"] == want["tracked"], how
    if "grad_feat" in got:
        why = seq.report(got["grad_feat"], seq.grad_feat_of(case), f"{how}: grad_feat:")
        assert not why, why


def written(res):
    for k, a in res.items():
        if isinstance(a, np.ndarray) and a.dtype != np.uint8:
            words = a.view(np.uint32)
            assert not (words == SENTINEL).any(), k                             # every element is written


def test_the_constants_of_the_tree():
    assert (ops.pillar_vfe_run(), ops.pillar_vfe_group()) == (seq.RUN, seq.GROUP)
    assert (ops.PILLAR_XYZ, ops.PILLAR_CLUSTER, ops.PILLAR_CENTER, ops.PILLAR_DIST) == (seq.XYZ, seq.CLUSTER, seq.CENTER, seq.DIST)


SCENES = ["abs_c64", "rel_c32", "dist_c64", "eval_c32", "two_steps", "eval_dist"]


@pytest.mark.parametrize("name", SCENES)
def test_recorded_scenes(gold, gpu, name):
    case, rec = gold[name]
    want = restated(("gold", name), case)
    ex = seq.exact(case, case["grad"] if case["training"] else None)
    for how, got in (("ops", through_ops(case, gpu)), ("the methods", through_modules(case, gpu))):
        compare(got, want, case, how, every=how == "ops")
        pairs = [("out", "pillar_features")] + ([(k, k) for k in ("running_mean", "running_var", "dW", "dgamma", "dbeta")] if case["training"] else [])
        for k, r in pairs:                                                      # ... and within the derived bound, like the recording
            why, _ = seq.bound_report(got[k], ex[k][0], ex[k][1], f"{how}: {k}")
            assert not why, why
            why = seq.pattern_report(got[k], rec[r], f"{how}: {k}")
            assert not why, why


@pytest.mark.parametrize("name", sorted(CASES))
def test_named_cases(gpu, name):
    case = CASES[name]
    want = restated(("case", name), case)
    got = through_ops(case, gpu)                          # into sentinel-filled outputs
    compare(got, want, case, "ops")
    written(got)
    again = through_ops(case, gpu, sentinel=False)        # the same bits on a second call, into torch.empty
    for k in got:
        assert got[k] is None or isinstance(got[k], int) or seq.same_bits(got[k], again[k]), k
    if case["parts"] & seq.CLUSTER and case["parts"] & seq.CENTER:      # the module always has both offsets
        compare(through_modules(case, gpu), want, case, "the methods", every=False)


def test_eval_mode_changes_no_buffer(gpu):
    case = CASES["eval"]
    vfe, sc, batch = seq.bare_modules(case, gpu)
    before = {k: v.clone() for k, v in vfe.state_dict().items()}
    with torch.no_grad():
        sc(vfe(dict(batch)))
    for k, v in vfe.state_dict().items():
        assert torch.equal(v, before[k]), k


@pytest.mark.parametrize("dtype", [np.float32, np.int32, np.int64])
def test_scatter_rows_out_of_range_inside_a_padded_buffer(gpu, dtype):
    """every index such a row could make lands inside the allocation; nothing outside the canvas is written"""
    case = CASES["run_at"]
    B, ny, nx = case["batch_size"], case["ny"], case["nx"]
    coords, pushed = out_of_range_coords(case, dtype)
    feat = seq.restate_steps(case)["out"]
    C = feat.shape[1]
    buf = filled((B + 2, C, ny, nx), torch.float32, gpu)
    canvas = ops.pillar_scatter(to(feat, gpu), to(coords, gpu), B, ny, nx, out=buf[1:B + 1])
    assert canvas.data_ptr() == buf[1].data_ptr()
    whole = buf.cpu().numpy()
    assert (whole[0].view(np.uint32) == SENTINEL).all() and (whole[-1].view(np.uint32) == SENTINEL).all()
    why = seq.report(whole[1:B + 1], seq.scatter(feat, coords, B, ny, nx), "canvas:")
    assert not why, why
    G = seq.grad_canvas_of(case)
    gbuf = filled((B + 2, C, ny, nx), torch.float32, gpu)
    gbuf[1:B + 1] = to(G, gpu)
    grad = ops.pillar_scatter_backward(gbuf[1:B + 1], to(coords, gpu), out=filled(feat.shape, torch.float32, gpu)).cpu().numpy()
    why = seq.report(grad, seq.scatter_backward(G, coords), "grad_feat:")
    assert not why, why
    assert not grad[pushed].any() and grad[len(pushed):].any()


def test_mid_size_run(gpu):
    """P = 64 000 x 32 x 4 -> 64 on the Lyft grid: many groups of the tree, many scatter tiles"""
    case = mid()
    want = restated(("mid", "lyft"), case)
    got = through_ops(case, gpu, sentinel=False)
    compare(got, want, case, "ops")
    got = through_modules(case, gpu)
    compare(got, want, case, "the methods", every=False)


def test_no_host_synchronisation(gpu):
    case = CASES["run_above"]
    vfe, sc, batch = seq.bare_modules(case, gpu)
    G = to(seq.grad_canvas_of(case), gpu)
    (sc(vfe(dict(batch)))["spatial_features"] * G).sum().backward()      # the library is loaded from here on
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            canvas = sc(vfe(dict(batch)))["spatial_features"]
            (canvas * G).sum().backward()
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    assert sum("called a synchronizing" in str(w.message) for w in seen) == 0
    assert tuple(canvas.shape) == (case["batch_size"], case["W"].shape[0], case["ny"], case["nx"])


def test_on_another_stream(gpu):
    case = CASES["c63"]
    want = restated(("case", "c63"), case)
    stream = torch.cuda.Stream(device=gpu)
    stream.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(stream):
        got = through_ops(case, gpu)
    stream.synchronize()
    compare(got, want, case, "ops on a side stream")


def test_refusals_of_the_modules(gpu):
    case = CASES["c32"]
    vfe, sc, batch = seq.bare_modules(case, gpu)
    two = seq.bare_modules(case, gpu)[0]
    two.pfn_layers.append(two.pfn_layers[0])
    with pytest.raises(NotImplementedError, match="2 PFN layers"):
        two(dict(batch))
    vfe.pfn_layers[0].use_norm = False
    with pytest.raises(NotImplementedError, match="USE_NORM: False"):
        vfe(dict(batch))
    vfe.pfn_layers[0].use_norm = True
    with pytest.raises(NotImplementedError, match="voxels that require grad"):
        vfe(dict(batch, voxels=batch["voxels"].clone().requires_grad_()))
    with pytest.raises(NotImplementedError, match="voxels of torch.float16"):
        vfe(dict(batch, voxels=batch["voxels"].half()))
    with pytest.raises(NotImplementedError, match="linear.weight of torch.float64"):
        seq.bare_modules(case, gpu)[0].double()(dict(batch))
    vfe.eval()
    with pytest.raises(NotImplementedError, match="gradients of PillarVFE in eval mode"):
        vfe(dict(batch))
    sc.nz = 2
    with pytest.raises(NotImplementedError, match="nz = 2"):
        sc(dict(batch, pillar_features=torch.zeros((6, 32), device=gpu)))


def test_every_refusal_of_the_ops_and_of_the_library(gpu):
    z = lambda *s, dtype=torch.float32: torch.zeros(s, dtype=dtype, device=gpu)      # noqa: E731
    geo = dict(voxel_size=(1.0, 1.0, 1.0), offsets=(0.0, 0.0, 0.0))

    def vfe(P=4, S=3, Cp=4, C=8, K=10, **kw):
        return ops.pillar_vfe(z(P, S, Cp), z(P) + 1, z(P, 4), z(C, K), z(C), z(C), z(C), z(C) + 1, **geo, **kw)

    # the limits, at them
    assert vfe(C=64)[0].shape == (4, 64) and vfe(S=255)[0].shape == (4, 8) and vfe(Cp=9, K=16, parts=15)[0].shape == (4, 8)
    assert vfe(K=1, parts=0)[0].shape == (4, 8)
    assert ops.pillar_scatter(z(4, 8), z(4, 4), 65535, 1, 1).shape == (65535, 8, 1, 1)
    assert vfe(P=0, training=False)[0].shape == (0, 8)
    # ... and one step past
    for fn, match in ((lambda: vfe(C=65), "C = 65 output channels is outside the limit of 1 .. 64"),
                      (lambda: vfe(C=0), "C = 0 output channels is outside the limit of 1 .. 64"),
                      (lambda: vfe(Cp=10, K=17, parts=15), "K = 17 features of a point is outside the limit of 1 .. 16"),
                      (lambda: vfe(Cp=3, K=0, parts=0), "K = 0 features of a point is outside the limit of 1 .. 16"),
                      (lambda: vfe(K=9), "weight has K = 9 columns"),
                      (lambda: vfe(S=256), "S = 256 slots of a pillar is outside the limit of 1 .. 255"),
                      (lambda: vfe(S=0), "S = 0 slots of a pillar is outside the limit of 1 .. 255"),
                      (lambda: ops.pillar_vfe(z(1, 1, 1).expand((1 << 31) // 255 + 1, 255, 4), z(1), z(1, 4), z(8, 10), z(8), z(8), **geo),
                       "above the limit of 2147483647 rows"),
                      (lambda: vfe(P=1, S=1), "Expected more than 1 value per channel when training"),
                      (lambda: ops.pillar_vfe(z(4, 3, 4), z(4), z(4, 4), z(8, 10), z(8), z(8), training=False, **geo), "eval mode needs running_mean"),
                      (lambda: ops.pillar_scatter(z(4, 8), z(4, 4), 65536, 1, 1), "batch_size = 65536 is outside the limit of 0 .. 65535"),
                      (lambda: ops.pillar_scatter(z(4, 65), z(4, 4), 1, 1, 1), "C = 65 channels is outside the limit of 1 .. 64"),
                      (lambda: ops.pillar_scatter(z(4, 8), z(4, 4), 1, 0, 1), "a grid of ny = 0, nx = 1"),
                      (lambda: ops.pillar_scatter(z(4, 8), z(5, 4), 1, 1, 1), "must be \\(P, C\\) and \\(P, 4\\)"),
                      (lambda: ops.pillar_scatter(z(4, 8), z(4, 4), 1, 2, 2, out=z(1, 8, 2, 3)), "out must be a contiguous float32 \\(1, 8, 2, 2\\)"),
                      (lambda: ops.pillar_scatter(torch.zeros(4, 8), z(4, 4), 1, 1, 1), "pillar_features must be a device tensor"),
                      (lambda: ops.pillar_scatter_backward(z(1, 8, 2, 2), z(4, 3)), "voxel_coords \\(4, 3\\) must be \\(P, 4\\)")):
        with pytest.raises(ValueError, match=match):
            fn()
    with pytest.raises(TypeError, match="voxels must be float32"):
        ops.pillar_vfe(z(4, 3, 4).half(), z(4), z(4, 4), z(8, 10), z(8), z(8), **geo)
    with pytest.raises(TypeError, match="voxel_coords must be float32, int32 or int64"):
        ops.pillar_scatter(z(4, 8), z(4, 4).double(), 1, 1, 1)
    # the library's own checks, past the wrapper: nothing is launched
    from modest_amd import _lib
    import ctypes as C
    lib = _lib.load()
    p = z(4096).data_ptr()
    geom = (C.c_float * 6)(1, 1, 1, 0, 0, 0)

    def fwd(P=4, S=3, Cp=4, Cout=8, parts=7, ncode=0, ccode=0, rm=p, training=1, ws=1 << 20, voxels=p):
        return lib.modest_pillar_vfe(P, S, Cp, Cout, parts, voxels, p, ncode, p, ccode, geom, p, p, p, rm, rm, p, 1e-3, 0.01, training, p, p, p, p, p, ws, None)

    def bwd(P=4, S=3, Cp=4, Cout=8, parts=7, ws=1 << 20, grad=p):
        return lib.modest_pillar_vfe_backward(P, S, Cp, Cout, parts, p, p, 0, p, 0, geom, p, p, p, p, grad, p, p, p, p, p, p, ws, None)

    for fn, text in ((lambda: fwd(Cout=65), b"output channels between 1 and 64"),
                     (lambda: fwd(S=256), b"slots of a pillar between 1 and 255"),
                     (lambda: fwd(Cp=2), b"point features between 3 and 19"),
                     (lambda: fwd(Cp=11, parts=15), b"features of a point between 1 and 16"),
                     (lambda: fwd(Cp=3, parts=0), b"features of a point between 1 and 16"),
                     (lambda: fwd(parts=16), b"parts is a mask"),
                     (lambda: fwd(P=(1 << 31) // 3 + 1), b"n_pillars * slots at most 2^31 - 1"),
                     (lambda: fwd(P=-1), b"n_pillars >= 0"),
                     (lambda: fwd(ncode=3), b"dtype code 0 (float32) 1 (int32) 2 (int64)"),
                     (lambda: fwd(P=1, S=1), b"more than one row"),
                     (lambda: fwd(rm=None, training=0), b"running_mean and running_var in eval mode"),
                     (lambda: fwd(voxels=None), b"NULL buffer"),
                     (lambda: fwd(voxels=p + 2), b"unaligned buffer"),
                     (lambda: lib.modest_pillar_vfe(4, 3, 4, 8, 7, p, p, 0, p + 4, 2, geom, p, p, p, p, p, p, 1e-3, 0.01, 1, p, p, p, p, p, 1 << 20, None),
                      b"unaligned buffer"),                                    # int64 coords on a 4-byte boundary
                     (lambda: fwd(ws=8), b"workspace of modest_pillar_vfe_workspace_bytes()"),
                     (lambda: bwd(Cout=0), b"output channels between 1 and 64"),
                     (lambda: bwd(P=1, S=1), b"more than one row"),
                     (lambda: bwd(grad=None), b"NULL buffer"),
                     (lambda: bwd(ws=8), b"workspace of modest_pillar_vfe_workspace_bytes()"),
                     (lambda: lib.modest_pillar_scatter(4, 65, 1, 1, 1, p, p, 0, p, None), b"channels between 1 and 64"),
                     (lambda: lib.modest_pillar_scatter(4, 8, 65536, 1, 1, p, p, 0, p, None), b"batch between 0 and 65535"),
                     (lambda: lib.modest_pillar_scatter(4, 8, 1, 0, 1, p, p, 0, p, None), b"a grid of ny, nx >= 1"),
                     (lambda: lib.modest_pillar_scatter(4, 8, 1, 1, 1, p, p, 3, p, None), b"dtype code"),
                     (lambda: lib.modest_pillar_scatter(4, 8, 1, 1, 1, None, p, 0, p, None), b"NULL buffer"),
                     (lambda: lib.modest_pillar_scatter(4, 8, 1, 1, 1, p, p, 0, None, None), b"NULL buffer"),
                     (lambda: lib.modest_pillar_scatter_backward(4, 8, 1, 1, 1, None, p, 0, p, None), b"NULL buffer"),
                     (lambda: lib.modest_pillar_scatter_backward(4, 8, 1, 1, 1, p, p + 4, 2, p, None), b"unaligned buffer"),
                     (lambda: lib.modest_pillar_vfe_workspace_bytes(-1, 8, 10), b"n_pillars between 0 and 2^31 - 1")):
        rc = fn()                                          # one at a time: the error text is the last call's
        assert rc != 0 and text in lib.modest_last_error(), (text, lib.modest_last_error())
