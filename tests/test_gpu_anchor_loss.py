"""GPU: modest_amd.utils.anchor_head_loss.get_loss (csrc/anchor_loss.hip) on a bare head object against
the values recorded from the reference's own AnchorHeadTemplate.get_loss and its autograd (tests/golden/anchor_loss.npz),
within the bound exact() derives, and against the numpy restatement tests/anchor_loss_seq.py bit for bit: the four scalars
and every element of the three gradients.  A mismatch reports (sample, anchor, column).  The cases of
tests/anchor_loss_cases.py cross the kernels' constants; they also run into sentinel-filled outputs with a pre-filled
workspace, twice, and from non-contiguous predictions."""
import os
import warnings

import numpy as np
import pytest
import torch

import anchor_loss_seq as seq
from anchor_loss_cases import CASES
from modest_amd import ops
from modest_amd.utils import anchor_head_loss as ahl

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "anchor_loss.npz")
EDGES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "anchor_loss_edges.npz")
F = np.float32
SENTINEL = 0x5A5A5A5A
_restated = {}


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def edges():
    return dict(np.load(EDGES))


def restated(key, cfg):
    """(inputs, restatement, exact) of a config, computed once and left unchanged"""
    if key not in _restated:
        inp = seq.make_inputs(cfg)
        ours, dec = seq._evaluate(inp, cfg, None)
        _restated[key] = (inp, ours, seq.exact(inp, cfg, dec))
    return _restated[key]


def losses_of(tb):
    return np.array([tb["rpn_loss_cls"], tb["rpn_loss_loc"], tb.get("rpn_loss_dir", 0.0), tb["rpn_loss"]], dtype=F)


def through_get_loss(cfg, inp, gpu, scale=None):
    head, preds = seq.bare_head(cfg, inp, device=gpu)
    loss, tb = ahl.get_loss(head)
    assert loss.ndim == 0 and loss.is_cuda and loss.dtype == torch.float32 and loss.requires_grad
    assert all(type(v) is float for v in tb.values()) and ("rpn_loss_dir" in tb) == bool(cfg["bins"])
    (loss if scale is None else scale * loss).backward()
    # a layout's predictions are (B, H, W, 6 * columns): their gradients come back in that shape
    got = {"losses": losses_of(tb), "grad_cls": preds["cls"].grad.cpu().numpy().reshape(inp["cls"].shape),
           "grad_box": preds["box"].grad.cpu().numpy().reshape(inp["box"].shape)}
    if "dir" in preds:
        assert preds["dir"].grad.shape == preds["dir"].shape
        got["grad_dir"] = preds["dir"].grad.cpu().numpy().reshape(inp["dir"].shape)
    dev_loss = loss.item()
    assert dev_loss == tb["rpn_loss"] or (np.isnan(dev_loss) and np.isnan(tb["rpn_loss"]))
    return got, head


def through_ops(cfg, inp, gpu, sentinel=True, noncontig=False, want_grad=True):
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(gpu) for k, v in inp.items() if v is not None}
    if noncontig:   # every second column of a wider tensor
        for k in ("cls", "box", "dir"):
            if k in t:
                wide = torch.full(tuple(t[k].shape[:2]) + (t[k].shape[2] * 2,), 7.0, device=gpu)
                view = wide[..., ::2]
                view.copy_(t[k])
                assert not view.is_contiguous()
                t[k] = view
    B, N = inp["labels"].shape
    fill = lambda shape: torch.full(shape, SENTINEL, dtype=torch.int32, device=gpu).view(torch.float32)      # noqa: E731
    out = None
    ws = None
    if sentinel:
        out = [fill((4,)), fill((B, N, cfg["num_class"])) if want_grad else None, fill((B, N, cfg["code"])) if want_grad else None,
               fill((B, N, cfg["bins"])) if (want_grad and cfg["bins"]) else None]
        ws = torch.full((ops.anchor_loss_workspace_bytes(B, N),), 0x5A, dtype=torch.uint8, device=gpu)
    losses, grads = ops.anchor_loss(t["cls"], t["box"], t.get("dir"), t["labels"], t["tg"], t["anchors"], t["cw"], beta=cfg["beta"],
                                    dir_offset=cfg["dir_offset"], cls_weight=cfg["cls_weight"], loc_weight=cfg["loc_weight"],
                                    dir_weight=cfg["dir_weight"] if cfg["bins"] else 0.0, want_grad=want_grad, workspace=ws, out=out)
    got = {"losses": losses.cpu().numpy()}
    if want_grad:
        got.update(grad_cls=grads[0].cpu().numpy(), grad_box=grads[1].cpu().numpy())
        if grads[2] is not None:
            got["grad_dir"] = grads[2].cpu().numpy()
    else:
        assert grads is None
    return got


@pytest.mark.parametrize("name", ["kitti", "lyft", "wide", "edge", "l1", "nan6"])
def test_fixture_scenes(gold, gpu, name):
    cfg = dict(seq.scenes(gold))[name]
    inp, want, ex = restated(("gold", name), cfg)
    labels_before = inp["labels"].copy()
    got, head = through_get_loss(cfg, inp, gpu)
    why, _ = seq.bound_report(got, ex, "the device")
    assert not why, f"against exact()\n{why}"
    why, _ = seq.bound_report(seq.recorded(gold, name), ex, "the reference")
    assert not why, why
    assert not seq.zero_report(got, seq.recorded(gold, name))
    why = seq.report(got, want)
    assert not why, f"against the restatement\n{why}"
    # the one visible difference to the reference: the labels in forward_ret_dict are left as they were
    assert np.array_equal(head.forward_ret_dict["box_cls_labels"].cpu().numpy(), labels_before)


@pytest.mark.parametrize("name", list(seq.edge_scene_cfgs()))
def test_fixture_edge_scenes(edges, gpu, name):
    """the second recorded set: bin edges, saturating and non-finite values, the head's real layout (three anchor tensors
    through get_loss's own flattening), al_finish past 256 and 2048 partials"""
    cfg = dict(seq.scenes(edges))[name]
    assert cfg == CASES[name]
    inp, want, ex = restated(("case", name), cfg)
    rec = seq.recorded(edges, name)
    got, head = through_get_loss(cfg, inp, gpu)
    why, _ = seq.bound_report(got, ex, "the device")
    assert not why, f"against exact()\n{why}"
    why, _ = seq.bound_report(rec, seq.only(ex, rec), "the reference")
    assert not why, why
    assert not seq.zero_report(seq.only(got, rec), rec)
    for k, v in rec.items():
        assert np.array_equal(np.isnan(got[k]), np.isnan(v)), k          # NaNs at the reference's places
    why = seq.report(got, want)
    assert not why, f"against the restatement\n{why}"
    if cfg.get("layout"):
        assert len(head.anchors) == 3 and np.array_equal(head._modest_anchor_loss_anchors.cpu().numpy(), inp["anchors"])


def test_no_anchors(gpu):
    """N = 0: the four scalars are 0 and nothing else is written, with and without gradients"""
    for bins in (2, 0):
        for want_grad in (True, False):
            z = lambda *shape: torch.zeros(shape, device=gpu)      # noqa: E731
            out = torch.full((4,), SENTINEL, dtype=torch.int32, device=gpu).view(torch.float32)
            ws = torch.full((max(ops.anchor_loss_workspace_bytes(2, 0), 256),), 0x5A, dtype=torch.uint8, device=gpu)
            before = ws.clone()
            grads_in = [z(2, 0, 3), z(2, 0, 7), z(2, 0, bins) if bins else None] if want_grad else [None, None, None]
            losses, grads = ops.anchor_loss(z(2, 0, 3), z(2, 0, 7), z(2, 0, bins) if bins else None,
                                            torch.zeros((2, 0), dtype=torch.int32, device=gpu), z(2, 0, 7), z(0, 7), torch.ones(7, device=gpu),
                                            want_grad=want_grad, workspace=ws, out=[out] + grads_in)
            assert losses.cpu().numpy().view(np.uint32).tolist() == [0, 0, 0, 0]
            assert (grads is None) == (not want_grad)
            if want_grad:
                assert [g.shape for g in grads if g is not None] == [(2, 0, 3), (2, 0, 7)] + ([(2, 0, bins)] if bins else [])
            # past the two counters the workspace is as it was
            assert torch.equal(ws[256:], before[256:])


@pytest.mark.parametrize("name", sorted(CASES))
def test_edge_cases(gpu, name):
    cfg = CASES[name]
    inp, want, ex = restated(("case", name), cfg)
    got = through_ops(cfg, inp, gpu)                   # sentinel-filled outputs, a pre-filled workspace
    why = seq.report(got, want)
    assert not why, why
    why, _ = seq.bound_report(got, ex, "the device")
    assert not why, why
    for v in got.values():
        assert not (v.view(np.uint32) == SENTINEL).any()
    again = through_ops(cfg, inp, gpu)
    assert all(np.array_equal(got[k].view(np.uint32), again[k].view(np.uint32)) for k in got)      # two runs, the same bits
    why = seq.report(through_ops(cfg, inp, gpu, sentinel=False, noncontig=True), want, "non-contiguous predictions")
    assert not why, why
    plain = through_ops(cfg, inp, gpu, want_grad=False)
    assert list(plain) == ["losses"] and np.array_equal(plain["losses"].view(np.uint32), got["losses"].view(np.uint32))
    got_head, _ = through_get_loss(cfg, inp, gpu)
    why = seq.report(got_head, want, "get_loss")
    assert not why, why


def test_backward_scales_by_the_upstream_gradient(gpu):
    cfg = CASES["c3"]
    inp, want, _ = restated(("case", "c3"), cfg)
    got, _ = through_get_loss(cfg, inp, gpu, scale=3.0)
    three = {k: (v * F(3.0) if k != "losses" else v) for k, v in want.items()}
    why = seq.report(got, three, "(3 * loss).backward()")
    assert not why, why
    # a second backward through the same loss: the buffers were scaled in place
    head, preds = seq.bare_head(cfg, inp, device=gpu)
    loss, _ = ahl.get_loss(head)
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="second time"):
        loss.backward()


def test_gradient_reaches_a_leaf_through_a_linear_layer(gpu):
    cfg = CASES["n257"]
    inp, want, _ = restated(("case", "n257"), cfg)
    head, preds = seq.bare_head(cfg, inp, device=gpu, requires_grad=False)
    feat = torch.randn((cfg["B"], cfg["N"], 5), device=gpu, generator=torch.Generator(device=gpu).manual_seed(1)).requires_grad_(True)
    lin = torch.nn.Linear(5, cfg["num_class"]).to(gpu)
    logits = lin(feat)
    logits.retain_grad()
    head.forward_ret_dict["cls_preds"] = logits
    loss, tb = ahl.get_loss(head)
    loss.backward()
    assert feat.grad is not None and lin.weight.grad is not None and float(feat.grad.abs().sum()) > 0
    # the gradient of the logits is the restatement's on these logits, and the layer hands it on
    want2 = seq.restate(dict(inp, cls=logits.detach().cpu().numpy()), cfg)
    why = seq.report({"losses": losses_of(tb), "grad_cls": logits.grad.cpu().numpy()}, {k: want2[k] for k in ("losses", "grad_cls")})
    assert not why, why
    assert torch.allclose(feat.grad, logits.grad @ lin.weight.detach(), rtol=1e-4, atol=1e-7)
    assert preds["box"].grad is None
    # no prediction requires a gradient: no gradient function, the same scalars
    head3, _ = seq.bare_head(cfg, inp, device=gpu, requires_grad=False)
    loss3, tb3 = ahl.get_loss(head3)
    assert not loss3.requires_grad
    with torch.no_grad():
        head4, _ = seq.bare_head(cfg, inp, device=gpu)
        loss4, tb4 = ahl.get_loss(head4)
    assert not loss4.requires_grad and tb3 == tb4 and np.array_equal(losses_of(tb3).view(np.uint32), want["losses"].view(np.uint32))


def test_one_host_synchronisation_per_get_loss(gpu):
    cfg = CASES["c3"]
    inp, _, _ = restated(("case", "c3"), cfg)
    head, preds = seq.bare_head(cfg, inp, device=gpu)
    ahl.get_loss(head)                       # the buffers kept on the head exist from here on
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            loss, tb = ahl.get_loss(head)
            loss.backward()
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    assert sum("called a synchronizing" in str(w.message) for w in seen) == 1
    assert head._modest_anchor_loss_table.is_pinned() and tb["rpn_loss"] == float(head._modest_anchor_loss_table[3])


def test_every_limit_raises_one_step_past_it(gpu):
    def call(B=1, N=4, C=3, code=7, bins=2, **kw):
        z = lambda *s: torch.zeros(s, device=gpu)      # noqa: E731
        return ops.anchor_loss(z(B, N, C), z(B, N, code), z(B, N, bins) if bins else None, torch.zeros((B, N), dtype=torch.int32, device=gpu),
                               z(B, N, code), z(N, 7), z(code), **kw)
    losses, grads = call(C=32, code=16, bins=8)
    assert np.isfinite(losses.cpu().numpy()).all() and grads[2].shape == (1, 4, 8)
    for kw, name in ((dict(C=33), "num_class = 33"), (dict(code=17), "code size = 17"), (dict(code=6), "code size = 6"),
                     (dict(bins=9), "NUM_DIR_BINS = 9"), (dict(B=65536, N=1), "batch_size = 65536"), (dict(gamma=1.5), "gamma = 1.5")):
        with pytest.raises(ValueError, match=name):
            call(**kw)
    assert call(B=65535, N=1, bins=0)[1][2] is None
    with pytest.raises(TypeError, match="labels must be int32 or int64"):
        ops.anchor_loss(torch.zeros((1, 4, 3), device=gpu), torch.zeros((1, 4, 7), device=gpu), None,
                        torch.zeros((1, 4), device=gpu), torch.zeros((1, 4, 7), device=gpu), torch.zeros((4, 7), device=gpu),
                        torch.zeros(7, device=gpu))
    with pytest.raises(ValueError, match="not repeated over the batch"):
        ops.anchor_loss(torch.zeros((2, 4, 3), device=gpu), torch.zeros((2, 4, 7), device=gpu), None,
                        torch.zeros((2, 4), dtype=torch.int32, device=gpu), torch.zeros((2, 4, 7), device=gpu),
                        torch.zeros((8, 7), device=gpu), torch.zeros(7, device=gpu))
    # the library's own check, past the wrapper
    from modest_amd import _lib
    lib = _lib.load()
    assert lib.modest_anchor_loss(1, 4, 33, 7, 0, None, None, None, None, 0, None, None, 7, None, 0.1, 0.0, 1.0, 1.0, 1.0, 0.25, 2.0,
                                  None, None, None, None, None, 0, None) != 0
    assert b"num_class between 1 and 32" in lib.modest_last_error()
