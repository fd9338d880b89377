"""GPU: modest_amd.utils.roi_head_loss.get_loss (csrc/roi_loss.hip) on a bare head object against the
values recorded from the reference's own RoIHeadTemplate.get_loss and its autograd (tests/golden/roi_loss.npz), within the
bound exact() derives, and against the numpy restatement tests/roi_loss_seq.py bit for bit: the scalars, fg_sum and every
element of the two gradients.  A mismatch reports the row and column.  The cases of tests/roi_loss_cases.py cross the kernels'
constants and branches; they also run into sentinel-filled outputs with a pre-filled workspace, twice, and from non-contiguous
predictions."""
import os
import warnings

import numpy as np
import pytest
import torch

import roi_loss_seq as seq
from roi_loss_cases import CASES
from modest_amd import ops
from modest_amd.utils import roi_head_loss as rhl

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "roi_loss.npz")
EDGES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "roi_loss_edges.npz")
F = np.float32
SENTINEL = 0x5A5A5A5A
_restated = {}


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def restated(key, cfg):
    """(inputs, restatement, exact) of a config, computed once and left unchanged"""
    if key not in _restated:
        inp = seq.make_inputs(cfg)
        ours, dec = seq._evaluate(inp, cfg, None)
        _restated[key] = (inp, ours, seq.exact(inp, cfg, dec))
    return _restated[key]


def table_of(tb, head):
    pinned = head._modest_roi_loss_table
    return np.array([tb["rcnn_loss_cls"], tb["rcnn_loss_reg"], tb.get("rcnn_loss_corner", 0.0), tb["rcnn_loss"], float(pinned[4]),
                     float(pinned[5])], dtype=F)


def through_get_loss(cfg, inp, gpu, scale=None):
    head, preds = seq.bare_head(cfg, inp, device=gpu)
    passed = {"kept": 1.0}
    loss, tb = rhl.get_loss(head, passed)
    assert tb is passed and tb["kept"] == 1.0
    assert loss.ndim == 0 and loss.is_cuda and loss.dtype == torch.float32 and loss.requires_grad
    assert all(type(v) is float for v in tb.values())
    n_fg = int((inp["mask"] > 0).sum())
    assert ("rcnn_loss_corner" in tb) == (bool(cfg["corner"]) and n_fg > 0)      # absent at fg_sum == 0
    (loss if scale is None else scale * loss).backward()
    got = {"table": table_of(tb, head), "grad_cls": preds["cls"].grad.cpu().numpy().reshape(-1), "grad_reg": preds["reg"].grad.cpu().numpy()}
    assert preds["cls"].grad.shape == preds["cls"].shape
    dev_loss = loss.item()
    assert dev_loss == tb["rcnn_loss"] or (np.isnan(dev_loss) and np.isnan(tb["rcnn_loss"]))
    return got, head


def through_ops(cfg, inp, gpu, sentinel=True, noncontig=False, want_grad=True):
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(gpu) for k, v in inp.items()}
    R, code = inp["reg"].shape
    if noncontig:   # every second element of a wider tensor
        for k in ("cls", "reg"):
            wide = torch.full(tuple(t[k].shape[:-1]) + (t[k].shape[-1] * 2,), 7.0, device=gpu)
            view = wide[..., ::2]
            view.copy_(t[k])
            assert not view.is_contiguous() or R == 1
            t[k] = view
    if cfg["gt_cols"] > code:
        assert t["gt"].stride(0) == cfg["gt_cols"] > code
    fill = lambda shape: torch.full(shape, SENTINEL, dtype=torch.int32, device=gpu).view(torch.float32)      # noqa: E731
    out = None
    ws = None
    if sentinel:
        out = [fill((6,)), fill((R,)) if want_grad else None, fill((R, code)) if want_grad else None]
        ws = torch.full((ops.roi_loss_workspace_bytes(R),), 0x5A, dtype=torch.uint8, device=gpu)
    table, grads = ops.roi_loss(t["cls"], t["reg"], t["labels"], t["mask"], t["gt"], t["src"], t["rois"], t["cw"], beta=cfg["beta"],
                                cls_weight=cfg["cls_weight"], reg_weight=cfg["reg_weight"], corner_weight=cfg["corner_weight"],
                                corner=cfg["corner"], want_grad=want_grad, workspace=ws, out=out)
    got = {"table": table.cpu().numpy()}
    if want_grad:
        got.update(grad_cls=grads[0].cpu().numpy(), grad_reg=grads[1].cpu().numpy())
    else:
        assert grads is None
    return got


@pytest.mark.parametrize("name", ["pointrcnn", "pvrcnn", "nofg", "nocorner", "wide", "edge"])
def test_fixture_scenes(gold, gpu, name):
    cfg = dict(seq.scenes(gold))[name]
    inp, want, ex = restated(("gold", name), cfg)
    gt_before = inp["gt"].copy()
    got, head = through_get_loss(cfg, inp, gpu)
    why, _ = seq.bound_report(got, ex, "the device")
    assert not why, f"against exact()\n{why}"
    why, _ = seq.bound_report(seq.recorded(gold, name), ex, "the reference")
    assert not why, why
    assert not seq.zero_report(got, seq.recorded(gold, name))
    assert got["table"][4] == seq.recorded(gold, name)["table"][4] == (inp["mask"] > 0).sum()
    why = seq.report(got, want)
    assert not why, f"against the restatement\n{why}"
    # the one visible difference to the reference: the sizes in forward_ret_dict['gt_of_rois'] are left as they were
    after = head.forward_ret_dict["gt_of_rois"].cpu().numpy().reshape(gt_before.shape)
    assert np.array_equal(after.view(np.uint32), gt_before.view(np.uint32))


@pytest.fixture(scope="module")
def edges():
    return dict(np.load(EDGES))


@pytest.mark.parametrize("name", list(seq.edge_scene_cfgs()))
def test_fixture_edge_scenes(edges, gpu, name):
    """the second recorded set: non-finite and huge values on foreground rows, with and without the corner term"""
    cfg = dict(seq.scenes(edges))[name]
    assert cfg == CASES[name]
    inp, want, ex = restated(("case", name), cfg)
    rec = seq.recorded(edges, name)
    got, head = through_get_loss(cfg, inp, gpu)
    why, _ = seq.bound_report(got, ex, "the device")
    assert not why, f"against exact()\n{why}"
    why, _ = seq.bound_report(rec, ex, "the reference")
    assert not why, why
    assert not seq.zero_report(got, rec)
    for k, v in rec.items():
        assert np.array_equal(np.isnan(got[k]), np.isnan(v)), k          # NaNs at the reference's places
    why = seq.report(got, want)
    assert not why, f"against the restatement\n{why}"


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
    assert list(plain) == ["table"] and np.array_equal(plain["table"].view(np.uint32), got["table"].view(np.uint32))
    got_head, _ = through_get_loss(cfg, inp, gpu)
    why = seq.report(got_head, want, "get_loss")
    assert not why, why


def test_backward_scales_by_the_upstream_gradient(gpu):
    cfg = CASES["r257"]
    inp, want, _ = restated(("case", "r257"), cfg)
    got, _ = through_get_loss(cfg, inp, gpu, scale=3.0)
    three = {k: (v * F(3.0) if k != "table" else v) for k, v in want.items()}
    why = seq.report(got, three, "(3 * loss).backward()")
    assert not why, why
    # a second backward through the same loss: the buffers were scaled in place
    head, preds = seq.bare_head(cfg, inp, device=gpu)
    loss, _ = rhl.get_loss(head)
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="second time"):
        loss.backward()


def test_gradient_reaches_a_leaf_through_a_linear_layer(gpu):
    cfg = CASES["r257"]
    inp, want, _ = restated(("case", "r257"), cfg)
    head, preds = seq.bare_head(cfg, inp, device=gpu, requires_grad=False)
    R = cfg["B"] * cfg["M"]
    feat = torch.randn((R, 5), device=gpu, generator=torch.Generator(device=gpu).manual_seed(1)).requires_grad_(True)
    lin = torch.nn.Linear(5, 1).to(gpu)
    logits = lin(feat)
    logits.retain_grad()
    head.forward_ret_dict["rcnn_cls"] = logits
    loss, tb = rhl.get_loss(head)
    loss.backward()
    assert feat.grad is not None and lin.weight.grad is not None and float(feat.grad.abs().sum()) > 0
    # the gradient of the logits is the restatement's on these logits, and the layer hands it on
    want2 = seq.restate(dict(inp, cls=logits.detach().cpu().numpy().reshape(-1)), cfg)
    got = {"table": table_of(tb, head), "grad_cls": logits.grad.cpu().numpy().reshape(-1), "grad_reg": want2["grad_reg"]}
    why = seq.report(got, want2)
    assert not why, why
    assert torch.allclose(feat.grad, logits.grad @ lin.weight.detach(), rtol=1e-4, atol=1e-7)
    assert preds["reg"].grad is None
    # no prediction requires a gradient: no gradient function, the same scalars
    head3, _ = seq.bare_head(cfg, inp, device=gpu, requires_grad=False)
    loss3, tb3 = rhl.get_loss(head3)
    assert not loss3.requires_grad and loss3.grad_fn is None
    with torch.no_grad():
        head4, _ = seq.bare_head(cfg, inp, device=gpu)
        loss4, tb4 = rhl.get_loss(head4)
    assert not loss4.requires_grad and tb3 == tb4
    assert np.array_equal(table_of(tb3, head3).view(np.uint32), want["table"].view(np.uint32))


def test_one_host_synchronisation_per_get_loss(gpu):
    cfg = CASES["r257"]
    inp, _, _ = restated(("case", "r257"), cfg)
    head, preds = seq.bare_head(cfg, inp, device=gpu)
    rhl.get_loss(head)                       # the buffers kept on the head exist from here on
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            loss, tb = rhl.get_loss(head)
            loss.backward()
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    assert sum("called a synchronizing" in str(w.message) for w in seen) == 1
    assert head._modest_roi_loss_table.is_pinned() and tb["rcnn_loss"] == float(head._modest_roi_loss_table[3])


def test_every_limit_raises_one_step_past_it(gpu):
    def call(R=4, code=7, labels=torch.int32, mask=torch.int32, cls_rows=None, reg=None, **kw):
        z = lambda *s: torch.zeros(s, device=gpu)      # noqa: E731
        return ops.roi_loss(z(R if cls_rows is None else cls_rows), z(R, code) if reg is None else reg,
                            torch.zeros((R,), dtype=labels, device=gpu),
                            torch.ones((R,), dtype=mask, device=gpu), z(R, code), z(R, code), z(R, code), z(code), **kw)
    table, grads = call(code=16)
    assert np.isfinite(table.cpu().numpy()).all() and grads[1].shape == (4, 16) and float(table[4]) == 4
    for kw, name in ((dict(code=17), "code size = 17"), (dict(code=6), "code size = 6"), (dict(cls_rows=5), "rcnn_cls has 5 elements")):
        with pytest.raises(ValueError, match=name):
            call(**kw)
    with pytest.raises(TypeError, match="rcnn_cls_labels must be int32, int64 or float32"):
        call(labels=torch.int16)
    with pytest.raises(TypeError, match="reg_valid_mask must be int32 or int64"):
        call(mask=torch.float32)
    with pytest.raises(ValueError, match="rcnn_reg must be a device tensor"):
        call(reg=torch.zeros(4, 7))
    with pytest.raises(ValueError, match=f"above the limit of {ops.ROI_LOSS_MAX_ROWS} rows"):
        call(reg=torch.empty((ops.ROI_LOSS_MAX_ROWS + 1, 7), device=gpu))
    # the library's own checks, past the wrapper
    from modest_amd import _lib
    lib = _lib.load()
    assert lib.modest_roi_loss_max_rows() == ops.ROI_LOSS_MAX_ROWS
    assert lib.modest_roi_loss_workspace_bytes(ops.ROI_LOSS_MAX_ROWS + 1) < 0
    args = lambda R, code: (R, code, None, None, None, 0, None, 0, None, code, None, code, None, None, 0.1, 1.0, 1.0, 1.0, 1,      # noqa: E731
                            None, None, None, None, 0, None)
    assert lib.modest_roi_loss(*args(4, 17)) != 0
    assert b"code size between 7 and 16" in lib.modest_last_error()
    assert lib.modest_roi_loss(*args(ops.ROI_LOSS_MAX_ROWS + 1, 7)) != 0
    assert b"n_rows between 0 and 2^20" in lib.modest_last_error()
    assert lib.modest_roi_loss_backward(ops.ROI_LOSS_MAX_ROWS + 1, 0, None, None, None, None) != 0
