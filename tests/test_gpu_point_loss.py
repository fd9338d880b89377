"""GPU: modest_amd.utils.point_head_loss.get_loss (csrc/point_loss.hip) on bare heads of the three kinds
against the values recorded from the reference's own get_loss methods and autograd (tests/golden/point_loss.npz), within the
bound exact() derives, and against the numpy restatement tests/point_loss_seq.py bit for bit: the table and every element of
the gradients.  A mismatch reports the row and column.  The cases of tests/point_loss_cases.py cross the kernels' constants
and branches; they also run into sentinel-filled outputs with a pre-filled workspace, twice, and from non-contiguous and
(B, N, C)-shaped predictions."""
import os
import warnings

import numpy as np
import pytest
import torch

import point_loss_seq as seq
from point_loss_cases import CASES
from modest_amd import ops
from modest_amd.utils import point_head_loss as phl

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "point_loss.npz")
EDGES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "point_loss_edges.npz")
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


def keys_of(cfg):
    terms = seq.terms_of(cfg)
    return ["point_loss_cls", "point_pos_num"] + (["point_loss_part"] if "part" in terms else []) + (
        ["point_loss_box"] if "box" in terms else [])


def through_get_loss(cfg, inp, gpu, scale=None):
    head, preds = seq.bare_head(cfg, inp, device=gpu)
    before = dict(head.forward_ret_dict)
    passed = {"kept": 1.0}
    loss, tb = head.get_loss(passed)
    assert tb is passed and tb["kept"] == 1.0
    assert list(tb) == ["kept"] + keys_of(cfg)                                   # the reference's keys in its order, no total
    assert loss.ndim == 0 and loss.is_cuda and loss.dtype == torch.float32 and loss.requires_grad
    assert all(type(v) is float for v in tb.values())
    assert all(head.forward_ret_dict[k] is v for k, v in before.items()) and len(head.forward_ret_dict) == len(before)
    (loss if scale is None else scale * loss).backward()
    got = seq.outputs_of(loss.item(), tb, preds)
    assert all(p.grad.shape == p.shape for p in preds.values())
    assert float(head._modest_point_loss_table[3]) == loss.item() or np.isnan(loss.item())
    return got, head


def through_ops(cfg, inp, gpu, sentinel=True, layout="rows", want_grad=True):
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(gpu) for k, v in inp.items()}
    terms = seq.terms_of(cfg)
    R, C, code = cfg["B"] * cfg["N"], cfg["num_class"], cfg["code"]
    for k in ("cls", "part", "box"):
        if k not in t:
            continue
        if layout == "noncontig":      # every second element of a wider tensor
            wide = torch.full((R, t[k].shape[-1] * 2), 7.0, device=gpu)
            view = wide[:, ::2]
            view.copy_(t[k])
            assert not view.is_contiguous()
            t[k] = view
        elif layout == "batched":      # (B, N, C)
            t[k] = t[k].view(cfg["B"], cfg["N"], -1)
    if layout == "batched":
        t["labels"] = t["labels"].view(cfg["B"], cfg["N"])
    fill = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.int32, device=gpu).view(torch.float32)      # noqa: E731
    out = ws = None
    if sentinel:
        out = [fill(5), fill(R, C) if want_grad else None, fill(R, 3) if want_grad and "part" in terms else None,
               fill(R, code) if want_grad and "box" in terms else None]
        ws = torch.full((ops.point_loss_workspace_bytes(R),), 0x5A, dtype=torch.uint8, device=gpu)
    table, grads = ops.point_loss(t["cls"], t["labels"], t.get("part"), t.get("part_t"), t.get("box"), t.get("box_t"), t.get("cw"),
                                  beta=cfg["beta"], cls_weight=cfg["cls_weight"], part_weight=cfg["part_weight"],
                                  box_weight=cfg["box_weight"], want_grad=want_grad, workspace=ws, out=out)
    got = {"table": table.cpu().numpy()}
    if want_grad:
        assert (grads[1] is not None) == ("part" in terms) and (grads[2] is not None) == ("box" in terms)
        got.update({f"grad_{k}": g.cpu().numpy() for k, g in zip(("cls", "part", "box"), grads) if g is not None})
    else:
        assert grads is None
    return got


SCENES = ["pointrcnn", "pointrcnn3", "parta2", "parta2_nobox", "pvrcnn", "nopos", "edge"]


@pytest.mark.parametrize("name", SCENES)
def test_fixture_scenes(gold, gpu, name):
    cfg = dict(seq.scenes(gold))[name]
    inp, want, ex = restated(("gold", name), cfg)
    rec = seq.recorded(gold, name)
    got, head = through_get_loss(cfg, inp, gpu)
    why, _ = seq.bound_report(got, ex, "the device")
    assert not why, f"against exact()\n{why}"
    why, _ = seq.bound_report(rec, ex, "the reference")
    assert not why, why
    assert not seq.zero_report(got, rec)
    assert got["table"][4] == rec["table"][4] == (inp["labels"] > 0).sum()
    why = seq.report(got, want)
    assert not why, f"against the restatement\n{why}"


@pytest.fixture(scope="module")
def edges():
    return dict(np.load(EDGES))


@pytest.mark.parametrize("name", list(seq.edge_scene_cfgs()))
def test_fixture_edge_scenes(edges, gpu, name):
    """the second recorded set: non-finite and huge values on positive rows"""
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


def test_the_three_kinds_of_head_are_all_among_the_scenes(gold):
    cfgs = dict(seq.scenes(gold))
    assert {c["head"] for c in cfgs.values()} == set(seq.HEADS)
    assert {seq.terms_of(c) for c in cfgs.values()} == {("cls",), ("cls", "box"), ("cls", "part"), ("cls", "part", "box")}


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
    if cfg["B"] * cfg["N"] > 1:
        why = seq.report(through_ops(cfg, inp, gpu, sentinel=False, layout="noncontig"), want, "non-contiguous predictions")
        assert not why, why
    why = seq.report(through_ops(cfg, inp, gpu, sentinel=False, layout="batched"), want, "(B, N, C) predictions")
    assert not why, why
    plain = through_ops(cfg, inp, gpu, want_grad=False)
    assert list(plain) == ["table"] and np.array_equal(plain["table"].view(np.uint32), got["table"].view(np.uint32))
    got_head, _ = through_get_loss(cfg, inp, gpu)
    why = seq.report(got_head, want, "get_loss")
    assert not why, why


def test_backward_scales_by_the_upstream_gradient(gpu):
    cfg = CASES["n257"]
    inp, want, _ = restated(("case", "n257"), cfg)
    got, _ = through_get_loss(cfg, inp, gpu, scale=3.0)
    three = {k: (v * F(3.0) if k != "table" else v) for k, v in want.items()}
    why = seq.report(got, three, "(3 * loss).backward()")
    assert not why, why
    # a second backward through the same loss: the buffers were scaled in place
    head, preds = seq.bare_head(cfg, inp, device=gpu)
    loss, _ = head.get_loss()
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="second time"):
        loss.backward()


def test_gradient_reaches_a_leaf_through_a_linear_layer(gpu):
    cfg = CASES["n257"]
    inp, want, _ = restated(("case", "n257"), cfg)
    head, preds = seq.bare_head(cfg, inp, device=gpu, requires_grad=False)
    R = cfg["B"] * cfg["N"]
    feat = torch.randn((R, 5), device=gpu, generator=torch.Generator(device=gpu).manual_seed(1)).requires_grad_(True)
    lin = torch.nn.Linear(5, 3).to(gpu)
    logits = lin(feat)
    logits.retain_grad()
    head.forward_ret_dict["point_part_preds"] = logits
    loss, tb = head.get_loss()
    loss.backward()
    assert feat.grad is not None and lin.weight.grad is not None and float(feat.grad.abs().sum()) > 0
    # the gradient of the logits is the restatement's on these logits, and the layer hands it on
    want2 = seq.restate(dict(inp, part=logits.detach().cpu().numpy()), cfg)
    got = {"table": seq.outputs_of(loss.item(), tb, {})["table"], "grad_cls": want2["grad_cls"], "grad_part": logits.grad.cpu().numpy(),
           "grad_box": want2["grad_box"]}
    why = seq.report(got, want2)
    assert not why, why
    assert torch.allclose(feat.grad, logits.grad @ lin.weight.detach(), rtol=1e-4, atol=1e-7)
    assert preds["cls"].grad is None and preds["box"].grad is None
    # no prediction requires a gradient: no gradient function, no gradient buffers, the same scalars
    head3, _ = seq.bare_head(cfg, inp, device=gpu, requires_grad=False)
    loss3, tb3 = head3.get_loss()
    assert not loss3.requires_grad and loss3.grad_fn is None
    with torch.no_grad():
        head4, _ = seq.bare_head(cfg, inp, device=gpu)
        loss4, tb4 = head4.get_loss()
    assert not loss4.requires_grad and tb3 == tb4
    assert np.array_equal(seq.outputs_of(loss3.item(), tb3, {})["table"].view(np.uint32), want["table"].view(np.uint32))


def test_one_host_synchronisation_per_get_loss(gpu):
    cfg = CASES["n257"]
    inp, _, _ = restated(("case", "n257"), cfg)
    head, preds = seq.bare_head(cfg, inp, device=gpu)
    head.get_loss()                          # the buffers kept on the head exist from here on
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            loss, tb = head.get_loss()
            loss.backward()
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    assert sum("called a synchronizing" in str(w.message) for w in seen) == 1
    assert head._modest_point_loss_table.is_pinned() and tb["point_loss_cls"] == float(head._modest_point_loss_table[0])


def test_every_limit_raises_one_step_past_it(gpu):
    def call(N=4, C=1, code=8, labels=torch.int32, cls=None, box=True, part=False, **kw):
        z = lambda *s: torch.zeros(s, device=gpu)      # noqa: E731
        return ops.point_loss(z(N, C) if cls is None else cls, torch.ones((N,), dtype=labels, device=gpu),
                              z(N, 3) if part else None, z(N, 3) if part else None,
                              z(N, code) if box else None, z(N, code) if box else None, z(code) if box else None, **kw)
    table, grads = call(C=32, code=16, part=True)
    assert np.isfinite(table.cpu().numpy()).all() and grads[0].shape == (4, 32) and grads[2].shape == (4, 16) and float(table[4]) == 4
    table, grads = call(code=1)
    assert grads[2].shape == (4, 1) and grads[1] is None
    for kw, name in ((dict(C=33), "num_class = 33"), (dict(code=17), "code size = 17"), (dict(cls=torch.zeros((5, 1), device=gpu)),
                                                                                         "cls_preds has 5 elements")):
        with pytest.raises(ValueError, match=name):
            call(**kw)
    with pytest.raises(ValueError, match="code size = 0"):
        ops.point_loss(torch.zeros((4, 1), device=gpu), torch.ones((4,), dtype=torch.int32, device=gpu), None, None,
                       torch.zeros((4, 0), device=gpu), torch.zeros((4, 0), device=gpu), torch.zeros((0,), device=gpu))
    with pytest.raises(TypeError, match="labels must be int32 or int64"):
        call(labels=torch.int16)
    with pytest.raises(ValueError, match="cls_preds must be a device tensor"):
        call(cls=torch.zeros(4, 1))
    with pytest.raises(ValueError, match=f"above the limit of {ops.POINT_LOSS_MAX_ROWS} rows"):
        ops.point_loss(torch.empty((1, 1), device=gpu).expand(ops.POINT_LOSS_MAX_ROWS + 1, 1),
                       torch.empty((1,), dtype=torch.int32, device=gpu).expand(ops.POINT_LOSS_MAX_ROWS + 1))
    # the library's own checks, past the wrapper
    from modest_amd import _lib
    lib = _lib.load()
    assert lib.modest_point_loss_max_rows() == ops.POINT_LOSS_MAX_ROWS
    assert lib.modest_point_loss_workspace_bytes(ops.POINT_LOSS_MAX_ROWS + 1) < 0
    one = torch.zeros((64,), device=gpu)
    p = one.data_ptr()
    args = lambda N, C, code: (N, C, code, p, p, 0, None, None, p, p, p, 0.1, 1.0, 1.0, 1.0, None, None, None, p, p, 256, None)      # noqa: E731
    for a, text in (((4, 33, 8), b"num_class between 1 and 32"), ((4, 0, 8), b"num_class between 1 and 32"),
                    ((4, 1, 17), b"code size between 1 and 16"), ((4, 1, 0), b"code size between 1 and 16"),
                    ((ops.POINT_LOSS_MAX_ROWS + 1, 1, 8), b"n_rows between 0 and 2^24")):
        assert lib.modest_point_loss(*args(*a)) != 0
        assert text in lib.modest_last_error(), (a, lib.modest_last_error())
    assert lib.modest_point_loss_backward(ops.POINT_LOSS_MAX_ROWS * 32 + 1, 0, 0, None, None, None, None, None) != 0
