"""GPU: the box decoding kernels (csrc/box_decode.hip) against the numpy restatement
tests/box_decode_seq.py BIT FOR BIT -- every element -- on the recorded scenes (tests/golden/box_decode.npz) and the named
cases (tests/box_decode_cases.py), through ops.anchor_decode / point_decode / roi_decode into sentinel-filled outputs and
through the three drop-in methods on minimal stand-in heads; inputs unchanged, no grad_fn on the boxes while the class
predictions keep theirs, no host synchronisation, the same bits on a second call, one mid-size run per head, and the refusals
of the ops and of the library, one step past each limit.  A mismatch reports the element."""
import os
import warnings

import numpy as np
import pytest
import torch

import box_decode_seq as seq
from box_decode_cases import CASES, MID
from modest_amd import ops

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "box_decode.npz")
F = np.float32
SENTINEL = 0x5A5A5A5A
_restated = {}


@pytest.fixture(scope="module")
def gold():
    return {name: (case, out) for name, case, out in seq.scenes(dict(np.load(GOLD)))}


def restated(key, case):
    """the restatement of a case, computed once and left unchanged"""
    if key not in _restated:
        _restated[key] = seq.restate(case)
    return _restated[key]


def through_ops(case, gpu, sentinel=True):
    """-> (boxes as numpy, the device inputs, their clones taken before the call)"""
    to = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)      # noqa: E731
    shape = seq.restate_shape(case)
    out = torch.full(shape, SENTINEL, dtype=torch.int32, device=gpu).view(torch.float32) if sentinel else None
    if case["kind"] == "anchor":
        inputs = [to(case["box"]), to(case["anchors"]), to(case.get("dir"))]
        before = [None if t is None else t.clone() for t in inputs]
        boxes = ops.anchor_decode(*inputs, dir_offset=case["dir_offset"], dir_limit_offset=case["dir_limit_offset"],
                                  sincos=case["sincos"], out=out)
    elif case["kind"] == "point":
        coords = to(case["coords"])
        points = coords[:, 1:4]                                       # the caller's strided view, read in place
        assert not points.is_contiguous() or len(coords) == 1
        inputs = [to(case["box"]), coords, to(case["cls"]), to(case.get("mean"))]
        before = [None if t is None else t.clone() for t in inputs]
        boxes = ops.point_decode(inputs[0], points, inputs[2], inputs[3], out=out)
    else:
        inputs = [to(case["rois"]), to(case["box"])]
        before = [t.clone() for t in inputs]
        boxes = ops.roi_decode(*inputs, out=out)
        shape = (shape[0], shape[1])
    assert tuple(boxes.shape) == shape and boxes.dtype == torch.float32 and not boxes.requires_grad
    assert out is None or boxes is out
    for a, b in zip(inputs, before):
        assert a is None or torch.equal(a.view(torch.int32), b.view(torch.int32))          # inputs are left untouched
    return boxes.cpu().numpy()


def through_head(case, gpu, per_class=None):
    head, args = seq.bare_head(case, device=gpu, per_class=per_class)
    before = [a.detach().clone() if torch.is_tensor(a) else a for a in args]
    cls_out, boxes = head.generate_predicted_boxes(*args)
    for a, b in zip(args, before):
        assert not torch.is_tensor(a) or torch.equal(a.detach().view(torch.int32), b.view(torch.int32))
    assert not boxes.requires_grad and boxes.grad_fn is None and boxes.dtype == torch.float32
    shape = seq.restate_shape(case)
    if case["kind"] == "anchor":
        assert tuple(boxes.shape) == shape and tuple(cls_out.shape) == (shape[0], shape[1], 2)
        assert cls_out.requires_grad and cls_out.grad_fn is not None and cls_out._base is args[1]      # a view: its graph is kept
    elif case["kind"] == "point":
        assert tuple(boxes.shape) == shape and cls_out is args[1] and cls_out.requires_grad
    else:
        B, M, code = case["rois"].shape
        assert tuple(boxes.shape) == (B, M, code) and tuple(cls_out.shape) == (B, M, 1)
        assert cls_out.requires_grad and cls_out._base is args[2]
    return boxes.cpu().numpy().reshape(shape)


SCENES = ["anchor_code7_dir", "anchor_code9_dir", "anchor_code7", "anchor_sincos", "point_k3", "point_k1", "point_no_mean",
          "roi_2x3", "roi_4x100"]


@pytest.mark.parametrize("name", SCENES)
def test_recorded_scenes(gold, gpu, name):
    case, rec = gold[name]
    want = restated(("gold", name), case)
    per_class = seq.anchor_grid(extra=want.shape[-1] - 7, seed=int(1 + SCENES.index(name))) if case["kind"] == "anchor" else None
    if per_class is not None:
        assert seq.same_bits(seq.flat_anchors(per_class), case["anchors"])                  # the list of per-class tensors, as a head holds it
    for how, got in (("ops", through_ops(case, gpu)), ("the method", through_head(case, gpu, per_class))):
        why = seq.report(got, want, how + ":")
        assert not why, f"against the restatement\n{why}"
        why, _ = seq.bound_report(got, seq.exact(case), "the device")
        assert not why, why
        why = seq.pattern_report(got, rec)
        assert not why, why
        cols = seq.exact_columns(case)
        why = seq.report(got[..., cols], rec.reshape(got.shape)[..., cols], f"{how}: columns {cols} of the recording:")
        assert not why, why


@pytest.mark.parametrize("name", sorted(CASES))
def test_named_cases(gpu, name):
    case = CASES[name]
    want = restated(("case", name), case)
    got = through_ops(case, gpu)                         # into a sentinel-filled output
    why = seq.report(got, want, "ops:")
    assert not why, why
    assert not (got.view(np.uint32) == SENTINEL).any()   # every element is written
    again = through_ops(case, gpu, sentinel=False)
    assert seq.same_bits(got, again)                     # the same bits on a second call, into torch.empty
    why = seq.report(through_head(case, gpu), want, "the method:")
    assert not why, why


@pytest.mark.parametrize("kind", sorted(MID))
def test_mid_size_run(gpu, kind):
    """more than one tile per workgroup column (and, for the anchors, the batch walked inside a workgroup)"""
    case = MID[kind]
    want = restated(("mid", kind), case)
    got = through_ops(case, gpu)
    why = seq.report(got, want, "ops:")
    assert not why, why
    assert seq.same_bits(got, through_ops(case, gpu, sentinel=False))
    why = seq.report(through_head(case, gpu), want, "the method:")
    assert not why, why


@pytest.mark.parametrize("kind", sorted(MID))
def test_no_host_synchronisation(gpu, kind):
    head, args = seq.bare_head(MID[kind], device=gpu)
    head.generate_predicted_boxes(*args)                 # the anchors' table exists from here on
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            _, boxes = head.generate_predicted_boxes(*args)
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    assert sum("called a synchronizing" in str(w.message) for w in seen) == 0
    why = seq.report(boxes.cpu().numpy().reshape(seq.restate_shape(MID[kind])), restated(("mid", kind), MID[kind]))
    assert not why, why


def test_on_another_stream_and_with_points_of_any_row_stride(gpu):
    case = CASES["point_rows257"]
    want = restated(("case", "point_rows257"), case)
    wide = torch.zeros((257, 9), device=gpu)
    wide[:, 5:8] = torch.from_numpy(case["coords"][:, 1:4]).to(gpu)
    box, cls, mean = (torch.from_numpy(case[k]).to(gpu) for k in ("box", "cls", "mean"))
    stream = torch.cuda.Stream(device=gpu)
    stream.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(stream):
        got = ops.point_decode(box, wide[:, 5:8], cls, mean)
    stream.synchronize()
    why = seq.report(got.cpu().numpy(), want)
    assert not why, why


def test_every_refusal_of_the_ops_and_of_the_library(gpu):
    z = lambda *s: torch.zeros(s, device=gpu)      # noqa: E731
    past = ops.BOX_DECODE_MAX_ROWS + 1
    # the limits, at them and one step past
    assert ops.anchor_decode(z(1, 4, 16), z(4, 16), z(1, 4, 8)).shape == (1, 4, 16)
    assert ops.anchor_decode(z(1, 4, 16), z(4, 15), z(1, 4, 1), sincos=True).shape == (1, 4, 15)
    assert ops.point_decode(z(4, 16), z(4, 3), z(4, 32), z(32, 3) + 1).shape == (4, 15)
    assert ops.roi_decode(z(2, 2, 16), z(4, 16)).shape == (4, 16)
    assert ops.anchor_decode(z(0, 4, 7), z(4, 7)).shape == (0, 4, 7) and ops.point_decode(z(0, 8), z(0, 3), z(0, 3)).shape == (0, 7)
    for fn, match in ((lambda: ops.anchor_decode(z(1, 4, 17), z(4, 17)), "code size = 17 is outside the limit of 7 .. 16"),
                      (lambda: ops.anchor_decode(z(1, 4, 6), z(4, 6)), "code size = 6 is outside the limit of 7 .. 16"),
                      (lambda: ops.anchor_decode(z(1, 4, 7), z(4, 6), sincos=True), "code size = 7 is outside the limit of 8 .. 16"),
                      (lambda: ops.anchor_decode(z(1, 4, 7), z(4, 7), z(1, 4, 9)), "NUM_DIR_BINS = 9 is outside the limit of 1 .. 8"),
                      (lambda: ops.anchor_decode(z(1, 4, 7), z(4, 7), z(1, 4, 0)), "NUM_DIR_BINS = 0 is outside the limit of 1 .. 8"),
                      (lambda: ops.anchor_decode(z(1, 4, 7), z(5, 7)), "anchors \\(5, 7\\) must be"),
                      (lambda: ops.anchor_decode(z(1, 1, 1).expand(past // 4 + 1, 4, 7), z(4, 7)), f"above the limit of {ops.BOX_DECODE_MAX_ROWS} rows"),
                      (lambda: ops.anchor_decode(z(1, 4, 14)[:, :, ::2], z(4, 7)), "box_preds must be contiguous"),
                      (lambda: ops.point_decode(z(4, 17), z(4, 3), z(4, 3)), "code size = 17 is outside the limit of 8 .. 16"),
                      (lambda: ops.point_decode(z(4, 7), z(4, 3), z(4, 3)), "code size = 7 is outside the limit of 8 .. 16"),
                      (lambda: ops.point_decode(z(4, 8), z(4, 3), z(4, 33)), "num_class = 33 is outside the limit of 1 .. 32"),
                      (lambda: ops.point_decode(z(4, 8), z(4, 3), z(4, 0)), "num_class = 0 is outside the limit of 1 .. 32"),
                      (lambda: ops.point_decode(z(4, 8), z(4, 3), z(4, 3), z(2, 3)), "mean_size \\(2, 3\\) must be"),
                      (lambda: ops.point_decode(z(4, 8), z(3, 4).t(), z(4, 3)), "points must have unit column stride"),
                      (lambda: ops.point_decode(z(1, 1).expand(past, 8), z(4, 3), z(1, 1).expand(past, 3)), f"above the limit of {ops.BOX_DECODE_MAX_ROWS} rows"),
                      (lambda: ops.roi_decode(z(4, 17), z(4, 17)), "code size = 17 is outside the limit of 7 .. 16"),
                      (lambda: ops.roi_decode(z(4, 6), z(4, 6)), "code size = 6 is outside the limit of 7 .. 16"),
                      (lambda: ops.roi_decode(z(5, 7), z(4, 7)), "rois \\(5, 7\\) must hold 4 rows"),
                      (lambda: ops.roi_decode(z(1, 1).expand(past, 7), z(1, 1).expand(past, 7)), f"above the limit of {ops.BOX_DECODE_MAX_ROWS} rows"),
                      (lambda: ops.roi_decode(z(4, 7), z(4, 7), out=z(4, 8)), "out must be a contiguous float32 \\(4, 7\\)"),
                      (lambda: ops.roi_decode(torch.zeros(4, 7), z(4, 7)), "rois must be a device tensor")):
        with pytest.raises(ValueError, match=match):
            fn()
    with pytest.raises(TypeError, match="box_preds must be float32"):
        ops.roi_decode(z(4, 7), z(4, 7).half())
    # the library's own checks, past the wrapper: nothing is launched
    from modest_amd import _lib
    lib = _lib.load()
    assert lib.modest_box_decode_max_rows() == ops.BOX_DECODE_MAX_ROWS
    p = z(64).data_ptr()
    for fn, text in ((lambda: lib.modest_anchor_decode(1, 4, 17, 0, p, p, None, 0, 0.0, 0.0, p, None), b"code size between 7 (8 with sincos) and 16"),
                     (lambda: lib.modest_anchor_decode(1, 4, 7, 1, p, p, None, 0, 0.0, 0.0, p, None), b"code size between 7 (8 with sincos) and 16"),
                     (lambda: lib.modest_anchor_decode(1, 4, 7, 0, p, p, p, 9, 0.0, 0.0, p, None), b"bins between 1 and 8"),
                     (lambda: lib.modest_anchor_decode(1, 4, 7, 0, p, p, p, 0, 0.0, 0.0, p, None), b"bins between 1 and 8"),
                     (lambda: lib.modest_anchor_decode(2, 1 << 30, 7, 0, p, p, None, 0, 0.0, 0.0, p, None), b"batch * n_anchors at most 2^31 - 1"),
                     (lambda: lib.modest_anchor_decode(1, 4, 7, 0, p, None, None, 0, 0.0, 0.0, p, None), b"NULL buffer"),
                     (lambda: lib.modest_anchor_decode(1, 4, 7, 0, p + 2, p, None, 0, 0.0, 0.0, p, None), b"unaligned buffer"),
                     (lambda: lib.modest_point_decode(past, 8, 3, p, p, 3, p, None, p, None), b"n_rows between 0 and 2^31 - 1"),
                     (lambda: lib.modest_point_decode(4, 17, 3, p, p, 3, p, None, p, None), b"code size between 8 and 16"),
                     (lambda: lib.modest_point_decode(4, 8, 33, p, p, 3, p, None, p, None), b"num_class between 1 and 32"),
                     (lambda: lib.modest_point_decode(4, 8, 3, p, p, 2, p, None, p, None), b"row stride of the points of at least 3"),
                     (lambda: lib.modest_point_decode(4, 8, 3, p, p, 3, None, None, p, None), b"NULL buffer"),
                     (lambda: lib.modest_roi_decode(4, 6, p, p, p, None), b"code size between 7 and 16"),
                     (lambda: lib.modest_roi_decode(-1, 7, p, p, p, None), b"n_rows between 0 and 2^31 - 1"),
                     (lambda: lib.modest_roi_decode(4, 7, p, p, None, None), b"NULL buffer")):
        rc = fn()                                          # one at a time: the error text is the last call's
        assert rc != 0 and text in lib.modest_last_error(), (text, lib.modest_last_error())
