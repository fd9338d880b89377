"""CPU: pcdet_bind.bind_roi_loss() -- a function of its own that sets
modest_amd.utils.roi_head_loss.get_loss on RoIHeadTemplate of pcdet.models.roi_heads.roi_head_template: None without pcdet,
install()'s signature and keys unchanged, idempotent, bound onto a fake module in sys.modules, a head that overrides a part of
the loss handed to the method that was replaced with its tb_dict, a head class with its own get_loss left alone, and every
NotImplementedError / ValueError naming its option."""
import importlib.util
import inspect
import sys
import types

import pytest

import roi_loss_seq as seq
from modest_amd.utils import pcdet_bind
from modest_amd.utils import roi_head_loss as rhl

NAME = "pcdet.models.roi_heads.roi_head_template"


def saved_modules():
    names = list(pcdet_bind.SHIMS) + list(pcdet_bind.STAND_INS) + ["spconv.utils", NAME]
    return {k: sys.modules.get(k) for k in names}


def restore(saved):
    for k, v in saved.items():
        if v is None:
            sys.modules.pop(k, None)
        else:
            sys.modules[k] = v


def template():
    return type("RoIHeadTemplate", (), {"get_loss": lambda self, tb_dict=None: ("reference", tb_dict),
                                        "get_box_reg_layer_loss": lambda self, d: "reg", "get_box_cls_layer_loss": lambda self, d: "cls",
                                        "assign_targets": lambda self, d: "reference", "proposal_layer": lambda self, d, c: "reference"})


def test_a_function_of_its_own():
    assert pcdet_bind.ROI_LOSS_NAME == NAME and pcdet_bind.ROI_LOSS == "modest_amd.utils.roi_head_loss"
    assert not inspect.signature(pcdet_bind.bind_roi_loss).parameters
    assert list(inspect.signature(pcdet_bind.install).parameters) == [
        "stand_ins", "sparse_conv", "point_stack", "anchor_targets", "roiaware_pool", "sparse_inverse", "point_targets",
        "proposal_layer"]                                                                     # install's signature stays
    params = inspect.signature(rhl.get_loss).parameters
    assert list(params) == ["self", "tb_dict"] and params["tb_dict"].default is None
    assert "bind_roi_loss" in pcdet_bind.__doc__


def test_none_without_pcdet():
    saved = saved_modules()
    try:
        for k in saved:
            sys.modules.pop(k, None)
        if importlib.util.find_spec("pcdet") is None:
            assert pcdet_bind.bind_roi_loss() is None and NAME not in sys.modules
        sys.modules[NAME] = types.ModuleType(NAME)            # a module without the class
        assert pcdet_bind.bind_roi_loss() is None
    finally:
        restore(saved)


def test_binds_onto_a_fake_module_idempotently_and_leaves_overrides_and_install_alone():
    saved = saved_modules()
    try:
        for k in saved:
            sys.modules.pop(k, None)
        before = sorted(pcdet_bind.install())
        fake = types.ModuleType(NAME)
        fake.RoIHeadTemplate = template()
        reference = fake.RoIHeadTemplate.__dict__["get_loss"]
        plain = type("PointRCNNHead", (fake.RoIHeadTemplate,), {})
        own_reg = type("OwnReg", (fake.RoIHeadTemplate,), {"get_box_reg_layer_loss": lambda self, d: "its own"})
        own_cls = type("OwnCls", (fake.RoIHeadTemplate,), {"get_box_cls_layer_loss": lambda self, d: "its own"})
        second = type("SECONDHead", (fake.RoIHeadTemplate,), {"get_loss": lambda self, tb_dict=None: "its own get_loss"})
        sys.modules[NAME] = fake
        assert plain().get_loss() == ("reference", None)
        assert pcdet_bind.bind_roi_loss() is fake and pcdet_bind.bind_roi_loss() is fake                 # idempotent
        assert fake.RoIHeadTemplate.get_loss is rhl.get_loss and plain.get_loss is rhl.get_loss
        assert rhl._ORIGINAL[fake.RoIHeadTemplate] is reference                                          # a second call changed nothing
        passed = {"kept": 1}
        assert own_reg().get_loss(passed) == ("reference", passed) and own_cls().get_loss() == ("reference", None)   # both kinds
        assert second().get_loss() == "its own get_loss"                                                 # only the template's attribute is set
        assert fake.RoIHeadTemplate.assign_targets(None, None) == "reference"                            # nothing else is touched
        assert fake.RoIHeadTemplate.proposal_layer(None, None, None) == "reference"
        assert sorted(pcdet_bind.install()) == before and NAME not in pcdet_bind.install()               # install's keys stay
    finally:
        restore(saved)


def test_bind_is_inherited_and_keeps_an_inherited_original():
    base = type("Base", (), {"get_loss": lambda self, tb_dict=None: "inherited", "get_box_reg_layer_loss": lambda self, d: 0,
                             "get_box_cls_layer_loss": lambda self, d: 0})
    mid = type("Template", (base,), {})
    sub = type("Sub", (mid,), {"get_box_reg_layer_loss": lambda self, d: 1})
    assert rhl.bind(mid) is mid and rhl.bind(mid) is mid and sub.get_loss is rhl.get_loss
    assert rhl._ORIGINAL[mid] is None and sub().get_loss() == "inherited"


def head_for(**kw):
    cfg = seq.base_cfg(B=1, M=70, seed=2, **kw)
    inp = seq.make_inputs(cfg)
    return seq.bare_head(cfg, inp)


def test_every_option_that_is_not_provided_is_named():
    import torch
    from modest_amd import ops
    for key, value, match in (("CLS_LOSS", "CrossEntropy", "CLS_LOSS: CrossEntropy"), ("REG_LOSS", "l1", "REG_LOSS: l1")):
        head, _ = head_for()
        head.model_cfg.LOSS_CONFIG[key] = value
        with pytest.raises(NotImplementedError, match=match):
            rhl.get_loss(head)
    head, _ = head_for()
    head.box_coder = seq.loss_stub("PreviousResidualDecoder", code_size=7)
    with pytest.raises(NotImplementedError, match="BOX_CODER: PreviousResidualDecoder"):
        rhl.get_loss(head)
    head, _ = head_for()
    head.box_coder.encode_angle_by_sincos = True
    with pytest.raises(NotImplementedError, match="encode_angle_by_sincos"):
        rhl.get_loss(head)
    head, _ = head_for()
    head.reg_loss_func = seq.loss_stub("WeightedL1Loss")
    with pytest.raises(NotImplementedError, match="reg_loss_func = WeightedL1Loss"):
        rhl.get_loss(head)
    for key in ("rcnn_cls", "rcnn_reg"):
        head, _ = head_for()
        head.forward_ret_dict[key] = head.forward_ret_dict[key].detach().half()
        with pytest.raises(NotImplementedError, match=key + " of torch.float16"):
            rhl.get_loss(head)
    # the limits, one step past each
    for code in (ops.ROI_LOSS_MIN_CODE - 1, ops.ROI_LOSS_MAX_CODE + 1):
        head, _ = head_for()
        head.box_coder.code_size = code
        with pytest.raises(ValueError, match=f"code size = {code} is outside the limit of 7 .. 16"):
            rhl.get_loss(head)
    head, _ = head_for()
    head.forward_ret_dict["rcnn_cls"] = torch.zeros((71, 1))
    with pytest.raises(ValueError, match="rcnn_cls has 71 elements, reg_valid_mask 70 rows"):
        rhl.get_loss(head)
    head, _ = head_for()
    head.forward_ret_dict["rcnn_reg"] = torch.zeros((70, 8))
    with pytest.raises(ValueError, match="rcnn_reg has 560 elements"):
        rhl.get_loss(head)
    head, _ = head_for()
    wide = ops.ROI_LOSS_MAX_ROWS + 1
    head.forward_ret_dict["reg_valid_mask"] = torch.zeros((1, 1), dtype=torch.int64).expand(1, wide)
    with pytest.raises(ValueError, match=f"reg_valid_mask has {wide} rows, above the limit of {ops.ROI_LOSS_MAX_ROWS}"):
        rhl.get_loss(head)
    head, _ = head_for()                                          # everything in order but the device
    with pytest.raises(ValueError, match="rcnn_cls must be a device tensor"):
        rhl.get_loss(head)
    assert (ops.ROI_LOSS_MIN_CODE, ops.ROI_LOSS_MAX_CODE, ops.ROI_LOSS_MAX_ROWS) == (7, 16, 1 << 20)


def test_rows_are_views_wherever_the_stride_allows():
    import torch
    gt = torch.arange(2 * 5 * 8, dtype=torch.float32).view(2, 5, 8)
    rows = rhl._rows(gt, 7, "gt_of_rois")
    assert rows.shape == (10, 8) and rows.data_ptr() == gt.data_ptr() and rows.stride() == (8, 1)      # the class column stays behind
    sliced = gt[..., 0:7]
    rows = rhl._rows(sliced, 7, "gt_of_rois")
    assert rows.shape == (10, 7) and rows.data_ptr() == gt.data_ptr() and rows.stride() == (8, 1)       # the slice: still no copy
    odd = gt.transpose(0, 1)[..., ::2]
    assert torch.equal(rhl._rows(odd, 4, "gt_of_rois"), odd.reshape(10, 4)) and rhl._rows(odd, 4, "gt_of_rois").is_contiguous()
    with pytest.raises(ValueError, match="gt_of_rois has 6 columns"):
        rhl._rows(gt[..., 0:6], 7, "gt_of_rois")
