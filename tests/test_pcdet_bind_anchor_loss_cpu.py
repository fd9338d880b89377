"""CPU: pcdet_bind.bind_anchor_loss() -- a function of its own that sets
modest_amd.utils.anchor_head_loss.get_loss on AnchorHeadTemplate of pcdet.models.dense_heads.anchor_head_template: None without
pcdet, install()'s signature and keys unchanged, idempotent, bound onto a fake module in sys.modules, a head that overrides a
part of the loss handed to the method that was replaced, and every NotImplementedError / ValueError naming its option."""
import importlib.util
import inspect
import sys
import types

import numpy as np
import pytest

import anchor_loss_seq as seq
from modest_amd.utils import anchor_head_loss as ahl
from modest_amd.utils import pcdet_bind

NAME = "pcdet.models.dense_heads.anchor_head_template"


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
    return type("AnchorHeadTemplate", (), {"get_loss": lambda self: "reference",
                                           "get_cls_layer_loss": lambda self: "cls", "get_box_reg_layer_loss": lambda self: "box",
                                           "assign_targets": lambda self, gt: "reference"})


def test_a_function_of_its_own():
    assert pcdet_bind.ANCHOR_LOSS_NAME == NAME and pcdet_bind.ANCHOR_LOSS == "modest_amd.utils.anchor_head_loss"
    assert not inspect.signature(pcdet_bind.bind_anchor_loss).parameters
    assert list(inspect.signature(pcdet_bind.install).parameters) == [
        "stand_ins", "sparse_conv", "point_stack", "anchor_targets", "roiaware_pool", "sparse_inverse", "point_targets",
        "proposal_layer"]                                                                     # install's signature stays
    assert list(inspect.signature(ahl.get_loss).parameters) == ["self"]


def test_none_without_pcdet():
    saved = saved_modules()
    try:
        for k in saved:
            sys.modules.pop(k, None)
        if importlib.util.find_spec("pcdet") is None:
            assert pcdet_bind.bind_anchor_loss() is None and NAME not in sys.modules
        sys.modules[NAME] = types.ModuleType(NAME)            # a module without the class
        assert pcdet_bind.bind_anchor_loss() is None
    finally:
        restore(saved)


def test_binds_onto_a_fake_module_idempotently_and_leaves_overrides_and_install_alone():
    saved = saved_modules()
    try:
        for k in saved:
            sys.modules.pop(k, None)
        before = sorted(pcdet_bind.install())
        fake = types.ModuleType(NAME)
        fake.AnchorHeadTemplate = template()
        reference = fake.AnchorHeadTemplate.__dict__["get_loss"]
        single = type("AnchorHeadSingle", (fake.AnchorHeadTemplate,), {})
        multi = type("AnchorHeadMulti", (fake.AnchorHeadTemplate,), {"get_cls_layer_loss": lambda self: "its own"})
        multi_box = type("Other", (fake.AnchorHeadTemplate,), {"get_box_reg_layer_loss": lambda self: "its own"})
        own = type("Own", (fake.AnchorHeadTemplate,), {"get_loss": lambda self: "its own get_loss"})
        sys.modules[NAME] = fake
        assert single().get_loss() == "reference"
        assert pcdet_bind.bind_anchor_loss() is fake and pcdet_bind.bind_anchor_loss() is fake           # idempotent
        assert fake.AnchorHeadTemplate.get_loss is ahl.get_loss and single.get_loss is ahl.get_loss
        assert ahl._ORIGINAL[fake.AnchorHeadTemplate] is reference                                      # a second call changed nothing
        assert multi().get_loss() == "reference" and multi_box().get_loss() == "reference"              # a part overridden: the original
        assert own().get_loss() == "its own get_loss"
        assert fake.AnchorHeadTemplate.assign_targets(None, None) == "reference"                         # nothing else is touched
        assert sorted(pcdet_bind.install()) == before and NAME not in pcdet_bind.install()               # install's keys stay
    finally:
        restore(saved)


def test_bind_is_inherited_and_keeps_an_inherited_original():
    base = type("Base", (), {"get_loss": lambda self: "inherited", "get_cls_layer_loss": lambda self: 0,
                             "get_box_reg_layer_loss": lambda self: 0})
    mid = type("Template", (base,), {})
    sub = type("Sub", (mid,), {"get_box_reg_layer_loss": lambda self: 1})
    assert ahl.bind(mid) is mid and ahl.bind(mid) is mid and sub.get_loss is ahl.get_loss
    assert ahl._ORIGINAL[mid] is None and sub().get_loss() == "inherited"


def head_for(**kw):
    cfg = seq.base_cfg(B=1, N=70, seed=2, pos=0.2, **kw)
    inp = seq.make_inputs(cfg)
    return seq.bare_head(cfg, inp)


def test_every_option_that_is_not_provided_is_named():
    import torch
    head, _ = head_for()
    head.model_cfg["USE_MULTIHEAD"] = True
    with pytest.raises(NotImplementedError, match="USE_MULTIHEAD"):
        ahl.get_loss(head)
    head, _ = head_for()
    head.use_multihead = True
    with pytest.raises(NotImplementedError, match="USE_MULTIHEAD"):
        ahl.get_loss(head)
    for attr, name in (("cls_loss_func", "cls_loss_func"), ("reg_loss_func", "reg_loss_func"), ("dir_loss_func", "dir_loss_func")):
        head, _ = head_for()
        setattr(head, attr, seq.loss_stub("SomethingElse"))
        with pytest.raises(NotImplementedError, match=name + " = SomethingElse"):
            ahl.get_loss(head)
    head, _ = head_for()
    head.cls_loss_func = seq.loss_stub("SigmoidFocalClassificationLoss", alpha=0.25, gamma=1.5)
    with pytest.raises(NotImplementedError, match="gamma = 1.5"):
        ahl.get_loss(head)
    head, _ = head_for(bins=0)
    head.dir_loss_func = seq.loss_stub("SomethingElse")          # not read without a direction head
    with pytest.raises(ValueError, match="device"):
        ahl.get_loss(head)
    for key in ("cls_preds", "box_preds", "dir_cls_preds"):
        head, _ = head_for()
        head.forward_ret_dict[key] = head.forward_ret_dict[key].detach().half()
        with pytest.raises(NotImplementedError, match=key + " of torch.float16"):
            ahl.get_loss(head)
    # the limits, one step past each
    from modest_amd import ops
    for kw, name in ((dict(num_class=ops.ANCHOR_LOSS_MAX_CLASS + 1), "num_class = 33"), (dict(code=ops.ANCHOR_LOSS_MAX_CODE + 1), "code size = 17"),
                     (dict(bins=ops.ANCHOR_LOSS_MAX_BINS + 1), "NUM_DIR_BINS = 9")):
        head, _ = head_for(**kw)
        with pytest.raises(ValueError, match=name + " is above the limit"):
            ahl.get_loss(head)
    head, _ = head_for()
    wide = ops.ANCHOR_LOSS_MAX_BATCH + 1
    for key, cols in (("cls_preds", 3), ("box_preds", 7), ("dir_cls_preds", 2)):
        head.forward_ret_dict[key] = torch.zeros((1, 1, cols)).expand(wide, 1, cols)
    with pytest.raises(ValueError, match="batch_size = 65536 is above the limit of 65535"):
        ahl.get_loss(head)
    assert (ops.ANCHOR_LOSS_MAX_CLASS, ops.ANCHOR_LOSS_MAX_CODE, ops.ANCHOR_LOSS_MAX_BINS, ops.ANCHOR_LOSS_MAX_BATCH) == (32, 16, 8, 65535)


def test_the_anchor_cache_is_keyed_on_the_tensors():
    head, _ = head_for()
    flat = ahl._flat_anchors(head)
    assert ahl._flat_anchors(head) is flat and flat.shape == (70, 7)
    assert np.array_equal(flat.numpy(), head.anchors[0].reshape(-1, 7).numpy())
    head.anchors[0].add_(1.0)                                    # written in place: rebuilt
    again = ahl._flat_anchors(head)
    assert again is not flat and np.array_equal(again.numpy(), head.anchors[0].reshape(-1, 7).numpy())
    head.anchors = head.anchors[0].reshape(-1, 7).clone()       # a tensor instead of a list
    assert ahl._flat_anchors(head).shape == (70, 7)
