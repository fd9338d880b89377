"""CPU: pcdet_bind.bind_point_loss() -- a function of its own that sets
modest_amd.utils.point_head_loss.get_loss on PointHeadBox, PointHeadSimple and PointIntraPartOffsetHead of
pcdet.models.dense_heads: None without pcdet, install()'s signature and keys unchanged, idempotent, bound onto fake modules in
sys.modules, a module without its class skipped, a head that overrides a part of the loss handed to the method that was
replaced with its tb_dict, and every NotImplementedError / ValueError naming its option."""
import importlib.util
import inspect
import sys
import types

import pytest

import point_loss_seq as seq
from modest_amd.utils import pcdet_bind
from modest_amd.utils import point_head_loss as phl

NAMES = {"pcdet.models.dense_heads.point_head_box": "PointHeadBox", "pcdet.models.dense_heads.point_head_simple": "PointHeadSimple",
         "pcdet.models.dense_heads.point_intra_part_head": "PointIntraPartOffsetHead"}
PARTS = ("get_cls_layer_loss", "get_part_layer_loss", "get_box_layer_loss")


def saved_modules():
    names = list(pcdet_bind.SHIMS) + list(pcdet_bind.STAND_INS) + ["spconv.utils"] + list(NAMES)
    return {k: sys.modules.get(k) for k in names}


def restore(saved):
    for k, v in saved.items():
        if v is None:
            sys.modules.pop(k, None)
        else:
            sys.modules[k] = v


def fake_modules():
    """the three modules, each head with a get_loss of its own over a shared template, as the reference has them"""
    template = type("PointHeadTemplate", (), dict({p: (lambda self, tb_dict=None: "reference") for p in PARTS},
                                                  assign_stack_targets=lambda self, *a, **k: "reference"))
    mods = {}
    for name, cls_name in NAMES.items():
        mod = types.ModuleType(name)
        setattr(mod, cls_name, type(cls_name, (template,), {"get_loss": lambda self, tb_dict=None, n=cls_name: (n, tb_dict)}))
        mods[name] = mod
    return template, mods


def test_a_function_of_its_own():
    assert pcdet_bind.POINT_LOSS_NAMES == NAMES and pcdet_bind.POINT_LOSS == "modest_amd.utils.point_head_loss"
    assert not inspect.signature(pcdet_bind.bind_point_loss).parameters
    assert list(inspect.signature(pcdet_bind.install).parameters) == [
        "stand_ins", "sparse_conv", "point_stack", "anchor_targets", "roiaware_pool", "sparse_inverse", "point_targets",
        "proposal_layer"]                                                                     # install's signature stays
    params = inspect.signature(phl.get_loss).parameters
    assert list(params) == ["self", "tb_dict"] and params["tb_dict"].default is None
    assert "bind_point_loss" in pcdet_bind.__doc__
    assert phl.TERMS == {"PointHeadSimple": ("cls",), "PointHeadBox": ("cls", "box"), "PointIntraPartOffsetHead": ("cls", "part", "box?")}


def test_none_without_pcdet_and_a_module_without_its_class_is_skipped():
    saved = saved_modules()
    try:
        for k in saved:
            sys.modules.pop(k, None)
        if importlib.util.find_spec("pcdet") is None:
            assert pcdet_bind.bind_point_loss() is None and not any(n in sys.modules for n in NAMES)
        template, mods = fake_modules()
        name = "pcdet.models.dense_heads.point_head_simple"
        sys.modules[name] = types.ModuleType(name)                  # a module without the class
        if importlib.util.find_spec("pcdet") is None:
            assert pcdet_bind.bind_point_loss() == {}                   # found, nothing to bind
        box = "pcdet.models.dense_heads.point_head_box"
        sys.modules[box] = mods[box]
        bound = pcdet_bind.bind_point_loss()
        assert bound[box] is mods[box] and name not in bound and mods[box].PointHeadBox.get_loss is phl.get_loss
    finally:
        restore(saved)


def test_binds_onto_fake_modules_idempotently_and_leaves_overrides_and_install_alone():
    saved = saved_modules()
    try:
        for k in saved:
            sys.modules.pop(k, None)
        before = sorted(pcdet_bind.install())
        template, mods = fake_modules()
        originals = {n: getattr(mods[n], c).__dict__["get_loss"] for n, c in NAMES.items()}
        sys.modules.update(mods)
        bound = pcdet_bind.bind_point_loss()
        assert bound == mods and pcdet_bind.bind_point_loss() == mods                                     # idempotent
        for name, cls_name in NAMES.items():
            head = getattr(mods[name], cls_name)
            assert head.get_loss is phl.get_loss and phl._ORIGINAL[head] is originals[name]             # a second call changed nothing
            assert phl._TERMS[head] == phl.TERMS[cls_name]
            for part in PARTS:                                                                          # an override below the bound class
                own = type("Own", (head,), {part: lambda self, tb_dict=None: "its own"})
                passed = {"kept": 1}
                assert own().get_loss(passed) == (cls_name, passed) and own().get_loss() == (cls_name, None)
            mine = type("Mine", (head,), {"get_loss": lambda self, tb_dict=None: "its own get_loss"})
            assert mine().get_loss() == "its own get_loss"
        assert "get_loss" not in template.__dict__ and template.assign_stack_targets(None) == "reference"   # the template is not touched
        assert sorted(pcdet_bind.install()) == before and not any(n in pcdet_bind.install() for n in NAMES)   # install's keys stay
    finally:
        restore(saved)


def test_bind_needs_terms_for_an_unknown_class_and_keeps_an_inherited_original():
    base = type("Base", (), dict({p: (lambda self, tb_dict=None: 0) for p in PARTS}, get_loss=lambda self, tb_dict=None: "inherited"))
    mid = type("MyPointHead", (base,), {})
    with pytest.raises(ValueError, match="bind\\(MyPointHead\\) needs its terms"):
        phl.bind(mid)
    with pytest.raises(ValueError, match="terms = \\('part',\\)"):
        phl.bind(mid, ("part",))
    assert phl.bind(mid, ("cls", "box")) is mid and phl.bind(mid) is mid and phl._TERMS[mid] == ("cls", "box")
    sub = type("Sub", (mid,), {"get_box_layer_loss": lambda self, tb_dict=None: 1})
    assert sub.get_loss is phl.get_loss and phl._ORIGINAL[mid] is None and sub().get_loss() == "inherited"


def head_for(head="PointIntraPartOffsetHead", **kw):
    cfg = seq.base_cfg(head=head, B=1, N=70, num_class=3, seed=2, **kw)
    inp = seq.make_inputs(cfg)
    return seq.bare_head(cfg, inp)


def test_every_option_that_is_not_provided_is_named():
    import torch
    from modest_amd import ops
    head, _ = head_for()
    head.cls_loss_func = seq.loss_stub("WeightedCrossEntropyLoss")
    with pytest.raises(NotImplementedError, match="cls_loss_func = WeightedCrossEntropyLoss"):
        head.get_loss()
    for attr, value in (("alpha", 0.5), ("gamma", 1.0)):
        head, _ = head_for()
        setattr(head.cls_loss_func, attr, value)
        with pytest.raises(NotImplementedError, match=f"{attr} = {value}"):
            head.get_loss()
    for kind in ("PointHeadBox", "PointIntraPartOffsetHead"):
        head, _ = head_for(kind)
        head.reg_loss_func = torch.nn.functional.smooth_l1_loss
        with pytest.raises(NotImplementedError, match="reg_loss_func = smooth_l1_loss"):
            head.get_loss()
        head.reg_loss_func = seq.loss_stub("WeightedL1Loss")
        with pytest.raises(NotImplementedError, match="reg_loss_func = WeightedL1Loss"):
            head.get_loss()
    # without the box term the reg_loss_func is not looked at: the next refusal is the device's
    for kind, kw in (("PointHeadSimple", {}), ("PointIntraPartOffsetHead", dict(box_layers=False))):
        head, _ = head_for(kind, **kw)
        assert head.reg_loss_func is torch.nn.functional.smooth_l1_loss
        with pytest.raises(ValueError, match="point_cls_preds must be a device tensor"):
            head.get_loss()
    for key in ("point_cls_preds", "point_part_preds", "point_box_preds"):
        head, _ = head_for()
        head.forward_ret_dict[key] = head.forward_ret_dict[key].detach().half()
        with pytest.raises(NotImplementedError, match=key + " of torch.float16"):
            head.get_loss()
    # the limits, one step past each
    for classes in (0, ops.POINT_LOSS_MAX_CLASS + 1):
        head, _ = head_for()
        head.num_class = classes
        with pytest.raises(ValueError, match=f"num_class = {classes} is outside the limit of 1 .. 32"):
            head.get_loss()
    for code in (0, ops.POINT_LOSS_MAX_CODE + 1):
        head, _ = head_for()
        head.forward_ret_dict["point_box_preds"] = torch.zeros((70, code))
        with pytest.raises(ValueError, match=f"code size = {code} is outside the limit of 1 .. 16"):
            head.get_loss()
    head, _ = head_for()
    wide = ops.POINT_LOSS_MAX_ROWS + 1
    head.forward_ret_dict["point_cls_labels"] = torch.zeros((1,), dtype=torch.int64).expand(wide)
    with pytest.raises(ValueError, match=f"point_cls_labels has {wide} rows, above the limit of {ops.POINT_LOSS_MAX_ROWS}"):
        head.get_loss()
    # element counts that do not agree with N
    for key, value, match in (("point_cls_preds", torch.zeros((71, 3)), "point_cls_preds has 213 elements, expected 70 rows of num_class = 3"),
                              ("point_part_preds", torch.zeros((71, 3)), "point_part_preds has 213 elements, expected 70 rows of 3 columns"),
                              ("point_part_labels", torch.zeros((70, 2)), "point_part_labels has 140 elements"),
                              ("point_box_preds", torch.zeros((69, 8)), "point_box_preds has 552 elements, expected 70 rows of code size 8"),
                              ("point_box_labels", torch.zeros((70, 7)), "point_box_labels has 490 elements")):
        head, _ = head_for()
        head.forward_ret_dict[key] = value
        with pytest.raises(ValueError, match=match):
            head.get_loss()
    head, _ = head_for()                                          # everything in order but the device
    before = dict(head.forward_ret_dict)
    with pytest.raises(ValueError, match="point_cls_preds must be a device tensor"):
        head.get_loss()
    assert all(head.forward_ret_dict[k] is v for k, v in before.items())      # the dict is left as found
    assert (ops.POINT_LOSS_MAX_CLASS, ops.POINT_LOSS_MAX_CODE, ops.POINT_LOSS_MAX_ROWS) == (32, 16, 1 << 24)


def test_loss_weights_as_attributes_or_a_dict():
    from modest_amd.utils.point_head_loss import _get
    ns = types.SimpleNamespace(LOSS_WEIGHTS={"point_cls_weight": 2.0})
    assert _get(ns, "LOSS_WEIGHTS")["point_cls_weight"] == 2.0 and _get({"LOSS_WEIGHTS": 1}, "LOSS_WEIGHTS") == 1
