"""CPU: pcdet_bind.bind_box_decode() -- a function of its own that sets the three
generate_predicted_boxes of modest_amd.utils.box_decode on AnchorHeadTemplate, PointHeadTemplate and RoIHeadTemplate: None
without pcdet, install()'s signature and keys unchanged, idempotent, bound onto fake modules in sys.modules and put back by
unbind, a module without its class skipped, a subclass that overrides the method left alone."""
import importlib.util
import inspect
import sys
import types

import pytest

from modest_amd.utils import box_decode as bd
from modest_amd.utils import pcdet_bind

NAMES = {"pcdet.models.dense_heads.anchor_head_template": "AnchorHeadTemplate",
         "pcdet.models.dense_heads.point_head_template": "PointHeadTemplate",
         "pcdet.models.roi_heads.roi_head_template": "RoIHeadTemplate"}
METHODS = {"AnchorHeadTemplate": bd.anchor_generate_predicted_boxes, "PointHeadTemplate": bd.point_generate_predicted_boxes,
           "RoIHeadTemplate": bd.roi_generate_predicted_boxes}


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
    mods = {}
    for name, cls_name in NAMES.items():
        mod = types.ModuleType(name)
        setattr(mod, cls_name, type(cls_name, (), {"generate_predicted_boxes": lambda self, *a, n=cls_name, **k: "reference " + n,
                                                   "get_loss": lambda self: "reference"}))
        mods[name] = mod
    return mods


def test_a_function_of_its_own_with_the_references_signatures():
    assert pcdet_bind.BOX_DECODE_NAMES == NAMES and pcdet_bind.BOX_DECODE == "modest_amd.utils.box_decode"
    assert not inspect.signature(pcdet_bind.bind_box_decode).parameters
    assert list(inspect.signature(pcdet_bind.install).parameters) == [
        "stand_ins", "sparse_conv", "point_stack", "anchor_targets", "roiaware_pool", "sparse_inverse", "point_targets",
        "proposal_layer"]                                                                     # install's signature stays
    assert "bind_box_decode" in pcdet_bind.__doc__ and bd.KINDS == METHODS
    params = inspect.signature(bd.anchor_generate_predicted_boxes).parameters
    assert list(params) == ["self", "batch_size", "cls_preds", "box_preds", "dir_cls_preds"] and params["dir_cls_preds"].default is None
    assert list(inspect.signature(bd.point_generate_predicted_boxes).parameters) == ["self", "points", "point_cls_preds", "point_box_preds"]
    assert list(inspect.signature(bd.roi_generate_predicted_boxes).parameters) == ["self", "batch_size", "rois", "cls_preds", "box_preds"]


def test_none_without_pcdet_and_a_module_without_its_class_is_skipped():
    saved = saved_modules()
    try:
        for k in saved:
            sys.modules.pop(k, None)
        if importlib.util.find_spec("pcdet") is None:
            assert pcdet_bind.bind_box_decode() is None and not any(n in sys.modules for n in NAMES)
        mods = fake_modules()
        empty = "pcdet.models.dense_heads.point_head_template"
        sys.modules[empty] = types.ModuleType(empty)                # a module without the class
        if importlib.util.find_spec("pcdet") is None:
            assert pcdet_bind.bind_box_decode() == {}                # found, nothing to bind
        roi = "pcdet.models.roi_heads.roi_head_template"
        sys.modules[roi] = mods[roi]
        bound = pcdet_bind.bind_box_decode()
        try:
            assert bound[roi] is mods[roi] and empty not in bound
            assert mods[roi].RoIHeadTemplate.generate_predicted_boxes is bd.roi_generate_predicted_boxes
        finally:
            bd.unbind(mods[roi].RoIHeadTemplate)
    finally:
        restore(saved)


def test_binds_idempotently_restores_and_leaves_overrides_and_install_alone():
    saved = saved_modules()
    try:
        for k in saved:
            sys.modules.pop(k, None)
        before = sorted(pcdet_bind.install())
        mods = fake_modules()
        originals = {n: getattr(mods[n], c).__dict__["generate_predicted_boxes"] for n, c in NAMES.items()}
        sys.modules.update(mods)
        bound = pcdet_bind.bind_box_decode()
        assert bound == mods and pcdet_bind.bind_box_decode() == mods                                  # idempotent
        for name, cls_name in NAMES.items():
            head = getattr(mods[name], cls_name)
            assert head.__dict__["generate_predicted_boxes"] is METHODS[cls_name]
            assert bd._ORIGINAL[head] is originals[name]                                                # a second call changed nothing
            assert head().get_loss() == "reference"                                                     # nothing else is touched
            own = type("Own", (head,), {"generate_predicted_boxes": lambda self, *a, **k: "its own"})
            assert own().generate_predicted_boxes() == "its own"                                        # an override keeps its own
            plain = type("Plain", (head,), {})
            assert plain.generate_predicted_boxes is METHODS[cls_name]                                  # a subclass without one gets ours
        assert sorted(pcdet_bind.install()) == before and not any(n in pcdet_bind.install() for n in NAMES)   # install's keys stay
        for name, cls_name in NAMES.items():                                                            # ... and put back
            head = getattr(mods[name], cls_name)
            assert bd.unbind(head) is head and head.__dict__["generate_predicted_boxes"] is originals[name] and head not in bd._ORIGINAL
            assert head().generate_predicted_boxes() == "reference " + cls_name
            assert bd.unbind(head) is head                                                              # nothing left to put back
    finally:
        restore(saved)


def test_bind_by_kind_and_a_class_without_a_method_of_its_own():
    base = type("Base", (), {"generate_predicted_boxes": lambda self, *a, **k: "inherited"})
    mid = type("MyRoIHead", (base,), {})
    with pytest.raises(ValueError, match="bind\\(MyRoIHead\\) needs its kind"):
        bd.bind(mid)
    assert bd.bind(mid, "RoIHeadTemplate") is mid and bd.bind(mid, "RoIHeadTemplate") is mid
    assert mid.generate_predicted_boxes is bd.roi_generate_predicted_boxes and bd._ORIGINAL[mid] is None
    bd.unbind(mid)
    assert "generate_predicted_boxes" not in mid.__dict__ and mid().generate_predicted_boxes() == "inherited"
