"""CPU: pcdet_bind.bind_optim_step() -- a function of its own that sets step and clip_and_step of
modest_amd.utils.optim_step on OptimWrapper of train_utils.optimization.fastai_optim and clip_grad_norm_ in
train_utils.train_utils: None where the modules are not importable, install()'s signature and keys unchanged, idempotent, bound
onto fake modules in sys.modules and put back by unbind, and a wrapper that is not the adam_onecycle one reaches the method that
was replaced."""
import importlib.util
import inspect
import sys
import types

import torch

from modest_amd.utils import optim_step as osd
from modest_amd.utils import pcdet_bind

NAMES = ("train_utils", "train_utils.optimization", "train_utils.optimization.fastai_optim", "train_utils.train_utils")


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
    def reference_clip(parameters, max_norm, norm_type=2.0):
        return "reference clip"
    wrapper = type("OptimWrapper", (), {"step": lambda self: "reference step", "zero_grad": lambda self: "reference zero_grad"})
    mods = {name: types.ModuleType(name) for name in NAMES}
    mods[NAMES[2]].OptimWrapper = wrapper
    mods[NAMES[2]].FastAIMixedOptim = type("FastAIMixedOptim", (wrapper,), {})
    mods[NAMES[3]].clip_grad_norm_ = reference_clip
    return mods


def test_a_function_of_its_own_with_torchs_signature():
    assert (pcdet_bind.OPTIM_STEP_WRAPPER_NAME, pcdet_bind.OPTIM_STEP_TRAIN_NAME) == (NAMES[2], NAMES[3])
    assert pcdet_bind.OPTIM_STEP == "modest_amd.utils.optim_step" and "bind_optim_step" in pcdet_bind.__doc__
    assert not inspect.signature(pcdet_bind.bind_optim_step).parameters
    assert list(inspect.signature(pcdet_bind.install).parameters) == [
        "stand_ins", "sparse_conv", "point_stack", "anchor_targets", "roiaware_pool", "sparse_inverse", "point_targets",
        "proposal_layer"]                                                                     # install's signature stays
    ours, torchs = inspect.signature(osd.clip_grad_norm_).parameters, inspect.signature(torch.nn.utils.clip_grad_norm_).parameters
    assert list(ours) == list(torchs) == ["parameters", "max_norm", "norm_type", "error_if_nonfinite", "foreach"]
    assert [p.default for p in ours.values()] == [p.default for p in torchs.values()]
    assert list(inspect.signature(osd.step).parameters) == ["self"]
    assert list(inspect.signature(osd.clip_and_step).parameters) == ["self", "max_norm"]


def test_none_where_the_modules_cannot_be_imported_or_lack_their_names():
    saved = saved_modules()
    try:
        for k in saved:
            sys.modules.pop(k, None)
        if importlib.util.find_spec("train_utils") is None:
            assert pcdet_bind.bind_optim_step() is None and not any(n in sys.modules for n in NAMES)
        mods = fake_modules()
        del mods[NAMES[3]].clip_grad_norm_
        sys.modules.update(mods)
        assert pcdet_bind.bind_optim_step() is None and mods[NAMES[2]].OptimWrapper.__dict__["step"](None) == "reference step"
    finally:
        restore(saved)


def test_binds_idempotently_restores_and_leaves_install_alone():
    saved = saved_modules()
    try:
        for k in saved:
            sys.modules.pop(k, None)
        before = sorted(pcdet_bind.install())
        mods = fake_modules()
        cls, train = mods[NAMES[2]].OptimWrapper, mods[NAMES[3]]
        original_step, original_clip = cls.__dict__["step"], train.clip_grad_norm_
        sys.modules.update(mods)
        bound = pcdet_bind.bind_optim_step()
        assert bound == (mods[NAMES[2]], train) and pcdet_bind.bind_optim_step() == bound                  # idempotent
        assert cls.__dict__["step"] is osd.step and cls.__dict__["clip_and_step"] is osd.clip_and_step
        assert train.clip_grad_norm_ is osd.clip_grad_norm_
        assert osd._ORIGINAL[cls] == {"step": original_step, "clip_and_step": None}                        # a second call changed nothing
        assert osd._ORIGINAL[train] == {"clip_grad_norm_": original_clip}
        assert cls().zero_grad() == "reference zero_grad"                                                   # nothing else is touched
        assert sorted(pcdet_bind.install()) == before and not any(n in pcdet_bind.install() for n in NAMES)   # install's keys stay
        # a wrapper that is not the adam_onecycle one reaches what was replaced: another optimiser, no true weight decay, mixed
        w = cls()
        w.opt, w.true_wd = torch.optim.SGD([torch.nn.Parameter(torch.zeros(2))], lr=0.1), True
        assert w.step() == "reference step"
        w.opt, w.true_wd = torch.optim.Adam([torch.nn.Parameter(torch.zeros(2))]), False
        assert w.step() == "reference step"
        m = mods[NAMES[2]].FastAIMixedOptim()
        m.opt, m.true_wd = torch.optim.Adam([torch.nn.Parameter(torch.zeros(2))]), True
        assert m.step() == "reference step"
        assert osd.unbind(cls, train) is cls and cls.__dict__["step"] is original_step and "clip_and_step" not in cls.__dict__
        assert train.clip_grad_norm_ is original_clip and cls not in osd._ORIGINAL and train not in osd._ORIGINAL
        assert osd.unbind(cls, train) is cls                                                                # nothing left to put back
    finally:
        restore(saved)
