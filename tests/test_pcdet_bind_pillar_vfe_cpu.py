"""CPU: pcdet_bind.bind_pillar_vfe() -- a function of its own that sets the two forward methods of
modest_amd.utils.pillar_vfe on PillarVFE and PointPillarScatter: None without pcdet, install()'s signature and keys unchanged,
idempotent, bound onto fake modules in sys.modules and put back by unbind, a module without its class skipped, a subclass that
overrides forward left alone; and the refusals of the two methods that need no GPU."""
import importlib.util
import inspect
import sys
import types

import pytest
import torch

from modest_amd.utils import pcdet_bind
from modest_amd.utils import pillar_vfe as pv

NAMES = {"pcdet.models.backbones_3d.vfe.pillar_vfe": "PillarVFE",
         "pcdet.models.backbones_2d.map_to_bev.pointpillar_scatter": "PointPillarScatter"}
METHODS = {"PillarVFE": pv.pillar_vfe_forward, "PointPillarScatter": pv.pillar_scatter_forward}


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
        setattr(mod, cls_name, type(cls_name, (), {"forward": lambda self, batch_dict, n=cls_name, **k: "reference " + n,
                                                   "get_output_feature_dim": lambda self: "reference"}))
        mods[name] = mod
    return mods


def test_a_function_of_its_own_with_the_references_signatures():
    assert pcdet_bind.PILLAR_VFE_NAMES == NAMES and pcdet_bind.PILLAR_VFE == "modest_amd.utils.pillar_vfe"
    assert not inspect.signature(pcdet_bind.bind_pillar_vfe).parameters
    assert list(inspect.signature(pcdet_bind.install).parameters) == [
        "stand_ins", "sparse_conv", "point_stack", "anchor_targets", "roiaware_pool", "sparse_inverse", "point_targets",
        "proposal_layer"]                                                                     # install's signature stays
    assert "bind_pillar_vfe" in pcdet_bind.__doc__ and pv.KINDS == METHODS
    for fn in METHODS.values():
        params = inspect.signature(fn).parameters
        assert list(params) == ["self", "batch_dict", "kwargs"] and params["kwargs"].kind is inspect.Parameter.VAR_KEYWORD


def test_none_without_pcdet_and_a_module_without_its_class_is_skipped():
    saved = saved_modules()
    try:
        for k in saved:
            sys.modules.pop(k, None)
        if importlib.util.find_spec("pcdet") is None:
            assert pcdet_bind.bind_pillar_vfe() is None and not any(n in sys.modules for n in NAMES)
        mods = fake_modules()
        empty = "pcdet.models.backbones_3d.vfe.pillar_vfe"
        sys.modules[empty] = types.ModuleType(empty)                 # a module without the class
        if importlib.util.find_spec("pcdet") is None:
            assert pcdet_bind.bind_pillar_vfe() == {}                # found, nothing to bind
        sc = "pcdet.models.backbones_2d.map_to_bev.pointpillar_scatter"
        sys.modules[sc] = mods[sc]
        bound = pcdet_bind.bind_pillar_vfe()
        try:
            assert bound[sc] is mods[sc] and empty not in bound
            assert mods[sc].PointPillarScatter.forward is pv.pillar_scatter_forward
        finally:
            pv.unbind(mods[sc].PointPillarScatter)
    finally:
        restore(saved)


def test_binds_idempotently_restores_and_leaves_overrides_and_install_alone():
    saved = saved_modules()
    try:
        for k in saved:
            sys.modules.pop(k, None)
        before = sorted(pcdet_bind.install())
        mods = fake_modules()
        originals = {n: getattr(mods[n], c).__dict__["forward"] for n, c in NAMES.items()}
        sys.modules.update(mods)
        bound = pcdet_bind.bind_pillar_vfe()
        assert bound == mods and pcdet_bind.bind_pillar_vfe() == mods                                  # idempotent
        for name, cls_name in NAMES.items():
            cls = getattr(mods[name], cls_name)
            assert cls.__dict__["forward"] is METHODS[cls_name]
            assert pv._ORIGINAL[cls] is originals[name]                                                 # a second call changed nothing
            assert cls().get_output_feature_dim() == "reference"                                        # nothing else is touched
            own = type("Own", (cls,), {"forward": lambda self, batch_dict, **k: "its own"})
            assert own().forward({}) == "its own"                                                       # an override keeps its own
            plain = type("Plain", (cls,), {})
            assert plain.forward is METHODS[cls_name]                                                   # a subclass without one gets ours
        assert sorted(pcdet_bind.install()) == before and not any(n in pcdet_bind.install() for n in NAMES)   # install's keys stay
        for name, cls_name in NAMES.items():                                                            # ... and put back
            cls = getattr(mods[name], cls_name)
            assert pv.unbind(cls) is cls and cls.__dict__["forward"] is originals[name] and cls not in pv._ORIGINAL
            assert cls().forward({}) == "reference " + cls_name
            assert pv.unbind(cls) is cls                                                                # nothing left to put back
    finally:
        restore(saved)


def test_bind_by_kind_and_a_class_without_a_method_of_its_own():
    base = type("Base", (), {"forward": lambda self, batch_dict, **k: "inherited"})
    mid = type("MyVFE", (base,), {})
    with pytest.raises(ValueError, match="bind\\(MyVFE\\) needs its kind"):
        pv.bind(mid)
    assert pv.bind(mid, "PillarVFE") is mid and pv.bind(mid, "PillarVFE") is mid
    assert mid.forward is pv.pillar_vfe_forward and pv._ORIGINAL[mid] is None
    pv.unbind(mid)
    assert "forward" not in mid.__dict__ and mid().forward({}) == "inherited"


def test_what_is_not_provided_is_refused_before_anything_is_launched():
    """on host tensors: every refusal below comes before the library is opened"""
    pfn = types.SimpleNamespace(use_norm=True, training=True, linear=torch.nn.Linear(10, 8, bias=False), norm=torch.nn.BatchNorm1d(8))
    vfe = types.SimpleNamespace(pfn_layers=[pfn, pfn], training=True, use_absolute_xyz=True, with_distance=False)
    batch = dict(voxels=torch.zeros(4, 3, 4), voxel_num_points=torch.ones(4), voxel_coords=torch.zeros(4, 4), batch_size=1)
    with pytest.raises(NotImplementedError, match="2 PFN layers"):
        pv.pillar_vfe_forward(vfe, batch)
    vfe.pfn_layers = [pfn]
    pfn.use_norm = False
    with pytest.raises(NotImplementedError, match="USE_NORM: False"):
        pv.pillar_vfe_forward(vfe, batch)
    pfn.use_norm = True
    with pytest.raises(NotImplementedError, match="voxels that require grad"):
        pv.pillar_vfe_forward(vfe, dict(batch, voxels=torch.zeros(4, 3, 4, requires_grad=True)))
    with pytest.raises(NotImplementedError, match="voxels of torch.float64"):
        pv.pillar_vfe_forward(vfe, dict(batch, voxels=torch.zeros(4, 3, 4, dtype=torch.float64)))
    pfn.linear.double()
    with pytest.raises(NotImplementedError, match="linear.weight of torch.float64"):
        pv.pillar_vfe_forward(vfe, batch)
    pfn.linear.float()
    vfe.training = False
    with pytest.raises(NotImplementedError, match="gradients of PillarVFE in eval mode"):
        pv.pillar_vfe_forward(vfe, batch)
    sc = types.SimpleNamespace(nz=2, ny=2, nx=2, num_bev_features=8)
    with pytest.raises(NotImplementedError, match="nz = 2"):
        pv.pillar_scatter_forward(sc, dict(batch, pillar_features=torch.zeros(4, 8)))
    sc.nz = 1
    with pytest.raises(NotImplementedError, match="pillar_features of torch.float16"):
        pv.pillar_scatter_forward(sc, dict(batch, pillar_features=torch.zeros(4, 8).half()))
    with pytest.raises(ValueError, match="must be \\(P, NUM_BEV_FEATURES\\)"):
        pv.pillar_scatter_forward(sc, dict(batch, pillar_features=torch.zeros(4, 9)))
    with pytest.raises(ValueError, match="pillar_features must be a device tensor"):      # no quiet fall-back on the host
        pv.pillar_scatter_forward(sc, dict(batch, pillar_features=torch.zeros(4, 8)))
