"""CPU: pcdet_bind.bind_post_processing() -- a function of its own that sets
modest_amd.utils.post_processing.post_processing on Detector3DTemplate of pcdet.models.detectors.detector3d_template: None
without pcdet, install()'s keys unchanged, idempotent, bound onto a fake module in sys.modules, a subclass's own override
left alone."""
import importlib.util
import inspect
import sys
import types

from modest_amd.utils import pcdet_bind
from modest_amd.utils import post_processing as pp

NAME = "pcdet.models.detectors.detector3d_template"


def saved_modules():
    names = list(pcdet_bind.SHIMS) + list(pcdet_bind.STAND_INS) + ["spconv.utils", NAME]
    return {k: sys.modules.get(k) for k in names}


def restore(saved):
    for k, v in saved.items():
        if v is None:
            sys.modules.pop(k, None)
        else:
            sys.modules[k] = v


def test_a_function_of_its_own():
    assert pcdet_bind.POST_PROCESSING_NAME == NAME and pcdet_bind.POST_PROCESSING == "modest_amd.utils.post_processing"
    assert not inspect.signature(pcdet_bind.bind_post_processing).parameters
    assert list(inspect.signature(pcdet_bind.install).parameters)[-1] == "proposal_layer"      # install's signature stays


def test_none_without_pcdet():
    saved = saved_modules()
    try:
        for k in saved:
            sys.modules.pop(k, None)
        if importlib.util.find_spec("pcdet") is None:
            assert pcdet_bind.bind_post_processing() is None and NAME not in sys.modules
        sys.modules[NAME] = types.ModuleType(NAME)            # a module without the class
        assert pcdet_bind.bind_post_processing() is None
    finally:
        restore(saved)


def test_binds_onto_a_fake_module_idempotently_and_leaves_overrides_and_install_alone():
    saved = saved_modules()
    try:
        for k in saved:
            sys.modules.pop(k, None)
        before = sorted(pcdet_bind.install())
        fake = types.ModuleType(NAME)
        fake.Detector3DTemplate = type("Detector3DTemplate", (), {"post_processing": lambda self, d: "reference",
                                                                  "generate_recall_record": staticmethod(lambda **k: "reference")})
        plain = type("PointPillar", (fake.Detector3DTemplate,), {})
        own = type("SECONDNetIoU", (fake.Detector3DTemplate,), {"post_processing": lambda self, d: "its own"})
        sys.modules[NAME] = fake
        assert plain().post_processing({}) == "reference"
        assert pcdet_bind.bind_post_processing() is fake and pcdet_bind.bind_post_processing() is fake       # idempotent
        assert fake.Detector3DTemplate.post_processing is pp.post_processing and plain.post_processing is pp.post_processing
        assert own().post_processing({}) == "its own"                                                          # the override stays
        assert fake.Detector3DTemplate.generate_recall_record() == "reference"                                 # nothing else is touched
        assert sorted(pcdet_bind.install()) == before                                                          # install's keys stay
        assert NAME not in pcdet_bind.install()
    finally:
        restore(saved)


def test_bind_is_inherited():
    base = type("Detector", (), {})
    sub = type("Sub", (base,), {})
    assert pp.bind(base) is base and sub.post_processing is pp.post_processing
    assert list(inspect.signature(pp.post_processing).parameters) == ["self", "batch_dict"]
