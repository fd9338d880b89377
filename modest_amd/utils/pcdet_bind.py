"""Bind this library's drop-in modules under the names the MODEST and OpenPCDet sources import.

    from modest_amd.utils import pcdet_bind
    pcdet_bind.install()          # before `import pcdet.models` / `import pcdet.datasets`

registers, in ``sys.modules``, the four extension shims PointRCNN is built from and the evaluation module, and -- with
``stand_ins=True`` -- stand-in modules for what ``import pcdet.models`` loads but no model of the reference's scripts
calls.  The ``spconv`` stand-in carries one real part, ``spconv.utils`` with the host voxel generators PointPillars'
data pipeline constructs (``modest_amd.utils.spconv_utils``); an installed spconv is left alone.  Any other attribute of
a stand-in is a class that can be named and subclassed at import time and raises ``NotImplementedError`` when it is called.  Calling ``install`` again changes nothing.  Nothing here touches the GPU:
the shims open the library at their first call.

``install(sparse_conv=True)`` binds ``modest_amd.utils.spconv`` -- the sparse 3-D convolutions SECOND's backbone is built
from -- as ``spconv`` instead of the stand-in; ``spconv.utils`` is the same module either way.

``install(point_stack=True)`` binds ``modest_amd.utils.pointnet2.pointnet2_stack.pointnet2_stack_cuda`` -- the
stacked-batch PointNet++ ops of PV-RCNN and Voxel R-CNN -- under the reference's name instead of
the stand-in.

``install(anchor_targets=True)`` binds ``modest_amd.utils.target_assigner`` -- the anchor target assignment of the anchor
heads on the GPU -- as ``pcdet.models.dense_heads.target_assigner.axis_aligned_target_assigner``.
Call it before ``pcdet.models`` is imported: ``anchor_head_template`` takes the class from that module when it is first
imported.  A module already imported under that name is left alone.

``install(roiaware_pool=True)`` binds ``modest_amd.utils.roiaware_voxel_pool_cuda`` -- the full ``roiaware_pool3d_cuda``
with PartA2's RoI-aware voxel pooling ``forward`` / ``backward`` -- under the reference's name
instead of the module whose ``forward`` / ``backward`` are not provided.  A module that is neither of ours is left alone.

``install(sparse_inverse=True)`` binds ``modest_amd.utils.spconv_inverse`` -- ``modest_amd.utils.spconv`` plus
``SparseInverseConv3d``, what PartA2's ``UNetV2`` is built from -- as ``spconv``, in place of the
stand-in or of ``modest_amd.utils.spconv``; an installed or imported spconv is left alone.

``install(point_targets=True)`` sets ``modest_amd.utils.point_head_targets.assign_stack_targets`` -- the target assignment
of the point heads in one call -- on ``PointHeadTemplate`` of
``pcdet.models.dense_heads.point_head_template``, which is imported for it if it is not yet (after every other binding,
so that the import finds the shims).  Where that module cannot be imported nothing is bound.

``install(proposal_layer=True)`` sets ``modest_amd.utils.proposal_layer.proposal_layer`` -- the RoI proposal layer of the
two-stage detectors in one call -- on ``RoIHeadTemplate`` of
``pcdet.models.roi_heads.roi_head_template``, imported for it if it is not yet, after every other binding.  Where that
module cannot be imported nothing is bound.

``bind_roi_targets()``, a function of its own, sets ``modest_amd.utils.roi_targets.assign_targets`` -- the RoI target
assignment of the two-stage heads in two calls -- on the same ``RoIHeadTemplate``; call it after
``install``.  ``install`` itself is unchanged by it.

``bind_post_processing()``, a function of its own too, sets ``modest_amd.utils.post_processing.post_processing`` -- the
test-time post-processing of every detector in one call -- on ``Detector3DTemplate`` of
``pcdet.models.detectors.detector3d_template``, imported for it if it is not yet; a detector with an override of its own
(``SECONDNetIoU``) keeps it.

``bind_anchor_loss()``, a function of its own as well, sets ``modest_amd.utils.anchor_head_loss.get_loss`` -- the loss of
the anchor heads with its gradients in one call -- on ``AnchorHeadTemplate`` of
``pcdet.models.dense_heads.anchor_head_template``, imported for it if it is not yet; a head that overrides a part of the
loss (``AnchorHeadMulti``) reaches the method that was replaced.

``bind_roi_loss()``, a function of its own like the others, sets ``modest_amd.utils.roi_head_loss.get_loss`` -- the loss of
the RoI heads with its gradients in one call -- on ``RoIHeadTemplate`` of
``pcdet.models.roi_heads.roi_head_template``, imported for it if it is not yet; a head that overrides
``get_box_reg_layer_loss`` or ``get_box_cls_layer_loss`` reaches the method that was replaced, and a head class with a
``get_loss`` of its own (``SECONDHead``) keeps it.

``bind_point_loss()``, a function of its own like the others, sets ``modest_amd.utils.point_head_loss.get_loss`` -- the loss
of the point heads with its gradients in one call -- on ``PointHeadBox``, ``PointHeadSimple`` and
``PointIntraPartOffsetHead`` of ``pcdet.models.dense_heads``, whose modules are imported for it if they are not yet (each
class defines its own ``get_loss``, so binding the template would do nothing); a head that overrides
``get_cls_layer_loss``, ``get_part_layer_loss`` or ``get_box_layer_loss`` reaches the method that was replaced.

``bind_box_decode()``, a function of its own like the others, sets the three ``generate_predicted_boxes`` of
``modest_amd.utils.box_decode`` -- the box decoding of every head in one call each -- on
``AnchorHeadTemplate``, ``PointHeadTemplate`` and ``RoIHeadTemplate``, whose modules are imported for it if they are not yet; a
head that overrides ``generate_predicted_boxes`` itself keeps its own.  The decoded boxes carry no ``grad_fn``.

``bind_pillar_vfe()``, a function of its own like the others, sets the two ``forward`` of ``modest_amd.utils.pillar_vfe`` --
PointPillars' feature encoder and BEV scatter with their fused backward -- on ``PillarVFE`` of
``pcdet.models.backbones_3d.vfe.pillar_vfe`` and ``PointPillarScatter`` of
``pcdet.models.backbones_2d.map_to_bev.pointpillar_scatter``, whose modules are imported for it if they are not yet; a subclass
that overrides ``forward`` keeps its own.  Parameters, buffers and ``state_dict`` stay the modules' own.

``bind_optim_step()``, a function of its own like the others, sets ``step`` and ``clip_and_step`` of
``modest_amd.utils.optim_step`` -- the ``adam_onecycle`` optimiser step: ``step`` is one launch, the bound pair of
``clip_grad_norm_`` and ``step`` three -- on ``OptimWrapper`` of
``train_utils.optimization.fastai_optim`` and its ``clip_grad_norm_`` as that name in ``train_utils.train_utils``; both modules
import only with the reference's ``tools/`` on ``sys.path``.  The optimiser's state stays torch's own.
"""
import importlib
import importlib.util
import sys
import types

SHIMS = {
    "iou3d_nms_cuda": "modest_amd.utils.iou3d_nms.iou3d_nms_cuda",
    "pcdet.ops.iou3d_nms.iou3d_nms_cuda": "modest_amd.utils.iou3d_nms.iou3d_nms_cuda",
    "pcdet.ops.pointnet2.pointnet2_batch.pointnet2_batch_cuda":
        "modest_amd.utils.pointnet2.pointnet2_batch.pointnet2_batch_cuda",
    "pcdet.ops.roipoint_pool3d.roipoint_pool3d_cuda": "modest_amd.utils.roipoint_pool3d.roipoint_pool3d_cuda",
    "pcdet.ops.roiaware_pool3d.roiaware_pool3d_cuda": "modest_amd.utils.roiaware_pool3d_cuda",
    "pcdet.datasets.kitti.kitti_object_eval_python.eval": "modest_amd.kitti_eval",
}
STAND_INS = ("pcdet.ops.pointnet2.pointnet2_stack.pointnet2_stack_cuda", "spconv")
SPCONV_UTILS = "modest_amd.utils.spconv_utils"   # bound as spconv.utils while spconv itself is a stand-in
SPCONV = "modest_amd.utils.spconv"               # bound as spconv by install(sparse_conv=True)
SPCONV_INVERSE = "modest_amd.utils.spconv_inverse"   # bound as spconv by install(sparse_inverse=True)
POINT_STACK_NAME = STAND_INS[0]                  # bound to POINT_STACK by install(point_stack=True)
POINT_STACK = "modest_amd.utils.pointnet2.pointnet2_stack.pointnet2_stack_cuda"
ANCHOR_TARGETS_NAME = "pcdet.models.dense_heads.target_assigner.axis_aligned_target_assigner"
ANCHOR_TARGETS = "modest_amd.utils.target_assigner"   # bound to ANCHOR_TARGETS_NAME by install(anchor_targets=True)
ROIAWARE_NAME = "pcdet.ops.roiaware_pool3d.roiaware_pool3d_cuda"
ROIAWARE_POOL = "modest_amd.utils.roiaware_voxel_pool_cuda"   # bound to ROIAWARE_NAME by install(roiaware_pool=True)
POINT_TARGETS_NAME = "pcdet.models.dense_heads.point_head_template"
POINT_TARGETS = "modest_amd.utils.point_head_targets"   # its method set on PointHeadTemplate by install(point_targets=True)
PROPOSAL_LAYER_NAME = "pcdet.models.roi_heads.roi_head_template"
PROPOSAL_LAYER = "modest_amd.utils.proposal_layer"   # its method set on RoIHeadTemplate by install(proposal_layer=True)
ROI_TARGETS_NAME = PROPOSAL_LAYER_NAME
ROI_TARGETS = "modest_amd.utils.roi_targets"         # its method set on RoIHeadTemplate by bind_roi_targets()
POST_PROCESSING_NAME = "pcdet.models.detectors.detector3d_template"
POST_PROCESSING = "modest_amd.utils.post_processing"   # its method set on Detector3DTemplate by bind_post_processing()
ANCHOR_LOSS_NAME = "pcdet.models.dense_heads.anchor_head_template"
ANCHOR_LOSS = "modest_amd.utils.anchor_head_loss"      # its method set on AnchorHeadTemplate by bind_anchor_loss()
ROI_LOSS_NAME = PROPOSAL_LAYER_NAME
ROI_LOSS = "modest_amd.utils.roi_head_loss"            # its method set on RoIHeadTemplate by bind_roi_loss()
POINT_LOSS_NAMES = {"pcdet.models.dense_heads.point_head_box": "PointHeadBox",
                    "pcdet.models.dense_heads.point_head_simple": "PointHeadSimple",
                    "pcdet.models.dense_heads.point_intra_part_head": "PointIntraPartOffsetHead"}
POINT_LOSS = "modest_amd.utils.point_head_loss"        # its method set on the three classes by bind_point_loss()
BOX_DECODE_NAMES = {"pcdet.models.dense_heads.anchor_head_template": "AnchorHeadTemplate",
                    "pcdet.models.dense_heads.point_head_template": "PointHeadTemplate",
                    "pcdet.models.roi_heads.roi_head_template": "RoIHeadTemplate"}
BOX_DECODE = "modest_amd.utils.box_decode"             # its methods set on the three templates by bind_box_decode()
PILLAR_VFE_NAMES = {"pcdet.models.backbones_3d.vfe.pillar_vfe": "PillarVFE",
                    "pcdet.models.backbones_2d.map_to_bev.pointpillar_scatter": "PointPillarScatter"}
PILLAR_VFE = "modest_amd.utils.pillar_vfe"             # its two forward methods set on the two classes by bind_pillar_vfe()
BATCH_PREP_DATASET_NAME = "pcdet.datasets.dataset"
BATCH_PREP_MODELS_NAME = "pcdet.models"
BATCH_PREP = "modest_amd.utils.batch_prep"             # prepare_data, collate_batch and load_data_to_gpu set by bind_batch_prep()
OPTIM_STEP_WRAPPER_NAME = "train_utils.optimization.fastai_optim"
OPTIM_STEP_TRAIN_NAME = "train_utils.train_utils"
OPTIM_STEP = "modest_amd.utils.optim_step"             # step, clip_and_step and clip_grad_norm_ set by bind_optim_step()


class StandIn(types.ModuleType):
    """a module that is not provided: it imports, and whatever is taken from it fails when called"""

    def __getattr__(self, name):
        if name.startswith("__") and name.endswith("__"):
            raise AttributeError(name)
        module = self.__name__

        def __init__(self, *args, **kwargs):
            raise NotImplementedError(f"{module}.{name} is not provided by modest_amd (PV-RCNN / PartA2 only)")

        missing = type(name, (), {"__init__": __init__, "__module__": module})
        setattr(self, name, missing)
        return missing


def _bind_spconv(ours_name, replaceable=()):
    """spconv := the module `ours_name` (SPCONV or SPCONV_INVERSE) unless a real spconv is imported or installed; a stand-in
    and those of our own modules named in `replaceable` give way -> the module bound, or None"""
    ours = importlib.import_module(ours_name)
    mod = sys.modules.get("spconv")
    if mod is None and importlib.util.find_spec("spconv") is not None:
        return None   # the real package is installed: leave it alone
    if mod is not None and mod is not ours and not isinstance(mod, StandIn) \
            and not any(mod is importlib.import_module(name) for name in replaceable):
        return None   # ... or already imported
    sys.modules["spconv"] = ours
    sys.modules["spconv.utils"] = ours.utils
    return ours


def _bind_point_stack():
    """the stack extension's name := our shim unless something else is bound there -> the module bound, or None"""
    ours = importlib.import_module(POINT_STACK)
    mod = sys.modules.get(POINT_STACK_NAME)
    if mod is not None and mod is not ours and not isinstance(mod, StandIn):
        return None   # neither ours nor a stand-in (the compiled extension): leave it alone
    sys.modules[POINT_STACK_NAME] = ours
    return ours


def _bind_anchor_targets():
    """the reference assigner's module name := our module unless the reference's is already imported -> the module bound, or None"""
    ours = importlib.import_module(ANCHOR_TARGETS)
    mod = sys.modules.get(ANCHOR_TARGETS_NAME)
    if mod is not None and mod is not ours:
        return None   # already imported (anchor_head_template holds its class): leave it alone
    sys.modules[ANCHOR_TARGETS_NAME] = ours
    return ours


def _bind_roiaware_pool(before):
    """the roiaware extension's name := the full drop-in unless `before`, what was bound there when install() was
    called, is neither absent nor ours -> the module bound, or None"""
    ours = importlib.import_module(ROIAWARE_POOL)
    if before is not None and before is not ours and before is not importlib.import_module(SHIMS[ROIAWARE_NAME]):
        sys.modules[ROIAWARE_NAME] = before   # a foreign module (the compiled extension): put it back
        return None
    sys.modules[ROIAWARE_NAME] = ours
    return ours


def _bind_onto(module_name, class_name, ours_name, *bind_args):
    """the class `class_name` of the reference's module `module_name`, which is imported for it if it is not yet, handed to
    ``bind`` of our module `ours_name` -> the reference's module, or None where it cannot be imported (no pcdet on the path, or
    one that does not import here: nothing to bind onto) or lacks the class"""
    mod = sys.modules.get(module_name)
    if mod is None:
        try:
            mod = importlib.import_module(module_name)
        except ImportError:
            return None
    cls = getattr(mod, class_name, None)
    if cls is None:
        return None
    importlib.import_module(ours_name).bind(cls, *bind_args)
    return mod


def _bind_onto_each(names, ours_name, with_class_name=False):
    """`_bind_onto` for every module -> class of `names` (`bind` is told the class name too with `with_class_name`)
    -> {module name: module} of the modules bound, or None where none of the modules can be imported"""
    bound, found = {}, False
    for name, cls_name in names.items():
        mod = _bind_onto(name, cls_name, ours_name, *((cls_name,) if with_class_name else ()))
        found = found or sys.modules.get(name) is not None      # imported before or just now, with or without its class
        if mod is not None:
            bound[name] = mod
    return bound if found else None


def _bind_point_targets():
    """PointHeadTemplate.assign_stack_targets := ours, in the reference's module if it is imported or can be
    -> that module, or None"""
    return _bind_onto(POINT_TARGETS_NAME, "PointHeadTemplate", POINT_TARGETS)


def _bind_proposal_layer():
    """RoIHeadTemplate.proposal_layer := ours, in the reference's module if it is imported or can be
    -> that module, or None"""
    return _bind_onto(PROPOSAL_LAYER_NAME, "RoIHeadTemplate", PROPOSAL_LAYER)


def bind_roi_targets():
    """RoIHeadTemplate.assign_targets := modest_amd.utils.roi_targets.assign_targets -- the RoI target assignment of the
    two-stage heads -- in the reference's module if it is imported or can be -> that module, or
    None.  A function of its own: install() and what it returns stay as they are.  Idempotent; before or after
    ``import pcdet.models``; touches no GPU state."""
    return _bind_onto(ROI_TARGETS_NAME, "RoIHeadTemplate", ROI_TARGETS)


def bind_post_processing():
    """Detector3DTemplate.post_processing := modest_amd.utils.post_processing.post_processing -- the test-time
    post-processing of the detectors -- in the reference's module if it is imported or can be -> that
    module, or None.  A function of its own: install() and what it returns stay as they are.  Only the template's own
    method is set, so a subclass that overrides it (SECONDNetIoU) keeps its own.  Idempotent; before or after
    ``import pcdet.models``; touches no GPU state."""
    return _bind_onto(POST_PROCESSING_NAME, "Detector3DTemplate", POST_PROCESSING)


def bind_anchor_loss():
    """AnchorHeadTemplate.get_loss := modest_amd.utils.anchor_head_loss.get_loss -- the loss of the anchor heads with its
    gradients -- in the reference's module if it is imported or can be -> that module, or None.  A
    function of its own: install() and what it returns stay as they are.  Only the template's own method is set, and the
    one it had is kept: a head that overrides get_cls_layer_loss or get_box_reg_layer_loss (AnchorHeadMulti) is handed to
    it.  Idempotent; before or after ``import pcdet.models``; touches no GPU state."""
    return _bind_onto(ANCHOR_LOSS_NAME, "AnchorHeadTemplate", ANCHOR_LOSS)


def bind_roi_loss():
    """RoIHeadTemplate.get_loss := modest_amd.utils.roi_head_loss.get_loss -- the loss of the RoI heads with its gradients
     -- in the reference's module if it is imported or can be -> that module, or None.  A function of
    its own: install() and what it returns stay as they are.  Only the template's own method is set, and the one it had is
    kept: a head that overrides get_box_reg_layer_loss or get_box_cls_layer_loss is handed to it, and a head class with a
    get_loss of its own (SECONDHead) keeps that.  Idempotent; before or after ``import pcdet.models``; touches no GPU
    state."""
    return _bind_onto(ROI_LOSS_NAME, "RoIHeadTemplate", ROI_LOSS)


def bind_point_loss():
    """PointHeadBox / PointHeadSimple / PointIntraPartOffsetHead .get_loss := modest_amd.utils.point_head_loss.get_loss -- the
    loss of the point heads with its gradients -- in the reference's modules where they are imported
    or can be -> {module name: module} of the modules bound, or None where pcdet cannot be imported.  A function of its own:
    install() and what it returns stay as they are.  Each class defines its own get_loss, so the three classes are bound,
    not their template; the method each had is kept: a head that overrides get_cls_layer_loss, get_part_layer_loss or
    get_box_layer_loss is handed to it.  A module that lacks its class is skipped.  Idempotent; before or after
    ``import pcdet.models``; touches no GPU state."""
    return _bind_onto_each(POINT_LOSS_NAMES, POINT_LOSS)


def bind_box_decode():
    """AnchorHeadTemplate / PointHeadTemplate / RoIHeadTemplate .generate_predicted_boxes := the three methods of
    modest_amd.utils.box_decode -- the box decoding of the heads -- in the reference's modules where they
    are imported or can be -> {module name: module} of the modules bound, or None where pcdet cannot be imported.  A function
    of its own: install() and what it returns stay as they are.  Only the templates' own methods are set, so a head that
    overrides generate_predicted_boxes keeps its own.  A module that lacks its class is skipped.  Idempotent; before or after
    ``import pcdet.models``; touches no GPU state."""
    return _bind_onto_each(BOX_DECODE_NAMES, BOX_DECODE, with_class_name=True)


def bind_pillar_vfe():
    """PillarVFE / PointPillarScatter .forward := the two methods of modest_amd.utils.pillar_vfe -- PointPillars' feature encoder
    and BEV scatter with their fused backward -- in the reference's modules where they are imported or
    can be -> {module name: module} of the modules bound, or None where pcdet cannot be imported.  A function of its own:
    install() and what it returns stay as they are.  Only the two classes' own methods are set, so a subclass that overrides
    forward keeps its own; parameters and buffers are untouched.  A module that lacks its class is skipped.  Idempotent; before
    or after ``import pcdet.models``; touches no GPU state."""
    return _bind_onto_each(PILLAR_VFE_NAMES, PILLAR_VFE, with_class_name=True)


def bind_batch_prep():
    """DatasetTemplate.prepare_data / .collate_batch and pcdet.models.load_data_to_gpu := the three functions of
    modest_amd.utils.batch_prep -- training-batch preparation on the device -- in the reference's modules
    if they are imported or can be -> (pcdet.datasets.dataset, pcdet.models), or None where either cannot be imported.  A
    function of its own, opt-in: install() and what it returns stay as they are.  In test mode, and for a batch that is not
    raw, the three call what they replaced.  Idempotent; touches no GPU state (the database is read at the first raw batch)."""
    mods = []
    for name in (BATCH_PREP_DATASET_NAME, BATCH_PREP_MODELS_NAME):
        mod = sys.modules.get(name)
        if mod is None:
            try:
                mod = importlib.import_module(name)
            except ImportError:
                return None
        mods.append(mod)
    if getattr(mods[0], "DatasetTemplate", None) is None or getattr(mods[1], "load_data_to_gpu", None) is None:
        return None
    importlib.import_module(BATCH_PREP).bind(mods[0].DatasetTemplate, mods[1])
    return tuple(mods)


def bind_optim_step():
    """OptimWrapper.step / .clip_and_step of train_utils.optimization.fastai_optim and the name clip_grad_norm_ of
    train_utils.train_utils := the three functions of modest_amd.utils.optim_step -- gradient clipping (two launches) and the
    adam_onecycle optimiser step (one launch): three for the pair -- in the reference's modules if they are imported or can be (they are
    importable only with the reference's ``tools/`` on ``sys.path``) -> (fastai_optim, train_utils), or None where either cannot be
    imported or lacks its name.  A function of its own, opt-in: install() and what it returns stay as they are.  A wrapper around
    anything but torch.optim.Adam with true weight decay reaches the method that was replaced.  Idempotent; touches no GPU state."""
    mods = []
    for name in (OPTIM_STEP_WRAPPER_NAME, OPTIM_STEP_TRAIN_NAME):
        mod = sys.modules.get(name)
        if mod is None:
            try:
                mod = importlib.import_module(name)
            except ImportError:
                return None
        mods.append(mod)
    if getattr(mods[0], "OptimWrapper", None) is None or getattr(mods[1], "clip_grad_norm_", None) is None:
        return None
    importlib.import_module(OPTIM_STEP).bind(mods[0].OptimWrapper, mods[1])
    return tuple(mods)


def install(stand_ins=True, sparse_conv=False, point_stack=False, anchor_targets=False, roiaware_pool=False,
            sparse_inverse=False, point_targets=False, proposal_layer=False):
    """-> {name: module} of everything bound (also what an earlier call bound)"""
    bound = {}
    roiaware_before = sys.modules.get(ROIAWARE_NAME)
    for name, target in SHIMS.items():
        bound[name] = sys.modules[name] = importlib.import_module(target)
    if roiaware_pool:
        bound[ROIAWARE_NAME] = _bind_roiaware_pool(roiaware_before) or roiaware_before
    if anchor_targets:
        ours = _bind_anchor_targets()
        if ours is not None:
            bound[ANCHOR_TARGETS_NAME] = ours
    if point_stack:
        ours = _bind_point_stack()
        if ours is not None and not stand_ins:
            bound[POINT_STACK_NAME] = ours
    if sparse_conv:
        ours = _bind_spconv(SPCONV)
        if ours is not None and not stand_ins:
            bound["spconv"] = ours
    if sparse_inverse:
        ours = _bind_spconv(SPCONV_INVERSE, replaceable=(SPCONV,))
        if ours is not None and not stand_ins:
            bound["spconv"] = ours
    if stand_ins:
        for name in STAND_INS:
            mod = sys.modules.get(name)
            if mod is None and "." not in name and importlib.util.find_spec(name) is not None:
                continue   # the real package is installed: leave it alone
            if mod is None:
                mod = sys.modules[name] = StandIn(name)
            bound[name] = mod
        spconv = sys.modules.get("spconv")
        if isinstance(spconv, StandIn):   # the one part of spconv that is provided: the voxel generators (PointPillars)
            utils = importlib.import_module(SPCONV_UTILS)
            spconv.utils = utils
            sys.modules["spconv.utils"] = utils   # `from spconv.utils import ...`: a stand-in has no __path__ to search
    if point_targets:
        mod = _bind_point_targets()
        if mod is not None:
            bound[POINT_TARGETS_NAME] = mod
    if proposal_layer:
        mod = _bind_proposal_layer()
        if mod is not None:
            bound[PROPOSAL_LAYER_NAME] = mod
    return bound
