"""Drop-in for the part of spconv 1.2 that SECOND's ``VoxelBackBone8x`` constructs and calls:
``SparseConvTensor``, ``SubMConv3d``, ``SparseConv3d``, ``SparseSequential``, ``SparseModule`` and ``.dense()``, on the
HIP kernels of ``modest_amd/csrc/spconv.hip``; ``utils`` is ``modest_amd.utils.spconv_utils`` (the voxel generators).

Bound as ``sys.modules["spconv"]`` by ``modest_amd.utils.pcdet_bind.install(sparse_conv=True)``.  Everything else of
spconv (inverse and transposed convolutions, pooling, ``ToDense`` ...) is a class that can be named and subclassed and
raises ``NotImplementedError`` when it is called: PartA2 / UNet only.  Importing this package does not open the GPU.
"""
from .. import spconv_utils as utils
from .conv import SparseConv3d, SparseConvolution, SubMConv3d
from .modules import SparseModule, SparseSequential
from .tensor import SparseConvTensor

__all__ = ["SparseConvTensor", "SparseModule", "SparseSequential", "SparseConvolution", "SparseConv3d", "SubMConv3d", "utils"]

NOT_PROVIDED = ("SparseConv2d", "SubMConv2d", "SparseConvTranspose2d", "SparseConvTranspose3d", "SparseInverseConv2d",
                "SparseInverseConv3d", "SparseMaxPool2d", "SparseMaxPool3d", "ToDense", "RemoveGrid", "ConvAlgo",
                "JoinTable", "AddTable", "ConcatTable", "Identity")


def _not_provided(name):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError(f"spconv.{name} is not provided by modest_amd (PartA2 / UNet only)")

    return type(name, (), {"__init__": __init__, "__module__": __name__})


for _name in NOT_PROVIDED:
    globals()[_name] = _not_provided(_name)
del _name


def __getattr__(name):
    """any other name of spconv: a class that imports, subclasses, and fails when called"""
    if name.startswith("__") and name.endswith("__"):
        raise AttributeError(name)
    missing = globals()[name] = _not_provided(name)
    return missing
