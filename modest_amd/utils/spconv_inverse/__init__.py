"""``modest_amd.utils.spconv`` plus ``SparseInverseConv3d``: the part of spconv 1.2 that PartA2's
``UNetV2`` constructs and calls.  The classes of ``modest_amd.utils.spconv`` are re-exported as the same objects, so a
tensor or a rulebook made under either name serves both; every other name of spconv is that package's class that can
be named and subclassed and raises ``NotImplementedError`` when it is called.

Bound as ``sys.modules["spconv"]`` by ``modest_amd.utils.pcdet_bind.install(sparse_inverse=True)``.  Importing this
package does not open the GPU.
"""
from .. import spconv as _base
from ..spconv import SparseConv3d, SparseConvolution, SparseConvTensor, SparseModule, SparseSequential, SubMConv3d, utils
from .conv import SparseInverseConv3d

__all__ = ["SparseConvTensor", "SparseModule", "SparseSequential", "SparseConvolution", "SparseConv3d", "SubMConv3d",
           "SparseInverseConv3d", "utils"]

NOT_PROVIDED = tuple(n for n in _base.NOT_PROVIDED if n != "SparseInverseConv3d")


def __getattr__(name):
    """any other name of spconv: modest_amd.utils.spconv's class that imports, subclasses, and fails when called"""
    if name.startswith("__") and name.endswith("__"):
        raise AttributeError(name)
    return getattr(_base, name)
