"""``spconv.SparseModule`` and ``spconv.SparseSequential`` of spconv 1.2."""
from collections import OrderedDict

from torch import nn

from .tensor import SparseConvTensor


class SparseModule(nn.Module):
    """marker: a child of ``SparseSequential`` with this base is handed the ``SparseConvTensor`` itself"""


class SparseSequential(SparseModule):
    """``SparseSequential(m1, m2)``, ``SparseSequential(OrderedDict(...))`` or ``SparseSequential(name=m1, ...)``.
    A ``SparseModule`` child gets the tensor; any other child (BatchNorm1d, ReLU) is applied to ``.features`` of a
    ``SparseConvTensor`` and to the input itself otherwise."""

    def __init__(self, *args, **kwargs):
        super().__init__()
        if len(args) == 1 and isinstance(args[0], OrderedDict):
            for key, module in args[0].items():
                self.add_module(key, module)
        else:
            for idx, module in enumerate(args):
                self.add_module(str(idx), module)
        for name, module in kwargs.items():
            if name in self._modules:
                raise ValueError(f"name {name!r} exists")
            self.add_module(name, module)

    def __getitem__(self, idx):
        if not (-len(self) <= idx < len(self)):
            raise IndexError(f"index {idx} is out of range")
        if idx < 0:
            idx += len(self)
        return list(self._modules.values())[idx]

    def __len__(self):
        return len(self._modules)

    def add(self, module, name=None):
        if name is None:
            name = str(len(self._modules))
            if name in self._modules:
                raise KeyError("name exists")
        self.add_module(name, module)
        return self

    def forward(self, input):
        for module in self._modules.values():
            if isinstance(module, SparseModule):
                input = module(input)
            elif isinstance(input, SparseConvTensor):
                if input.indices.shape[0] != 0:
                    input.features = module(input.features)
            else:
                input = module(input)
        return input
