"""The front the extension-module drop-ins share (``pointnet2_batch_cuda``, ``pointnet2_stack_cuda``,
``roipoint_pool3d_cuda``, ``roiaware_pool3d_cuda``, ``roiaware_voxel_pool_cuda``): argument checks that raise
``RuntimeError``, and the call into the C ABI of libmodest_hip.so on the tensors' device and the current torch stream.
The library is opened by the first call that gets past its checks, never by an import.
"""
import torch as _torch

from .. import _lib


def _t(t, name, dtype, shape):
    """a contiguous CUDA tensor of `dtype` and `shape` (None entries are free), below 2^31 in every dimension"""
    if not isinstance(t, _torch.Tensor):
        raise RuntimeError(f"{name} must be a tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be CUDA tensor")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous tensor")
    if t.dtype != dtype:
        raise RuntimeError(f"{name} must be {dtype}, got {t.dtype}")
    have = tuple(t.shape)
    if have != shape and (len(have) != len(shape) or any(w is not None and h != w for h, w in zip(have, shape))):
        want = tuple("*" if s is None else s for s in shape)   # (the first test: one comparison where nothing is free)
        raise RuntimeError(f"{name} has shape {have}, the arguments say {want}")
    if have and max(have) > 2147483647:
        raise RuntimeError(f"{name} has shape {have}: more than 2^31 - 1 rows")
    return t


def _ints(**kw):
    for k, v in kw.items():
        if isinstance(v, bool) or not isinstance(v, int):
            raise RuntimeError(f"{k} must be an int")
        if v < 0 or v > 2147483647:
            raise RuntimeError(f"{k} = {v} is out of range")


def _dims(t, name, ndim, last):
    """the shape of a tensor of `ndim` dimensions whose last one is `last` (None: free), for sizes taken from tensors"""
    if not isinstance(t, _torch.Tensor):
        raise RuntimeError(f"{name} must be a tensor")
    if t.dim() != ndim or (last is not None and t.shape[-1] != last):
        raise RuntimeError(f"{name} has shape {tuple(t.shape)}, expected {ndim} dimensions"
                           + (f" with the last one {last}" if last is not None else ""))
    return tuple(t.shape)


def _call(name, tensors, *args):
    dev = tensors[0].device
    for t in tensors[1:]:
        if t.device != dev:
            raise RuntimeError("all tensors must be on one device")
    fn = _fns.get(name)
    if fn is None:
        fn = _fns[name] = getattr(_lib.load(), name)
    ptrs = iter(t.data_ptr() for t in tensors)
    argv = [next(ptrs) if a is _P else a for a in args]
    if dev.index == _torch.cuda.current_device():
        rc = fn(*argv, _torch.cuda.current_stream().cuda_stream)
    else:
        with _torch.cuda.device(dev):
            rc = fn(*argv, _torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        _lib.check(rc, name)
    return 1


_fns = {}
_P = object()   # placeholder: the next tensor's device pointer
_F, _I = _torch.float32, _torch.int32
