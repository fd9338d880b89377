"""Drop-in for the reference's pybind11 extension module ``roiaware_pool3d_cuda``
(``pcdet/ops/roiaware_pool3d/src/roiaware_pool3d.cpp:171-176``), as far as PointRCNN and the dataset
code use it:

* ``points_in_boxes_gpu(boxes, pts, box_idx_of_points) -> 1`` -- ``modest_points_in_boxes`` of
  libmodest_hip.so on the current torch stream.  A tensor that is not a
  contiguous CUDA tensor of the expected dtype, or whose shape contradicts the others, raises
  ``RuntimeError``.
* ``points_in_boxes_cpu(boxes, pts, pts_indices) -> 1`` -- pure host code (numpy,
  ``kitti_infos.points_in_boxes_host``: the reference's host predicate with the host C library's
  ``cosf`` / ``sinf``).  OpenPCDet calls it from DataLoader workers; it never opens the GPU.
* ``forward`` / ``backward`` -- the RoI-aware voxel pooling of PartA2 is not provided BY THIS MODULE: they raise
  ``NotImplementedError``.  The full drop-in, with both, is ``modest_amd.utils.roiaware_voxel_pool_cuda``
  (``pcdet_bind.install(roiaware_pool=True)``).

Bound as ``sys.modules["pcdet.ops.roiaware_pool3d.roiaware_pool3d_cuda"]`` (INTEGRATION.md,
``modest_amd.utils.pcdet_bind.install``).
"""
import torch as _torch

from ._ext import _F, _I, _P, _call, _dims, _t


def points_in_boxes_gpu(boxes_tensor, pts_tensor, box_idx_of_points_tensor):
    """boxes (B, M, 7), pts (B, N, 3), box_idx_of_points (B, N) int32 (the caller fills -1)"""
    b, m, _ = _dims(boxes_tensor, "boxes", 3, 7)
    n = _dims(pts_tensor, "pts", 3, 3)[1]
    ts = (_t(boxes_tensor, "boxes", _F, (b, m, 7)), _t(pts_tensor, "pts", _F, (b, n, 3)),
          _t(box_idx_of_points_tensor, "box_idx_of_points", _I, (b, n)))
    return _call("modest_points_in_boxes", ts, b, m, n, _P, _P, _P)


def points_in_boxes_cpu(boxes_tensor, pts_tensor, pts_indices_tensor):
    """boxes (M, 7), pts (N, 3), pts_indices (M, N) int32, all on the host: pts_indices[i, k] = 1 if box i holds point k"""
    from ..kitti_infos import points_in_boxes_host
    for t, name in ((boxes_tensor, "boxes"), (pts_tensor, "pts"), (pts_indices_tensor, "pts_indices")):
        if not isinstance(t, _torch.Tensor):
            raise RuntimeError(f"{name} must be a tensor")
        if t.is_cuda:
            raise RuntimeError(f"{name} must be a CPU tensor")
        if not t.is_contiguous():
            raise RuntimeError(f"{name} must be contiguous tensor")
    m, _ = _dims(boxes_tensor, "boxes", 2, 7)
    n, _ = _dims(pts_tensor, "pts", 2, 3)
    if boxes_tensor.dtype != _F or pts_tensor.dtype != _F or pts_indices_tensor.dtype != _I:
        raise RuntimeError("boxes and pts must be float32, pts_indices int32")
    if tuple(pts_indices_tensor.shape) != (m, n):
        raise RuntimeError(f"pts_indices has shape {tuple(pts_indices_tensor.shape)}, boxes and pts say {(m, n)}")
    pts_indices_tensor.copy_(_torch.from_numpy(points_in_boxes_host(pts_tensor.numpy(), boxes_tensor.numpy())))
    return 1


def forward(*args, **kwargs):
    raise NotImplementedError("RoI-aware voxel pooling (PartA2's roiaware_pool3d_cuda.forward) is not provided")


def backward(*args, **kwargs):
    raise NotImplementedError("RoI-aware voxel pooling (PartA2's roiaware_pool3d_cuda.backward) is not provided")
