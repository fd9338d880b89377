"""The full drop-in for the reference's pybind11 extension module ``roiaware_pool3d_cuda``
(``pcdet/ops/roiaware_pool3d/src/roiaware_pool3d.cpp:171-176``): the RoI-aware voxel pooling of PartA2 besides the two
membership functions.

* ``forward(rois, pts, pts_feature, argmax, pts_idx_of_voxels, pooled_features, pool_method) -> 1`` --
  ``modest_roiaware_pool3d_forward`` of libmodest_hip.so on the current torch stream;
* ``backward(pts_idx_of_voxels, argmax, grad_out, grad_in, pool_method) -> 1`` -- ``modest_roiaware_pool3d_backward``;
  its ``(npoints, N)`` int32 workspace is a torch tensor allocated here (torch's caching allocator, no device allocation
  inside the library);
* ``points_in_boxes_gpu`` / ``points_in_boxes_cpu`` -- those of ``modest_amd.utils.roiaware_pool3d_cuda``.

The argument order is the reference's; every size is taken from the tensors.  A tensor that is not a contiguous CUDA
tensor of the expected dtype, or whose shape contradicts the others, raises ``RuntimeError``.  What the ops compute, and
where they deviate from the reference (the count word of a voxel's list is written, not incremented; the backward's
sum has one set of bits), is DESIGN.md section 7j.

Bound as ``sys.modules["pcdet.ops.roiaware_pool3d.roiaware_pool3d_cuda"]`` by
``modest_amd.utils.pcdet_bind.install(roiaware_pool=True)``; OpenPCDet's own ``roiaware_pool3d_utils.py`` runs on top of
it unchanged.  ``modest_amd.utils.roiaware_pool3d_cuda`` -- what the default ``install()`` binds -- keeps answering
``NotImplementedError`` for ``forward`` / ``backward``.
"""
import torch as _torch

from ._ext import _F, _I, _P, _call, _dims, _t
from .roiaware_pool3d_cuda import points_in_boxes_cpu, points_in_boxes_gpu  # noqa: F401  (re-exported)


def _method(pool_method):
    if isinstance(pool_method, bool) or not isinstance(pool_method, int) or pool_method not in (0, 1):
        raise RuntimeError(f"pool_method must be 0 (max) or 1 (avg), got {pool_method!r}")
    return pool_method


def forward(rois, pts, pts_feature, argmax, pts_idx_of_voxels, pooled_features, pool_method):
    """rois (N, 7), pts (npoints, 3), pts_feature (npoints, C), argmax int32 and pooled_features float32
    (N, out_x, out_y, out_z, C), pts_idx_of_voxels (N, out_x, out_y, out_z, max_pts_each_voxel) int32"""
    method = _method(pool_method)
    n = _dims(rois, "rois", 2, 7)[0]
    npts = _dims(pts, "pts", 2, 3)[0]
    c = _dims(pts_feature, "pts_feature", 2, None)[1]
    _, ox, oy, oz, max_pts = _dims(pts_idx_of_voxels, "pts_idx_of_voxels", 5, None)
    ts = (_t(rois, "rois", _F, (n, 7)), _t(pts, "pts", _F, (npts, 3)), _t(pts_feature, "pts_feature", _F, (npts, c)),
          _t(argmax, "argmax", _I, (n, ox, oy, oz, c)),
          _t(pts_idx_of_voxels, "pts_idx_of_voxels", _I, (n, ox, oy, oz, max_pts)),
          _t(pooled_features, "pooled_features", _F, (n, ox, oy, oz, c)))
    return _call("modest_roiaware_pool3d_forward", ts, n, npts, c, max_pts, ox, oy, oz, _P, _P, _P, _P, _P, _P, method)


def backward(pts_idx_of_voxels, argmax, grad_out, grad_in, pool_method):
    """pts_idx_of_voxels and argmax of ONE forward call, grad_out (N, out_x, out_y, out_z, C); ADDS into grad_in
    (npoints, C)"""
    method = _method(pool_method)
    n, ox, oy, oz, max_pts = _dims(pts_idx_of_voxels, "pts_idx_of_voxels", 5, None)
    c = _dims(grad_out, "grad_out", 5, None)[4]
    npts = _dims(grad_in, "grad_in", 2, None)[0]
    ts = [_t(pts_idx_of_voxels, "pts_idx_of_voxels", _I, (n, ox, oy, oz, max_pts)),
          _t(argmax, "argmax", _I, (n, ox, oy, oz, c)), _t(grad_out, "grad_out", _F, (n, ox, oy, oz, c)),
          _t(grad_in, "grad_in", _F, (npts, c))]
    work = _torch.empty((npts, n), dtype=_I, device=grad_in.device)   # T[p][b]; the library presets it
    ts.append(work)
    return _call("modest_roiaware_pool3d_backward", ts, n, npts, ox, oy, oz, c, max_pts, _P, _P, _P, _P, method, _P,
                 work.numel() * 4)
