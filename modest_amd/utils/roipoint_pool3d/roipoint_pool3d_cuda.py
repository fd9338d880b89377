"""Drop-in for the reference's pybind11 extension module ``roipoint_pool3d_cuda``
(``pcdet/ops/roipoint_pool3d/src/roipoint_pool3d.cpp:28-59``): ``forward`` with the same five
tensor arguments and return value 1, forwarded to ``modest_roipoint_pool3d`` of libmodest_hip.so
on the current torch stream.  The reference asserts contiguity and takes every size from the
tensors; here a tensor that is not a contiguous CUDA tensor of the expected dtype, or whose
shape contradicts the others, raises ``RuntimeError`` (``modest_amd/utils/_ext.py``).

Bound as ``sys.modules["pcdet.ops.roipoint_pool3d.roipoint_pool3d_cuda"]`` (INTEGRATION.md,
``modest_amd.utils.pcdet_bind.install``), OpenPCDet's own ``roipoint_pool3d_utils.py`` runs on
top of it unchanged.  What the op computes is DESIGN.md section 7e.
"""
from .._ext import _F, _I, _P, _call, _dims, _t


def forward(xyz, boxes3d, pts_feature, pooled_features, pooled_empty_flag):
    """xyz (B, N, 3), boxes3d (B, M, 7), pts_feature (B, N, C), pooled_features (B, M, S, 3 + C),
    pooled_empty_flag (B, M) int32"""
    b, n, _ = _dims(xyz, "xyz", 3, 3)
    m = _dims(boxes3d, "boxes3d", 3, 7)[1]
    c = _dims(pts_feature, "pts_feature", 3, None)[2]
    s = _dims(pooled_features, "pooled_features", 4, None)[2]
    ts = (_t(xyz, "xyz", _F, (b, n, 3)), _t(boxes3d, "boxes3d", _F, (b, m, 7)),
          _t(pts_feature, "pts_feature", _F, (b, n, c)), _t(pooled_features, "pooled_features", _F, (b, m, s, 3 + c)),
          _t(pooled_empty_flag, "pooled_empty_flag", _I, (b, m)))
    return _call("modest_roipoint_pool3d", ts, b, n, m, c, s, _P, _P, _P, _P, _P)
