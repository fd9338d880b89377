"""Drop-in for the reference's pybind11 extension module ``pointnet2_stack_cuda``
(``pcdet/ops/pointnet2/pointnet2_stack/src/pointnet2_api.cpp``): the same eight functions
with the same integer and tensor arguments and return value 1, forwarded to the C ABI of
libmodest_hip.so on the current torch stream.  The reference checks little; here a tensor
that is not a contiguous CUDA tensor of the expected dtype, whose shape contradicts the
integer arguments or the other tensors or has a dimension above 2^31 - 1 raises
``RuntimeError`` (the checks all drop-ins share, ``modest_amd/utils/_ext.py``).

All scans of a batch are rows of one ``(N1 + N2 + ..., C)`` tensor; the ``*_batch_cnt``
tensors are int32 of shape ``(B,)`` on the device and are never read on the host.

Bound as ``sys.modules["pcdet.ops.pointnet2.pointnet2_stack.pointnet2_stack_cuda"]`` by
``pcdet_bind.install(point_stack=True)``, OpenPCDet's own
``pointnet2_stack/pointnet2_utils.py``, ``voxel_query_utils.py`` and the modules on top of
them run on it unchanged.
"""
from ..._ext import _F, _I, _P, _call, _ints, _t


def ball_query_wrapper(B, M, radius, nsample, new_xyz_tensor, new_xyz_batch_cnt_tensor, xyz_tensor, xyz_batch_cnt_tensor,
                       idx_tensor):
    _ints(B=B, M=M, nsample=nsample)
    ts = (_t(new_xyz_tensor, "new_xyz", _F, (M, 3)), _t(new_xyz_batch_cnt_tensor, "new_xyz_batch_cnt", _I, (B,)),
          _t(xyz_tensor, "xyz", _F, (None, 3)), _t(xyz_batch_cnt_tensor, "xyz_batch_cnt", _I, (B,)),
          _t(idx_tensor, "idx", _I, (M, nsample)))
    return _call("modest_pn2s_ball_query", ts, B, M, float(radius), nsample, _P, _P, _P, _P, xyz_tensor.shape[0], _P)


def voxel_query_wrapper(M, R1, R2, R3, nsample, radius, z_range, y_range, x_range, new_xyz_tensor, xyz_tensor,
                        new_coords_tensor, point_indices_tensor, idx_tensor):
    _ints(M=M, R1=R1, R2=R2, R3=R3, nsample=nsample, z_range=z_range, y_range=y_range, x_range=x_range)
    ts = (_t(new_xyz_tensor, "new_xyz", _F, (M, 3)), _t(xyz_tensor, "xyz", _F, (None, 3)),
          _t(new_coords_tensor, "new_coords", _I, (M, 4)), _t(point_indices_tensor, "point_indices", _I, (None, R1, R2, R3)),
          _t(idx_tensor, "idx", _I, (M, nsample)))
    return _call("modest_pn2s_voxel_query", ts, point_indices_tensor.shape[0], M, R1, R2, R3, nsample, float(radius),
                 z_range, y_range, x_range, _P, _P, xyz_tensor.shape[0], _P, _P, _P)


def furthest_point_sampling_wrapper(b, n, m, points_tensor, temp_tensor, idx_tensor):
    # the stack extension's sampling kernel is the batch one (tools/make_golden_pointnet2_stack.py asserts it)
    _ints(b=b, n=n, m=m)
    if n < 1:
        raise RuntimeError("furthest point sampling needs n >= 1")
    ts = (_t(points_tensor, "points", _F, (b, n, 3)), _t(temp_tensor, "temp", _F, (b, n)),
          _t(idx_tensor, "idx", _I, (b, m)))
    return _call("modest_pn2_furthest_point_sample", ts, b, n, m, _P, _P, _P)


def group_points_wrapper(B, M, C, nsample, features_tensor, features_batch_cnt_tensor, idx_tensor, idx_batch_cnt_tensor,
                         out_tensor):
    _ints(B=B, M=M, C=C, nsample=nsample)
    ts = (_t(features_tensor, "features", _F, (None, C)), _t(features_batch_cnt_tensor, "features_batch_cnt", _I, (B,)),
          _t(idx_tensor, "idx", _I, (M, nsample)), _t(idx_batch_cnt_tensor, "idx_batch_cnt", _I, (B,)),
          _t(out_tensor, "out", _F, (M, C, nsample)))
    return _call("modest_pn2s_group", ts, B, M, C, nsample, features_tensor.shape[0], _P, _P, _P, _P, _P)


def group_points_grad_wrapper(B, M, C, N, nsample, grad_out_tensor, idx_tensor, idx_batch_cnt_tensor,
                              features_batch_cnt_tensor, grad_features_tensor):
    _ints(B=B, M=M, C=C, N=N, nsample=nsample)
    ts = (_t(grad_out_tensor, "grad_out", _F, (M, C, nsample)), _t(idx_tensor, "idx", _I, (M, nsample)),
          _t(idx_batch_cnt_tensor, "idx_batch_cnt", _I, (B,)), _t(features_batch_cnt_tensor, "features_batch_cnt", _I, (B,)),
          _t(grad_features_tensor, "grad_features", _F, (N, C)))
    return _call("modest_pn2s_group_grad", ts, B, M, C, N, nsample, _P, _P, _P, _P, _P)


def three_nn_wrapper(unknown_tensor, unknown_batch_cnt_tensor, known_tensor, known_batch_cnt_tensor, dist2_tensor,
                     idx_tensor):
    ts = [_t(unknown_tensor, "unknown", _F, (None, 3)), _t(unknown_batch_cnt_tensor, "unknown_batch_cnt", _I, (None,)),
          _t(known_tensor, "known", _F, (None, 3))]
    B, N, M = unknown_batch_cnt_tensor.shape[0], unknown_tensor.shape[0], known_tensor.shape[0]
    ts += [_t(known_batch_cnt_tensor, "known_batch_cnt", _I, (B,)), _t(dist2_tensor, "dist2", _F, (N, 3)),
           _t(idx_tensor, "idx", _I, (N, 3))]
    return _call("modest_pn2s_three_nn", ts, B, N, M, _P, _P, _P, _P, _P, _P)


def three_interpolate_wrapper(features_tensor, idx_tensor, weight_tensor, out_tensor):
    ts = [_t(features_tensor, "features", _F, (None, None)), _t(idx_tensor, "idx", _I, (None, 3))]
    M, C, N = features_tensor.shape[0], features_tensor.shape[1], idx_tensor.shape[0]
    ts += [_t(weight_tensor, "weight", _F, (N, 3)), _t(out_tensor, "out", _F, (N, C))]
    return _call("modest_pn2s_three_interpolate", ts, N, C, M, _P, _P, _P, _P)


def three_interpolate_grad_wrapper(grad_out_tensor, idx_tensor, weight_tensor, grad_features_tensor):
    ts = [_t(grad_out_tensor, "grad_out", _F, (None, None))]
    N, C = grad_out_tensor.shape
    ts += [_t(idx_tensor, "idx", _I, (N, 3)), _t(weight_tensor, "weight", _F, (N, 3)),
           _t(grad_features_tensor, "grad_features", _F, (None, C))]
    return _call("modest_pn2s_three_interpolate_grad", ts, N, C, grad_features_tensor.shape[0], _P, _P, _P, _P)
