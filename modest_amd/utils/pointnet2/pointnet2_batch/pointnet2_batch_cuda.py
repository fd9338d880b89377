"""Drop-in for the reference's pybind11 extension module ``pointnet2_batch_cuda``
(``pcdet/ops/pointnet2/pointnet2_batch/src/pointnet2_api.cpp:10-24``): the same nine
functions with the same integer and tensor arguments and return value 1, forwarded to
the C ABI of libmodest_hip.so on the current torch stream.  The reference checks
nothing; here a tensor that is not a contiguous CUDA tensor of the expected dtype, whose
shape contradicts the integer arguments or has a dimension above 2^31 - 1 raises
``RuntimeError`` (the checks all drop-ins share, ``modest_amd/utils/_ext.py``).

Bound as ``sys.modules["pcdet.ops.pointnet2.pointnet2_batch.pointnet2_batch_cuda"]``
(INTEGRATION.md), OpenPCDet's own ``pointnet2_utils.py`` / ``pointnet2_modules.py`` run
on top of it unchanged.
"""
from ..._ext import _F, _I, _P, _call, _ints, _t


def ball_query_wrapper(b, n, m, radius, nsample, new_xyz_tensor, xyz_tensor, idx_tensor):
    _ints(b=b, n=n, m=m, nsample=nsample)
    ts = (_t(new_xyz_tensor, "new_xyz", _F, (b, m, 3)), _t(xyz_tensor, "xyz", _F, (b, n, 3)),
          _t(idx_tensor, "idx", _I, (b, m, nsample)))
    return _call("modest_pn2_ball_query", ts, b, n, m, float(radius), nsample, _P, _P, _P)


def group_points_wrapper(b, c, n, npoints, nsample, points_tensor, idx_tensor, out_tensor):
    _ints(b=b, c=c, n=n, npoints=npoints, nsample=nsample)
    ts = (_t(points_tensor, "points", _F, (b, c, n)), _t(idx_tensor, "idx", _I, (b, npoints, nsample)),
          _t(out_tensor, "out", _F, (b, c, npoints, nsample)))
    return _call("modest_pn2_group", ts, b, c, n, npoints, nsample, _P, _P, _P)


def group_points_grad_wrapper(b, c, n, npoints, nsample, grad_out_tensor, idx_tensor, grad_points_tensor):
    _ints(b=b, c=c, n=n, npoints=npoints, nsample=nsample)
    ts = (_t(grad_out_tensor, "grad_out", _F, (b, c, npoints, nsample)), _t(idx_tensor, "idx", _I, (b, npoints, nsample)),
          _t(grad_points_tensor, "grad_points", _F, (b, c, n)))
    return _call("modest_pn2_group_grad", ts, b, c, n, npoints, nsample, _P, _P, _P)


def gather_points_wrapper(b, c, n, npoints, points_tensor, idx_tensor, out_tensor):
    _ints(b=b, c=c, n=n, npoints=npoints)
    ts = (_t(points_tensor, "points", _F, (b, c, n)), _t(idx_tensor, "idx", _I, (b, npoints)),
          _t(out_tensor, "out", _F, (b, c, npoints)))
    return _call("modest_pn2_gather", ts, b, c, n, npoints, _P, _P, _P)


def gather_points_grad_wrapper(b, c, n, npoints, grad_out_tensor, idx_tensor, grad_points_tensor):
    _ints(b=b, c=c, n=n, npoints=npoints)
    ts = (_t(grad_out_tensor, "grad_out", _F, (b, c, npoints)), _t(idx_tensor, "idx", _I, (b, npoints)),
          _t(grad_points_tensor, "grad_points", _F, (b, c, n)))
    return _call("modest_pn2_gather_grad", ts, b, c, n, npoints, _P, _P, _P)


def furthest_point_sampling_wrapper(b, n, m, points_tensor, temp_tensor, idx_tensor):
    _ints(b=b, n=n, m=m)
    if n < 1:
        raise RuntimeError("furthest point sampling needs n >= 1")
    ts = (_t(points_tensor, "points", _F, (b, n, 3)), _t(temp_tensor, "temp", _F, (b, n)),
          _t(idx_tensor, "idx", _I, (b, m)))
    return _call("modest_pn2_furthest_point_sample", ts, b, n, m, _P, _P, _P)


def three_nn_wrapper(b, n, m, unknown_tensor, known_tensor, dist2_tensor, idx_tensor):
    _ints(b=b, n=n, m=m)
    ts = (_t(unknown_tensor, "unknown", _F, (b, n, 3)), _t(known_tensor, "known", _F, (b, m, 3)),
          _t(dist2_tensor, "dist2", _F, (b, n, 3)), _t(idx_tensor, "idx", _I, (b, n, 3)))
    return _call("modest_pn2_three_nn", ts, b, n, m, _P, _P, _P, _P)


def three_interpolate_wrapper(b, c, m, n, points_tensor, idx_tensor, weight_tensor, out_tensor):
    _ints(b=b, c=c, m=m, n=n)
    ts = (_t(points_tensor, "points", _F, (b, c, m)), _t(idx_tensor, "idx", _I, (b, n, 3)),
          _t(weight_tensor, "weight", _F, (b, n, 3)), _t(out_tensor, "out", _F, (b, c, n)))
    return _call("modest_pn2_three_interpolate", ts, b, c, m, n, _P, _P, _P, _P)


def three_interpolate_grad_wrapper(b, c, n, m, grad_out_tensor, idx_tensor, weight_tensor, grad_points_tensor):
    _ints(b=b, c=c, m=m, n=n)
    ts = (_t(grad_out_tensor, "grad_out", _F, (b, c, n)), _t(idx_tensor, "idx", _I, (b, n, 3)),
          _t(weight_tensor, "weight", _F, (b, n, 3)), _t(grad_points_tensor, "grad_points", _F, (b, c, m)))
    return _call("modest_pn2_three_interpolate_grad", ts, b, c, n, m, _P, _P, _P, _P)
