"""Named cases for the PillarVFE / BEV scatter kernels (csrc/pillar_vfe.hip) at the smallest shapes that
can go wrong: the seams of the partial-sum tree (pillar_vfe_seq.RUN pillars a wavefront, RUN * GROUP pillars a group), the ends
of every limit, degenerate statistics and non-finite points.  Shared by the CPU and the GPU tests; built once."""
import numpy as np

import pillar_vfe_seq as seq

F = np.float32
RUN, SEAM = seq.RUN, seq.RUN * seq.GROUP


def _case(seed, P, S, **kw):
    tweak = kw.pop("tweak", None)
    case = seq.make_case(seed, P, S, **kw)
    if tweak:
        tweak(case)
    return case


def _set(key, index, value):
    def tweak(case):
        case[key][index] = value
    return tweak


def _nonfinite(value):
    def tweak(case):
        case["voxels"][1, 0, 1] = value
    return tweak


CASES = {
    # one pillar (training needs two rows), counts at their ends
    "p1": _case(101, 1, 4, C=8),
    "num_all_1": _case(102, 5, 6, C=8, num=1),
    "num_all_S": _case(103, 5, 6, C=8, num=6),
    "num_0_train": _case(104, 5, 6, C=8, num=[3, 0, 6, 1, 2]),
    "num_0_eval": _case(105, 5, 6, C=8, num=[3, 0, 6, 1, 2], training=False),
    # a wavefront's run of pillars: one below, at, one above
    "run_below": _case(106, RUN - 1, 3, C=64),
    "run_at": _case(107, RUN, 3, C=64),
    "run_above": _case(108, RUN + 1, 3, C=64),
    # the second seam: a group of runs
    "group_below": _case(109, SEAM - 1, 2, C=8, ny=50, nx=50),
    "group_at": _case(110, SEAM, 2, C=8, ny=50, nx=50),
    "group_above": _case(111, SEAM + 1, 2, C=8, ny=50, nx=50),
    # channels
    "c1": _case(112, 6, 5, C=1),
    "c32": _case(113, 6, 5, C=32),
    "c63": _case(114, 6, 5, C=63),
    "c64": _case(115, 6, 5, C=64),
    # features of a point at 1 and 16
    "k1": _case(116, 6, 5, Cp=4, C=16, parts=0),
    "k16": _case(117, 6, 5, Cp=9, C=16, parts=seq.XYZ | seq.CLUSTER | seq.CENTER | seq.DIST),
    # slots
    "s1": _case(118, 7, 1, C=16),
    "s20": _case(119, 4, 20, C=16),
    "s32": _case(120, 4, 32, C=16),
    "s255": _case(121, 3, 255, C=16),
    # degenerate statistics and gradients
    "zero_weight_row": _case(122, 6, 5, C=8, tweak=_set("W", (3, slice(None)), 0.0)),         # var = 0
    "relu_zeroes_channel": _case(123, 6, 5, C=8, tweak=_set("beta", 2, -1000.0)),               # its gradient is zero
    "gamma_0": _case(124, 6, 5, C=8, tweak=_set("gamma", 5, 0.0)),
    # non-finite points
    "nan_point_train": _case(125, 6, 5, C=8, num=5, tweak=_nonfinite(np.nan)),
    "inf_point_train": _case(126, 6, 5, C=8, num=5, tweak=_nonfinite(np.inf)),
    "nan_point_eval": _case(127, 6, 5, C=8, num=5, training=False, tweak=_nonfinite(np.nan)),
    "inf_point_eval": _case(128, 6, 5, C=8, num=5, training=False, tweak=_nonfinite(-np.inf)),
    # the index tensors as they may arrive
    "num_i32_coords_i64": _case(129, 6, 5, C=8, num_dtype=np.int32, coord_dtype=np.int64),
    "num_i64_coords_i32": _case(130, 6, 5, C=8, num_dtype=np.int64, coord_dtype=np.int32),
    "num_f32_coords_i32": _case(131, 6, 5, C=8, num_dtype=F, coord_dtype=np.int32),
    # the module's own eps and momentum, the cumulative average, two steps
    "eps_momentum": _case(132, 6, 5, C=8, eps=1e-5, momentum=0.1, fresh=False),
    "momentum_none": _case(133, 6, 5, C=8, momentum=None, steps=3),
    "eval": _case(134, 6, 5, C=8, training=False),
    "rel_dist": _case(135, 6, 5, Cp=5, C=8, use_abs=False, with_dist=True),
}

# P = 64 000 x 32 x 4 -> 64, B = 4 on a 560 x 496 grid as the Lyft config has it
MID = {"lyft": dict(seed=140, P=64000, S=32, Cp=4, C=64, B=4, ny=496, nx=560)}


def mid(name="lyft"):
    return seq.make_case(**MID[name])


def out_of_range_coords(case, dtype):
    """the case's coords with one row pushed out of range by one on each side of each column -> (coords, the rows pushed)"""
    B, ny, nx = case["batch_size"], case["ny"], case["nx"]
    c = case["coords"].astype(np.int64).copy()
    moves = [(0, B), (0, -1), (1, 1), (1, -1), (2, ny), (2, -1), (3, nx), (3, -1)]
    assert len(c) >= len(moves) + 2
    for row, (col, value) in enumerate(moves):
        c[row, col] = value
    return c.astype(dtype), list(range(len(moves)))
