"""Thin Python wrappers over the C ABI (include/modest_hip.h).

PyTorch-ROCm tensors are used only as device-memory handles and for the
current HIP stream; every computation happens inside libmodest_hip.so.  All
functions raise if the library or a GPU is missing (no CPU fallback).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import Context, check, default_context, load


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream() -> int:
    """handle of PyTorch's current HIP stream (the raw getter skips the Stream object: ~8 us per call)"""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _dev(t: torch.Tensor, dtype, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise ValueError(f"{name} must be a device tensor (PyTorch-ROCm 'cuda')")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


def _ctx(ctx: Optional[Context], t: torch.Tensor) -> Context:
    return ctx if ctx is not None else default_context(t.device.index or 0)


def _np_ptr(a: np.ndarray) -> int:
    return a.ctypes.data


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    """the address of a tensor's data; None for None"""
    return t.data_ptr() if t is not None else None


def _ptr_filled(t: Optional[torch.Tensor]) -> Optional[int]:
    """the address of a tensor's data; None for None and for a tensor without elements"""
    return t.data_ptr() if t is not None and t.numel() else None


# --------------------------------------------------------------------------- what the detector ops do with their arguments
def _device_tensors(named, dtypes=None, optional=(), dtype_error=ValueError, same_device=False):
    """The loop a detector op opens with, over `named` = ((name, tensor), ...) in the order in which they are refused: each
    must be a device tensor, and then of float32, or of one of the types `dtypes` ({name: tuple}) gives its name; another
    type raises `dtype_error` (None: types are not looked at).  A None is passed over for a name among `optional`.
    same_device: each must also lie on the device of the first.  -> that device"""
    dev = None
    for name, t in named:
        if t is None and name in optional:
            continue
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError(f"{name} must be a device tensor (PyTorch-ROCm 'cuda')")
        if dtype_error is not None:
            allowed = (dtypes or {}).get(name, (torch.float32,))
            if t.dtype not in allowed:
                *head, last = (str(d).replace("torch.", "") for d in allowed)
                raise dtype_error(f"{name} must be {', '.join(head) + ' or ' + last if head else last}, got {t.dtype}")   # "int32, int64 or float32"
        dev = t.device if dev is None else dev
        if same_device and t.device != dev:
            raise ValueError(f"{name} is on {t.device}, {named[0][0]} on {dev}")
    return dev


def _outputs(want, out, dev, anchor=None, absent=None):
    """The output buffers of a call.  `want`: (name, dtype, shape, due) per buffer.  out None: new ones on `dev`, None where
    none is due.  Else `out` must hold as many entries; one that is not due must be None and one that is due a tensor, refused
    as "out <name> " + `absent`[0] / `absent`[1] (absent None: every buffer is due and its presence is not looked at); a
    tensor must pass `_dev` as "out <name>" and have the shape and the device, refused in two messages that name the device
    of the argument `anchor`, or, without an anchor, in one.  -> the buffers"""
    if out is None:
        return [torch.empty(shape, dtype=dtype, device=dev) if due else None for _, dtype, shape, due in want]
    if len(out) != len(want):
        raise ValueError(f"out must be ({', '.join(name for name, _, _, _ in want)})")
    for t, (name, dtype, shape, due) in zip(out, want):
        if absent is not None:
            if not due and t is not None:
                raise ValueError(f"out {name} {absent[0]}")
            if due and not torch.is_tensor(t):
                raise ValueError(f"out {name} {absent[1]}")
            if not due:
                continue
        _dev(t, dtype, f"out {name}")
        if anchor is None:
            if tuple(t.shape) != shape or t.device != dev:
                raise ValueError(f"out {name} has shape {tuple(t.shape)} on {t.device}, expected {shape} on {dev}")
            continue
        if tuple(t.shape) != shape:
            raise ValueError(f"out {name} has shape {tuple(t.shape)}, expected {shape}")
        if t.device != dev:
            raise ValueError(f"out {name} is on {t.device}, {anchor} on {dev}")
    return out


def _workspace(nbytes: int, workspace: Optional[torch.Tensor], dev) -> torch.Tensor:
    """`workspace` if it holds `nbytes` on `dev`, else a new one: an uint8 device tensor either way"""
    if workspace is None or workspace.numel() < nbytes or workspace.device != dev:
        workspace = torch.empty((max(nbytes, 256),), dtype=torch.uint8, device=dev)
    return _dev(workspace, torch.uint8, "workspace")


def _workspace_bytes(fn_name: str, *ints) -> int:
    """the library's `fn_name`(ints): the bytes of a workspace, or the library's refusal raised"""
    nb = int(getattr(load(), fn_name)(*(int(a) for a in ints)))
    if nb < 0:
        check(nb, fn_name)
    return nb


def _cfg_get(cfg, name, *default):
    """cfg[name] of a dict, cfg.name of anything else; `default` where it is absent"""
    if isinstance(cfg, dict):
        return cfg.get(name, *default) if default else cfg[name]
    return getattr(cfg, name, *default)


# --------------------------------------------------------------------------- PP score
def pp_count(live_xyz: torch.Tensor, hist_xyz: torch.Tensor, trav_offsets: Sequence[int],
             radius: float = 0.3, ctx: Optional[Context] = None) -> torch.Tensor:
    """count_neighbors (pre_compute_pp_score.py:54-60): (N,T) int32 on device."""
    lib = load()
    _dev(live_xyz, torch.float32, "live_xyz")
    _dev(hist_xyz, torch.float32, "hist_xyz")
    off = np.ascontiguousarray(np.asarray(trav_offsets, dtype=np.int64))
    T = off.shape[0] - 1
    n = live_xyz.shape[0]
    assert live_xyz.ndim == 2 and live_xyz.shape[1] == 3
    assert hist_xyz.ndim == 2 and hist_xyz.shape[1] == 3 and off[-1] <= hist_xyz.shape[0]
    counts = torch.empty((n, T), dtype=torch.int32, device=live_xyz.device)
    c = _ctx(ctx, live_xyz)
    check(lib.modest_pp_count(c.handle, live_xyz.data_ptr(), n, hist_xyz.data_ptr(), _np_ptr(off), T,
                              float(radius), counts.data_ptr(), _stream()), "modest_pp_count")
    return counts


def pp_entropy(counts: torch.Tensor, ctx: Optional[Context] = None) -> torch.Tensor:
    """compute_ephe_score (pre_compute_pp_score.py:68-75) + float32 cast (:195-196)."""
    lib = load()
    _dev(counts, torch.int32, "counts")
    n, T = counts.shape
    H = torch.empty((n,), dtype=torch.float32, device=counts.device)
    c = _ctx(ctx, counts)
    check(lib.modest_pp_entropy(c.handle, counts.data_ptr(), n, T, H.data_ptr(), _stream()),
          "modest_pp_entropy")
    return H


def pp_score(live_xyz: torch.Tensor, hist_xyz: torch.Tensor, trav_offsets: Sequence[int],
             radius: float = 0.3, ctx: Optional[Context] = None, return_counts: bool = False,
             out: Optional[torch.Tensor] = None):
    """Fused count + entropy: (N,) float32 PP score on device."""
    lib = load()
    _dev(live_xyz, torch.float32, "live_xyz")
    _dev(hist_xyz, torch.float32, "hist_xyz")
    off = np.ascontiguousarray(np.asarray(trav_offsets, dtype=np.int64))
    T = off.shape[0] - 1
    n = live_xyz.shape[0]
    assert hist_xyz.ndim == 2 and hist_xyz.shape[1] == 3 and off[-1] <= hist_xyz.shape[0]
    H = out if out is not None else torch.empty((n,), dtype=torch.float32, device=live_xyz.device)
    counts = torch.empty((n, T), dtype=torch.int32, device=live_xyz.device) if return_counts else None
    c = _ctx(ctx, live_xyz)
    check(lib.modest_pp_score(c.handle, live_xyz.data_ptr(), n, hist_xyz.data_ptr(), _np_ptr(off), T,
                              float(radius), counts.data_ptr() if counts is not None else None,
                              H.data_ptr(), _stream()), "modest_pp_score")
    return (H, counts) if return_counts else H


# --------------------------------------------------------------------------- transform
def transform_points(pts: torch.Tensor, T: np.ndarray, remove_center: bool = False,
                     ctx: Optional[Context] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """transform_points (utils/pointcloud_utils.py:11-19) of an (n,3|4) float32 frame,
    optionally preceded by remove_center (pre_compute_pp_score.py:48-52)."""
    lib = load()
    _dev(pts, torch.float32, "pts")
    assert pts.ndim == 2 and pts.shape[1] in (3, 4)
    n = pts.shape[0]
    T16 = np.ascontiguousarray(np.asarray(T, dtype=np.float32).reshape(4, 4))
    if out is None:
        out = torch.empty((n, 3), dtype=torch.float32, device=pts.device)
    else:
        _dev(out, torch.float32, "out")
        assert out.shape == (n, 3)
    c = _ctx(ctx, pts)
    if not remove_center:
        check(lib.modest_transform_points(c.handle, pts.data_ptr(), n, pts.shape[1], _np_ptr(T16), 0,
                                          out.data_ptr(), None, _stream()), "modest_transform_points")
        return out
    n_out = torch.zeros((1,), dtype=torch.int64, device=pts.device)
    check(lib.modest_transform_points(c.handle, pts.data_ptr(), n, pts.shape[1], _np_ptr(T16), 1,
                                      out.data_ptr(), n_out.data_ptr(), _stream()), "modest_transform_points")
    return out[: int(n_out.item())]


def project_velo_to_rect(pts: torch.Tensor, V2C: np.ndarray, R0: np.ndarray, ctx: Optional[Context] = None) -> torch.Tensor:
    """Calibration.project_velo_to_rect (kitti_util.py:327-329) of the scan rows: (n,3) float64 on the
    device, bit-identical to numpy's two dgemm products."""
    lib = load()
    _dev(pts, torch.float32, "pts")
    v = np.ascontiguousarray(V2C, dtype=np.float64).reshape(12)
    r = np.ascontiguousarray(R0, dtype=np.float64).reshape(9)
    out = torch.empty((pts.shape[0], 3), dtype=torch.float64, device=pts.device)
    c = _ctx(ctx, pts)
    check(lib.modest_project_velo_to_rect(c.handle, pts.data_ptr(), pts.shape[0], pts.shape[1], _np_ptr(v), _np_ptr(r),
                                          out.data_ptr(), _stream()), "modest_project_velo_to_rect")
    return out


# --------------------------------------------------------------------------- plane / RANSAC
def plane_candidates(pts: torch.Tensor, max_hs: float, ptc_range, ctx: Optional[Context] = None):
    """Candidate mask of estimate_plane (pointcloud_utils.py:45-49), compacted in input order.
    Returns (cand_xyz (m,3) f32, cand_idx (m,) i32)."""
    lib = load()
    _dev(pts, torch.float32, "pts")
    n = pts.shape[0]
    cand = torch.empty((n, 3), dtype=torch.float32, device=pts.device)
    idx = torch.empty((n,), dtype=torch.int32, device=pts.device)
    c = _ctx(ctx, pts)
    cnt = c.host_counter()   # pinned host word, always written by the call (n == 0: a memset)
    (xlo, xhi), (ylo, yhi) = ptc_range
    check(lib.modest_plane_candidates(c.handle, pts.data_ptr(), n, pts.shape[1], float(max_hs), float(xlo),
                                      float(xhi), float(ylo), float(yhi), cand.data_ptr(), idx.data_ptr(),
                                      cnt.data_ptr(), _stream()), "modest_plane_candidates")
    torch.cuda.current_stream().synchronize()
    m = int(cnt[0])
    return cand[:m], idx[:m]


def plane_prepare(pts: torch.Tensor, specs, ctx: Optional[Context] = None):
    """Candidates and MAD thresholds of two estimate_plane calls on one scan ((max_hs, ptc_range) each):
    one pass over the rows, one stream sync.  Returns [(cand (m,3) f32 device, thr np.float32 | None)] x 2."""
    lib = load()
    _dev(pts, torch.float32, "pts")
    assert len(specs) == 2
    n = pts.shape[0]
    flat = []
    for max_hs, ((xlo, xhi), (ylo, yhi)) in specs:
        flat += [max_hs, xlo, xhi, ylo, yhi]
    spec = np.ascontiguousarray(flat, dtype=np.float32)
    cands = [torch.empty((n, 3), dtype=torch.float32, device=pts.device) for _ in range(2)]
    cnt, mad = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.float32)
    c = _ctx(ctx, pts)
    check(lib.modest_plane_prepare(c.handle, pts.data_ptr(), n, pts.shape[1], _np_ptr(spec), cands[0].data_ptr(),
                                   cands[1].data_ptr(), _np_ptr(cnt), _np_ptr(mad), _stream()), "modest_plane_prepare")
    return [(cands[k][: int(cnt[k])], np.float32(mad[k]) if cnt[k] >= 1 else None) for k in range(2)]


def mad_threshold(cand: torch.Tensor, ctx: Optional[Context] = None) -> np.float32:
    lib = load()
    _dev(cand, torch.float32, "cand")
    out = C.c_float(0)
    c = _ctx(ctx, cand)
    check(lib.modest_mad_threshold(c.handle, cand.data_ptr(), cand.shape[0], C.byref(out), _stream()),
          "modest_mad_threshold")
    return np.float32(out.value)


def mad_threshold_batch(cands: Sequence[torch.Tensor], ctx: Optional[Context] = None) -> np.ndarray:
    """MAD thresholds of several candidate sets from one call (one workgroup per set, up to 16 sets per launch)."""
    lib = load()
    for t in cands:
        _dev(t, torch.float32, "cand")
    k = len(cands)
    ptrs = (C.c_void_p * k)(*[t.data_ptr() for t in cands])
    ns = np.ascontiguousarray([t.shape[0] for t in cands], dtype=np.int32)
    out = np.zeros(k, dtype=np.float32)
    c = _ctx(ctx, cands[0])
    check(lib.modest_mad_threshold_batch(c.handle, ptrs, _np_ptr(ns), k, _np_ptr(out), _stream()),
          "modest_mad_threshold_batch")
    return out


def ransac_score_trials(cand: torch.Tensor, models: np.ndarray, thr: float, ctx: Optional[Context] = None):
    """Inlier counts (+ SSE / sum z / sum z^2 over the inliers, float64) of K trial planes."""
    lib = load()
    _dev(cand, torch.float32, "cand")
    models = np.ascontiguousarray(models, dtype=np.float32).reshape(-1, 3)
    K = models.shape[0]
    n_in = np.zeros(K, dtype=np.int32)
    sse, sy, syy = (np.zeros(K, dtype=np.float64) for _ in range(3))
    c = _ctx(ctx, cand)
    check(lib.modest_ransac_score_trials(c.handle, cand.data_ptr(), cand.shape[0], _np_ptr(models), K,
                                         float(np.float32(thr)), _np_ptr(n_in), _np_ptr(sse), _np_ptr(sy),
                                         _np_ptr(syy), _stream()), "modest_ransac_score_trials")
    return n_in, sse, sy, syy


def ransac_trials(cand: torch.Tensor, triplets: np.ndarray, thr: Optional[float] = None,
                  ctx: Optional[Context] = None):
    """MAD threshold (when thr is None) + exact-fit planes of the triplets + their scores, one
    device round trip.  Returns (thr, models (K,3) f32, n_inliers, sse, sy, syy)."""
    lib = load()
    _dev(cand, torch.float32, "cand")
    trip = np.ascontiguousarray(triplets, dtype=np.int32).reshape(-1, 3)
    K = trip.shape[0]
    thr_io = C.c_float(-1.0 if thr is None else float(np.float32(thr)))
    models = np.zeros((K, 3), dtype=np.float32)
    n_in = np.zeros(K, dtype=np.int32)
    sse, sy, syy = (np.zeros(K, dtype=np.float64) for _ in range(3))
    c = _ctx(ctx, cand)
    check(lib.modest_ransac_trials(c.handle, cand.data_ptr(), cand.shape[0], _np_ptr(trip), K, C.byref(thr_io),
                                   _np_ptr(models), _np_ptr(n_in), _np_ptr(sse), _np_ptr(sy), _np_ptr(syy),
                                   _stream()), "modest_ransac_trials")
    return np.float32(thr_io.value), models, n_in, sse, sy, syy


def ransac_plane_native(cand: torch.Tensor, rs: np.random.RandomState, thr: float, max_trials: int = 100,
                        stop_probability: float = 0.99, batch: int = 48, ctx: Optional[Context] = None):
    """The whole RANSAC fit behind one library call (include/modest_hip.h: modest_ransac_plane): `rs`
    (legacy MT19937 RandomState) is advanced in place by the executed trials.
    Returns (status, model64 (3,), best_model (3,) f32, triplets (n_trials,3), n_trials, n_inliers)."""
    lib = load()
    _dev(cand, torch.float32, "cand")
    st = rs.get_state()
    assert st[0] == "MT19937"
    key = np.ascontiguousarray(st[1], dtype=np.uint32).copy()
    pos = C.c_int32(int(st[2]))
    model64, best = np.zeros(3, dtype=np.float64), np.zeros(3, dtype=np.float32)
    trip = np.zeros((max_trials, 3), dtype=np.int32)
    n_trials, n_in, status = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    c = _ctx(ctx, cand)
    check(lib.modest_ransac_plane(c.handle, cand.data_ptr(), cand.shape[0], float(np.float32(thr)), _np_ptr(key),
                                  C.byref(pos), int(max_trials), float(stop_probability), int(batch), _np_ptr(model64),
                                  _np_ptr(best), _np_ptr(trip), C.byref(n_trials), C.byref(n_in), C.byref(status),
                                  _stream()), "modest_ransac_plane")
    rs.set_state((st[0], key, int(pos.value), st[3], st[4]))
    return int(status.value), model64, best, trip[: n_trials.value].astype(np.int64), int(n_trials.value), int(n_in.value)


def mt19937_triplets(rs: np.random.RandomState, n_population: int, n_trials: int) -> np.ndarray:
    """n_trials draws of sklearn's sample_without_replacement(n_population > 300, 3) from `rs`, made by
    the library's generator (host only); `rs` is advanced in place."""
    lib = load()
    st = rs.get_state()
    key = np.ascontiguousarray(st[1], dtype=np.uint32).copy()
    pos = C.c_int32(int(st[2]))
    out = np.zeros((n_trials, 3), dtype=np.int32)
    check(lib.modest_mt19937_triplets(_np_ptr(key), C.byref(pos), int(n_population), int(n_trials), _np_ptr(out)),
          "modest_mt19937_triplets")
    rs.set_state((st[0], key, int(pos.value), st[3], st[4]))
    return out


def ransac_refit(cand: torch.Tensor, model: np.ndarray, thr: float, ctx: Optional[Context] = None):
    lib = load()
    _dev(cand, torch.float32, "cand")
    model = np.ascontiguousarray(model, dtype=np.float32).reshape(3)
    out = np.zeros(3, dtype=np.float64)
    n_in = C.c_int32(0)
    c = _ctx(ctx, cand)
    check(lib.modest_ransac_refit(c.handle, cand.data_ptr(), cand.shape[0], _np_ptr(model),
                                  float(np.float32(thr)), _np_ptr(out), C.byref(n_in), _stream()),
          "modest_ransac_refit")
    return out, int(n_in.value)


def plane_range_mask(pts: torch.Tensor, plane: np.ndarray, offset: float, only_range, limit_range,
                     ctx: Optional[Context] = None):
    """above_plane (pointcloud_utils.py:68-74) AND the limit_range mask (generate_mask.py:61-65).
    Returns (mask (n,) bool device, kept_xyz (m,3) f32, kept_idx (m,) i32)."""
    lib = load()
    _dev(pts, torch.float32, "pts")
    n = pts.shape[0]
    plane = np.ascontiguousarray(plane, dtype=np.float64).reshape(4)
    lim = np.ascontiguousarray(np.asarray(limit_range, dtype=np.float64).reshape(4))
    onl = None if only_range is None else np.ascontiguousarray(np.asarray(only_range, dtype=np.float64).reshape(4))
    mask = torch.empty((n,), dtype=torch.uint8, device=pts.device)
    kept = torch.empty((n, 3), dtype=torch.float32, device=pts.device)
    idx = torch.empty((n,), dtype=torch.int32, device=pts.device)
    c = _ctx(ctx, pts)
    cnt = c.host_counter()   # pinned host word, always written by the call
    check(lib.modest_plane_range_mask(c.handle, pts.data_ptr(), n, pts.shape[1], _np_ptr(plane), float(offset),
                                      None if onl is None else _np_ptr(onl), _np_ptr(lim), mask.data_ptr(),
                                      kept.data_ptr(), idx.data_ptr(), cnt.data_ptr(), _stream()),
          "modest_plane_range_mask")
    torch.cuda.current_stream().synchronize()
    m = int(cnt[0])
    return mask.view(torch.bool), kept[:m], idx[:m]   # 0/1 bytes reinterpreted, no kernel


# --------------------------------------------------------------------------- clustering
GRAPH_TYPES = {"radius_mutual_knn": 0, "radius": 1, "knn": 2, "sym_knn": 3, "mutual_knn": 4}
AFFINITY_TYPES = {"l1": 0, "exp": 1, "3d_l2_distance": 2}


def cluster_dbscan(xyz: torch.Tensor, pp: torch.Tensor, n_neighbors: int = 70, radius: float = 2.0,
                   eps: float = 0.1, min_samples: int = 10, return_kth: bool = False,
                   ctx: Optional[Context] = None, neighbor_type: str = "radius_mutual_knn",
                   affinity_type: str = "l1", intensity: Optional[torch.Tensor] = None):
    """Affinity graph (precompute_affinity_matrix, clustering_utils.py:7-60) + DBSCAN(precomputed)
    labels, (n,) int32 on device.  neighbor_type radius_mutual_knn | radius; affinity_type l1 | exp |
    3d_l2_distance (the latter needs the scan's intensity column, see include/modest_hip.h)."""
    lib = load()
    _dev(xyz, torch.float32, "xyz")
    _dev(pp, torch.float32, "pp")
    if neighbor_type not in GRAPH_TYPES:
        raise NotImplementedError(neighbor_type)
    if affinity_type not in AFFINITY_TYPES:
        raise NotImplementedError(affinity_type)
    n = xyz.shape[0]
    assert pp.shape[0] == n
    if affinity_type == "3d_l2_distance":
        if intensity is None:
            raise ValueError("3d_l2_distance needs the intensity column of the scan rows")
        _dev(intensity, torch.float32, "intensity")
        assert intensity.shape[0] == n
    labels = torch.empty((n,), dtype=torch.int32, device=xyz.device)
    kth = torch.empty((n,), dtype=torch.float64, device=xyz.device) if return_kth else None
    ncl = C.c_int32(0)
    c = _ctx(ctx, xyz)
    check(lib.modest_cluster_dbscan_ex(c.handle, xyz.data_ptr(), pp.data_ptr(),
                                       intensity.data_ptr() if intensity is not None else None, n,
                                       GRAPH_TYPES[neighbor_type], AFFINITY_TYPES[affinity_type], int(n_neighbors),
                                       float(radius), float(eps), int(min_samples), labels.data_ptr(),
                                       kth.data_ptr() if kth is not None else None, C.byref(ncl), _stream()),
          "modest_cluster_dbscan_ex")
    return (labels, int(ncl.value), kth) if return_kth else (labels, int(ncl.value))


def mask_cluster(pts: torch.Tensor, pp: torch.Tensor, plane: np.ndarray, offset: float, only_range, limit_range,
                 n_neighbors: int = 70, radius: float = 2.0, eps: float = 0.1, min_samples: int = 10,
                 neighbor_type: str = "radius_mutual_knn", affinity_type: str = "l1",
                 ctx: Optional[Context] = None):
    """plane_range_mask + cluster_dbscan + ``labels[ptc_mask] = ...`` (generate_mask.py:57-88) in one
    call.  Returns (labels (n,) int32 device, -1 = masked out or noise; number of kept rows)."""
    lib = load()
    _dev(pts, torch.float32, "pts")
    _dev(pp, torch.float32, "pp")
    if neighbor_type not in GRAPH_TYPES:
        raise NotImplementedError(neighbor_type)
    if affinity_type not in AFFINITY_TYPES:
        raise NotImplementedError(affinity_type)
    n = pts.shape[0]
    assert pp.shape[0] == n
    plane = np.ascontiguousarray(plane, dtype=np.float64).reshape(4)
    lim = np.ascontiguousarray(np.asarray(limit_range, dtype=np.float64).reshape(4))
    onl = None if only_range is None else np.ascontiguousarray(np.asarray(only_range, dtype=np.float64).reshape(4))
    labels = torch.empty((n,), dtype=torch.int32, device=pts.device)
    n_kept, ncl = C.c_int32(0), C.c_int32(0)
    c = _ctx(ctx, pts)
    rc = lib.modest_mask_cluster(c.handle, pts.data_ptr(), n, pts.shape[1], pp.data_ptr(), _np_ptr(plane), float(offset),
                                 None if onl is None else _np_ptr(onl), _np_ptr(lim), GRAPH_TYPES[neighbor_type],
                                 AFFINITY_TYPES[affinity_type], int(n_neighbors), float(radius), float(eps),
                                 int(min_samples), labels.data_ptr(), C.byref(n_kept), C.byref(ncl), _stream())
    if rc and neighbor_type != "radius" and 0 < n_kept.value <= n_neighbors:
        raise ValueError(f"Expected n_neighbors <= n_samples_fit, but n_neighbors = {n_neighbors + 1}, "
                         f"n_samples_fit = {n_kept.value}, n_samples = {n_kept.value}")
    check(rc, "modest_mask_cluster")
    return labels, int(n_kept.value)


class MaskParams(C.Structure):
    """modest_mask_params (include/modest_hip.h)"""
    _fields_ = [("max_hs1", C.c_float), ("range1", C.c_float * 4), ("max_hs2", C.c_float), ("range2", C.c_float * 4),
                ("offset", C.c_double), ("use_only_range", C.c_int32), ("only_range", C.c_double * 4),
                ("limit_range", C.c_double * 4), ("neighbor_type", C.c_int32), ("affinity_type", C.c_int32),
                ("k_neighbors", C.c_int32), ("min_samples", C.c_int32), ("radius", C.c_double), ("eps", C.c_double),
                ("min_points", C.c_int32), ("max_min_height", C.c_double), ("min_max_height", C.c_double),
                ("quantile", C.c_double), ("min_percentile_pp_score", C.c_float), ("max_trials", C.c_int32),
                ("batch", C.c_int32), ("stop_probability", C.c_double)]


STAGE_STATUS = {1: "small candidate set", 2: "no consensus set", 3: "degenerate consensus set", 4: "too few kept rows",
                5: "RANSAC trial bound on a rounding boundary (the host loop decides)"}


def mask_stage(pts: torch.Tensor, pp: torch.Tensor, params: MaskParams, rs: np.random.RandomState,
               ctx: Optional[Context] = None):
    """generate_mask_scan up to ``labels_filtered`` behind one library call (modest_mask_stage).
    Returns None when the library hands the scan back to the host statement (rare inputs: see
    STAGE_STATUS; ``rs`` is untouched then), else (labels_filtered (n,) int64, plane1, plane2, info):
    ``rs`` has been advanced by the executed RANSAC trials of both fits."""
    lib = load()
    _dev(pts, torch.float32, "pts")
    _dev(pp, torch.float32, "pp")
    n = pts.shape[0]
    assert pp.shape[0] == n and n >= 1
    st = rs.get_state()
    assert st[0] == "MT19937"
    key = np.ascontiguousarray(st[1], dtype=np.uint32).copy()
    pos = C.c_int32(int(st[2]))
    plane1, plane2 = np.zeros(4, dtype=np.float64), np.zeros(4, dtype=np.float64)
    labels = np.empty(n, dtype=np.int64)
    info = np.zeros(8, dtype=np.int32)
    c = _ctx(ctx, pts)
    check(lib.modest_mask_stage(c.handle, pts.data_ptr(), n, pts.shape[1], pp.data_ptr(), C.byref(params), _np_ptr(key),
                                C.byref(pos), _np_ptr(plane1), _np_ptr(plane2), _np_ptr(labels), _np_ptr(info),
                                _stream()), "modest_mask_stage")
    if info[3] != 0:
        return None
    rs.set_state((st[0], key, int(pos.value), st[3], st[4]))
    return labels, plane1, plane2, info


class MaskStageScan(C.Structure):
    """modest_mask_stage_scan (include/modest_hip.h)"""
    _fields_ = [("ctx", C.c_void_p), ("pts_dev", C.c_void_p), ("n", C.c_int32), ("stride", C.c_int32), ("pp_dev", C.c_void_p),
                ("mt_key624", C.c_void_p), ("mt_pos", C.c_void_p), ("plane1_out", C.c_void_p), ("plane2_out", C.c_void_p),
                ("labels_out", C.c_void_p), ("info_out", C.c_void_p), ("members_out", C.c_void_p), ("n_members_out", C.c_void_p)]


_CHAIN_CTXS = {}


def chain_contexts(n: int, device: int = 0):
    """`n` library contexts of the calling thread for the scans of a chain (every scan of a chain works in its own
    context: scratch, pinned words, persistent counters)"""
    import threading
    key = (threading.get_ident(), int(device))
    have = _CHAIN_CTXS.setdefault(key, [])
    while len(have) < n:
        have.append(Context(int(device)))
    return have[:n]


def mask_stage_batch(items, params: MaskParams, ctxs=None):
    """modest_mask_stage_batch: generate_mask_scan up to ``labels_filtered`` for a CHAIN of scans -- the ground fits per
    scan, the mask / graph / DBSCAN block and the cluster statistics as one launch per kernel for the whole chain.
    items: [(pts_dev (n,3|4) f32, pp_dev (n,) f32, RandomState)]; returns a list with, per scan, what mask_stage
    returns (None: the library hands that scan back to the host statement, its generator untouched)."""
    lib = load()
    B = len(items)
    if B == 0:
        return []
    if ctxs is None:
        ctxs = chain_contexts(B, items[0][0].device.index or 0)
    arr = (MaskStageScan * B)()
    keep = []
    for i, (pts, pp, rs) in enumerate(items):
        _dev(pts, torch.float32, "pts")
        _dev(pp, torch.float32, "pp")
        n = pts.shape[0]
        assert pp.shape[0] == n and n >= 1
        st = rs.get_state()
        assert st[0] == "MT19937"
        key = np.ascontiguousarray(st[1], dtype=np.uint32).copy()
        pos = np.array([int(st[2])], dtype=np.int32)
        plane1, plane2 = np.zeros(4, dtype=np.float64), np.zeros(4, dtype=np.float64)
        labels = np.empty(n, dtype=np.int64)
        info = np.zeros(8, dtype=np.int32)
        members, n_mem = np.empty(n, dtype=np.int32), np.full(1, -1, dtype=np.int32)
        keep.append((st, key, pos, plane1, plane2, labels, info, members, n_mem))
        a = arr[i]
        a.ctx = C.cast(ctxs[i].handle, C.c_void_p).value
        a.pts_dev, a.n, a.stride, a.pp_dev = pts.data_ptr(), n, pts.shape[1], pp.data_ptr()
        a.mt_key624, a.mt_pos = _np_ptr(key), _np_ptr(pos)
        a.plane1_out, a.plane2_out, a.labels_out, a.info_out = _np_ptr(plane1), _np_ptr(plane2), _np_ptr(labels), _np_ptr(info)
        a.members_out, a.n_members_out = _np_ptr(members), _np_ptr(n_mem)
    check(lib.modest_mask_stage_batch(C.byref(arr), B, C.byref(params), _stream()), "modest_mask_stage_batch")
    out = []
    for (pts, pp, rs), (st, key, pos, plane1, plane2, labels, info, members, n_mem) in zip(items, keep):
        if info[3] != 0:
            out.append(None)
            continue
        rs.set_state((st[0], key, int(pos[0]), st[3], st[4]))
        # (a fifth entry: the indices of the points with a label > 0, ascending -- None when the library did not list them)
        out.append((labels, plane1, plane2, info, members[:int(n_mem[0])] if n_mem[0] >= 0 else None))
    return out


class BoxesParams(C.Structure):
    """modest_boxes_params (include/modest_hip.h)"""
    _fields_ = [("V2C", C.c_double * 12), ("R0", C.c_double * 9), ("angles", C.c_void_p), ("cossin", C.c_void_p),
                ("cossin90", C.c_void_p), ("n_angles", C.c_int32), ("d0", C.c_double), ("min_volume", C.c_double),
                ("max_volume", C.c_double)]


class LabelsParams(C.Structure):
    """modest_labels_params (include/modest_hip.h)"""
    _fields_ = [("P", C.c_double * 12), ("nms_enable", C.c_int32), ("nms_threshold", C.c_float), ("fov_only", C.c_int32),
                ("image_h", C.c_double), ("image_w", C.c_double)]


def scan_boxes(pts_dev: torch.Tensor, pts_host: np.ndarray, labels_filtered: np.ndarray, n_lab: int, V2C, R0,
               angles: np.ndarray, cossin: np.ndarray, cossin90: np.ndarray, d0: float, min_volume: float,
               max_volume: float, ctx: Optional[Context] = None):
    """The box tail of generate_mask.py:88-103 behind one library call (modest_scan_boxes): members, rect
    points, closeness fit, get_obj, volume gate, relabelling.  Returns None when the library hands the scan
    back to the host statement, else (final labels (n,) int64, objs (n_lab,8) float64 rows
    {t0, t1, t2, l, w, h, ry, volume}, keep (n_lab,) bool)."""
    lib = load()
    _dev(pts_dev, torch.float32, "pts")
    assert pts_host.dtype == np.float32 and pts_host.flags.c_contiguous and pts_host.shape == tuple(pts_dev.shape)
    n = pts_host.shape[0]
    P = BoxesParams()
    P.V2C[:] = [float(x) for x in np.asarray(V2C, dtype=np.float64).reshape(12)]
    P.R0[:] = [float(x) for x in np.asarray(R0, dtype=np.float64).reshape(9)]
    assert angles.dtype == np.float64 and cossin.dtype == np.float64 and cossin90.dtype == np.float64
    assert cossin.flags.c_contiguous and cossin90.flags.c_contiguous and angles.flags.c_contiguous
    P.angles, P.cossin, P.cossin90, P.n_angles = _np_ptr(angles), _np_ptr(cossin), _np_ptr(cossin90), angles.shape[0]
    P.d0, P.min_volume, P.max_volume = float(d0), float(min_volume), float(max_volume)
    labels = np.ascontiguousarray(labels_filtered, dtype=np.int64).copy()
    objs = np.zeros((max(n_lab, 1), 8), dtype=np.float64)
    keep = np.zeros(max(n_lab, 1), dtype=np.int32)
    info = np.zeros(2, dtype=np.int32)
    c = _ctx(ctx, pts_dev)
    check(lib.modest_scan_boxes(c.handle, pts_dev.data_ptr(), _np_ptr(pts_host), n, pts_host.shape[1], _np_ptr(labels),
                                int(n_lab), C.byref(P), _np_ptr(objs), _np_ptr(keep), _np_ptr(info), _stream()),
          "modest_scan_boxes")
    if info[1] != 0:
        return None
    return labels, objs[:n_lab], keep[:n_lab].astype(bool)


class BoxesScan(C.Structure):
    """modest_boxes_scan (include/modest_hip.h)"""
    _fields_ = [("ctx", C.c_void_p), ("pts_dev", C.c_void_p), ("pts_host", C.c_void_p), ("n", C.c_int32), ("stride", C.c_int32),
                ("labels_inout", C.c_void_p), ("n_lab", C.c_int32), ("objs_out", C.c_void_p), ("keep_out", C.c_void_p),
                ("info_out", C.c_void_p), ("members", C.c_void_p), ("n_members", C.c_int32)]


def scan_boxes_batch(items, V2C, R0, angles: np.ndarray, cossin: np.ndarray, cossin90: np.ndarray, d0: float,
                     min_volume: float, max_volume: float, ctxs=None):
    """modest_scan_boxes_batch: the box tail of a CHAIN of scans (one calibration) -- host phases per scan, one
    closeness launch over all clusters, one lowest-point launch over all boxes.  items: [(pts_dev, pts_host,
    labels_filtered, n_lab[, members])] -- members: the ascending indices of the points with a label > 0 as mask_stage_batch
    lists them (the host passes then touch those only); returns per scan what scan_boxes returns (None: host statement)."""
    lib = load()
    B = len(items)
    if B == 0:
        return []
    if ctxs is None:
        ctxs = chain_contexts(B, items[0][0].device.index or 0)
    P = BoxesParams()
    P.V2C[:] = [float(x) for x in np.asarray(V2C, dtype=np.float64).reshape(12)]
    P.R0[:] = [float(x) for x in np.asarray(R0, dtype=np.float64).reshape(9)]
    assert angles.dtype == np.float64 and cossin.dtype == np.float64 and cossin90.dtype == np.float64
    assert cossin.flags.c_contiguous and cossin90.flags.c_contiguous and angles.flags.c_contiguous
    P.angles, P.cossin, P.cossin90, P.n_angles = _np_ptr(angles), _np_ptr(cossin), _np_ptr(cossin90), angles.shape[0]
    P.d0, P.min_volume, P.max_volume = float(d0), float(min_volume), float(max_volume)
    arr = (BoxesScan * B)()
    keepalive = []
    for i, item in enumerate(items):
        pts_dev, pts_host, labels_filtered, n_lab = item[:4]
        members = item[4] if len(item) > 4 else None
        _dev(pts_dev, torch.float32, "pts")
        assert pts_host.dtype == np.float32 and pts_host.flags.c_contiguous and pts_host.shape == tuple(pts_dev.shape)
        labels = np.ascontiguousarray(labels_filtered, dtype=np.int64).copy()
        objs = np.zeros((max(n_lab, 1), 8), dtype=np.float64)
        keep = np.zeros(max(n_lab, 1), dtype=np.int32)
        info = np.zeros(2, dtype=np.int32)
        if members is not None:
            members = np.ascontiguousarray(members, dtype=np.int32)
        keepalive.append((labels, objs, keep, info, int(n_lab), members))
        a = arr[i]
        a.ctx = C.cast(ctxs[i].handle, C.c_void_p).value
        a.pts_dev, a.pts_host, a.n, a.stride = pts_dev.data_ptr(), _np_ptr(pts_host), pts_host.shape[0], pts_host.shape[1]
        a.labels_inout, a.n_lab = _np_ptr(labels), int(n_lab)
        a.objs_out, a.keep_out, a.info_out = _np_ptr(objs), _np_ptr(keep), _np_ptr(info)
        a.members, a.n_members = (_np_ptr(members), int(members.shape[0])) if members is not None else (None, 0)
    check(lib.modest_scan_boxes_batch(C.byref(arr), B, C.byref(P), _stream()), "modest_scan_boxes_batch")
    return [None if info[1] != 0 else (labels, objs[:n_lab], keep[:n_lab].astype(bool))
            for labels, objs, keep, info, n_lab, _m in keepalive]


class SeedScan(C.Structure):
    """modest_seed_scan (include/modest_hip.h)"""
    _fields_ = [("ctx", C.c_void_p), ("pts_dev", C.c_void_p), ("pts_host", C.c_void_p), ("n", C.c_int32), ("stride", C.c_int32),
                ("pp_dev", C.c_void_p), ("mt_key624", C.c_void_p), ("mt_pos", C.c_void_p), ("plane1_out", C.c_void_p),
                ("plane2_out", C.c_void_p), ("labels_out", C.c_void_p), ("members_scratch", C.c_void_p), ("objs_out", C.c_void_p),
                ("iou_out", C.c_void_p), ("info_out", C.c_void_p)]


def _boxes_params(V2C, R0, angles, cossin, cossin90, d0, min_volume, max_volume) -> BoxesParams:
    P = BoxesParams()
    P.V2C[:] = [float(x) for x in np.asarray(V2C, dtype=np.float64).reshape(12)]
    P.R0[:] = [float(x) for x in np.asarray(R0, dtype=np.float64).reshape(9)]
    assert angles.dtype == np.float64 and cossin.dtype == np.float64 and cossin90.dtype == np.float64
    assert cossin.flags.c_contiguous and cossin90.flags.c_contiguous and angles.flags.c_contiguous
    P.angles, P.cossin, P.cossin90, P.n_angles = _np_ptr(angles), _np_ptr(cossin), _np_ptr(cossin90), angles.shape[0]
    P.d0, P.min_volume, P.max_volume = float(d0), float(min_volume), float(max_volume)
    return P


SEED_MAX_BOXES = 96   # clusters per scan the one-call chain has room for (a Lyft-shape scan has 10-40; more: the scan takes the separate calls)


def seed_chain(items, mparams: MaskParams, V2C, R0, angles: np.ndarray, cossin: np.ndarray, cossin90: np.ndarray, d0: float,
               min_volume: float, max_volume: float, nms_enable: bool, ctxs=None):
    """modest_seed_chain: stages 2 + 3 of a CHAIN of scans (one calibration) behind ONE library call -- mask stage, box tail and the
    IoU matrices of the kept boxes.  items: [(pts_dev (n,3|4) f32, pts_host (same, numpy), pp_dev (n,) f32, RandomState)].
    Returns per scan (status, labels (n,) int64, rows (k,8) f64, iou (k,k) f32 | None, plane1, info): status 0 = all of it is final;
    1 = the mask stage handed the scan back (its generator is untouched: run the host statement); 2 / 3 = labels are
    `labels_filtered` and the generator is advanced, the box tail is the caller's (scan_boxes / host statement)."""
    lib = load()
    B = len(items)
    if B == 0:
        return []
    if ctxs is None:
        ctxs = chain_contexts(B, items[0][0].device.index or 0)
    P = _boxes_params(V2C, R0, angles, cossin, cossin90, d0, min_volume, max_volume)
    K = SEED_MAX_BOXES
    ns = [int(it[0].shape[0]) for it in items]
    offs = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    labels_all = np.empty(int(offs[-1]), dtype=np.int64)       # one allocation per kind for the whole chain
    members_all = np.empty(int(offs[-1]), dtype=np.int32)
    keys_all = np.empty((B, 624), dtype=np.uint32)
    pos_all = np.zeros(B, dtype=np.int32)
    planes_all = np.zeros((B, 2, 4), dtype=np.float64)
    rows_all = np.zeros((B, K, 8), dtype=np.float64)
    iou_all = np.zeros((B, K * K), dtype=np.float32) if nms_enable else None
    info_all = np.zeros((B, 12), dtype=np.int32)
    arr = (SeedScan * B)()
    states = []
    for i, (pts, pts_host, pp, rs) in enumerate(items):
        _dev(pts, torch.float32, "pts")
        _dev(pp, torch.float32, "pp")
        n = ns[i]
        assert pp.shape[0] == n and n >= 1 and pts_host.dtype == np.float32 and pts_host.flags.c_contiguous and pts_host.shape == tuple(pts.shape)
        st = rs.get_state()
        assert st[0] == "MT19937"
        keys_all[i] = st[1]
        pos_all[i] = int(st[2])
        states.append(st)
        a = arr[i]
        a.ctx = C.cast(ctxs[i].handle, C.c_void_p).value
        a.pts_dev, a.pts_host, a.n, a.stride, a.pp_dev = pts.data_ptr(), _np_ptr(pts_host), n, pts.shape[1], pp.data_ptr()
        a.mt_key624, a.mt_pos = keys_all[i].ctypes.data, pos_all[i:].ctypes.data
        a.plane1_out, a.plane2_out = planes_all[i, 0].ctypes.data, planes_all[i, 1].ctypes.data
        a.labels_out, a.members_scratch = labels_all[offs[i]:].ctypes.data, members_all[offs[i]:].ctypes.data
        a.objs_out = rows_all[i].ctypes.data
        a.iou_out = iou_all[i].ctypes.data if nms_enable else None
        a.info_out = info_all[i].ctypes.data
    check(lib.modest_seed_chain(C.byref(arr), B, C.byref(mparams), C.byref(P), K, int(bool(nms_enable)), _stream()), "modest_seed_chain")
    out = []
    for i, (pts, pts_host, pp, rs) in enumerate(items):
        info = info_all[i]
        status = int(info[10])
        if status != 1:
            st = states[i]
            rs.set_state((st[0], keys_all[i], int(pos_all[i]), st[3], st[4]))
        k = int(info[9])
        out.append((status, labels_all[offs[i]:offs[i + 1]], rows_all[i, :k], (iou_all[i, :k * k].reshape(k, k) if nms_enable else None),
                    planes_all[i, 0], info))
    return out


def objs_iou(objs8: np.ndarray, ctx: Optional[Context] = None) -> np.ndarray:
    """BEV IoU matrix (k,k) float32 of objs_nms' float32 boxes (modest_objs_iou)."""
    lib = load()
    objs8 = np.ascontiguousarray(objs8, dtype=np.float64).reshape(-1, 8)
    k = objs8.shape[0]
    out = np.zeros((k, k), dtype=np.float32)
    if k:
        c = ctx if ctx is not None else default_context(torch.cuda.current_device())
        check(lib.modest_objs_iou(c.handle, _np_ptr(objs8), k, _np_ptr(out), _stream()), "modest_objs_iou")
    return out


def objs_iou_batch(objs_list, ctx: Optional[Context] = None):
    """objs_iou of the box sets of a chain of scans: one launch, one round trip (modest_objs_iou_batch)."""
    lib = load()
    B = len(objs_list)
    rows = [np.ascontiguousarray(o, dtype=np.float64).reshape(-1, 8) for o in objs_list]
    outs = [np.zeros((r.shape[0], r.shape[0]), dtype=np.float32) for r in rows]
    if B == 0 or not any(r.shape[0] for r in rows):
        return outs
    k = np.array([r.shape[0] for r in rows], dtype=np.int32)
    ip = np.array([r.ctypes.data if r.shape[0] else 0 for r in rows], dtype=np.uint64)
    op = np.array([o.ctypes.data if o.size else 0 for o in outs], dtype=np.uint64)
    c = ctx if ctx is not None else default_context(torch.cuda.current_device())
    check(lib.modest_objs_iou_batch(c.handle, ip.ctypes.data, k.ctypes.data, B, op.ctypes.data, _stream()), "modest_objs_iou_batch")
    return outs


def label_lines(objs8: np.ndarray, order: Optional[np.ndarray], iou: Optional[np.ndarray], P34, nms_enable: bool,
                nms_threshold: float, fov_only: bool, image_shape) -> tuple:
    """objs_nms' greedy walk in `order`, is_within_fov, objs2label (modest_label_lines): (text, kept indices)."""
    lib = load()
    objs8 = np.ascontiguousarray(objs8, dtype=np.float64).reshape(-1, 8)
    k = objs8.shape[0]
    if k == 0:
        return "", np.zeros(0, dtype=np.int32)
    cs = np.ascontiguousarray(np.stack([np.cos(objs8[:, 6]), np.sin(objs8[:, 6])], axis=1))   # numpy's roty values
    Q = LabelsParams()
    Q.P[:] = [float(x) for x in np.asarray(P34, dtype=np.float64).reshape(12)]
    Q.nms_enable, Q.nms_threshold, Q.fov_only = int(bool(nms_enable)), float(nms_threshold), int(bool(fov_only))
    Q.image_h, Q.image_w = float(image_shape[0]), float(image_shape[1])
    if nms_enable:
        order = np.ascontiguousarray(order, dtype=np.int64)
        iou = np.ascontiguousarray(iou, dtype=np.float32)
        assert order.shape == (k,) and iou.shape == (k, k)
    kept = np.zeros(k, dtype=np.int32)
    nk, tl = C.c_int32(0), C.c_int32(0)
    cap = 256 * k + 16
    for _ in range(2):   # 256 bytes per line hold every sane box; a corner next to the image plane prints longer numbers
        buf = C.create_string_buffer(cap)
        rc = lib.modest_label_lines(_np_ptr(objs8), _np_ptr(cs), k, _np_ptr(order) if nms_enable else None,
                                    _np_ptr(iou) if nms_enable else None, C.byref(Q), _np_ptr(kept), C.byref(nk), buf, cap,
                                    C.byref(tl))
        if rc != -3 or cap >= 4096 * k + 16:   # MODEST_ERR_CAPACITY: once more with the library's own line bound
            break
        cap = 4096 * k + 16
    check(rc, "modest_label_lines")
    return buf.raw[: tl.value].decode("ascii"), kept[: nk.value]


def cluster_stats(pts: torch.Tensor, pp: torch.Tensor, labels: torch.Tensor, n_clusters: int,
                  plane: np.ndarray, quantile: float, ctx: Optional[Context] = None) -> np.ndarray:
    """Per-cluster (count, min dist, max dist, a, b, gamma) for is_valid_cluster; (C,6) float64 host."""
    lib = load()
    _dev(pts, torch.float32, "pts")
    _dev(pp, torch.float32, "pp")
    _dev(labels, torch.int32, "labels")
    out = np.zeros((n_clusters, 6), dtype=np.float64)
    if n_clusters == 0:
        return out
    plane = np.ascontiguousarray(plane, dtype=np.float64).reshape(4)
    c = _ctx(ctx, pts)
    check(lib.modest_cluster_stats(c.handle, pts.data_ptr(), pts.shape[0], pts.shape[1], pp.data_ptr(),
                                   labels.data_ptr(), int(n_clusters), _np_ptr(plane), float(quantile),
                                   _np_ptr(out), _stream()), "modest_cluster_stats")
    return out


def boxes_pp_stats(rect_xyz: torch.Tensor, pp: torch.Tensor, boxes12: np.ndarray, quantile: float,
                   ctx: Optional[Context] = None) -> np.ndarray:
    """filter_by_ppscore statistics (combine_labels.py:41-60): per box (points inside, a, b, gamma);
    (K,4) float64 host.  boxes12 = the twelve float64 scalars of include/modest_hip.h."""
    lib = load()
    _dev(rect_xyz, torch.float64, "rect_xyz")
    _dev(pp, torch.float32, "pp")
    assert rect_xyz.ndim == 2 and rect_xyz.shape[1] == 3 and pp.shape[0] == rect_xyz.shape[0]
    boxes12 = np.ascontiguousarray(boxes12, dtype=np.float64).reshape(-1, 12)
    out = np.zeros((boxes12.shape[0], 4), dtype=np.float64)
    if boxes12.shape[0] == 0:
        return out
    c = _ctx(ctx, rect_xyz)
    check(lib.modest_boxes_pp_stats(c.handle, rect_xyz.data_ptr(), rect_xyz.shape[0], pp.data_ptr(),
                                    _np_ptr(boxes12), boxes12.shape[0], float(quantile), _np_ptr(out),
                                    _stream()), "modest_boxes_pp_stats")
    return out


# --------------------------------------------------------------------------- box fitting
def fit_boxes_closeness(pts_xz: torch.Tensor, offsets: Sequence[int], cossin: np.ndarray, d0: float = 1e-2,
                        return_beta: bool = False, ctx: Optional[Context] = None):
    """Index of the first strict maximum of the closeness criterion per cluster."""
    lib = load()
    _dev(pts_xz, torch.float64, "pts_xz")
    off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int32))
    cs = np.ascontiguousarray(cossin, dtype=np.float64).reshape(-1, 2)
    ncl, na = off.shape[0] - 1, cs.shape[0]
    best = np.full(ncl, -1, dtype=np.int32)
    beta = np.zeros((ncl, na), dtype=np.float64) if return_beta else None
    c = _ctx(ctx, pts_xz)
    check(lib.modest_fit_boxes_closeness(c.handle, pts_xz.data_ptr(), _np_ptr(off), ncl, _np_ptr(cs), na,
                                         float(d0), _np_ptr(best), _np_ptr(beta) if return_beta else None,
                                         _stream()), "modest_fit_boxes_closeness")
    return (best, beta) if return_beta else best


def fit_boxes_closeness_host(pts_xz: np.ndarray, offsets: Sequence[int], cossin: np.ndarray, d0: float = 1e-2,
                             cossin90: Optional[np.ndarray] = None, ctx: Optional[Context] = None):
    """fit_boxes_closeness for cluster points in host memory ((m,2) float64): points and tables go to
    the device in one staged copy.  With ``cossin90`` ((cos, sin) of every table angle + pi/2) also returns
    the (C,8) extents of every cluster at the chosen heading and at heading + pi/2."""
    lib = load()
    pts = np.ascontiguousarray(pts_xz, dtype=np.float64).reshape(-1, 2)
    off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int32))
    assert off[-1] == pts.shape[0]
    cs = np.ascontiguousarray(cossin, dtype=np.float64).reshape(-1, 2)
    ncl, na = off.shape[0] - 1, cs.shape[0]
    best = np.full(ncl, -1, dtype=np.int32)
    ext = None
    if cossin90 is not None:
        cossin90 = np.ascontiguousarray(cossin90, dtype=np.float64).reshape(na, 2)
        ext = np.zeros((ncl, 8), dtype=np.float64)
    c = ctx if ctx is not None else default_context(torch.cuda.current_device())
    check(lib.modest_fit_boxes_closeness_host(c.handle, _np_ptr(pts), _np_ptr(off), ncl, _np_ptr(cs), na, float(d0),
                                              _np_ptr(best), None if ext is None else _np_ptr(cossin90),
                                              None if ext is None else _np_ptr(ext), _stream()),
          "modest_fit_boxes_closeness_host")
    return best if ext is None else (best, ext)


def fit_boxes_variance(pts_xz: torch.Tensor, offsets: Sequence[int], cossin: np.ndarray, return_crit: bool = False,
                       ctx: Optional[Context] = None):
    """Index of the first strict maximum of the variance_to_edge criterion per cluster."""
    lib = load()
    _dev(pts_xz, torch.float64, "pts_xz")
    off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int32))
    cs = np.ascontiguousarray(cossin, dtype=np.float64).reshape(-1, 2)
    ncl, na = off.shape[0] - 1, cs.shape[0]
    best = np.full(ncl, -1, dtype=np.int32)
    crit = np.zeros((ncl, na), dtype=np.float64) if return_crit else None
    c = _ctx(ctx, pts_xz)
    check(lib.modest_fit_boxes_variance(c.handle, pts_xz.data_ptr(), _np_ptr(off), ncl, _np_ptr(cs), na,
                                        _np_ptr(best), _np_ptr(crit) if return_crit else None, _stream()),
          "modest_fit_boxes_variance")
    return (best, crit) if return_crit else best


def fit_boxes_pca(pts_xz: torch.Tensor, offsets: Sequence[int], ctx: Optional[Context] = None) -> np.ndarray:
    """(K,8): PCA components (row-major 2x2) and the extent of every cluster along them."""
    lib = load()
    _dev(pts_xz, torch.float64, "pts_xz")
    off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int32))
    out = np.zeros((off.shape[0] - 1, 8), dtype=np.float64)
    c = _ctx(ctx, pts_xz)
    check(lib.modest_fit_boxes_pca(c.handle, pts_xz.data_ptr(), _np_ptr(off), off.shape[0] - 1, _np_ptr(out),
                                   _stream()), "modest_fit_boxes_pca")
    return out


def lowest_point(pts_rect: torch.Tensor, boxes6: np.ndarray, ctx: Optional[Context] = None) -> np.ndarray:
    lib = load()
    _dev(pts_rect, torch.float64, "pts_rect")
    b = np.ascontiguousarray(boxes6, dtype=np.float64).reshape(-1, 6)
    out = np.zeros(b.shape[0], dtype=np.float64)
    c = _ctx(ctx, pts_rect)
    check(lib.modest_lowest_point(c.handle, pts_rect.data_ptr(), pts_rect.shape[0], _np_ptr(b), b.shape[0],
                                  _np_ptr(out), _stream()), "modest_lowest_point")
    return out


# --------------------------------------------------------------------------- BEV IoU / NMS
def boxes_iou_bev(a: torch.Tensor, b: torch.Tensor, overlap_only: bool = False) -> torch.Tensor:
    lib = load()
    _dev(a, torch.float32, "boxes_a")
    _dev(b, torch.float32, "boxes_b")
    assert a.shape[1] == 7 and b.shape[1] == 7
    out = torch.zeros((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    fn = lib.modest_boxes_overlap_bev if overlap_only else lib.modest_boxes_iou_bev
    check(fn(a.data_ptr(), a.shape[0], b.data_ptr(), b.shape[0], out.data_ptr(), _stream()),
          "modest_boxes_iou_bev")
    return out


def boxes_iou_bev_host(a: np.ndarray, b: np.ndarray, ctx: Optional[Context] = None) -> np.ndarray:
    """Rotated BEV IoU of host box arrays (n,7) float32 -> (na, nb) float32 host matrix: boxes and matrix
    go through the context's pinned block, no device tensors and no copies."""
    lib = load()
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 7)
    b = np.ascontiguousarray(b, dtype=np.float32).reshape(-1, 7)
    out = np.zeros((a.shape[0], b.shape[0]), dtype=np.float32)
    c = ctx if ctx is not None else default_context(torch.cuda.current_device())
    check(lib.modest_boxes_iou_bev_host(c.handle, _np_ptr(a), a.shape[0], _np_ptr(b), b.shape[0], _np_ptr(out),
                                        _stream()), "modest_boxes_iou_bev_host")
    return out


def nms(boxes: torch.Tensor, thresh: float, rotated: bool = True, ctx: Optional[Context] = None) -> np.ndarray:
    """Greedy NMS over boxes already sorted by score; returns kept indices (int64, host)."""
    lib = load()
    _dev(boxes, torch.float32, "boxes")
    n = boxes.shape[0]
    keep = np.zeros(n, dtype=np.int64)
    num = C.c_int(0)
    c = _ctx(ctx, boxes)
    fn = lib.modest_nms_bev if rotated else lib.modest_nms_normal
    check(fn(c.handle, boxes.data_ptr(), n, float(thresh), _np_ptr(keep), C.byref(num), _stream()), "modest_nms")
    return keep[: num.value]


# --------------------------------------------------------------------------- ground planes (RANSAC.py)
# numpy images of modest_gp_frame / modest_gp_params / modest_gp_result (include/modest_hip.h)
GP_FRAME = np.dtype([("row_offset", "<i8"), ("n", "<i4"), ("pos", "<i4"), ("v2c", "<f8", (12,)), ("r0", "<f8", (9,)),
                     ("key", "<u4", (624,))])
GP_PARAMS = np.dtype([("min_h", "<f8"), ("max_h", "<f8"), ("stop_probability", "<f8"), ("max_trials", "<i4"),
                      ("chain", "<i4")])
GP_RESULT = np.dtype([("plane", "<f8", (4,)), ("median", "<f8"), ("mad", "<f8"), ("n_cand", "<i4"), ("n_trials", "<i4"),
                      ("n_inliers", "<i4"), ("status", "<i4")])
GP_FITTED, GP_DEFAULT, GP_HOST, GP_NO_CONSENSUS = 0, 1, 2, 3
assert GP_FRAME.itemsize == 2680 and GP_PARAMS.itemsize == 32 and GP_RESULT.itemsize == 64


def ground_planes(rows: torch.Tensor, frames: np.ndarray, min_h: float, max_h: float, chain: bool = False,
                  max_trials: int = 100, stop_probability: float = 0.99, return_triplets: bool = False,
                  ctx: Optional[Context] = None):
    """RANSAC.py's fit of a batch of frames (modest_ground_planes).  rows: packed (R,4) float32 device rows;
    frames: GP_FRAME array (row offset, n, calibration, generator), updated in place with the advanced generators.
    Returns (GP_RESULT array, GPU milliseconds of the batch, triplets (F, max_trials, 3) int32 or None).
    A GP_HOST row always holds n_cand, and median / mad above 300 candidates.  One handed back during its trials (a
    collinear triplet, a trial bound next to an integer) also holds n_trials and the triplet rows drawn so far; one
    handed back at the refit (a consensus set of fewer than three points, a collinear one, or one of one height) holds
    the n_trials, n_inliers and triplet rows of the finished trial loop.  Rows handed back by the candidate count, and
    the chained rows after a hand-back, hold n_trials = 0 and no triplets.  The plane of a GP_HOST row is not a fit."""
    lib = load()
    _dev(rows, torch.float32, "rows")
    assert rows.ndim == 2 and rows.shape[1] == 4
    assert frames.dtype == GP_FRAME and frames.flags.c_contiguous
    if len(frames):
        assert int((frames["row_offset"] + frames["n"]).max()) <= rows.shape[0]
    P = np.zeros((), dtype=GP_PARAMS)
    P["min_h"], P["max_h"], P["stop_probability"] = min_h, max_h, stop_probability
    P["max_trials"], P["chain"] = max_trials, int(bool(chain))
    res = np.zeros(len(frames), dtype=GP_RESULT)
    trip = np.full((len(frames), max_trials, 3), -1, dtype=np.int32) if return_triplets else None
    ms = C.c_float(0.0)
    c = _ctx(ctx, rows)
    check(lib.modest_ground_planes(c.handle, rows.data_ptr(), _np_ptr(frames), len(frames), _np_ptr(P), _np_ptr(res),
                                   _np_ptr(trip) if trip is not None else None, C.byref(ms), _stream()),
          "modest_ground_planes")
    return res, float(ms.value), trip


# --------------------------------------------------------------------------- KITTI-style AP evaluation (kitti_eval.hip)
def eval_overlaps(frames: torch.Tensor, n_frames: int, pair_base: int, n_pairs: int, dt_boxes: torch.Tensor,
                  gt_boxes: torch.Tensor, dt_bbox: torch.Tensor, gt_bbox: torch.Tensor, crit=(-1, -1, -1),
                  bev: Optional[torch.Tensor] = None, d3: Optional[torch.Tensor] = None,
                  img: Optional[torch.Tensor] = None) -> None:
    """modest_eval_overlaps: pairs [pair_base, pair_base + n_pairs) of a set of frames (EVAL_FRAME rows as bytes on the
    device) into float32 bev / 3-D and float64 image-box outputs (enqueue only, on PyTorch's current stream)."""
    lib = load()
    for t, dt, nm in ((dt_boxes, torch.float64, "dt_boxes"), (gt_boxes, torch.float64, "gt_boxes"),
                      (dt_bbox, torch.float64, "dt_bbox"), (gt_bbox, torch.float64, "gt_bbox")):
        _dev(t, dt, nm)
    for t, dt, nm in ((bev, torch.float32, "bev"), (d3, torch.float32, "d3"), (img, torch.float64, "img")):
        if t is not None:
            _dev(t, dt, nm)
            assert t.numel() >= n_pairs, f"{nm} holds fewer than n_pairs values"
    check(lib.modest_eval_overlaps(frames.data_ptr(), int(n_frames), int(pair_base), int(n_pairs), dt_boxes.data_ptr(),
                                   gt_boxes.data_ptr(), dt_bbox.data_ptr(), gt_bbox.data_ptr(), int(crit[0]),
                                   int(crit[1]), int(crit[2]), bev.data_ptr() if bev is not None else None,
                                   d3.data_ptr() if d3 is not None else None, img.data_ptr() if img is not None else None,
                                   _stream()), "modest_eval_overlaps")


def eval_statistics(stage: int, args, frame_begin: int = 0, frame_end: int = 0,
                    overlaps: Optional[torch.Tensor] = None, pair_base: int = 0,
                    sorted_scores: Optional[torch.Tensor] = None, pr: Optional[torch.Tensor] = None) -> None:
    """modest_eval_statistics: stage 0 pass A / 1 thresholds / 2 pass B / 3 sums (enqueue only).  args: the
    kitti_eval._StatsArgs of the run (device pointers)."""
    lib = load()
    f64 = 0
    if overlaps is not None:
        assert overlaps.is_cuda and overlaps.dtype in (torch.float32, torch.float64)
        f64 = int(overlaps.dtype == torch.float64)
    if sorted_scores is not None:
        _dev(sorted_scores, torch.float64, "sorted_scores")
    if pr is not None:
        _dev(pr, torch.float64, "pr")
    check(lib.modest_eval_statistics(int(stage), C.byref(args), int(frame_begin), int(frame_end),
                                     overlaps.data_ptr() if overlaps is not None else None, f64, int(pair_base),
                                     sorted_scores.data_ptr() if sorted_scores is not None else None,
                                     pr.data_ptr() if pr is not None else None, _stream()), "modest_eval_statistics")


# --------------------------------------------------------------------------- dataset infos + gt database (kitti_infos.hip)
# numpy images of modest_infos_frame / modest_infos_box (include/modest_hip.h)
INFOS_FRAME = np.dtype([("row_offset", "<i8"), ("cnt_offset", "<i8"), ("n", "<i4"), ("box_begin", "<i4"), ("box_count", "<i4"),
                        ("height", "<i4"), ("width", "<i4"), ("fov_only", "<i4"), ("pad", "<i4", (2,)),
                        ("m1", "<f4", (12,)), ("p2t", "<f4", (12,))])
INFOS_BOX = np.dtype([("b", "<f8", (7,)), ("cs", "<f8", (2,)), ("tau", "<f8"), ("bf", "<f4", (7,)), ("cosa", "<f4"),
                      ("sina", "<f4"), ("reject", "<f4"), ("pad", "<f4", (2,))])
INFOS_MAX_PASS = 256
assert INFOS_FRAME.itemsize == 144 and INFOS_BOX.itemsize == 128


def infos_chunk_rows() -> int:
    return int(load().modest_infos_chunk_rows())


class InfosBatch:
    """device state of one modest_infos_count call, kept for the read-back and for modest_infos_gather"""

    def read(self):
        """(hull_count, und_n, und_idx (n_boxes, und_cap), db_count) as numpy; synchronises"""
        r = self.results.cpu().numpy()
        nb, cap = self.n_boxes, self.und_cap
        self.db_count = np.ascontiguousarray(r[2 * nb:3 * nb])
        return r[:nb], r[nb:2 * nb], r[3 * nb:(3 + cap) * nb].reshape(nb, cap), self.db_count


def infos_count(rows: torch.Tensor, n_rows: int, frames: np.ndarray, boxes: np.ndarray, wcount_words: Optional[int] = None,
                pass_boxes: int = INFOS_MAX_PASS, und_cap: int = 32, want_fov: bool = False, dense_stride: int = 0) -> InfosBatch:
    """modest_infos_count on PyTorch's current stream (enqueue only).  rows: packed (R,4) float32 device rows; frames /
    boxes: INFOS_FRAME / INFOS_BOX host tables.  want_fov: also the FOV flag of every row (st.fov, uint8);
    dense_stride > 0: also the dense (n_boxes, dense_stride) int32 database mask (st.dense)."""
    lib = load()
    _dev(rows, torch.float32, "rows")
    assert rows.ndim == 2 and rows.shape[1] == 4 and 0 <= n_rows <= rows.shape[0]
    assert frames.dtype == INFOS_FRAME and frames.flags.c_contiguous and boxes.dtype == INFOS_BOX and boxes.flags.c_contiguous
    st = InfosBatch()
    nf, nb = len(frames), len(boxes)
    if wcount_words is None:
        ch = infos_chunk_rows()
        wcount_words = int(sum(-(-int(n) // ch) * int(c) for n, c in zip(frames["n"], frames["box_count"])))
    st.rows, st.n_rows, st.frames, st.n_boxes, st.und_cap, st.pass_boxes = rows, int(n_rows), frames, nb, int(und_cap), int(pass_boxes)
    st.wcount_words = int(wcount_words)
    dev = rows.device
    tb = int(lib.modest_infos_table_bytes(nf, nb))
    st.tables = torch.empty((tb + 256,), dtype=torch.uint8, device=dev)
    assert st.tables.data_ptr() % 256 == 0
    st.wcount = torch.empty((max(st.wcount_words, 1),), dtype=torch.int32, device=dev)
    st.results = torch.empty((max((3 + st.und_cap) * nb, 4),), dtype=torch.int32, device=dev)   # hull | und_n | db_count | und_idx
    st.fov = torch.empty((max(st.n_rows, 1),), dtype=torch.uint8, device=dev) if want_fov else None
    st.dense = torch.zeros((max(nb, 1), int(dense_stride)), dtype=torch.int32, device=dev) if dense_stride else None
    base = st.results.data_ptr()
    check(lib.modest_infos_count(rows.data_ptr(), st.n_rows, _np_ptr(frames), nf, _np_ptr(boxes) if nb else None, nb,
                                 st.pass_boxes, st.und_cap, st.tables.data_ptr(), tb, st.wcount.data_ptr(), st.wcount_words,
                                 base, base + 4 * nb, (base + 12 * nb) if st.und_cap else None, base + 8 * nb,
                                 st.fov.data_ptr() if want_fov else None, st.dense.data_ptr() if dense_stride else None,
                                 int(dense_stride), _stream()), "modest_infos_count")
    return st


def infos_gather(st: InfosBatch) -> np.ndarray:
    """modest_infos_gather after st.read(): the database rows of the batch, box after box, as a (total, 4) float32 numpy
    array (synchronises)."""
    lib = load()
    db_count = st.db_count
    base = np.concatenate([[0], np.cumsum(db_count, dtype=np.int64)]).astype(np.int64)
    total = int(base[-1])
    dev = st.rows.device
    out = torch.empty((max(total, 1), 4), dtype=torch.float32, device=dev)
    base_dev = torch.from_numpy(base[:-1].copy() if st.n_boxes else np.zeros(1, dtype=np.int64)).to(dev)
    check(lib.modest_infos_gather(st.rows.data_ptr(), st.n_rows, _np_ptr(st.frames), len(st.frames), st.n_boxes, st.pass_boxes,
                                  st.tables.data_ptr(), st.wcount.data_ptr(), st.wcount_words, base_dev.data_ptr(),
                                  _np_ptr(db_count) if st.n_boxes else _np_ptr(np.zeros(1, dtype=np.int32)),
                                  _np_ptr(base), out.data_ptr(), total, _stream()), "modest_infos_gather")
    return out[:total].cpu().numpy()


# --------------------------------------------------------------------------- point-to-voxel grouping
VOXELIZE_DEFAULT_BATCH_CAP = 256   # clouds a batch may hold when the caller does not say how many it has


def voxelize_workspace_bytes(n_rows: int, batch_size: int, grid_size) -> int:
    """scratch bytes of `voxelize` for n_rows stacked rows: does not depend on the grid (which is only checked)"""
    g = np.ascontiguousarray(grid_size, dtype=np.int32)
    assert g.shape == (3,)
    return _workspace_bytes("modest_voxelize_workspace_bytes", n_rows, batch_size, _np_ptr(g))


class VoxelizeGeometry:
    """float32 lower corner and voxel size, the int32 grid [nx, ny, nz], as the C ABI takes them"""

    def __init__(self, voxel_size, point_cloud_range):
        from .utils.spconv_utils import grid_size_f32
        self.lo, self.vs, self.grid_size = grid_size_f32(voxel_size, point_cloud_range)
        self.grid32 = np.ascontiguousarray(self.grid_size, dtype=np.int32)


class VoxelizePlan:
    """what `voxelize_plan` leaves for `voxelize_fill`: the arguments, the workspace and the counts read back"""


def voxelize_plan(points: torch.Tensor, voxel_size, point_cloud_range, max_num_points: int, max_voxels: int,
                  batch_size: Optional[int] = None, workspace: Optional[torch.Tensor] = None,
                  counts_pinned: Optional[torch.Tensor] = None, geometry: Optional[VoxelizeGeometry] = None) -> VoxelizePlan:
    """modest_voxelize_plan on PyTorch's current stream: everything up to the per-cloud voxel counts, ONE stream
    synchronise.  Arguments as `voxelize`.  -> plan with .counts (B,) int32 numpy = V_b and .total = their sum."""
    lib = load()
    _dev(points, torch.float32, "points")
    if points.ndim != 2 or points.shape[1] < 4:
        raise ValueError(f"points has shape {tuple(points.shape)}, expected (N, 1 + C) with C >= 3")
    pl = VoxelizePlan()
    pl.geo = geo = geometry if geometry is not None else VoxelizeGeometry(voxel_size, point_cloud_range)
    pl.points, pl.n, pl.c = points, int(points.shape[0]), int(points.shape[1]) - 1
    pl.p, pl.m = int(max_num_points), int(max_voxels)
    pl.cap = cap = VOXELIZE_DEFAULT_BATCH_CAP if batch_size is None else int(batch_size)
    if cap < 1:
        raise ValueError("batch_size must be positive")
    dev = points.device
    pl.workspace = workspace = _workspace(voxelize_workspace_bytes(pl.n, cap, geo.grid32), workspace, dev)
    if counts_pinned is None or counts_pinned.numel() < 4 + cap:
        counts_pinned = torch.empty((4 + cap,), dtype=torch.int32).pin_memory()
    if counts_pinned.dtype != torch.int32 or not counts_pinned.is_pinned():
        raise ValueError("counts_pinned must be a pinned int32 host tensor")
    pl.counts_pinned = counts_pinned
    with torch.cuda.device(dev):
        check(lib.modest_voxelize_plan(points.data_ptr(), pl.n, pl.c, cap, _np_ptr(geo.lo), _np_ptr(geo.vs), _np_ptr(geo.grid32),
                                       pl.p, pl.m, workspace.data_ptr(), workspace.numel(), counts_pinned.data_ptr(), _stream()),
              "modest_voxelize_plan")
    head = counts_pinned[:4].tolist()
    nb = head[1] if batch_size is None else cap
    pl.counts = counts_pinned[4:4 + nb].numpy().copy()
    pl.opened, pl.total = head[2], head[3]
    return pl


def voxelize_fill(pl: VoxelizePlan, voxels: Optional[torch.Tensor] = None, coords: Optional[torch.Tensor] = None,
                  num_points: Optional[torch.Tensor] = None, point_mask: Optional[torch.Tensor] = None):
    """modest_voxelize_fill (enqueue only, the stream of the plan call): writes every element of the four outputs,
    (total, P, C) float32, (total, 4) int32, (total,) int32, (total, P) int32 -- allocated here unless given."""
    dev = pl.points.device
    shapes = ((pl.total, pl.p, pl.c), (pl.total, 4), (pl.total,), (pl.total, pl.p))
    dtypes = (torch.float32, torch.int32, torch.int32, torch.int32)
    outs = []
    for t, shape, dtype, name in zip((voxels, coords, num_points, point_mask), shapes, dtypes,
                                     ("voxels", "coords", "num_points", "point_mask")):
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=dev)
        _dev(t, dtype, name)
        if tuple(t.shape) != shape or t.device != dev:
            raise ValueError(f"{name} has shape {tuple(t.shape)}, the plan says {shape}")
        outs.append(t)
    with torch.cuda.device(dev):
        check(load().modest_voxelize_fill(pl.points.data_ptr(), pl.n, pl.c, pl.cap, _np_ptr(pl.geo.grid32), pl.p, pl.m,
                                          pl.workspace.data_ptr(), pl.workspace.numel(), pl.opened, pl.total,
                                          *(t.data_ptr() for t in outs), _stream()), "modest_voxelize_fill")
    return tuple(outs)


def voxelize(points: torch.Tensor, voxel_size, point_cloud_range, max_num_points: int, max_voxels: int,
             batch_size: Optional[int] = None, workspace: Optional[torch.Tensor] = None,
             counts_pinned: Optional[torch.Tensor] = None, geometry: Optional[VoxelizeGeometry] = None):
    """spconv's hard voxelisation of a collated batch on the device, as `collate_batch` would have stacked the per-cloud
    host results.  points (sum N, 1 + C) float32, batch index in column 0, non-decreasing; max_voxels per cloud.
    -> voxels (sum V, P, C) float32, voxel_coords (sum V, 4) int32 [b, z, y, x], voxel_num_points (sum V,) int32,
    voxel_point_mask (sum V, P) int32 (row indices into points, -1 in unused slots), counts (B,) int32 numpy = V_b.
    batch_size None: the clouds seen (last batch index + 1, at most 256).  One stream synchronise (the counts size the
    outputs); workspace (uint8, device) and counts_pinned (int32, pinned) are reused when given and large enough.
    A batch column that is out of order or not integral raises and produces nothing."""
    pl = voxelize_plan(points, voxel_size, point_cloud_range, max_num_points, max_voxels, batch_size, workspace,
                       counts_pinned, geometry)
    return (*voxelize_fill(pl), pl.counts)


# --------------------------------------------------------------------------- sparse 3-D convolutions
SPCONV_CALLS = {"rulebook": 0, "forward": 0, "input_grad": 0, "weight_grad": 0}   # library calls made, by kind


def _triple(v, name: str):
    if isinstance(v, (int, np.integer)):
        return (int(v),) * 3
    t = tuple(int(a) for a in v)
    if len(t) != 3:
        raise ValueError(f"{name} must be an int or three ints, got {v!r}")
    return t


def spconv_out_shape(spatial_shape, kernel, stride, padding, subm: bool = False):
    """[D, H, W] of the output: the input's for a submanifold convolution, else (in + 2 p - k) // s + 1 per axis"""
    shape, k, s, p = (_triple(v, n) for v, n in ((spatial_shape, "spatial_shape"), (kernel, "kernel_size"),
                                                  (stride, "stride"), (padding, "padding")))
    if min(shape) < 1 or min(k) < 1:
        raise ValueError(f"spatial shape {list(shape)} and kernel {list(k)} must be positive")
    if subm:
        if any(a % 2 == 0 for a in k):
            raise ValueError(f"a submanifold convolution needs odd kernel sizes, got {list(k)}")
        return list(shape)
    if min(s) < 1 or min(p) < 0:
        raise ValueError(f"stride {list(s)} must be positive and padding {list(p)} non-negative")
    out = [(shape[j] + 2 * p[j] - k[j]) // s[j] + 1 for j in range(3)]
    if min(out) <= 0:
        raise ValueError(f"output shape {out} of input {list(shape)}, kernel {list(k)}, stride {list(s)}, padding {list(p)}")
    return out


class SpconvRulebook:
    """what one geometry on one set of sites needs: .out_indices (N_out, 4) int32 (the input's own tensor when subm),
    .out_shape, .nbr (K, N_out) / .nbr_t (K, N_in) int32 with -1 for an absent neighbour, and the geometry it was built for"""

    def same_geometry(self, batch_size, spatial_shape, kernel, stride, padding, subm) -> bool:
        want = (int(batch_size), _triple(spatial_shape, "spatial_shape"), _triple(kernel, "kernel_size"), bool(subm))
        if not subm:
            want += (_triple(stride, "stride"), _triple(padding, "padding"))
        return self.geometry == want


def spconv_rulebook(indices: torch.Tensor, batch_size: int, spatial_shape, kernel, stride=1, padding=0, subm: bool = False,
                    workspace: Optional[torch.Tensor] = None, counts_pinned: Optional[torch.Tensor] = None) -> SpconvRulebook:
    """Output sites and neighbour maps of a sparse convolution on PyTorch's current stream; ONE stream synchronise (the
    output count sizes the maps, and a duplicate or out-of-range row must be reported before anything is produced)."""
    _dev(indices, torch.int32, "indices")
    if indices.ndim != 2 or indices.shape[1] != 4:
        raise ValueError(f"indices has shape {tuple(indices.shape)}, expected (N, 4) [b, z, y, x]")
    rb = SpconvRulebook()
    rb.subm = bool(subm)
    rb.batch_size = int(batch_size)
    rb.in_shape = list(_triple(spatial_shape, "spatial_shape"))
    rb.kernel, rb.stride, rb.padding = (_triple(v, n) for v, n in ((kernel, "kernel_size"), (stride, "stride"), (padding, "padding")))
    rb.out_shape = spconv_out_shape(rb.in_shape, rb.kernel, rb.stride, rb.padding, rb.subm)
    rb.geometry = (rb.batch_size, tuple(rb.in_shape), rb.kernel, rb.subm) + (() if rb.subm else (rb.stride, rb.padding))
    rb.kvol = rb.kernel[0] * rb.kernel[1] * rb.kernel[2]
    rb.indices, rb.n_in = indices, int(indices.shape[0])
    dev = indices.device
    lib = load()
    geo = [np.ascontiguousarray(v, dtype=np.int32) for v in (rb.in_shape, rb.kernel, rb.stride, rb.padding)]
    workspace = _workspace(_workspace_bytes("modest_spconv_rulebook_workspace_bytes", rb.n_in, rb.kvol, rb.subm), workspace, dev)
    if counts_pinned is None:
        counts_pinned = torch.zeros((2,), dtype=torch.int32).pin_memory()
    if counts_pinned.dtype != torch.int32 or not counts_pinned.is_pinned() or counts_pinned.numel() < 2:
        raise ValueError("counts_pinned must be a pinned int32 host tensor of two words")
    SPCONV_CALLS["rulebook"] += 1
    with torch.cuda.device(dev):
        check(lib.modest_spconv_rulebook_plan(indices.data_ptr(), rb.n_in, rb.batch_size, *(_np_ptr(g) for g in geo),
                                              int(rb.subm), workspace.data_ptr(), workspace.numel(), counts_pinned.data_ptr(),
                                              _stream()), "modest_spconv_rulebook_plan")
        rb.n_out = int(counts_pinned[1]) if not rb.subm else rb.n_in
        rb.out_indices = indices if rb.subm else torch.empty((rb.n_out, 4), dtype=torch.int32, device=dev)
        rb.nbr = torch.empty((rb.kvol, rb.n_out), dtype=torch.int32, device=dev)
        rb.nbr_t = torch.empty((rb.kvol, rb.n_in), dtype=torch.int32, device=dev)
        check(lib.modest_spconv_rulebook_fill(indices.data_ptr(), rb.n_in, rb.batch_size, *(_np_ptr(g) for g in geo),
                                              int(rb.subm), workspace.data_ptr(), workspace.numel(), rb.n_out,
                                              rb.out_indices.data_ptr(), rb.nbr.data_ptr(), rb.nbr_t.data_ptr(), _stream()),
              "modest_spconv_rulebook_fill")
    rb.workspace = workspace   # (the fill kernels read it: it must outlive them on this stream)
    return rb


def _spconv_weight(weight: torch.Tensor, rb: SpconvRulebook):
    _dev(weight, torch.float32, "weight")
    if weight.ndim == 5:
        if tuple(weight.shape[:3]) != tuple(rb.kernel):
            raise ValueError(f"weight has kernel {tuple(weight.shape[:3])}, the rulebook {tuple(rb.kernel)}")
    elif weight.ndim != 3 or weight.shape[0] != rb.kvol:
        raise ValueError(f"weight has shape {tuple(weight.shape)}, expected (kz, ky, kx, Cin, Cout) or (K, Cin, Cout)")
    cin, cout = int(weight.shape[-2]), int(weight.shape[-1])
    if not (1 <= cin <= 128 and 1 <= cout <= 128):
        raise ValueError("channels must lie in 1 .. 128")
    return cin, cout


def spconv_forward(features: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], rb: SpconvRulebook,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """features (N_in, Cin), weight (kz, ky, kx, Cin, Cout) or (K, Cin, Cout), bias (Cout,) or None -> (N_out, Cout), every
    element written, in the fixed order of DESIGN.md section 7g.  Enqueue only."""
    cin, cout = _spconv_weight(weight, rb)
    _dev(features, torch.float32, "features")
    if tuple(features.shape) != (rb.n_in, cin):
        raise ValueError(f"features has shape {tuple(features.shape)}, expected {(rb.n_in, cin)}")
    if bias is not None:
        _dev(bias, torch.float32, "bias")
        if tuple(bias.shape) != (cout,):
            raise ValueError(f"bias has shape {tuple(bias.shape)}, expected {(cout,)}")
    if out is None:
        out = torch.empty((rb.n_out, cout), dtype=torch.float32, device=features.device)
    _dev(out, torch.float32, "out")
    if tuple(out.shape) != (rb.n_out, cout):
        raise ValueError(f"out has shape {tuple(out.shape)}, expected {(rb.n_out, cout)}")
    SPCONV_CALLS["forward"] += 1
    with torch.cuda.device(features.device):
        check(load().modest_spconv_gather_gemm(features.data_ptr(), rb.n_in, cin, weight.data_ptr(), rb.kvol, cin, cout, 0,
                                               bias.data_ptr() if bias is not None else None, rb.nbr.data_ptr(), rb.n_out,
                                               out.data_ptr(), _stream()), "modest_spconv_gather_gemm")
    return out


def spconv_backward(features: torch.Tensor, weight: torch.Tensor, grad_out: torch.Tensor, rb: SpconvRulebook,
                    need_input_grad: bool = True, need_weight_grad: bool = True, need_bias_grad: bool = True,
                    grad_input: Optional[torch.Tensor] = None, grad_weight: Optional[torch.Tensor] = None,
                    grad_bias: Optional[torch.Tensor] = None):
    """-> (grad_input (N_in, Cin) | None, grad_weight (shape of weight) | None, grad_bias (Cout,) | None).  A gradient
    that is not needed launches nothing.  Enqueue only."""
    cin, cout = _spconv_weight(weight, rb)
    _dev(features, torch.float32, "features")
    _dev(grad_out, torch.float32, "grad_out")
    if tuple(features.shape) != (rb.n_in, cin) or tuple(grad_out.shape) != (rb.n_out, cout):
        raise ValueError(f"features {tuple(features.shape)} / grad_out {tuple(grad_out.shape)}, expected "
                         f"{(rb.n_in, cin)} / {(rb.n_out, cout)}")
    dev = features.device
    lib = load()

    def given(t, shape, name):
        if t is None:
            return torch.empty(shape, dtype=torch.float32, device=dev)
        _dev(t, torch.float32, name)
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
        return t
    dx = dw = db = None
    with torch.cuda.device(dev):
        if need_input_grad:
            dx = given(grad_input, (rb.n_in, cin), "grad_input")
            SPCONV_CALLS["input_grad"] += 1
            check(lib.modest_spconv_gather_gemm(grad_out.data_ptr(), rb.n_out, cout, weight.data_ptr(), rb.kvol, cin, cout, 1,
                                                None, rb.nbr_t.data_ptr(), rb.n_in, dx.data_ptr(), _stream()),
                  "modest_spconv_gather_gemm")
        if need_weight_grad or need_bias_grad:
            dw = given(grad_weight, tuple(weight.shape), "grad_weight")
            if need_bias_grad:
                db = given(grad_bias, (cout,), "grad_bias")
            nbytes = _workspace_bytes("modest_spconv_wgrad_workspace_bytes", rb.n_out, rb.kvol, cin, cout)
            ws = torch.empty((max(nbytes, 256),), dtype=torch.uint8, device=dev)
            SPCONV_CALLS["weight_grad"] += 1
            check(lib.modest_spconv_wgrad(features.data_ptr(), rb.n_in, cin, grad_out.data_ptr(), rb.n_out, cout,
                                          rb.nbr.data_ptr(), rb.kvol, ws.data_ptr(), ws.numel(), dw.data_ptr(),
                                          db.data_ptr() if db is not None else None, _stream()), "modest_spconv_wgrad")
            if not need_weight_grad:
                dw = None
    return dx, dw, db


# --------------------------------------------------------------------------- inverse sparse convolution
SPCONV_INVERSE_CALLS = {"class_order": 0, "forward": 0, "input_grad": 0, "weight_grad": 0}   # library calls made, by kind
SPCONV_INVERSE_ORDER = "classes"   # the default `order` of spconv_inverse_forward ("Measurement")
SPCONV_CLASSES_MAX = 64            # the class tiles apply for 2 .. 64 classes, the rows of nbr_t otherwise


def spconv_classes(rb: SpconvRulebook) -> int:
    """s_z s_y s_x of a strided rulebook: the classes its input rows fall into"""
    return rb.stride[0] * rb.stride[1] * rb.stride[2]


def _spconv_inverse_rulebook(rb: SpconvRulebook):
    if not isinstance(rb, SpconvRulebook):
        raise ValueError("an inverse convolution needs the rulebook of a strided convolution")
    if rb.subm:
        raise ValueError("an inverse convolution needs the rulebook of a strided convolution, this one is submanifold")


def spconv_class_order(rb: SpconvRulebook):
    """-> (perm (N_in,) int32, class_start (C + 1,) int32) on the device: the input rows of a strided rulebook stably
    ordered by the class ((z + p_z) % s_z, (y + p_y) % s_y, (x + p_x) % s_x), and the exclusive counts.  Built at the
    first call and kept on the rulebook.  Enqueue only."""
    _spconv_inverse_rulebook(rb)
    cached = getattr(rb, "class_order", None)
    if cached is not None:
        return cached
    _dev(rb.indices, torch.int32, "indices")
    dev = rb.indices.device
    lib = load()
    classes = spconv_classes(rb)
    nbytes = _workspace_bytes("modest_spconv_class_order_workspace_bytes", rb.n_in, classes)
    stride, pad = (np.ascontiguousarray(v, dtype=np.int32) for v in (rb.stride, rb.padding))
    with torch.cuda.device(dev):
        ws = torch.empty((max(nbytes, 256),), dtype=torch.uint8, device=dev)
        perm = torch.empty((rb.n_in,), dtype=torch.int32, device=dev)
        class_start = torch.empty((classes + 1,), dtype=torch.int32, device=dev)
        SPCONV_INVERSE_CALLS["class_order"] += 1
        check(lib.modest_spconv_class_order(rb.indices.data_ptr(), rb.n_in, _np_ptr(stride), _np_ptr(pad), ws.data_ptr(),
                                            ws.numel(), perm.data_ptr(), class_start.data_ptr(), _stream()),
              "modest_spconv_class_order")
    rb.class_order = (perm, class_start)
    return rb.class_order


def _spconv_inverse_args(features, weight, rb):
    _spconv_inverse_rulebook(rb)
    cin, cout = _spconv_weight(weight, rb)
    _dev(features, torch.float32, "features")
    if tuple(features.shape) != (rb.n_out, cin):
        raise ValueError(f"features has shape {tuple(features.shape)}, expected {(rb.n_out, cin)}: the rows of the strided "
                         f"convolution's output")
    return cin, cout


def spconv_inverse_forward(features: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], rb: SpconvRulebook,
                           out: Optional[torch.Tensor] = None, order: Optional[str] = None) -> torch.Tensor:
    """The strided rulebook rb run backwards: features (rb.n_out, Cin) on the coarse sites, weight (kz, ky, kx, Cin, Cout)
    or (K, Cin, Cout), bias (Cout,) or None -> (rb.n_in, Cout) on the fine sites, every element written, in the fixed
    order of DESIGN.md section 7k.  order "classes": tiles of one class (2 .. 64 classes; otherwise the rows are used);
    "rows": modest_spconv_gather_gemm on nbr_t.  The same bits either way.  Enqueue only."""
    order = SPCONV_INVERSE_ORDER if order is None else order
    if order not in ("classes", "rows"):
        raise ValueError(f"order must be 'classes' or 'rows', got {order!r}")
    cin, cout = _spconv_inverse_args(features, weight, rb)
    if bias is not None:
        _dev(bias, torch.float32, "bias")
        if tuple(bias.shape) != (cout,):
            raise ValueError(f"bias has shape {tuple(bias.shape)}, expected {(cout,)}")
    if out is None:
        out = torch.empty((rb.n_in, cout), dtype=torch.float32, device=features.device)
    _dev(out, torch.float32, "out")
    if tuple(out.shape) != (rb.n_in, cout):
        raise ValueError(f"out has shape {tuple(out.shape)}, expected {(rb.n_in, cout)}")
    lib = load()
    bias_ptr = bias.data_ptr() if bias is not None else None
    if order == "classes" and 2 <= spconv_classes(rb) <= SPCONV_CLASSES_MAX:
        perm, class_start = spconv_class_order(rb)
        kernel, stride = (np.ascontiguousarray(v, dtype=np.int32) for v in (rb.kernel, rb.stride))
        SPCONV_INVERSE_CALLS["forward"] += 1
        with torch.cuda.device(features.device):
            check(lib.modest_spconv_gather_gemm_classes(features.data_ptr(), rb.n_out, cin, weight.data_ptr(), _np_ptr(kernel),
                                                        _np_ptr(stride), cout, bias_ptr, rb.nbr_t.data_ptr(), rb.n_in,
                                                        perm.data_ptr(), class_start.data_ptr(), out.data_ptr(), _stream()),
                  "modest_spconv_gather_gemm_classes")
        return out
    SPCONV_INVERSE_CALLS["forward"] += 1
    with torch.cuda.device(features.device):
        check(lib.modest_spconv_gather_gemm(features.data_ptr(), rb.n_out, cin, weight.data_ptr(), rb.kvol, cin, cout, 0,
                                            bias_ptr, rb.nbr_t.data_ptr(), rb.n_in, out.data_ptr(), _stream()),
              "modest_spconv_gather_gemm")
    return out


def spconv_inverse_backward(features: torch.Tensor, weight: torch.Tensor, grad_out: torch.Tensor, rb: SpconvRulebook,
                            need_input_grad: bool = True, need_weight_grad: bool = True, need_bias_grad: bool = True,
                            grad_input: Optional[torch.Tensor] = None):
    """-> (grad_input (rb.n_out, Cin) | None, grad_weight (shape of weight) | None, grad_bias (Cout,) | None) for grad_out
    (rb.n_in, Cout).  The feature gradient is the gather-GEMM with the transposed weights on nbr, the weight gradient
    modest_spconv_wgrad over the coarse rows with the two sides exchanged, (K, Cout, Cin), transposed once; the bias
    gradient is the column sum of grad_out.  A gradient that is not needed launches nothing.  Enqueue only."""
    cin, cout = _spconv_inverse_args(features, weight, rb)
    _dev(grad_out, torch.float32, "grad_out")
    if tuple(grad_out.shape) != (rb.n_in, cout):
        raise ValueError(f"grad_out has shape {tuple(grad_out.shape)}, expected {(rb.n_in, cout)}")
    dev = features.device
    lib = load()
    dx = dw = db = None
    with torch.cuda.device(dev):
        if need_input_grad:
            if grad_input is None:
                grad_input = torch.empty((rb.n_out, cin), dtype=torch.float32, device=dev)
            dx = _dev(grad_input, torch.float32, "grad_input")
            if tuple(dx.shape) != (rb.n_out, cin):
                raise ValueError(f"grad_input has shape {tuple(dx.shape)}, expected {(rb.n_out, cin)}")
            SPCONV_INVERSE_CALLS["input_grad"] += 1
            check(lib.modest_spconv_gather_gemm(grad_out.data_ptr(), rb.n_in, cout, weight.data_ptr(), rb.kvol, cin, cout, 1,
                                                None, rb.nbr.data_ptr(), rb.n_out, dx.data_ptr(), _stream()),
                  "modest_spconv_gather_gemm")
        if need_weight_grad:
            nbytes = _workspace_bytes("modest_spconv_wgrad_workspace_bytes", rb.n_out, rb.kvol, cout, cin)
            ws = torch.empty((max(nbytes, 256),), dtype=torch.uint8, device=dev)
            dwt = torch.empty((rb.kvol, cout, cin), dtype=torch.float32, device=dev)
            SPCONV_INVERSE_CALLS["weight_grad"] += 1
            check(lib.modest_spconv_wgrad(grad_out.data_ptr(), rb.n_in, cout, features.data_ptr(), rb.n_out, cin,
                                          rb.nbr.data_ptr(), rb.kvol, ws.data_ptr(), ws.numel(), dwt.data_ptr(), None,
                                          _stream()), "modest_spconv_wgrad")
            dw = dwt.transpose(1, 2).contiguous().view(weight.shape)
        if need_bias_grad:
            db = grad_out.sum(0)
    return dx, dw, db


# --------------------------------------------------------------------------- anchor target assignment
def anchor_targets_workspace_bytes(batch_size: int, n_cls: int, m: int) -> int:
    return _workspace_bytes("modest_anchor_targets_workspace_bytes", batch_size, n_cls, m)


def anchor_targets(gt: torch.Tensor, anchors: torch.Tensor, cls_table: torch.Tensor, thresholds: torch.Tensor,
                   name_match: torch.Tensor, max_cls_rows: int, n_out: int, sincos: bool = False,
                   workspace: Optional[torch.Tensor] = None, out=None):
    """modest_anchor_targets on PyTorch's current stream: enqueue only, nothing is read back.
    gt (B, M, 7 + Cg + 1) float32, any strides; anchors (sum of rows, 7 + Ca) float32, the classes' blocks one after the
    other; cls_table (n_cls, 5) int64 [first row, rows, k, stride, offset] (row i of a class -> output row
    (i / k) * stride + offset + i % k); thresholds (n_cls, 2) float32 [matched, unmatched]; name_match (n_cls, n_names)
    uint8.  -> labels (B, n_out) int32, targets (B, n_out, 7 + sincos + min(Ca, Cg)) float32, weights (B, n_out) float32:
    freshly allocated, or the three tensors of `out` (of exactly these shapes and types, contiguous, on gt's device), every
    element of which is written."""
    lib = load()
    if not gt.is_cuda or gt.dtype != torch.float32 or gt.ndim != 3:
        raise ValueError("gt must be a (B, M, 8 + C) float32 device tensor")
    _dev(anchors, torch.float32, "anchors")
    _dev(cls_table, torch.int64, "cls_table")
    _dev(thresholds, torch.float32, "thresholds")
    _dev(name_match, torch.uint8, "name_match")
    B, M, G = (int(v) for v in gt.shape)
    n_cls = int(cls_table.shape[0])
    if anchors.ndim != 2 or anchors.shape[1] < 7 or G < 8:
        raise ValueError(f"anchors has shape {tuple(anchors.shape)} and gt {tuple(gt.shape)}: expected (N, 7 + Ca) and (B, M, 7 + Cg + 1)")
    A = int(anchors.shape[1])
    if tuple(cls_table.shape) != (n_cls, 5) or tuple(thresholds.shape) != (n_cls, 2) or name_match.ndim != 2 \
            or name_match.shape[0] != n_cls:
        raise ValueError("cls_table (n_cls, 5), thresholds (n_cls, 2) and name_match (n_cls, n_names) disagree")
    dev = gt.device
    code = 7 + int(bool(sincos)) + min(A - 7, G - 8)
    labels, targets, weights = _outputs((("labels", torch.int32, (B, int(n_out)), True), ("targets", torch.float32, (B, int(n_out), code), True),
                                         ("weights", torch.float32, (B, int(n_out)), True)), out, dev, anchor="gt")
    workspace = _workspace(anchor_targets_workspace_bytes(B, n_cls, M), workspace, dev)
    sb, sm, sc = (int(v) for v in gt.stride())
    with torch.cuda.device(dev):
        check(lib.modest_anchor_targets(B, M, G, gt.data_ptr(), sb, sm, sc, anchors.data_ptr(), A, n_cls,
                                        cls_table.data_ptr(), thresholds.data_ptr(), name_match.data_ptr(),
                                        int(name_match.shape[1]), int(max_cls_rows), int(bool(sincos)), int(n_out),
                                        labels.data_ptr(), targets.data_ptr(), weights.data_ptr(), workspace.data_ptr(),
                                        workspace.numel(), _stream()), "modest_anchor_targets")
    return labels, targets, weights


# --------------------------------------------------------------------------- point-head target assignment
def point_targets(points: torch.Tensor, gt_boxes: torch.Tensor, extend_gt_boxes: torch.Tensor, num_class: int,
                  mean_size: Optional[torch.Tensor] = None, want_box: bool = False, want_part: bool = False, out=None):
    """modest_point_targets on PyTorch's current stream: enqueue only, nothing is read back.
    points (N, 4) float32 [bs_idx, x, y, z], rows of any stride; gt_boxes and extend_gt_boxes (B, M, 8) float32, any
    strides; mean_size (n_cls, 3) float32 contiguous, or None for a coder with use_mean_size=False.
    -> point_cls_labels (N) int64, point_box_labels (N, 8) float32 or None, point_part_labels (N, 3) float32 or None:
    freshly allocated, or the three entries of `out` (None where the label is not asked for; else of exactly these shapes
    and types, contiguous, on the points' device), every element of which is written."""
    _device_tensors((("points", points), ("gt_boxes", gt_boxes), ("extend_gt_boxes", extend_gt_boxes)))
    if points.ndim != 2 or points.shape[1] != 4:
        raise ValueError(f"points has shape {tuple(points.shape)}, expected (N, 4)")
    if gt_boxes.ndim != 3 or gt_boxes.shape[2] != 8 or tuple(extend_gt_boxes.shape) != tuple(gt_boxes.shape):
        raise ValueError(f"gt_boxes has shape {tuple(gt_boxes.shape)} and extend_gt_boxes {tuple(extend_gt_boxes.shape)}: "
                         f"expected (B, M, 8) twice")
    dev = points.device
    if gt_boxes.device != dev or extend_gt_boxes.device != dev:
        raise ValueError("points, gt_boxes and extend_gt_boxes are on different devices")
    n_mean = 0
    if mean_size is not None:
        if not torch.is_tensor(mean_size) or not mean_size.is_cuda or mean_size.device != dev:
            raise ValueError("mean_size must be a device tensor on the points' device")
        if mean_size.dtype != torch.float32 or mean_size.ndim != 2 or mean_size.shape[1] != 3 or mean_size.shape[0] == 0 \
                or not mean_size.is_contiguous():
            raise ValueError("mean_size must be a contiguous (n_cls, 3) float32 tensor with n_cls >= 1")
        n_mean = int(mean_size.shape[0])
    if int(num_class) < 1:
        raise ValueError(f"num_class is {num_class}")
    N = int(points.shape[0])
    B, M = int(gt_boxes.shape[0]), int(gt_boxes.shape[1])
    if points.stride(1) != 1:
        points = points.contiguous()
    labels, box, part = _outputs((("point_cls_labels", torch.int64, (N,), True), ("point_box_labels", torch.float32, (N, 8), bool(want_box)),
                                  ("point_part_labels", torch.float32, (N, 3), bool(want_part))), out, dev, anchor="points",
                                 absent=("is given but not asked for", "is missing"))
    if N == 0:
        return labels, box, part   # nothing to write, nothing launched
    lib = load()
    gs = [int(v) for v in gt_boxes.stride()] if B and M else [0, 0, 0]
    es = [int(v) for v in extend_gt_boxes.stride()] if B and M else [0, 0, 0]
    with torch.cuda.device(dev):
        check(lib.modest_point_targets(N, points.data_ptr(), int(points.stride(0)) if N > 1 else 4, B, M,
                                       gt_boxes.data_ptr() if B and M else None, *gs,
                                       extend_gt_boxes.data_ptr() if B and M else None, *es,
                                       mean_size.data_ptr() if n_mean else None, n_mean, int(num_class), labels.data_ptr(),
                                       _ptr(box), _ptr(part), _stream()), "modest_point_targets")
    return labels, box, part


# --------------------------------------------------------------------------- RoI proposal layer
def proposals_workspace_bytes(n_rows: int) -> int:
    return _workspace_bytes("modest_proposals_workspace_bytes", n_rows)


_BATCH_INDEX_KINDS = {torch.float32: 1, torch.int64: 2, torch.int32: 3}


def _ranked_rows(box_preds, cls_preds, batch_size, pre_maxsize, post_maxsize, batch_index, dense_only=False):
    """The rows `proposals` and `post_process` rank, in their two forms: dense, (B, N, 7 + C) and (B, N, K), or stacked, (N, 7 + C)
    and (N, K) with `batch_index` (N).  dense_only: the call carries what only the dense form takes, so that the stacked form is
    refused.  -> dev, B, rows per sample (0 when stacked), the kind of batch_index (0: none), batch_index as the library reads
    it or None, 7 + C, K, the two tensors contiguous, the rows, post_maxsize"""
    dev = _device_tensors((("box_preds", box_preds), ("cls_preds", cls_preds)))
    if cls_preds.device != dev:
        raise ValueError("box_preds and cls_preds are on different devices")
    B = int(batch_size)
    if batch_index is None:
        if box_preds.ndim != 3 or cls_preds.ndim != 3 or box_preds.shape[:2] != cls_preds.shape[:2] or box_preds.shape[0] != B:
            raise ValueError(f"dense form: box_preds {tuple(box_preds.shape)} and cls_preds {tuple(cls_preds.shape)} must be "
                             f"(batch_size = {B}, N, 7 + C) and (batch_size, N, K)")
        per, kind, bidx = int(box_preds.shape[1]), 0, None
    else:
        if box_preds.ndim != 2 or cls_preds.ndim != 2 or box_preds.shape[0] != cls_preds.shape[0] \
                or not torch.is_tensor(batch_index) or batch_index.numel() != box_preds.shape[0]:
            raise ValueError(f"stacked form: box_preds {tuple(box_preds.shape)}, cls_preds {tuple(cls_preds.shape)} and "
                             f"batch_index must be (N, 7 + C), (N, K) and (N)")
        if dense_only:
            raise NotImplementedError("given labels or rois together with batch_index: no head produces that combination")
        if batch_index.device != dev:
            raise ValueError("batch_index is on another device than box_preds")
        bidx = batch_index.reshape(-1)
        if bidx.dtype not in _BATCH_INDEX_KINDS:
            bidx = bidx.float() if bidx.dtype.is_floating_point else bidx.long()
        bidx = bidx.contiguous()
        per, kind = 0, _BATCH_INDEX_KINDS[bidx.dtype]
    cols, K = int(box_preds.shape[-1]), int(cls_preds.shape[-1])
    if cols < 7 or K < 1:
        raise ValueError(f"box_preds needs 7 + C columns and cls_preds K >= 1, got {cols} and {K}")
    box, cls = box_preds.contiguous(), cls_preds.contiguous()
    n = int(box.numel() // cols)
    P = int(post_maxsize)
    if P < 0 or B < 0 or int(pre_maxsize) < 0:
        raise ValueError("batch_size, pre_maxsize and post_maxsize must not be negative")
    return dev, B, per, kind, bidx, cols, K, box, cls, n, P


def proposals(box_preds: torch.Tensor, cls_preds: torch.Tensor, batch_size: int, pre_maxsize: int, post_maxsize: int,
              thresh: float, rotated: bool = True, batch_index: Optional[torch.Tensor] = None,
              workspace: Optional[torch.Tensor] = None, out=None):
    """modest_proposals on PyTorch's current stream: enqueue only, nothing is read back.
    Dense form: box_preds (B, N, 7 + C) and cls_preds (B, N, K) float32 with B == batch_size.  Stacked form: (N1 + N2 + ..,
    7 + C) and (N1 + N2 + .., K) with batch_index (N1 + N2 + ..), a float or integer tensor of sample numbers in any order.
    Per sample the min(pre_maxsize, rows) highest class maxima (NaN first, equal scores by ascending row, the lowest class
    among equal maxima) are walked by greedy NMS at `thresh` (rotated: nms_gpu, else nms_normal_gpu) up to the
    post_maxsize-th survivor.  -> rois (B, post_maxsize, 7 + C) float32, roi_scores (B, post_maxsize) float32, roi_labels
    (B, post_maxsize) int64 (label + 1; 1 in the padding): freshly allocated, or the three tensors of `out` (of exactly
    these shapes and types, contiguous, on the boxes' device), every element of which is written.  workspace: an uint8
    tensor of at least proposals_workspace_bytes(rows) bytes, allocated when missing or too small."""
    dev, B, per, kind, bidx, cols, K, box, cls, n, P = _ranked_rows(box_preds, cls_preds, batch_size, pre_maxsize, post_maxsize, batch_index)
    rois, scores, labels = _outputs((("rois", torch.float32, (B, P, cols), True), ("roi_scores", torch.float32, (B, P), True),
                                     ("roi_labels", torch.int64, (B, P), True)), out, dev, anchor="box_preds")
    workspace = _workspace(proposals_workspace_bytes(n), workspace, dev)
    with torch.cuda.device(dev):
        check(load().modest_proposals(n, B, per, box.data_ptr(), cols, cls.data_ptr(), K, _ptr(bidx), kind, int(pre_maxsize), P, float(thresh),
                                   int(bool(rotated)), rois.data_ptr(), scores.data_ptr(), labels.data_ptr(),
                                   workspace.data_ptr(), workspace.numel(), _stream()), "modest_proposals")
    return rois, scores, labels


# --------------------------------------------------------------------------- RoI target assignment
ROI_LISTS = ("fg", "hard", "easy")          # list ids of a pick, and the order of a sample's three counts
ROI_SCORE_TYPES = {"cls": 0, "roi_iou": 1}
ROI_BATCH_MAX = 65535                       # samples per call
ROI_COLS_MAX = 4096                         # 7 + C


def roi_targets_gt_tile() -> int:
    """gts a match workgroup stages in LDS at a time"""
    return int(load().modest_roi_targets_gt_tile())


def roi_targets_workspace_bytes(batch_size: int, n_rois: int) -> int:
    return _workspace_bytes("modest_roi_targets_workspace_bytes", batch_size, n_rois)


def roi_target_draws(counts, cfg, np_random=None, generator=None, sample=0):
    """the picks of one sample from its (fg, hard, easy) counts: exactly the reference's calls in the reference's order
    (subsample_rois, sample_bg_inds of proposal_target_layer.py) on numpy's and torch's CPU generators
    -> (ROI_PER_IMAGE, 2) int32 of (list, position)"""
    npr = np.random if np_random is None else np_random
    M = int(_cfg_get(cfg, "ROI_PER_IMAGE"))
    nf, nh, ne = (int(v) for v in counts)
    nb = nh + ne
    fg_per = int(np.round(_cfg_get(cfg, "FG_RATIO") * M))

    def randint(high, n):
        return torch.randint(low=0, high=high, size=(n,), generator=generator).long().numpy()

    def bg(n):
        if nh > 0 and ne > 0:
            hn = min(int(n * _cfg_get(cfg, "HARD_BG_RATIO")), nh)
            hard = randint(nh, hn)
            easy = randint(ne, n - hn)
            return [(1, hard), (2, easy)]
        if nh > 0:
            return [(1, randint(nh, n))]
        return [(2, randint(ne, n))]

    if nf > 0 and nb > 0:
        n_fg = min(fg_per, nf)
        parts = [(0, npr.permutation(nf)[:n_fg])] + bg(M - n_fg)
    elif nf > 0:
        parts = [(0, np.floor(npr.rand(M) * nf).astype(np.float32).astype(np.int64))]
    elif nb > 0:
        parts = bg(M)
    else:
        raise NotImplementedError(f"sample {sample}: FG={nf}, BG={nb}: no roi has a number for its maximum IoU")
    out = np.concatenate([np.stack([np.full(len(pos), lid, np.int64), np.asarray(pos, np.int64)], 1) for lid, pos in parts])
    if len(out) != M:   # a negative bg share (FG_RATIO above 1): the reference fails on the shape too
        raise ValueError(f"sample {sample}: {len(out)} picks for ROI_PER_IMAGE = {M}")
    return out.astype(np.int32)


def _roi_args(rois, roi_scores, roi_labels, gt_boxes):
    _device_tensors((("rois", rois), ("roi_scores", roi_scores), ("roi_labels", roi_labels), ("gt_boxes", gt_boxes)), dtype_error=None)
    if rois.ndim != 3 or gt_boxes.ndim != 3 or roi_scores.shape != rois.shape[:2] or roi_labels.shape != rois.shape[:2] \
            or gt_boxes.shape[0] != rois.shape[0] or gt_boxes.shape[2] != rois.shape[2] + 1:
        raise ValueError(f"rois {tuple(rois.shape)}, roi_scores {tuple(roi_scores.shape)}, roi_labels "
                         f"{tuple(roi_labels.shape)} and gt_boxes {tuple(gt_boxes.shape)} must be (B, N, 7 + C), (B, N), "
                         f"(B, N) and (B, G, 7 + C + 1)")


def roi_targets_limits(batch_size: int, cols: int, roi_per_image: int, n_rois: int = 0, n_gt: int = 0):
    """the limits of the two calls, each a ValueError that names it; needs no device"""
    if cols < 7 or cols > ROI_COLS_MAX:
        raise ValueError(f"rois have {cols} columns: 7 + C, at most {ROI_COLS_MAX}")
    if batch_size > ROI_BATCH_MAX:
        raise ValueError(f"batch_size = {batch_size} is above the limit of {ROI_BATCH_MAX} samples per call")
    if roi_per_image < 1:
        raise ValueError(f"ROI_PER_IMAGE = {roi_per_image} is below the limit of 1")
    if batch_size * max(n_rois, n_gt, roi_per_image) > 2 ** 31 - 1:
        raise ValueError(f"{batch_size} samples of {n_rois} rois, {n_gt} gts and {roi_per_image} outputs are above the "
                         f"limit of {2 ** 31 - 1} rows per call")


def roi_targets_match(rois, roi_labels, gt_boxes, fg_thresh, bg_thresh_lo, reg_fg_thresh, by_class, workspace, counts_pinned):
    """modest_roi_targets_match on PyTorch's current stream: BLOCKING (one synchronise).  rois (B, N, 7 + C) float32 and
    roi_labels (B, N) int64 contiguous, gt_boxes (B, G, 7 + C + 1) float32 of any strides; workspace uint8 of
    roi_targets_workspace_bytes(B, N); counts_pinned a pinned int32 tensor of at least 3 B words -> its (B, 3) view of
    (fg, hard, easy) list lengths, valid on return"""
    B, N, cols = (int(v) for v in rois.shape)
    G = int(gt_boxes.shape[1])
    _dev(rois, torch.float32, "rois"), _dev(roi_labels, torch.int64, "roi_labels"), _dev(workspace, torch.uint8, "workspace")
    if gt_boxes.dtype != torch.float32 or not gt_boxes.is_cuda:
        raise ValueError("gt_boxes must be a float32 device tensor")
    if not counts_pinned.is_pinned() or counts_pinned.dtype != torch.int32 or counts_pinned.numel() < 3 * B:
        raise ValueError("counts_pinned must be a pinned int32 tensor of at least 3 * B words")
    with torch.cuda.device(rois.device):
        check(load().modest_roi_targets_match(B, N, G, rois.data_ptr() if B * N else None, cols,
                                              roi_labels.data_ptr() if B * N else None, gt_boxes.data_ptr() if B * G else None,
                                              *(int(s) for s in gt_boxes.stride()), float(fg_thresh), float(bg_thresh_lo),
                                              float(reg_fg_thresh), int(bool(by_class)), workspace.data_ptr(), workspace.numel(),
                                              counts_pinned.data_ptr(), _stream()), "modest_roi_targets_match")
    return counts_pinned[:3 * B].view(B, 3)


def roi_targets_lists(workspace: torch.Tensor, batch_size: int, n_rois: int):
    """test helper: what a match call left in `workspace` -> (counts (B, 3), max_iou (B, N) float32, assignment (B, N),
    [fg, hard, easy] lists per sample) as numpy arrays; the byte offsets are the library's own
    (modest_roi_targets_workspace_offsets)"""
    B, N = int(batch_size), int(n_rois)
    raw = workspace.cpu().numpy()
    off = np.zeros(6, np.int64)
    check(load().modest_roi_targets_workspace_offsets(B, N, off.ctypes.data), "modest_roi_targets_workspace_offsets")
    counts = raw[off[0]:off[0] + 12 * B].view(np.int32).reshape(B, 3).copy()
    iou = raw[off[1]:off[1] + 4 * B * N].view(np.float32).reshape(B, N).copy()
    arr = [raw[off[k]:off[k] + 4 * B * N].view(np.int32).reshape(B, N) for k in (2, 3, 4, 5)]
    lists = [[arr[1 + l][b, :counts[b, l]].copy() for l in range(3)] for b in range(B)]
    return counts, iou, arr[0].copy(), lists


def roi_targets_sample(picks, rois, roi_scores, roi_labels, gt_boxes, reg_fg_thresh, cls_fg_thresh, cls_bg_thresh, score_type,
                       workspace):
    """modest_roi_targets_sample on PyTorch's current stream: enqueue only.  picks (B, M, 2) int32, pinned host or device
    memory -> the eight outputs as a dict in the reference's key order.  A pinned table is read by the kernel through its
    raw pointer, which PyTorch's host allocator does not see: the caller keeps it alive and unwritten until the stream has
    passed this call (a freed pinned block can be handed out and overwritten before the kernel has read it).  A device
    table is held by PyTorch's allocator in stream order and may be dropped at once."""
    B, N, cols = (int(v) for v in rois.shape)
    G, M = int(gt_boxes.shape[1]), int(picks.shape[1])
    if picks.dtype != torch.int32 or picks.ndim != 3 or picks.shape[0] != B or picks.shape[2] != 2 or not picks.is_contiguous() \
            or not (picks.is_cuda or picks.is_pinned()):
        raise ValueError("picks must be a contiguous (B, M, 2) int32 tensor in pinned host or device memory")
    if score_type not in ROI_SCORE_TYPES:
        raise NotImplementedError(f"CLS_SCORE_TYPE {score_type!r}")
    _dev(rois, torch.float32, "rois"), _dev(roi_scores, torch.float32, "roi_scores"), _dev(roi_labels, torch.int64, "roi_labels")
    dev = rois.device
    f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    i = lambda *shape: torch.empty(shape, dtype=torch.int64, device=dev)
    out = {"rois": f(B, M, cols), "gt_of_rois": f(B, M, cols + 1), "gt_iou_of_rois": f(B, M), "roi_scores": f(B, M),
           "roi_labels": i(B, M), "reg_valid_mask": i(B, M), "rcnn_cls_labels": i(B, M) if score_type == "cls" else f(B, M),
           "gt_of_rois_src": f(B, M, cols + 1)}
    den = float(cls_fg_thresh) - float(cls_bg_thresh)      # in double, rounded once by the float argument
    with torch.cuda.device(dev):
        check(load().modest_roi_targets_sample(B, N, G, M, picks.data_ptr(), rois.data_ptr() if B * N else None, cols,
                                               roi_scores.data_ptr() if B * N else None,
                                               roi_labels.data_ptr() if B * N else None,
                                               gt_boxes.data_ptr() if B * G else None, *(int(s) for s in gt_boxes.stride()),
                                               float(reg_fg_thresh), float(cls_fg_thresh), float(cls_bg_thresh), den,
                                               ROI_SCORE_TYPES[score_type], workspace.data_ptr(), workspace.numel(),
                                               out["rois"].data_ptr(), out["gt_of_rois"].data_ptr(),
                                               out["gt_iou_of_rois"].data_ptr(), out["roi_scores"].data_ptr(),
                                               out["roi_labels"].data_ptr(), out["reg_valid_mask"].data_ptr(),
                                               out["rcnn_cls_labels"].data_ptr(), out["gt_of_rois_src"].data_ptr(), _stream()),
              "modest_roi_targets_sample")
    return out


def roi_targets(rois: torch.Tensor, roi_scores: torch.Tensor, roi_labels: torch.Tensor, gt_boxes: torch.Tensor, cfg, *,
                np_random=None, generator=None, workspace: Optional[torch.Tensor] = None,
                counts_pinned: Optional[torch.Tensor] = None, picks_pinned: Optional[torch.Tensor] = None):
    """RoIHeadTemplate.assign_targets of a batch on PyTorch's current stream: modest_roi_targets_match (one synchronise: the
    list lengths reach the host), the reference's draws per sample from numpy's and torch's CPU generators (the global ones
    when np_random / generator are None), modest_roi_targets_sample.  cfg: the TARGET_CONFIG (attributes or a dict).
    rois (B, N, 7 + C), roi_scores (B, N), roi_labels (B, N), gt_boxes (B, G, 7 + C + 1, any strides): device tensors;
    other floating types go through float32 and come back in rois' type.  -> the reference's dict of eight (B, M, .) tensors.
    workspace (uint8, device), counts_pinned (int32, pinned, 3 B words) and picks_pinned (int32, pinned, 2 B M words) are
    allocated when missing or too small.  Lifetime of picks_pinned: the sample kernel, which is only enqueued, reads the
    caller's table where it lies, so the caller keeps it alive and unwritten until the stream has passed this call's work
    (the next call here on the same stream may write it: its match call synchronises first); calls on several streams
    need a table each.  Without one the picks go through a pinned block and a device copy that PyTorch's allocators hold
    back by themselves, at the price of one small copy."""
    _roi_args(rois, roi_scores, roi_labels, gt_boxes)
    score_type = _cfg_get(cfg, "CLS_SCORE_TYPE")
    if score_type not in ROI_SCORE_TYPES:
        raise NotImplementedError(f"CLS_SCORE_TYPE {score_type!r}")
    B, N, cols = (int(v) for v in rois.shape)
    M = int(_cfg_get(cfg, "ROI_PER_IMAGE"))
    roi_targets_limits(B, cols, M, N, int(gt_boxes.shape[1]))
    dev, dtype = rois.device, rois.dtype
    r32 = rois.float().contiguous()
    s32 = roi_scores.float().contiguous()
    lab = roi_labels.long().contiguous()
    gt = gt_boxes if gt_boxes.dtype == torch.float32 else gt_boxes.float()
    workspace = _workspace(roi_targets_workspace_bytes(B, N), workspace, dev)
    if counts_pinned is None or counts_pinned.numel() < 3 * B:
        counts_pinned = torch.zeros((max(3 * B, 16),), dtype=torch.int32).pin_memory()
    if picks_pinned is not None and picks_pinned.numel() < 2 * B * M:
        picks_pinned = None
    reg_fg, cls_fg = _cfg_get(cfg, "REG_FG_THRESH"), _cfg_get(cfg, "CLS_FG_THRESH")
    counts = roi_targets_match(r32, lab, gt, min(reg_fg, cls_fg), _cfg_get(cfg, "CLS_BG_THRESH_LO"), reg_fg,
                               _cfg_get(cfg, "SAMPLE_ROI_BY_EACH_CLASS", False), workspace, counts_pinned).numpy()
    if picks_pinned is not None:
        # the caller's table, read by the sample kernel where it lies.  It may be written here: the match call above has
        # synchronised this stream, so the sample kernel of the call before on this stream has read it.  The caller keeps it
        # alive until this call's work on the stream is complete.
        staged = picks_pinned[:2 * B * M].view(B, M, 2)
    else:
        # a table of this call's own dies when the call returns, before the sample kernel need have started, and PyTorch's
        # host allocator knows nothing of a kernel that reads a block through its raw pointer: it would hand the block to the
        # next pin_memory().  So the kernel reads a device copy; the non-blocking copy records the event that holds the
        # pinned block back until it has been read, and the device copy is freed in stream order.
        staged = torch.empty((B, M, 2), dtype=torch.int32, pin_memory=True)
    table = staged.numpy()
    for b in range(B):
        table[b] = roi_target_draws(counts[b], cfg, np_random, generator, sample=b)
    picks = staged if picks_pinned is not None else staged.to(dev, non_blocking=True)
    out = roi_targets_sample(picks, r32, s32, lab, gt, reg_fg, cls_fg, _cfg_get(cfg, "CLS_BG_THRESH"), score_type, workspace)
    if dtype != torch.float32:
        for k in ("rois", "gt_of_rois", "gt_iou_of_rois", "roi_scores", "gt_of_rois_src"):
            out[k] = out[k].to(dtype)
        if score_type == "roi_iou":
            out["rcnn_cls_labels"] = out["rcnn_cls_labels"].to(dtype)
    if roi_labels.dtype != torch.int64:
        out["roi_labels"] = out["roi_labels"].to(roi_labels.dtype)
    return out


# --------------------------------------------------------------------------- post-processing
POST_PROCESS_THRESH_MAX = 16                # len(RECALL_THRESH_LIST): modest_post_process_max_thresholds()


def post_process_tile() -> int:
    """boxes of a list a recall workgroup stages in LDS at a time"""
    return int(load().modest_post_process_tile())


def post_process_workspace_bytes(n_rows: int, batch_size: int) -> int:
    return _workspace_bytes("modest_post_process_workspace_bytes", n_rows, batch_size)


def post_process_table_words(batch_size: int, n_thresh: int) -> int:
    """int32 words of the pinned table of a call: per sample its survivors, its valid gts, rcnn and roi counts per threshold"""
    return int(batch_size) * (2 + 2 * int(n_thresh))


def post_process(box_preds: torch.Tensor, cls_preds: torch.Tensor, batch_size: int, pre_maxsize: int, post_maxsize: int,
                 nms_thresh: float, *, rotated: bool = True, score_thresh: Optional[float] = None, normalized: bool = True,
                 output_raw_score: bool = False, labels: Optional[torch.Tensor] = None,
                 batch_index: Optional[torch.Tensor] = None, gt_boxes: Optional[torch.Tensor] = None,
                 rois: Optional[torch.Tensor] = None, recall_thresh=(), workspace: Optional[torch.Tensor] = None,
                 table: Optional[torch.Tensor] = None, out=None):
    """modest_post_process on PyTorch's current stream: BLOCKING (one synchronise, inside the library).
    box_preds / cls_preds / batch_index: the two forms of `proposals`, float32.  Per sample the rows whose score -- the class
    maximum, its sigmoid (the double function rounded once) unless `normalized` -- is >= score_thresh (None: all rows) are
    walked, the min(pre_maxsize, rows) highest first, by greedy NMS at nms_thresh up to the post_maxsize-th survivor.
    labels: (B, N) int64 given labels (dense form), else the class column + 1.  gt_boxes (B, G, 7 + C + 1) float32 of any
    strides switches the recall counters on; rois (B, R, 7 + C') float32 (dense form, needs gt_boxes) makes the "rcnn" list
    all rows of the sample and adds the "roi" list.
    -> (pred_boxes (B, post, 7 + C) float32, pred_scores (B, post) float32, pred_labels (B, post) int64, counts, recall):
    padded buffers, freshly allocated (or the three tensors of `out`), of which sample b's first counts[b] rows are written
    and the rest is not; counts a numpy (B,) int32 of the call's own; recall None without gt_boxes, else
    {"gt": int, "rcnn": [int per threshold], "roi": [int per threshold]} summed over the samples.
    workspace: uint8 device tensor of post_process_workspace_bytes(rows, B); table: pinned int32 tensor of
    post_process_table_words(B, len(recall_thresh)); both allocated when missing or too small.  A table serves one stream
    at a time: the kernels write it, and it is read here once the stream has been synchronised."""
    dev, B, per, kind, bidx, cols, K, box, cls, n, P = _ranked_rows(box_preds, cls_preds, batch_size, pre_maxsize, post_maxsize, batch_index,
                                                                    dense_only=labels is not None or rois is not None)
    if labels is not None:
        if not torch.is_tensor(labels) or labels.device != dev or labels.numel() != n:
            raise ValueError(f"labels must be a device tensor of (batch_size, N) = ({B}, {per}) elements")
        labels = labels.reshape(B, per).long().contiguous()
    thr = np.ascontiguousarray(np.asarray(list(recall_thresh), dtype=np.float64).astype(np.float32))   # as torch compares
    T = int(thr.size)
    if T > POST_PROCESS_THRESH_MAX:
        raise ValueError(f"RECALL_THRESH_LIST has {T} thresholds, above the limit of {POST_PROCESS_THRESH_MAX}")
    G, R, rcols = 0, -1, 7
    gt = None
    if gt_boxes is not None:
        if not torch.is_tensor(gt_boxes) or not gt_boxes.is_cuda or gt_boxes.dtype != torch.float32 or gt_boxes.device != dev:
            raise ValueError("gt_boxes must be a float32 device tensor on the boxes' device")
        if gt_boxes.ndim != 3 or gt_boxes.shape[0] != B or gt_boxes.shape[2] != cols + 1:
            raise ValueError(f"gt_boxes {tuple(gt_boxes.shape)} must be (batch_size = {B}, G, 7 + C + 1 = {cols + 1})")
        gt, G = gt_boxes, int(gt_boxes.shape[1])
    if rois is not None:
        if gt_boxes is None:
            rois = None          # read by the recall counters only
        else:
            if not torch.is_tensor(rois) or not rois.is_cuda or rois.dtype != torch.float32 or rois.device != dev:
                raise ValueError("rois must be a float32 device tensor on the boxes' device")
            if rois.ndim != 3 or rois.shape[0] != B or rois.shape[2] < 7:
                raise ValueError(f"rois {tuple(rois.shape)} must be (batch_size = {B}, R, 7 + C)")
            rois = rois.contiguous()
            R, rcols = int(rois.shape[1]), int(rois.shape[2])
    boxes, scores, labs = _outputs((("pred_boxes", torch.float32, (B, P, cols), True), ("pred_scores", torch.float32, (B, P), True),
                                    ("pred_labels", torch.int64, (B, P), True)), out, dev, anchor="box_preds")
    workspace = _workspace(post_process_workspace_bytes(n, B), workspace, dev)
    stride = 2 + 2 * T
    words = post_process_table_words(B, T)
    if table is None or table.numel() < words:
        table = torch.zeros((max(words, 16),), dtype=torch.int32).pin_memory()
    if not table.is_pinned() or table.dtype != torch.int32 or not table.is_contiguous():
        raise ValueError("table must be a contiguous pinned int32 tensor")
    ptr = _ptr_filled
    gs = tuple(int(s) for s in gt.stride()) if gt is not None else (0, 0, 0)
    with torch.cuda.device(dev):
        check(load().modest_post_process(n, B, per, ptr(box), cols, ptr(cls), K, _ptr(bidx), kind,
                                      int(bool(normalized)), int(score_thresh is not None),
                                      float(score_thresh) if score_thresh is not None else 0.0, int(bool(output_raw_score)),
                                      _ptr(labels), int(pre_maxsize), P, float(nms_thresh),
                                      int(bool(rotated)), int(gt is not None), G, ptr(gt), *gs, R, ptr(rois), rcols, T,
                                      _np_ptr(thr) if T else None, ptr(boxes), ptr(scores), ptr(labs), table.data_ptr(),
                                      workspace.data_ptr(), workspace.numel(), _stream()), "modest_post_process")
    tab = table[:words].view(B, stride).numpy().copy() if B else np.zeros((0, stride), np.int32)
    counts = np.ascontiguousarray(tab[:, 0]) if B else np.zeros((0,), np.int32)
    recall = None
    if gt is not None:
        tot = tab[:, 1:].astype(np.int64).sum(0)
        recall = {"gt": int(tot[0]), "rcnn": [int(v) for v in tot[1:1 + T]], "roi": [int(v) for v in tot[1 + T:1 + 2 * T]]}
    return boxes, scores, labs, counts, recall


# --------------------------------------------------------------------------- what the three head losses share
def _loss_out(want, out, dev):
    """`want`: (name, shape, needed) per buffer -> the float32 buffers on `dev`, None where none is needed (`_outputs`)"""
    return _outputs([(name, torch.float32, shape, bool(need)) for name, shape, need in want], out, dev,
                    absent=("must be None", "must be a tensor"))


def _loss_backward(fn_name: str, names, grads, upstream: torch.Tensor):
    """`fn_name` on PyTorch's current stream: the gradient buffers `grads` (`names`; None where a term is absent) times the
    float32 device scalar `upstream`, IN PLACE, enqueue only.  -> grads"""
    if not torch.is_tensor(upstream) or not upstream.is_cuda or upstream.dtype != torch.float32 or upstream.numel() != 1:
        raise ValueError("upstream must be a float32 device tensor of one element")
    if len(grads) != len(names):
        raise ValueError(f"grads must be ({', '.join(names)})")
    for g in grads:
        if g is not None:
            _dev(g, torch.float32, "a gradient buffer")
            if g.device != upstream.device:
                raise ValueError("the gradient buffers and upstream are on different devices")
    with torch.cuda.device(upstream.device):
        check(getattr(load(), fn_name)(*(int(g.numel()) if g is not None else 0 for g in grads),
                                       *(g.data_ptr() if g is not None else None for g in grads),
                                       upstream.data_ptr(), _stream()), fn_name)
    return grads


# --------------------------------------------------------------------------- anchor-head loss
ANCHOR_LOSS_MAX_CLASS = 32      # class columns of an anchor
ANCHOR_LOSS_MAX_CODE = 16       # box code columns
ANCHOR_LOSS_MAX_BINS = 8        # NUM_DIR_BINS
ANCHOR_LOSS_MAX_BATCH = 65535   # samples per call: the grid's second dimension


def anchor_loss_workspace_bytes(batch_size: int, n_anchors: int) -> int:
    return _workspace_bytes("modest_anchor_loss_workspace_bytes", batch_size, n_anchors)


def anchor_loss(cls_preds: torch.Tensor, box_preds: torch.Tensor, dir_preds: Optional[torch.Tensor], labels: torch.Tensor,
                reg_targets: torch.Tensor, anchors: torch.Tensor, code_weights: torch.Tensor, *, beta: float = 1.0 / 9.0,
                dir_offset: float = 0.0, cls_weight: float = 1.0, loc_weight: float = 1.0, dir_weight: float = 1.0,
                alpha: float = 0.25, gamma: float = 2.0, want_grad: bool = True, workspace: Optional[torch.Tensor] = None,
                out=None):
    """modest_anchor_loss on PyTorch's current stream: enqueue only, nothing is read back.
    cls_preds (B, N, C), box_preds (B, N, code), dir_preds (B, N, bins) or None: float32 device tensors, made contiguous when
    they are not; labels (B, N) int32 or int64; reg_targets (B, N, code), anchors (N, >= 7), code_weights (code): float32,
    contiguous.  The scalars are rounded to float32, as torch rounds a Python scalar that meets a float32 tensor.
    -> (losses (4) float32 [rpn_loss_cls, rpn_loss_loc, rpn_loss_dir, rpn_loss], grads): grads is None without want_grad, else
    (grad_cls, grad_box, grad_dir or None) of the predictions' shapes, d rpn_loss / d prediction, every element written.
    `out` = (losses, grad_cls, grad_box, grad_dir) supplies the buffers (the gradients None without want_grad)."""
    dev = _device_tensors((("cls_preds", cls_preds), ("box_preds", box_preds), ("dir_preds", dir_preds), ("labels", labels),
                           ("reg_targets", reg_targets), ("anchors", anchors), ("code_weights", code_weights)),
                          dtypes={"labels": (torch.int32, torch.int64)}, optional=("dir_preds",), dtype_error=TypeError)
    if cls_preds.ndim != 3 or box_preds.ndim != 3 or cls_preds.shape[:2] != box_preds.shape[:2]:
        raise ValueError(f"cls_preds {tuple(cls_preds.shape)} and box_preds {tuple(box_preds.shape)} must be (B, N, C) and (B, N, code)")
    B, N, K = (int(v) for v in cls_preds.shape)
    code = int(box_preds.shape[2])
    bins = 0
    if dir_preds is not None:
        if dir_preds.ndim != 3 or tuple(dir_preds.shape[:2]) != (B, N):
            raise ValueError(f"dir_preds {tuple(dir_preds.shape)} must be (B, N, bins) = ({B}, {N}, bins)")
        bins = int(dir_preds.shape[2])
    if tuple(labels.shape) != (B, N) or tuple(reg_targets.shape) != (B, N, code):
        raise ValueError(f"labels {tuple(labels.shape)} and reg_targets {tuple(reg_targets.shape)} must be ({B}, {N}) and ({B}, {N}, {code})")
    if anchors.ndim != 2 or anchors.shape[0] != N or anchors.shape[1] < 7:
        raise ValueError(f"anchors {tuple(anchors.shape)} must be (N, >= 7) = ({N}, >= 7), not repeated over the batch")
    if tuple(code_weights.shape) != (code,):
        raise ValueError(f"code_weights {tuple(code_weights.shape)} must be (code,) = ({code},)")
    if K < 1 or K > ANCHOR_LOSS_MAX_CLASS:
        raise ValueError(f"num_class = {K} is outside the limit of 1 .. {ANCHOR_LOSS_MAX_CLASS} class columns")
    if code < 7 or code > ANCHOR_LOSS_MAX_CODE:
        raise ValueError(f"code size = {code} is outside the limit of 7 .. {ANCHOR_LOSS_MAX_CODE} box columns")
    if dir_preds is not None and (bins < 1 or bins > ANCHOR_LOSS_MAX_BINS):
        raise ValueError(f"NUM_DIR_BINS = {bins} is outside the limit of 1 .. {ANCHOR_LOSS_MAX_BINS} direction bins")
    if B < 1 or B > ANCHOR_LOSS_MAX_BATCH:
        raise ValueError(f"batch_size = {B} is outside the limit of 1 .. {ANCHOR_LOSS_MAX_BATCH} samples per call")
    if float(gamma) != 2.0:
        raise ValueError(f"gamma = {gamma}: only gamma = 2 is provided (the focal power is the product pt * pt)")
    for t, name in ((labels, "labels"), (reg_targets, "reg_targets"), (anchors, "anchors"), (code_weights, "code_weights")):
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        if t.device != dev:
            raise ValueError(f"{name} is on {t.device}, cls_preds on {dev}")
    cls, box = cls_preds.contiguous(), box_preds.contiguous()
    dirp = dir_preds.contiguous() if dir_preds is not None else None
    losses, gcls, gbox, gdir = _loss_out((("losses", (4,), True), ("grad_cls", (B, N, K), want_grad), ("grad_box", (B, N, code), want_grad),
                                          ("grad_dir", (B, N, bins), want_grad and dirp is not None)), out, dev)
    workspace = _workspace(anchor_loss_workspace_bytes(B, N), workspace, dev)
    ptr = _ptr
    with torch.cuda.device(dev):
        check(load().modest_anchor_loss(B, N, K, code, bins, ptr(cls), ptr(box), ptr(dirp), ptr(labels),
                                        int(labels.dtype == torch.int64), ptr(reg_targets), ptr(anchors), int(anchors.shape[1]),
                                        ptr(code_weights), float(beta), float(dir_offset), float(cls_weight), float(loc_weight),
                                        float(dir_weight), float(alpha), float(gamma), ptr(losses), ptr(gcls), ptr(gbox),
                                        ptr(gdir), workspace.data_ptr(), workspace.numel(), _stream()), "modest_anchor_loss")
    return losses, ((gcls, gbox, gdir) if want_grad else None)


def anchor_loss_backward(grads, upstream: torch.Tensor):
    """modest_anchor_loss_backward on PyTorch's current stream: the gradient buffers of `anchor_loss` (grad_dir may be None)
    times the float32 device scalar `upstream`, IN PLACE, enqueue only.  -> grads"""
    return _loss_backward("modest_anchor_loss_backward", ("grad_cls", "grad_box", "grad_dir"), grads, upstream)


# --------------------------------------------------------------------------- RoI-head loss
ROI_LOSS_MAX_ROWS = 1 << 20     # R = B x ROI_PER_IMAGE: every workgroup counts over all rows
ROI_LOSS_MIN_CODE = 7           # box code columns
ROI_LOSS_MAX_CODE = 16
ROI_LOSS_TABLE = ("rcnn_loss_cls", "rcnn_loss_reg", "rcnn_loss_corner", "rcnn_loss", "fg_sum", "cls_valid")
_ROI_LOSS_LABELS = {torch.int32: 0, torch.int64: 1, torch.float32: 2}


def roi_loss_workspace_bytes(n_rows: int) -> int:
    return _workspace_bytes("modest_roi_loss_workspace_bytes", n_rows)


def roi_loss(rcnn_cls: torch.Tensor, rcnn_reg: torch.Tensor, rcnn_cls_labels: torch.Tensor, reg_valid_mask: torch.Tensor,
             gt_of_rois: torch.Tensor, gt_of_rois_src: torch.Tensor, rois: torch.Tensor, code_weights: torch.Tensor, *,
             beta: float = 1.0 / 9.0, cls_weight: float = 1.0, reg_weight: float = 1.0, corner_weight: float = 1.0,
             corner: bool = True, want_grad: bool = True, workspace: Optional[torch.Tensor] = None, out=None):
    """modest_roi_loss on PyTorch's current stream: enqueue only, nothing is read back.
    rcnn_cls (R) or (R, 1) logits and rcnn_reg (R, code): float32 device tensors, made contiguous when they are not;
    rcnn_cls_labels (R) int32, int64 or float32 (a row counts iff label >= 0); reg_valid_mask (R) int32 or int64 (foreground
    iff > 0); gt_of_rois and gt_of_rois_src (R, >= code) float32 with unit column stride, read through their row strides;
    rois (R, code) and code_weights (code) float32, contiguous.  The scalars are rounded to float32, as torch rounds a Python
    scalar that meets a float32 tensor.
    -> (table (6) float32 [rcnn_loss_cls, rcnn_loss_reg, rcnn_loss_corner, rcnn_loss, fg_sum, cls_valid], grads): grads is None
    without want_grad, else (grad_cls (R), grad_reg (R, code)), d rcnn_loss / d prediction, every element written.
    `out` = (table, grad_cls, grad_reg) supplies the buffers (the gradients None without want_grad)."""
    named = (("rcnn_cls", rcnn_cls), ("rcnn_reg", rcnn_reg), ("rcnn_cls_labels", rcnn_cls_labels), ("reg_valid_mask", reg_valid_mask),
             ("gt_of_rois", gt_of_rois), ("gt_of_rois_src", gt_of_rois_src), ("rois", rois), ("code_weights", code_weights))
    dev = _device_tensors(named, dtypes={"rcnn_cls_labels": tuple(_ROI_LOSS_LABELS), "reg_valid_mask": (torch.int32, torch.int64)},
                          dtype_error=TypeError)
    if rcnn_reg.ndim != 2:
        raise ValueError(f"rcnn_reg {tuple(rcnn_reg.shape)} must be (R, code)")
    R, code = (int(v) for v in rcnn_reg.shape)
    if code < ROI_LOSS_MIN_CODE or code > ROI_LOSS_MAX_CODE:
        raise ValueError(f"code size = {code} is outside the limit of {ROI_LOSS_MIN_CODE} .. {ROI_LOSS_MAX_CODE} box columns")
    if R > ROI_LOSS_MAX_ROWS:
        raise ValueError(f"rcnn_reg has {R} rows, above the limit of {ROI_LOSS_MAX_ROWS} rows per call")
    if rcnn_cls.numel() != R:
        raise ValueError(f"rcnn_cls has {rcnn_cls.numel()} elements, rcnn_reg {R} rows")
    for name, t in (("rcnn_cls_labels", rcnn_cls_labels), ("reg_valid_mask", reg_valid_mask)):
        if tuple(t.shape) != (R,) or not t.is_contiguous():
            raise ValueError(f"{name} {tuple(t.shape)} must be a contiguous ({R},)")
    for name, t in (("gt_of_rois", gt_of_rois), ("gt_of_rois_src", gt_of_rois_src)):
        if t.ndim != 2 or t.shape[0] != R or t.shape[1] < code:
            raise ValueError(f"{name} {tuple(t.shape)} must be (R, >= code) = ({R}, >= {code})")
        if R and (t.stride(1) != 1 or (R > 1 and t.stride(0) < code)):
            raise ValueError(f"{name} must have unit column stride and a row stride of at least {code}, got strides {tuple(t.stride())}")
    if tuple(rois.shape) != (R, code) or not rois.is_contiguous():
        raise ValueError(f"rois {tuple(rois.shape)} must be a contiguous (R, code) = ({R}, {code})")
    if tuple(code_weights.shape) != (code,) or not code_weights.is_contiguous():
        raise ValueError(f"code_weights {tuple(code_weights.shape)} must be a contiguous (code,) = ({code},)")
    for name, t in named[1:]:
        if t.device != dev:
            raise ValueError(f"{name} is on {t.device}, rcnn_cls on {dev}")
    cls, reg = rcnn_cls.reshape(-1).contiguous(), rcnn_reg.contiguous()
    table, gcls, greg = _loss_out((("table", (6,), True), ("grad_cls", (R,), want_grad), ("grad_reg", (R, code), want_grad)), out, dev)
    workspace = _workspace(roi_loss_workspace_bytes(R), workspace, dev)
    ptr = _ptr
    stride = lambda t: int(t.stride(0)) if R > 1 else int(t.shape[1])      # noqa: E731
    with torch.cuda.device(dev):
        check(load().modest_roi_loss(R, code, ptr(cls), ptr(reg), ptr(rcnn_cls_labels), _ROI_LOSS_LABELS[rcnn_cls_labels.dtype],
                                     ptr(reg_valid_mask), int(reg_valid_mask.dtype == torch.int64), ptr(gt_of_rois),
                                     stride(gt_of_rois), ptr(gt_of_rois_src), stride(gt_of_rois_src), ptr(rois),
                                     ptr(code_weights), float(beta), float(cls_weight), float(reg_weight), float(corner_weight),
                                     int(bool(corner)), ptr(table), ptr(gcls), ptr(greg), workspace.data_ptr(),
                                     workspace.numel(), _stream()), "modest_roi_loss")
    return table, ((gcls, greg) if want_grad else None)


def roi_loss_backward(grads, upstream: torch.Tensor):
    """modest_roi_loss_backward on PyTorch's current stream: the two gradient buffers of `roi_loss` times the float32 device
    scalar `upstream`, IN PLACE, enqueue only.  -> grads"""
    return _loss_backward("modest_roi_loss_backward", ("grad_cls", "grad_reg"), grads, upstream)


# --------------------------------------------------------------------------- point-head loss
POINT_LOSS_MAX_ROWS = 1 << 24   # N of the stacked batch: the count of positives stays exact in float32
POINT_LOSS_MAX_CLASS = 32       # class columns of a point
POINT_LOSS_MAX_CODE = 16        # box code columns
POINT_LOSS_PART = 3             # intra-object part columns
POINT_LOSS_TABLE = ("point_loss_cls", "point_loss_part", "point_loss_box", "point_loss", "point_pos_num")


def point_loss_workspace_bytes(n_rows: int) -> int:
    return _workspace_bytes("modest_point_loss_workspace_bytes", n_rows)


def point_loss(cls_preds: torch.Tensor, labels: torch.Tensor, part_preds: Optional[torch.Tensor] = None,
               part_labels: Optional[torch.Tensor] = None, box_preds: Optional[torch.Tensor] = None,
               box_labels: Optional[torch.Tensor] = None, code_weights: Optional[torch.Tensor] = None, *,
               beta: float = 1.0 / 9.0, cls_weight: float = 1.0, part_weight: float = 1.0, box_weight: float = 1.0,
               want_grad: bool = True, workspace: Optional[torch.Tensor] = None, out=None):
    """modest_point_loss on PyTorch's current stream: enqueue only, nothing is read back.
    cls_preds (N, C) or (B, n, C) logits, part_preds (.., 3) with part_labels, box_preds (.., code) with box_labels and
    code_weights (code): float32 device tensors; a term whose tensors are None is absent.  Predictions and their labels are
    flattened to rows (a copy only where the strides demand one); labels (N elements) int32 or int64, contiguous.  The scalars
    are rounded to float32, as torch rounds a Python scalar that meets a float32 tensor.
    -> (table (5) float32 [point_loss_cls, point_loss_part, point_loss_box, point_loss, point_pos_num], grads): grads is None
    without want_grad, else (grad_cls (N, C), grad_part (N, 3) or None, grad_box (N, code) or None), d point_loss / d
    prediction, every element written.  `out` = (table, grad_cls, grad_part, grad_box) supplies the buffers (None where no
    buffer is due)."""
    with_part, with_box = part_preds is not None, box_preds is not None
    if with_part != (part_labels is not None):
        raise ValueError("part_preds and part_labels come together")
    if with_box != (box_labels is not None) or with_box != (code_weights is not None):
        raise ValueError("box_preds, box_labels and code_weights come together")
    named = (("cls_preds", cls_preds), ("labels", labels), ("part_preds", part_preds), ("part_labels", part_labels),
             ("box_preds", box_preds), ("box_labels", box_labels), ("code_weights", code_weights))
    dev = _device_tensors(named, dtypes={"labels": (torch.int32, torch.int64)}, optional=[name for name, _ in named[2:]],
                          dtype_error=TypeError)
    if cls_preds.ndim < 2:
        raise ValueError(f"cls_preds {tuple(cls_preds.shape)} must be (N, num_class) or (B, n, num_class)")
    K = int(cls_preds.shape[-1])
    if K < 1 or K > POINT_LOSS_MAX_CLASS:
        raise ValueError(f"num_class = {K} is outside the limit of 1 .. {POINT_LOSS_MAX_CLASS} class columns")
    N = int(labels.numel())
    if N > POINT_LOSS_MAX_ROWS:
        raise ValueError(f"labels has {N} rows, above the limit of {POINT_LOSS_MAX_ROWS} rows per call")
    if cls_preds.numel() != N * K:
        raise ValueError(f"cls_preds has {cls_preds.numel()} elements, expected {N} rows of {K} classes")
    code = 0
    if with_box:
        if box_preds.ndim < 2:
            raise ValueError(f"box_preds {tuple(box_preds.shape)} must be (N, code) or (B, n, code)")
        code = int(box_preds.shape[-1])
        if code < 1 or code > POINT_LOSS_MAX_CODE:
            raise ValueError(f"code size = {code} is outside the limit of 1 .. {POINT_LOSS_MAX_CODE} box columns")
        for name, t in (("box_preds", box_preds), ("box_labels", box_labels)):
            if t.numel() != N * code:
                raise ValueError(f"{name} has {t.numel()} elements, expected {N} rows of code size {code}")
        if tuple(code_weights.shape) != (code,) or not code_weights.is_contiguous():
            raise ValueError(f"code_weights {tuple(code_weights.shape)} must be a contiguous (code,) = ({code},)")
    if with_part:
        for name, t in (("part_preds", part_preds), ("part_labels", part_labels)):
            if t.numel() != N * POINT_LOSS_PART:
                raise ValueError(f"{name} has {t.numel()} elements, expected {N} rows of {POINT_LOSS_PART} columns")
    for name, t in named[1:]:
        if t is not None and t.device != dev:
            raise ValueError(f"{name} is on {t.device}, cls_preds on {dev}")
    rows = lambda t, c: t.reshape(-1, c).contiguous() if t is not None else None      # noqa: E731
    cls, labels = rows(cls_preds, K), labels.reshape(-1).contiguous()
    part, part_t = rows(part_preds, POINT_LOSS_PART), rows(part_labels, POINT_LOSS_PART)
    box, box_t = rows(box_preds, max(code, 1)), rows(box_labels, max(code, 1))
    table, gcls, gpart, gbox = _loss_out((("table", (5,), True), ("grad_cls", (N, K), want_grad),
                                          ("grad_part", (N, POINT_LOSS_PART), want_grad and with_part),
                                          ("grad_box", (N, code), want_grad and with_box)), out, dev)
    workspace = _workspace(point_loss_workspace_bytes(N), workspace, dev)
    ptr = _ptr
    with torch.cuda.device(dev):
        check(load().modest_point_loss(N, K, code, ptr(cls), ptr(labels), int(labels.dtype == torch.int64), ptr(part), ptr(part_t),
                                       ptr(box), ptr(box_t), ptr(code_weights), float(beta), float(cls_weight), float(part_weight),
                                       float(box_weight), ptr(gcls), ptr(gpart), ptr(gbox), ptr(table), workspace.data_ptr(),
                                       workspace.numel(), _stream()), "modest_point_loss")
    return table, ((gcls, gpart, gbox) if want_grad else None)


def point_loss_backward(grads, upstream: torch.Tensor):
    """modest_point_loss_backward on PyTorch's current stream: the gradient buffers of `point_loss` (grad_part and grad_box
    may be None) times the float32 device scalar `upstream`, IN PLACE, enqueue only.  -> grads"""
    return _loss_backward("modest_point_loss_backward", ("grad_cls", "grad_part", "grad_box"), grads, upstream)


# --------------------------------------------------------------------------- box decoding
BOX_DECODE_MAX_ROWS = (1 << 31) - 1   # rows per call (B * N for the anchor head): a row index is an int, element offsets int64
BOX_DECODE_MAX_CODE = 16              # box code columns
BOX_DECODE_MAX_BINS = 8               # direction bins
BOX_DECODE_MAX_CLASS = 32             # class columns of a point


def _decode_out(out, shape, dev):      # one buffer, refused in one message of its own: not a call of _outputs
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=dev)
    if (not torch.is_tensor(out) or out.dtype != torch.float32 or tuple(out.shape) != tuple(shape) or out.device != dev
            or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous float32 {tuple(shape)} tensor on {dev}")
    return out


def _decode_code(code: int, low: int, what: str = "code size"):
    if code < low or code > BOX_DECODE_MAX_CODE:
        raise ValueError(f"{what} = {code} is outside the limit of {low} .. {BOX_DECODE_MAX_CODE} box columns")


def _decode_rows(rows: int, name: str):
    if rows > BOX_DECODE_MAX_ROWS:
        raise ValueError(f"{name} has {rows} rows, above the limit of {BOX_DECODE_MAX_ROWS} rows per call")


def anchor_decode(box_preds: torch.Tensor, anchors: torch.Tensor, dir_cls_preds: Optional[torch.Tensor] = None, *,
                  dir_offset: float = 0.0, dir_limit_offset: float = 0.0, sincos: bool = False, out=None) -> torch.Tensor:
    """modest_anchor_decode on PyTorch's current stream: enqueue only, nothing is read back.
    box_preds (B, N, code), anchors (N, 7 + C) with code = 7 + C (8 + C with sincos), dir_cls_preds (B, N, bins) or None:
    contiguous float32 device tensors; the anchors are read once per row for every sample.  The scalars are rounded to float32,
    as torch rounds a Python scalar that meets a float32 tensor.
    -> boxes (B, N, 7 + C) float32 (`out` supplies it), every element written"""
    dev = _device_tensors((("box_preds", box_preds), ("anchors", anchors), ("dir_cls_preds", dir_cls_preds)),
                          optional=("dir_cls_preds",), dtype_error=TypeError, same_device=True)
    if box_preds.ndim != 3 or anchors.ndim != 2:
        raise ValueError(f"box_preds {tuple(box_preds.shape)} must be (B, N, code) and anchors {tuple(anchors.shape)} (N, 7 + C)")
    B, N, code = (int(v) for v in box_preds.shape)
    _decode_code(code, 8 if sincos else 7)
    cols = code - 1 if sincos else code
    if tuple(anchors.shape) != (N, cols):
        raise ValueError(f"anchors {tuple(anchors.shape)} must be (N, columns) = ({N}, {cols}) for a code size of {code}"
                         + (" with sincos" if sincos else ""))
    _decode_rows(B * N, "box_preds")
    bins = 0
    if dir_cls_preds is not None:
        if dir_cls_preds.ndim != 3 or tuple(dir_cls_preds.shape[:2]) != (B, N):
            raise ValueError(f"dir_cls_preds {tuple(dir_cls_preds.shape)} must be (B, N, bins) = ({B}, {N}, bins)")
        bins = int(dir_cls_preds.shape[2])
        if bins < 1 or bins > BOX_DECODE_MAX_BINS:
            raise ValueError(f"NUM_DIR_BINS = {bins} is outside the limit of 1 .. {BOX_DECODE_MAX_BINS} direction bins")
    for name, t in (("box_preds", box_preds), ("anchors", anchors), ("dir_cls_preds", dir_cls_preds)):
        if t is not None and not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous, got strides {tuple(t.stride())}")
    boxes = _decode_out(out, (B, N, cols), dev)
    ptr = _ptr
    with torch.cuda.device(dev):
        check(load().modest_anchor_decode(B, N, code, int(bool(sincos)), ptr(box_preds), ptr(anchors), ptr(dir_cls_preds), bins,
                                          float(dir_offset), float(dir_limit_offset), ptr(boxes), _stream()), "modest_anchor_decode")
    return boxes


def point_decode(point_box_preds: torch.Tensor, points: torch.Tensor, point_cls_preds: torch.Tensor,
                 mean_size: Optional[torch.Tensor] = None, *, out=None) -> torch.Tensor:
    """modest_point_decode on PyTorch's current stream: enqueue only, nothing is read back.
    point_box_preds (N, 8 + C) and point_cls_preds (N, K) contiguous; points (N, 3) with unit column stride and any row stride
    of at least 3 (the view point_coords[:, 1:4] is read in place); mean_size (K, 3) contiguous, or None for use_mean_size =
    False: float32 device tensors.
    -> boxes (N, 7 + C) float32 (`out` supplies it), every element written"""
    dev = _device_tensors((("point_box_preds", point_box_preds), ("points", points), ("point_cls_preds", point_cls_preds),
                           ("mean_size", mean_size)), optional=("mean_size",), dtype_error=TypeError, same_device=True)
    if point_box_preds.ndim != 2 or point_cls_preds.ndim != 2 or points.ndim != 2:
        raise ValueError(f"point_box_preds {tuple(point_box_preds.shape)}, point_cls_preds {tuple(point_cls_preds.shape)} and "
                         f"points {tuple(points.shape)} must be (N, 8 + C), (N, K) and (N, 3)")
    N, code = (int(v) for v in point_box_preds.shape)
    _decode_code(code, 8)
    K = int(point_cls_preds.shape[1])
    if K < 1 or K > BOX_DECODE_MAX_CLASS:
        raise ValueError(f"num_class = {K} is outside the limit of 1 .. {BOX_DECODE_MAX_CLASS} class columns")
    _decode_rows(N, "point_box_preds")
    if int(point_cls_preds.shape[0]) != N:
        raise ValueError(f"point_cls_preds has {int(point_cls_preds.shape[0])} rows, point_box_preds {N}")
    if tuple(points.shape) != (N, 3):
        raise ValueError(f"points {tuple(points.shape)} must be (N, 3) = ({N}, 3)")
    if N and (points.stride(1) != 1 or (N > 1 and points.stride(0) < 3)):
        raise ValueError(f"points must have unit column stride and a row stride of at least 3, got strides {tuple(points.stride())}")
    if mean_size is not None and (tuple(mean_size.shape) != (K, 3) or not mean_size.is_contiguous()):
        raise ValueError(f"mean_size {tuple(mean_size.shape)} must be a contiguous (num_class, 3) = ({K}, 3)")
    for name, t in (("point_box_preds", point_box_preds), ("point_cls_preds", point_cls_preds)):
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous, got strides {tuple(t.stride())}")
    boxes = _decode_out(out, (N, code - 1), dev)
    stride = int(points.stride(0)) if N > 1 else 3
    with torch.cuda.device(dev):
        check(load().modest_point_decode(N, code, K, point_box_preds.data_ptr(), points.data_ptr(), stride,
                                         point_cls_preds.data_ptr(), mean_size.data_ptr() if mean_size is not None else None,
                                         boxes.data_ptr(), _stream()), "modest_point_decode")
    return boxes


def roi_decode(rois: torch.Tensor, box_preds: torch.Tensor, *, out=None) -> torch.Tensor:
    """modest_roi_decode on PyTorch's current stream: enqueue only, nothing is read back.
    rois (R, code) or (B, M, code) and box_preds (R, code) or (B, M, code), contiguous float32 device tensors with the same
    number of rows; neither is written.
    -> boxes (R, code) float32 (`out` supplies it), every element written"""
    dev = _device_tensors((("rois", rois), ("box_preds", box_preds)), dtype_error=TypeError, same_device=True)
    if rois.ndim < 2 or box_preds.ndim < 2:
        raise ValueError(f"rois {tuple(rois.shape)} and box_preds {tuple(box_preds.shape)} must be (R, code) or (B, M, code)")
    code = int(box_preds.shape[-1])
    _decode_code(code, 7)
    R = box_preds.numel() // code
    _decode_rows(R, "box_preds")
    if int(rois.shape[-1]) != code or rois.numel() != R * code:
        raise ValueError(f"rois {tuple(rois.shape)} must hold {R} rows of the code size {code}")
    for name, t in (("rois", rois), ("box_preds", box_preds)):
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous, got strides {tuple(t.stride())}")
    boxes = _decode_out(out, (R, code), dev)
    with torch.cuda.device(dev):
        check(load().modest_roi_decode(R, code, rois.data_ptr(), box_preds.data_ptr(), boxes.data_ptr(), _stream()),
              "modest_roi_decode")
    return boxes


# --------------------------------------------------------------------------- PillarVFE and the BEV scatter
PILLAR_MAX_CHANNELS = 64              # output channels: a lane each
PILLAR_MAX_FEATURES = 16              # K, the features of a point
PILLAR_MAX_SLOTS = 255                # the winner is a byte
PILLAR_MAX_ROWS = (1 << 31) - 1       # P * S
PILLAR_MAX_BATCH = 65535
PILLAR_XYZ, PILLAR_CLUSTER, PILLAR_CENTER, PILLAR_DIST = 1, 2, 4, 8      # the parts of a feature row
_PILLAR_CODES = {torch.float32: 0, torch.int32: 1, torch.int64: 2}      # the dtype codes of voxel_num_points and voxel_coords


def pillar_vfe_run() -> int:
    """pillars whose rows one wavefront sums: the first seam of the partial-sum tree"""
    return int(load().modest_pillar_vfe_run())


def pillar_vfe_group() -> int:
    """wavefront partials one group sums: the second seam lies at pillar_vfe_run() * pillar_vfe_group() pillars"""
    return int(load().modest_pillar_vfe_group())


def pillar_features(point_features: int, parts: int) -> int:
    """K, the features of a point, for voxels of `point_features` columns and the mask `parts`"""
    return ((point_features if parts & PILLAR_XYZ else point_features - 3) + (3 if parts & PILLAR_CLUSTER else 0)
            + (3 if parts & PILLAR_CENTER else 0) + (1 if parts & PILLAR_DIST else 0))


def _pillar_inputs(voxels, num_points, coords, weight, parts, extra=()):
    """the checks pillar_vfe and pillar_vfe_backward share -> (dev, P, S, Cp, C, K)"""
    index = (torch.float32, torch.int32, torch.int64)
    named = (("voxels", voxels), ("voxel_num_points", num_points), ("voxel_coords", coords), ("weight", weight)) + tuple(extra)
    dev = _device_tensors(named, dtypes={"voxel_num_points": index, "voxel_coords": index, "winner": (torch.uint8,),
                                         "sums": (torch.float64,), "num_batches_tracked": (torch.int64,)},
                          optional=[name for name, _ in extra], dtype_error=TypeError, same_device=True)
    if voxels.ndim != 3 or weight.ndim != 2:
        raise ValueError(f"voxels {tuple(voxels.shape)} must be (P, S, point features) and weight {tuple(weight.shape)} (C, K)")
    P, S, Cp = (int(v) for v in voxels.shape)
    C, K = (int(v) for v in weight.shape)
    parts = int(parts)
    if parts < 0 or parts > 15 or Cp < 3:
        raise ValueError(f"parts = {parts} must be a mask of 1 | 2 | 4 | 8 and voxels need at least 3 point features, got {Cp}")
    if C < 1 or C > PILLAR_MAX_CHANNELS:
        raise ValueError(f"C = {C} output channels is outside the limit of 1 .. {PILLAR_MAX_CHANNELS}")
    if K < 1 or K > PILLAR_MAX_FEATURES:
        raise ValueError(f"K = {K} features of a point is outside the limit of 1 .. {PILLAR_MAX_FEATURES}")
    if pillar_features(Cp, parts) != K:
        raise ValueError(f"weight has K = {K} columns, voxels of {Cp} point features with parts = {parts} make {pillar_features(Cp, parts)}")
    if S < 1 or S > PILLAR_MAX_SLOTS:
        raise ValueError(f"S = {S} slots of a pillar is outside the limit of 1 .. {PILLAR_MAX_SLOTS}")
    if P * S > PILLAR_MAX_ROWS:
        raise ValueError(f"voxels has P * S = {P * S} rows, above the limit of {PILLAR_MAX_ROWS} rows per call")
    if tuple(num_points.shape) != (P,) or tuple(coords.shape) != (P, 4):
        raise ValueError(f"voxel_num_points {tuple(num_points.shape)} and voxel_coords {tuple(coords.shape)} must be ({P},) and ({P}, 4)")
    for name, t in named:
        if t is not None and not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous, got strides {tuple(t.stride())}")
    return dev, P, S, Cp, C, K


def _pillar_geometry(voxel_size, offsets):
    if len(voxel_size) != 3 or len(offsets) != 3:
        raise ValueError("voxel_size and offsets are three values each")
    return np.array([float(v) for v in voxel_size] + [float(v) for v in offsets], dtype=np.float32)      # rounded to float32 once


def pillar_vfe(voxels: torch.Tensor, num_points: torch.Tensor, coords: torch.Tensor, weight: torch.Tensor, gamma: torch.Tensor,
               beta: torch.Tensor, running_mean: Optional[torch.Tensor] = None, running_var: Optional[torch.Tensor] = None,
               num_batches_tracked: Optional[torch.Tensor] = None, *, voxel_size, offsets,
               parts: int = PILLAR_XYZ | PILLAR_CLUSTER | PILLAR_CENTER, eps: float = 1e-3, momentum: Optional[float] = 0.01,
               training: bool = True, workspace: Optional[torch.Tensor] = None, out=None):
    """modest_pillar_vfe on PyTorch's current stream: enqueue only, nothing is read back.
    voxels (P, S, Cp) float32; num_points (P,) and coords (P, 4) = [b, z, y, x] float32, int32 or int64, read as they are;
    weight (C, K), gamma and beta (C,) float32; running_mean / running_var (C,) float32 and num_batches_tracked () int64 or None.
    voxel_size: (vx, vy, vz); offsets: (voxel / 2 + range) x, y, z; both rounded to float32.  momentum None: the cumulative
    average.  training: batch statistics, and the running buffers are updated IN PLACE; else the running buffers are read.
    -> (out (P, C) float32, winner (P, C) uint8, sums (2 C + K C + K) float64, stat (2, C) float32 = mean32, invstd32);
    without `training` winner, sums and stat are None.  `out` = (out, winner, sums, stat) supplies the buffers."""
    extra = (("gamma", gamma), ("beta", beta), ("running_mean", running_mean), ("running_var", running_var),
             ("num_batches_tracked", num_batches_tracked))
    dev, P, S, Cp, C, K = _pillar_inputs(voxels, num_points, coords, weight, parts, extra)
    if gamma is None or beta is None:
        raise ValueError("gamma and beta must be device tensors")
    for name, t in extra[:4]:
        if t is not None and tuple(t.shape) != (C,):
            raise ValueError(f"{name} {tuple(t.shape)} must be (C,) = ({C},)")
    if (running_mean is None) != (running_var is None):
        raise ValueError("running_mean and running_var come together")
    if not training and running_mean is None:
        raise ValueError("eval mode needs running_mean and running_var")
    if num_batches_tracked is not None and num_batches_tracked.numel() != 1:
        raise ValueError("num_batches_tracked must hold one int64")
    if training and P * S < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got P * S = {P * S} rows")
    geometry = _pillar_geometry(voxel_size, offsets)
    Q = 2 * C + K * C + K
    res, winner, sums, stat = _outputs((("out", torch.float32, (P, C), True), ("winner", torch.uint8, (P, C), training),
                                        ("sums", torch.float64, (Q,), training), ("stat", torch.float32, (2, C), training)),
                                       out, dev, absent=("is not due in eval mode", "must be a tensor"))
    if training:
        workspace = _workspace(_workspace_bytes("modest_pillar_vfe_workspace_bytes", P, C, K), workspace, dev)
    ptr = _ptr
    with torch.cuda.device(dev):
        check(load().modest_pillar_vfe(P, S, Cp, C, int(parts), ptr(voxels), ptr(num_points), _PILLAR_CODES[num_points.dtype],
                                       ptr(coords), _PILLAR_CODES[coords.dtype], geometry.ctypes.data, ptr(weight), ptr(gamma),
                                       ptr(beta), ptr(running_mean), ptr(running_var), ptr(num_batches_tracked) if training else None,
                                       float(eps), -1.0 if momentum is None else float(momentum), int(bool(training)), ptr(res),
                                       ptr(winner), ptr(sums), ptr(stat), ptr(workspace) if training else None,
                                       workspace.numel() if training else 0, _stream()), "modest_pillar_vfe")
    return res, winner, sums, stat


def pillar_vfe_backward(voxels: torch.Tensor, num_points: torch.Tensor, coords: torch.Tensor, weight: torch.Tensor,
                        gamma: torch.Tensor, out_features: torch.Tensor, winner: torch.Tensor, grad_out: torch.Tensor,
                        sums: torch.Tensor, stat: torch.Tensor, *, voxel_size, offsets,
                        parts: int = PILLAR_XYZ | PILLAR_CLUSTER | PILLAR_CENTER, workspace: Optional[torch.Tensor] = None, out=None):
    """modest_pillar_vfe_backward on PyTorch's current stream: enqueue only, nothing is read back.
    The inputs of `pillar_vfe` as they were, what it returned in training mode (out_features, winner, sums, stat) and grad_out
    (P, C) float32.  -> (grad_weight (C, K), grad_gamma (C,), grad_beta (C,)) float32 (`out` supplies them), every element
    written.  The voxels get no gradient."""
    extra = (("gamma", gamma), ("out_features", out_features), ("winner", winner), ("grad_out", grad_out), ("sums", sums), ("stat", stat))
    dev, P, S, Cp, C, K = _pillar_inputs(voxels, num_points, coords, weight, parts, extra)
    Q = 2 * C + K * C + K
    for name, t, shape in (("gamma", gamma, (C,)), ("out_features", out_features, (P, C)), ("winner", winner, (P, C)),
                           ("grad_out", grad_out, (P, C)), ("sums", sums, (Q,)), ("stat", stat, (2, C))):
        if t is None or tuple(t.shape) != shape:
            raise ValueError(f"{name} must be a {shape} tensor" + ("" if t is None else f", got {tuple(t.shape)}"))
    if P * S < 2:
        raise ValueError(f"the backward of a training forward needs more than 1 row, got P * S = {P * S}")
    geometry = _pillar_geometry(voxel_size, offsets)
    dW, dg, db = _outputs((("grad_weight", torch.float32, (C, K), True), ("grad_gamma", torch.float32, (C,), True),
                           ("grad_beta", torch.float32, (C,), True)), out, dev)
    workspace = _workspace(_workspace_bytes("modest_pillar_vfe_workspace_bytes", P, C, K), workspace, dev)
    ptr = _ptr
    with torch.cuda.device(dev):
        check(load().modest_pillar_vfe_backward(P, S, Cp, C, int(parts), ptr(voxels), ptr(num_points), _PILLAR_CODES[num_points.dtype],
                                                ptr(coords), _PILLAR_CODES[coords.dtype], geometry.ctypes.data, ptr(weight),
                                                ptr(gamma), ptr(out_features), ptr(winner), ptr(grad_out), ptr(sums), ptr(stat),
                                                ptr(dW), ptr(dg), ptr(db), ptr(workspace), workspace.numel(), _stream()),
              "modest_pillar_vfe_backward")
    return dW, dg, db


def _scatter_inputs(rows, rows_name, coords, batch_size, ny, nx):
    index = (torch.float32, torch.int32, torch.int64)
    dev = _device_tensors(((rows_name, rows), ("voxel_coords", coords)), dtypes={"voxel_coords": index}, dtype_error=TypeError,
                          same_device=True)
    B, ny, nx = int(batch_size), int(ny), int(nx)
    if B < 0 or B > PILLAR_MAX_BATCH:
        raise ValueError(f"batch_size = {B} is outside the limit of 0 .. {PILLAR_MAX_BATCH}")
    if ny < 1 or nx < 1 or ny * nx > PILLAR_MAX_ROWS:
        raise ValueError(f"a grid of ny = {ny}, nx = {nx} must have between 1 and {PILLAR_MAX_ROWS} cells")
    return dev, B, ny, nx


def pillar_scatter(features: torch.Tensor, coords: torch.Tensor, batch_size: int, ny: int, nx: int, *, out=None) -> torch.Tensor:
    """modest_pillar_scatter on PyTorch's current stream: enqueue only, nothing is read back.
    features (P, C) float32, coords (P, 4) = [b, z, y, x] float32, int32 or int64, contiguous.
    -> canvas (batch_size, C, ny, nx) float32 (`out` supplies it): zeros, then canvas[b, c, y, x] = features[p, c]; a row whose b,
    z, y or x is out of range (nz = 1) is skipped.  Two rows of one cell must not occur."""
    dev, B, ny, nx = _scatter_inputs(features, "pillar_features", coords, batch_size, ny, nx)
    if features.ndim != 2 or tuple(coords.shape) != (int(features.shape[0]), 4):
        raise ValueError(f"pillar_features {tuple(features.shape)} and voxel_coords {tuple(coords.shape)} must be (P, C) and (P, 4)")
    P, C = (int(v) for v in features.shape)
    if C < 1 or C > PILLAR_MAX_CHANNELS:
        raise ValueError(f"C = {C} channels is outside the limit of 1 .. {PILLAR_MAX_CHANNELS}")
    for name, t in (("pillar_features", features), ("voxel_coords", coords)):
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous, got strides {tuple(t.stride())}")
    canvas = _decode_out(out, (B, C, ny, nx), dev)
    with torch.cuda.device(dev):
        check(load().modest_pillar_scatter(P, C, B, ny, nx, _ptr_filled(features), _ptr_filled(coords), _PILLAR_CODES[coords.dtype],
                                           _ptr_filled(canvas), _stream()), "modest_pillar_scatter")
    return canvas


def pillar_scatter_backward(grad_canvas: torch.Tensor, coords: torch.Tensor, *, out=None) -> torch.Tensor:
    """modest_pillar_scatter_backward on PyTorch's current stream: enqueue only, nothing is read back.
    grad_canvas (B, C, ny, nx) float32 contiguous, coords (P, 4) as pillar_scatter read them.
    -> grad_features (P, C) float32 (`out` supplies it), every element written: grad_canvas[b, :, y, x], zeros for a row out of
    range."""
    if not torch.is_tensor(grad_canvas) or grad_canvas.ndim != 4:
        raise ValueError("grad_canvas must be a (B, C, ny, nx) device tensor (PyTorch-ROCm 'cuda')")
    B, C, ny, nx = (int(v) for v in grad_canvas.shape)
    dev, B, ny, nx = _scatter_inputs(grad_canvas, "grad_canvas", coords, B, max(ny, 1), max(nx, 1))
    if coords.ndim != 2 or int(coords.shape[1]) != 4:
        raise ValueError(f"voxel_coords {tuple(coords.shape)} must be (P, 4)")
    P = int(coords.shape[0])
    if C < 1 or C > PILLAR_MAX_CHANNELS:
        raise ValueError(f"C = {C} channels is outside the limit of 1 .. {PILLAR_MAX_CHANNELS}")
    for name, t in (("grad_canvas", grad_canvas), ("voxel_coords", coords)):
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous, got strides {tuple(t.stride())}")
    grad = _decode_out(out, (P, C), dev)
    with torch.cuda.device(dev):
        check(load().modest_pillar_scatter_backward(P, C, B, ny, nx, _ptr_filled(grad_canvas), _ptr_filled(coords),
                                                    _PILLAR_CODES[coords.dtype], _ptr_filled(grad), _stream()),
              "modest_pillar_scatter_backward")
    return grad


# --------------------------------------------------------------------------- training-batch preparation
BATCH_PREP_STEPS = {"flip_x": 1, "flip_y": 2, "rotation": 3, "scaling": 4}
BATCH_PREP_MAX_BATCH = 65535
BATCH_PREP_TABLE = ("points", "far", "boxes", "candidates_kept", "candidates_dropped")
_BP_SAMP_COLS = 10


def batch_prep_max_boxes() -> int:
    """gts plus candidates of a sample the box workgroup stages in LDS"""
    return int(load().modest_batch_prep_max_boxes())


def batch_prep_tile() -> int:
    """rows of a points workgroup; a tile never spans two samples"""
    return int(load().modest_batch_prep_tile())


def batch_prep_workspace_bytes(n_rows: int, batch_size: int) -> int:
    return _workspace_bytes("modest_batch_prep_workspace_bytes", n_rows, batch_size)


def _host_trig4(h: np.ndarray) -> np.ndarray:
    """(n, 4) float32 cosf(h), sinf(h), cosf(-h), sinf(-h) of the host's C library (kitti_infos.host_cos_sin_f32)"""
    from .kitti_infos import host_cos_sin_f32
    h = np.asarray(h, np.float32).ravel()
    cp, sp = host_cos_sin_f32(-h)
    cn, sn = host_cos_sin_f32(h)
    return np.stack([cp, sp, cn, sn], axis=1).astype(np.float32).reshape(-1, 4)


class BatchPrepPlan:
    """the host tables of a batch (include/modest_hip.h, a39) and their totals"""
    __slots__ = ("B", "F", "steps", "road_plane", "samp", "boxes", "cand", "cand_f64", "cand_group", "xf", "n_rows", "n_scene",
                 "n_boxes", "n_cand", "gt_capacity")


def _bp_boxes(a, name, b):
    a = np.asarray(a, dtype=np.float32)
    if a.ndim != 2 and a.size == 0:
        a = a.reshape(0, 7)
    if a.ndim != 2 or a.shape[1] < 7:
        raise ValueError(f"sample {b}: {name} {a.shape} must be (n, 7)")
    if a.shape[1] > 7:
        raise NotImplementedError(f"sample {b}: {name} has {a.shape[1]} columns: boxes with more than 7 columns (the velocity "
                                  f"columns) are not provided")
    return a


def batch_prep_plan(samples, db_offsets, features: int, steps=(), road_plane: bool = False) -> BatchPrepPlan:
    """The host half of stage 1: numpy only, no device data.  samples: per sample a dict with n_points (its scene rows, stacked
    in sample order), gt_boxes (G, 7), gt_classes (G,) (0: a name outside class_names), cand_boxes (C, 7), cand_classes (C,),
    cand_groups (C,) (a run of equal numbers is a class group, in the sampler's order), cand_objects (C,) rows of db_offsets,
    with road_plane mv_height (C,) float64 and cand_z (C,) the lowered z, and the draws: flip_x, flip_y, cos, sin, angle, scale
    (each read only if its step is in `steps`, names of BATCH_PREP_STEPS in the augmentors' order, each at most once).
    db_offsets (objects + 1,) int64: the objects' first rows in the packed database points."""
    steps = [str(s) for s in steps]
    for s in steps:
        if s not in BATCH_PREP_STEPS:
            raise NotImplementedError(f"augmentor step {s!r} is not provided: {sorted(BATCH_PREP_STEPS)}")
    if len(set(steps)) != len(steps):
        raise NotImplementedError(f"augmentor steps {steps}: a step that occurs twice is not provided")
    F, B = int(features), len(samples)
    if not 4 <= F <= 8:
        raise ValueError(f"features = {F}: 4 to 8 point features")
    if B > BATCH_PREP_MAX_BATCH:
        raise ValueError(f"batch of {B} samples is above the limit of {BATCH_PREP_MAX_BATCH}")
    off = np.asarray(db_offsets, dtype=np.int64).ravel()
    if off.size < 1 or off[0] != 0 or (np.diff(off) < 0).any():
        raise ValueError("db_offsets must start at 0 and never fall")
    limit, tile = batch_prep_max_boxes(), batch_prep_tile()
    pl = BatchPrepPlan()
    pl.B, pl.F, pl.steps, pl.road_plane = B, F, np.array([BATCH_PREP_STEPS[s] for s in steps], np.int32), bool(road_plane)
    samp = np.zeros((B, _BP_SAMP_COLS), np.int64)
    xf = np.zeros((B, 8), np.float32)
    boxes, cands, cf64, groups = [], [], [], []
    vrow = scene = nbox = ncand = ntile = 0
    for b, s in enumerate(samples):
        gt = _bp_boxes(s["gt_boxes"], "gt_boxes", b)
        cb = _bp_boxes(s.get("cand_boxes", np.zeros((0, 7), np.float32)), "cand_boxes", b)
        G, Cn = len(gt), len(cb)
        if G + Cn > limit:
            raise ValueError(f"sample {b}: {G} gts plus {Cn} candidates are above the limit of {limit} boxes")
        gcls = np.asarray(s["gt_classes"], np.int64).ravel()
        ccls = np.asarray(s.get("cand_classes", np.zeros(0)), np.int64).ravel()
        grp = np.asarray(s.get("cand_groups", np.zeros(0)), np.int64).ravel()
        objs = np.asarray(s.get("cand_objects", np.zeros(0)), np.int64).ravel()
        if len(gcls) != G or len(ccls) != Cn or len(grp) != Cn or len(objs) != Cn:
            raise ValueError(f"sample {b}: gt_classes, cand_classes, cand_groups and cand_objects must have a number per box")
        if Cn and (objs.min() < 0 or objs.max() >= off.size - 1):
            raise ValueError(f"sample {b}: cand_objects outside the database's {off.size - 1} objects")
        n = int(s["n_points"])
        if n < 0:
            raise ValueError(f"sample {b}: n_points = {n}")
        cnt = off[objs + 1] - off[objs] if Cn else np.zeros(0, np.int64)
        first = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        nobj = int(first[-1])
        samp[b] = (vrow, nobj, scene, n, nbox, G, Cn, ncand, ntile, 0)
        allb = np.concatenate([gt, cb], axis=0)
        row = np.zeros((G + Cn, 12), np.float32)
        row[:, :7] = allb
        row[:, 7:11] = _host_trig4(allb[:, 6])
        row[:, 11] = np.concatenate([gcls, ccls]).astype(np.float32)
        boxes.append(row)
        cands.append(np.stack([off[objs] if Cn else cnt, cnt, first[:-1]], axis=1).astype(np.int64).reshape(-1, 3))
        f64 = np.zeros((Cn, 2), np.float64)
        if road_plane and Cn:
            mv, cz = np.asarray(s["mv_height"], np.float64).ravel(), np.asarray(s["cand_z"], np.float32).ravel()
            if len(mv) != Cn or len(cz) != Cn:
                raise ValueError(f"sample {b}: mv_height and cand_z must have a number per candidate")
            f64[:, 0], f64[:, 1] = mv, cz.astype(np.float64)
        cf64.append(f64)
        groups.append(grp.astype(np.int32))
        if "flip_x" in steps:
            xf[b, 0] = 1.0 if s["flip_x"] else 0.0
        if "flip_y" in steps:
            xf[b, 1] = 1.0 if s["flip_y"] else 0.0
        if "rotation" in steps:
            xf[b, 2], xf[b, 3], xf[b, 4] = np.float32(s["cos"]), np.float32(s["sin"]), np.float32(s["angle"])
        if "scaling" in steps:
            xf[b, 5] = np.float32(s["scale"])
        vrow += nobj + n
        scene += n
        nbox += G + Cn
        ncand += Cn
        ntile += (nobj + n + tile - 1) // tile
    if vrow > 2 ** 31 - 1:
        raise ValueError(f"{vrow} rows in a call are above the limit of 2^31 - 1")
    pl.samp, pl.xf = samp, xf
    pl.boxes = np.concatenate(boxes, axis=0) if boxes else np.zeros((0, 12), np.float32)
    pl.cand = np.concatenate(cands, axis=0) if cands else np.zeros((0, 3), np.int64)
    pl.cand_f64 = np.concatenate(cf64, axis=0) if cf64 else np.zeros((0, 2), np.float64)
    pl.cand_group = np.concatenate(groups) if groups else np.zeros((0,), np.int32)
    pl.n_rows, pl.n_scene, pl.n_boxes, pl.n_cand = vrow, scene, nbox, ncand
    pl.gt_capacity = int((samp[:, 5] + samp[:, 6]).max()) if B else 0
    return pl


class BatchPrepStage1:
    """what a stage-1 call leaves: the buffers stage 2 reads, and the pinned table's counts (numpy, the call's own)"""
    __slots__ = ("B", "F", "n_rows", "points", "lists", "gt_boxes", "valid", "table", "table_pinned", "workspace", "want_near")

    def counts(self, name: str) -> np.ndarray:
        return self.table[:, BATCH_PREP_TABLE.index(name)]


def _bp_upload(arrays, staging, dev):
    """the arrays packed 8-byte aligned into one pinned buffer and copied to the device in one asynchronous copy
    -> (device views, staging)"""
    sizes = [(a.nbytes + 7) // 8 * 8 for a in arrays]
    total = max(sum(sizes), 8)
    if staging is None or staging.numel() < total:
        staging = torch.empty((max(total, 4096),), dtype=torch.uint8).pin_memory()
    if not staging.is_pinned() or staging.dtype != torch.uint8:
        raise ValueError("staging must be a pinned uint8 tensor")
    host = staging.numpy()
    o = 0
    for a, sz in zip(arrays, sizes):
        host[o:o + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).ravel()
        o += sz
    dev_buf = staging[:total].to(dev, non_blocking=True)
    views, o = [], 0
    for a, sz in zip(arrays, sizes):
        views.append(dev_buf[o:o + a.nbytes])
        o += sz
    return views, staging


def batch_prep_stage1(plan: BatchPrepPlan, scene_points: torch.Tensor, db_points: torch.Tensor, point_cloud_range, *,
                      remove_extra_width=(0.0, 0.0, 0.0), want_near: bool = False, remove_outside_boxes: bool = True,
                      min_num_corners: int = 1, workspace: Optional[torch.Tensor] = None, table: Optional[torch.Tensor] = None,
                      staging: Optional[torch.Tensor] = None, out=None):
    """modest_batch_prep_stage1 on PyTorch's current stream: BLOCKING (one synchronise, inside the library).
    scene_points (plan.n_scene, F) float32: the raw scans stacked in sample order; db_points (rows, F) float32: the packed
    database objects.  The candidates that collide are dropped, the kept ones' object rows and the scene rows outside their
    enlarged boxes go through the plan's augmentor steps and the x / y range mask, stably compacted; the boxes go through the
    same steps, limit_period, the class filter and (remove_outside_boxes) the corner mask.
    -> (BatchPrepStage1, staging): points (n_rows, 1 + F) of which the first table[:, 0].sum() rows are written, stacked with the
    sample in column 0; gt_boxes (B, plan.gt_capacity, 8) zero-padded; valid (n_cand,) int32; table (B, 5) int32 of
    BATCH_PREP_TABLE.  workspace, table (pinned int32), staging (pinned uint8): reused when large enough, else allocated."""
    if not isinstance(plan, BatchPrepPlan):
        raise ValueError("plan must be a BatchPrepPlan (ops.batch_prep_plan)")
    dev = _device_tensors((("scene_points", scene_points), ("db_points", db_points)), same_device=True)
    B, F = plan.B, plan.F
    for name, t, rows in (("scene_points", scene_points, plan.n_scene), ("db_points", db_points, None)):
        if t.ndim != 2 or int(t.shape[1]) != F or (rows is not None and int(t.shape[0]) != rows) or not t.is_contiguous():
            raise ValueError(f"{name} {tuple(t.shape)} must be a contiguous ({'rows' if rows is None else rows}, {F}) tensor")
    rng = np.ascontiguousarray(np.asarray(point_cloud_range, dtype=np.float32).ravel())
    extra = np.ascontiguousarray(np.asarray(remove_extra_width, dtype=np.float32).ravel())
    if rng.size != 6 or extra.size != 3:
        raise ValueError("point_cloud_range must hold 6 numbers and remove_extra_width 3")
    if int(min_num_corners) < 0 or int(min_num_corners) > 8:
        raise ValueError(f"min_num_corners = {min_num_corners} is outside 0 .. 8")
    n, G = plan.n_rows, plan.gt_capacity
    points, lists, gt, valid = _outputs((("points", torch.float32, (n, 1 + F), True), ("lists", torch.int32, (n,), True),
                                         ("gt_boxes", torch.float32, (B, G, 8), True),
                                         ("valid", torch.int32, (plan.n_cand,), True)), out, dev)
    workspace = _workspace(batch_prep_workspace_bytes(n, B), workspace, dev)
    words = B * 6
    if table is None or table.numel() < words:
        table = torch.zeros((max(words, 16),), dtype=torch.int32).pin_memory()
    if not table.is_pinned() or table.dtype != torch.int32 or not table.is_contiguous():
        raise ValueError("table must be a contiguous pinned int32 tensor")
    st = BatchPrepStage1()
    st.B, st.F, st.n_rows, st.points, st.lists, st.gt_boxes, st.valid = B, F, n, points, lists, gt, valid
    st.workspace, st.want_near, st.table_pinned = workspace, bool(want_near), table
    if B == 0:
        st.table = np.zeros((0, 5), np.int32)
        return st, staging
    (samp_d, boxes_d, cand_d, f64_d, grp_d, xf_d), staging = _bp_upload(
        [plan.samp, plan.boxes, plan.cand, plan.cand_f64, plan.cand_group, plan.xf], staging, dev)
    ptr = _ptr_filled
    with torch.cuda.device(dev):
        check(load().modest_batch_prep_stage1(
            B, F, plan.n_scene, ptr(scene_points), int(db_points.shape[0]), ptr(db_points), _np_ptr(plan.samp), samp_d.data_ptr(),
            plan.n_boxes, ptr(boxes_d), plan.n_cand, _np_ptr(plan.cand) if plan.n_cand else None, ptr(cand_d), ptr(f64_d),
            ptr(grp_d), xf_d.data_ptr(), len(plan.steps), _np_ptr(plan.steps) if len(plan.steps) else None, _np_ptr(rng),
            _np_ptr(extra), int(plan.road_plane), int(bool(want_near)), int(bool(remove_outside_boxes)), int(min_num_corners), n,
            ptr(valid), ptr(points), ptr(lists), ptr(gt), G, table.data_ptr(), workspace.data_ptr(), workspace.numel(),
            _stream()), "modest_batch_prep_stage1")
    st.table = table[:words].view(B, 6).numpy()[:, :5].copy()
    return st, staging


def batch_prep_order_draws(table: np.ndarray, num_points: Optional[int] = None, shuffle: bool = False, np_random=None,
                           shuffle_first: bool = False):
    """Stage 2 on the host, from the counts alone: for samples 0 .. B - 1 the reference's draws of sample_points
    (data_processor.py:82-118; num_points None: not configured) and then of shuffle_points (shuffle), on `np_random` (None: the
    global np.random).  choice(array, k, replace=False) is array[permutation(len)[:k]], so positions are drawn as positions.
    shuffle_first: shuffle_points stands AHEAD of sample_points in the config: per sample its permutation is drawn first, and
    the places and lists of the picks are those of the shuffled sample (the device rebuilds its near / far lists from the
    permutation, ops.batch_prep_order).
    -> (picks (n_out, 2) int32 of (4 sample + list, place), list 0 the survivors, 1 the near list, 2 the far list; rows per
    sample (B,) int64), and with shuffle_first a third entry: perm (sum of the points kept,) int32, the samples' permutations
    stacked"""
    npr = np.random if np_random is None else np_random
    table = np.asarray(table)
    picks, rows, perms = [], [], []
    for b in range(len(table)):
        k, far = int(table[b, 0]), int(table[b, 1])
        lid, pos = np.zeros(k, np.int64), np.arange(k, dtype=np.int64)
        if shuffle_first:
            perms.append(np.asarray(npr.permutation(k), np.int32) if shuffle else np.arange(k, dtype=np.int32))
        if num_points is not None and int(num_points) != -1:
            m = int(num_points)
            if k == 0 and m > 0:
                raise ValueError(f"sample {b}: sample_points on a sample without points (the reference does not end)")
            if m < k:
                if m > far:
                    sel = npr.permutation(k - far)[:m - far]
                    lid = np.concatenate([np.full(len(sel), 1, np.int64), np.full(far, 2, np.int64)])
                    pos = np.concatenate([np.asarray(sel, np.int64), np.arange(far, dtype=np.int64)])
                else:
                    pos = np.asarray(npr.permutation(k)[:m], np.int64)
                    lid = np.zeros(m, np.int64)
            else:
                while m > len(pos):
                    pos = np.concatenate([pos, np.asarray(npr.permutation(k)[:min(k, m - len(pos))], np.int64)])
                lid = np.zeros(len(pos), np.int64)
            order = np.arange(len(pos))
            npr.shuffle(order)
            lid, pos = lid[order], pos[order]
        if shuffle and not shuffle_first:
            order = npr.permutation(len(pos))
            lid, pos = lid[order], pos[order]
        picks.append(np.stack([4 * b + lid, pos], axis=1))
        rows.append(len(pos))
    out = np.concatenate(picks, axis=0).astype(np.int32) if picks else np.zeros((0, 2), np.int32)
    if shuffle_first:
        return out, np.asarray(rows, np.int64), (np.concatenate(perms) if perms else np.zeros(0, np.int32))
    return out, np.asarray(rows, np.int64)


def batch_prep_order(st: BatchPrepStage1, picks: np.ndarray, *, perm: Optional[np.ndarray] = None,
                     staging: Optional[torch.Tensor] = None, out=None):
    """modest_batch_prep_order on PyTorch's current stream: enqueue only.  picks (n_out, 2) int32 (batch_prep_order_draws),
    checked against the stage-1 table before the launch.  perm: the third entry of batch_prep_order_draws(shuffle_first=True),
    checked to hold, per sample, places of its survivors only; one more launch then rebuilds the near / far lists in the
    shuffled order.  -> (points (n_out, 1 + F) float32, staging)"""
    if not isinstance(st, BatchPrepStage1):
        raise ValueError("st must be the BatchPrepStage1 of ops.batch_prep_stage1")
    picks = np.ascontiguousarray(picks)
    if picks.dtype != np.int32 or picks.ndim != 2 or picks.shape[1] != 2:
        raise ValueError(f"picks {picks.shape} {picks.dtype} must be (n_out, 2) int32")
    n_out = len(picks)
    if n_out > 2 ** 31 - 1:
        raise ValueError(f"{n_out} rows in a call are above the limit of 2^31 - 1")
    if n_out:
        b, lid, pos = picks[:, 0] >> 2, picks[:, 0] & 3, picks[:, 1]
        if b.min() < 0 or b.max() >= st.B or lid.max() > 2 or pos.min() < 0:
            raise ValueError("picks name a sample or a list that does not exist")
        if lid.any() and not st.want_near:
            raise ValueError("picks name the near / far lists of a stage 1 run without want_near")
        kept, far = st.table[b, 0], st.table[b, 1]
        if (pos >= np.where(lid == 0, kept, np.where(lid == 1, kept - far, far))).any():
            raise ValueError("picks name a place behind the end of its list")
    dev = st.points.device
    if perm is not None:
        perm = np.ascontiguousarray(perm)
        kept = st.table[:, 0].astype(np.int64)
        if perm.dtype != np.int32 or perm.ndim != 1 or len(perm) != int(kept.sum()):
            raise ValueError(f"perm {perm.shape} {perm.dtype} must be ({int(kept.sum())},) int32: a place per point kept")
        if len(perm) and ((perm < 0) | (perm >= np.repeat(kept, kept))).any():
            raise ValueError("perm names a survivor its sample does not have")
    (res,) = _outputs((("points", torch.float32, (n_out, 1 + st.F), True),), None if out is None else (out,), dev)
    if n_out == 0:
        return res, staging
    if perm is not None:
        (picks_d, perm_d), staging = _bp_upload([picks, perm], staging, dev)
        lists2 = torch.empty((max(st.n_rows, 1),), dtype=torch.int32, device=dev)
    else:
        (picks_d,), staging = _bp_upload([picks], staging, dev)
        perm_d = lists2 = None
    with torch.cuda.device(dev):
        check(load().modest_batch_prep_order(st.B, st.F, st.n_rows, _ptr_filled(st.points), _ptr_filled(st.lists),
                                             st.workspace.data_ptr(), st.workspace.numel(), n_out, picks_d.data_ptr(),
                                             _ptr_filled(perm_d), _ptr(lists2), res.data_ptr(), _stream()),
              "modest_batch_prep_order")
    return res, staging


# --------------------------------------------------------------------------- the optimiser step
OPTIM_STATIC = np.dtype([("p", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i8"), ("first_chunk", "<i4"), ("pad", "<i4")])
OPTIM_STEP = np.dtype([("g", "<u8"), ("dec", "<f4"), ("w", "<f4"), ("omw", "<f4"), ("b2", "<f4"), ("omb2", "<f4"), ("bc2s", "<f4"),
                       ("eps", "<f4"), ("nss", "<f4"), ("flags", "<u4"), ("norm_first", "<i4")])
OPTIM_LERP_HIGH = 1
_optim_chunk = None


def optim_chunk() -> int:
    """elements of a chunk: a tensor of n elements owns ceil(n / optim_chunk()) chunks"""
    global _optim_chunk
    if _optim_chunk is None:
        _optim_chunk = int(load().modest_optim_chunk())
    return _optim_chunk


def optim_workspace_bytes(n_tensors: int, n_chunks: int) -> int:
    return _workspace_bytes("modest_optim_workspace_bytes", n_tensors, n_chunks)


def _optim_call(fn_name, static, step, upload_static, workspace, middle, ctx):
    """what the four optimiser calls share: the two host tables (structured arrays of OPTIM_STATIC / OPTIM_STEP, one record per
    tensor), the workspace, PyTorch's current stream"""
    if not isinstance(static, np.ndarray) or static.dtype != OPTIM_STATIC or static.ndim != 1 or not static.flags.c_contiguous:
        raise TypeError("static must be a contiguous 1-d array of ops.OPTIM_STATIC")
    if not isinstance(step, np.ndarray) or step.dtype != OPTIM_STEP or step.shape != static.shape or not step.flags.c_contiguous:
        raise TypeError("step must be a contiguous array of ops.OPTIM_STEP with one record per record of static")
    T = int(static.shape[0])
    if T < 1:
        raise ValueError("the table holds no tensor")
    n_chunks = int(static["first_chunk"][-1]) + -(-int(static["n"][-1]) // optim_chunk())
    _dev(workspace, torch.uint8, "workspace")
    nb = optim_workspace_bytes(T, n_chunks)
    if workspace.numel() < nb:
        raise ValueError(f"workspace holds {workspace.numel()} bytes, {nb} are needed")
    for name, t in middle:
        if isinstance(t, (float, int)):
            continue
        if _dev(t, torch.float32, name).numel() != 1 or t.device != workspace.device:
            raise ValueError(f"{name} must be one float32 on {workspace.device}")
    ctx = _ctx(ctx, workspace)
    args = [a.data_ptr() if torch.is_tensor(a) else a for _, a in middle]
    with torch.cuda.device(workspace.device):
        check(getattr(load(), fn_name)(ctx.handle, T, n_chunks, _np_ptr(static), _np_ptr(step), 1 if upload_static else 0, *args,
                                       workspace.data_ptr(), workspace.numel(), _stream()), fn_name)


def optim_grad_norm(static, step, workspace: torch.Tensor, norm_out: torch.Tensor, *, upload_static: bool = True,
                    ctx: Optional[Context] = None) -> torch.Tensor:
    """modest_optim_grad_norm on PyTorch's current stream: enqueue only.  -> norm_out (one float32 on the device) :=
    (float) sqrt(sum g^2) over the gradients the step table names."""
    _optim_call("modest_optim_grad_norm", static, step, upload_static, workspace, (("norm_out", norm_out),), ctx)
    return norm_out


def optim_clip(static, step, max_norm: float, workspace: torch.Tensor, norm_out: torch.Tensor, *, upload_static: bool = True,
               finish_launch: bool = False, ctx: Optional[Context] = None) -> torch.Tensor:
    """modest_optim_clip: the norm as optim_grad_norm leaves it, then every gradient *= coef in place (two launches; three with
    finish_launch, where one workgroup sums the chunk partials once instead of every workgroup of the clip: the same bits)."""
    _optim_call("modest_optim_clip", static, step, upload_static, workspace,
                (("max_norm", float(max_norm)), ("finish_launch", int(bool(finish_launch))), ("norm_out", norm_out)), ctx)
    return norm_out


def optim_step(static, step, workspace: torch.Tensor, *, upload_static: bool = True, ctx: Optional[Context] = None) -> None:
    """modest_optim_step: decay and Adam update of every tensor of the table in one launch, the gradients as they are."""
    _optim_call("modest_optim_step", static, step, upload_static, workspace, (), ctx)


def optim_norm_step(static, step, max_norm: float, workspace: torch.Tensor, norm_out: torch.Tensor, *, upload_static: bool = True,
                    finish_launch: bool = False, ctx: Optional[Context] = None) -> torch.Tensor:
    """modest_optim_norm_step: the norm, then the step on fl(g * coef) (two launches; three with finish_launch, as in optim_clip);
    the gradients are not written."""
    _optim_call("modest_optim_norm_step", static, step, upload_static, workspace,
                (("max_norm", float(max_norm)), ("finish_launch", int(bool(finish_launch))), ("norm_out", norm_out)), ctx)
    return norm_out
