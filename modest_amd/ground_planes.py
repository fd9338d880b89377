"""Road planes for detector training: a drop-in for the reference's ``data_preprocessing/RANSAC.py``.

Every frame of a KITTI-format tree gets ``planes_dir/<idx>.txt``, the file OpenPCDet's ``kitti_dataset.py`` reads when
``USE_ROAD_PLANE: True``: rect-frame points of the velodyne rows (``calib.project_velo_to_rect``, float64), the window
``min_h < y < max_h, -10 < z < 70, -20 < x < 20``, sklearn's ``RANSACRegressor()`` defaults fitted to y ~ (x, z), and
``w = (c0, -1, c1) / |.|, h = b / |.|`` -- or ``w = (0, -1, 0), h = 1.65`` below 5 candidates.

The fits run batched on the GPU (``ops.ground_planes``: csrc/ground_planes.hip); frames with 5..300 candidates and the
rare hand-backs are fitted by the float64 host mirror (utils/ransac.py: ransac_plane64).

RNG policy.  The reference never seeds, so its planes depend on the process's stream.
  --seed S (default 0)  frame ``idx`` draws from ``RandomState(S + int(idx))``: a frame's plane does not depend on the
                        batch, the part or the other frames;
  --global_seed S       the reference run preceded by ``np.random.seed(S)``: one RandomState consumed in sorted frame
                        order by the frames with >= 5 candidates (one part only).

    python -m modest_amd.ground_planes --calib_dir .../training/calib --lidar_dir .../training/velodyne \\
        --planes_dir .../training/planes --min_h 1.5 --max_h 2.5
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import os.path as osp
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

W_DEFAULT = [0, -1, 0]
H_DEFAULT = 1.65


# ---- the reference's pieces, on the host ------------------------------------------------------------------------------
def list_frames(lidar_dir, split_file=None):
    """RANSAC.py:10-17: the split file's stripped lines longer than one character, or every *.bin of lidar_dir, sorted"""
    if split_file is not None:
        with open(split_file) as f:
            return sorted([x.strip() for x in f.readlines() if len(x) > 1])
    return sorted([x[:-4] for x in os.listdir(lidar_dir) if x[-4:] == ".bin"])


def plane_text(w, h) -> str:
    """RANSAC.py:61-66 (no trailing newline)"""
    return "\n".join(["# Plane", "Width 4", "Height 1", "{:e} {:e} {:e} {:e}".format(w[0], w[1], w[2], h)])


def plane_from_fit(c0, c1, b):
    """RANSAC.py:46-52"""
    w = np.zeros(3)
    w[0] = c0
    w[2] = c1
    w[1] = -1.0
    norm = np.linalg.norm(w)
    return w / norm, b / norm


def calib_mats(text: str):
    """(V2C (3,4), R0 (3,3)) float64 of a calib file's text, parsed as kitti_util.Calibration.read_calib_file does"""
    data = {}
    for line in text.splitlines():
        line = line.rstrip()
        if len(line) == 0:
            continue
        key, value = line.split(":", 1)
        try:
            data[key] = np.array([float(x) for x in value.split()])
        except ValueError:
            pass
    return np.reshape(data["Tr_velo_to_cam"], [3, 4]), np.reshape(data["R0_rect"], [3, 3])


def frame_candidates(rows: np.ndarray, V2C: np.ndarray, R0: np.ndarray, min_h: float, max_h: float) -> np.ndarray:
    """RANSAC.py:27-38 with kitti_util.Calibration.project_velo_to_rect's numpy products: (m,3) float64 rect points"""
    pts = rows[:, :3]
    ref = np.dot(np.hstack((pts, np.ones((pts.shape[0], 1)))), np.transpose(V2C))
    pc_rect = np.transpose(np.dot(R0, np.transpose(ref)))
    valid = (pc_rect[:, 1] > min_h) & (pc_rect[:, 1] < max_h) & (pc_rect[:, 2] > -10) & (pc_rect[:, 2] < 70) & \
            (pc_rect[:, 0] > -20) & (pc_rect[:, 0] < 20)
    return pc_rect[valid]


def fit_frame_host(cand: np.ndarray, rs):
    """RANSAC.py:39-52 on the host mirror: (w, h, GroundFit or None)"""
    from .utils.ransac import ransac_plane64
    if len(cand) < 5:
        return W_DEFAULT, H_DEFAULT, None
    fit = ransac_plane64(cand[:, [0, 2]], cand[:, 1], random_state=rs)
    w, h = plane_from_fit(fit.coef[0], fit.coef[1], fit.intercept)
    return w, h, fit


def frame_seed(seed: int, idx: str) -> int:
    try:
        return int(seed) + int(idx)
    except ValueError:
        raise ValueError(f"frame name {idx!r} is not an integer: --seed mode seeds RandomState(seed + int(name)); "
                         f"use --global_seed for such trees") from None


def _state_of(rs):
    st = rs.get_state()
    assert st[0] == "MT19937"
    return st[1], int(st[2])


def _set_state(rs, key, pos):
    rs.set_state(("MT19937", np.asarray(key, dtype=np.uint32), int(pos), 0, 0.0))


# ---- the batched GPU path ---------------------------------------------------------------------------------------------
class _Reader:
    """the .bin files of a batch -> one pinned float32 buffer (modest_host_read_files: size probe, reader threads);
    two slots used in turn, so the next batch is read while the GPU fits this one"""

    def __init__(self, readers: int = 8):
        from . import _lib
        self.lib = _lib.load()
        self.readers = int(readers)
        self.slots = [None, None]
        self.turn = 0

    def read(self, paths):
        import torch
        n = len(paths)
        cp = (C.c_char_p * n)(*[p.encode() for p in paths])
        sizes = np.zeros(n, dtype=np.uint64)
        r = self.turn = (self.turn + 1) % 2
        buf = self.slots[r]
        cap = 0 if buf is None else buf.numel() * 4
        rc = int(self.lib.modest_host_read_files(cp, n, buf.data_ptr() if buf is not None else None, cap, sizes.ctypes.data,
                                                 self.readers))
        if rc > 0 or (rc == 0 and buf is None):
            need = max(rc, 16)
            self.slots[r] = buf = torch.empty((need // 4 + need // 32 + 4096,), dtype=torch.float32, pin_memory=True)
            rc = int(self.lib.modest_host_read_files(cp, n, buf.data_ptr(), buf.numel() * 4, sizes.ctypes.data, self.readers))
        if rc < 0:
            raise IOError(f"cannot read {paths[-rc - 2]}" if rc < -1 else "modest_host_read_files: bad arguments")
        if (sizes % 16).any():
            raise ValueError("velodyne .bin files hold (n,4) float32 rows")
        offs = np.concatenate([[0], np.cumsum(sizes // 16)]).astype(np.int64)
        return buf[: int(offs[-1]) * 4].view(-1, 4), offs, int(sizes.sum())


def extract_ransac(calib_dir, lidar_dir, planes_dir, min_h=1.5, max_h=2, split_file=None, *, seed=0, global_seed=None,
                   total_part=1, part=0, batch=256, readers=8, device=0, stats=None):
    """RANSAC.py:9-68 (``extract_ransac``) with the fits on the GPU.  Writes ``planes_dir/<idx>.txt`` for every frame of
    this part; ``stats`` (a dict) receives the counters of the JSON summary."""
    import torch
    from . import dist, ops
    from ._lib import default_context
    idx_list = [str(x) for x in dist.shard(list_frames(lidar_dir, split_file), total_part, part)]
    if global_seed is not None and total_part > 1:
        raise ValueError("--global_seed reproduces ONE sorted run of the reference: it cannot be split into parts")
    if not osp.isdir(planes_dir):
        os.makedirs(planes_dir, exist_ok=True)
    if global_seed is None:
        seeds = [frame_seed(seed, i) for i in idx_list]   # (every name checked before any work)
    dev = torch.device("cuda", device)
    torch.cuda.set_device(dev)
    ctx = default_context(device)
    reader = _Reader(readers)
    calib_cache, text_cache = {}, {}
    t = dict(read_s=0.0, h2d_s=0.0, gpu_s=0.0, write_s=0.0, host_fits=0, frames=0, bytes=0)
    rows_dev = torch.empty((0, 4), dtype=torch.float32, device=dev)
    chain_rs = np.random.RandomState(global_seed) if global_seed is not None else None

    def load(ids):
        t0 = time.perf_counter()
        host, offs, nbytes = reader.read([osp.join(lidar_dir, i + ".bin") for i in ids])
        fr = np.zeros(len(ids), dtype=ops.GP_FRAME)
        mats = []
        for k, i in enumerate(ids):
            with open(osp.join(calib_dir, i + ".txt")) as f:
                text = f.read()
            m = calib_cache.get(text)
            if m is None:
                m = calib_cache[text] = calib_mats(text)
            mats.append(m)
            fr["v2c"][k], fr["r0"][k] = m[0].reshape(-1), m[1].reshape(-1)
        fr["row_offset"], fr["n"] = offs[:-1], np.diff(offs)
        t["read_s"] += time.perf_counter() - t0
        t["bytes"] += nbytes
        return host, offs, fr, mats

    def write(items):
        t0 = time.perf_counter()
        for i, w, h in items:
            with open(osp.join(planes_dir, i + ".txt"), "w") as f:
                f.write(plane_text(w, h))
        t["write_s"] += time.perf_counter() - t0

    batches = [idx_list[b:b + batch] for b in range(0, len(idx_list), batch)]
    wall0 = time.perf_counter()
    with ThreadPoolExecutor(1) as rd, ThreadPoolExecutor(1) as wr:
        nxt = rd.submit(load, batches[0]) if batches else None
        pending = []
        for b, ids in enumerate(batches):
            host, offs, fr, mats = nxt.result()
            R = int(offs[-1])
            if rows_dev.shape[0] < R:
                rows_dev = torch.empty((R + R // 8, 4), dtype=torch.float32, device=dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rows_dev[:R].copy_(host, non_blocking=True)
            e1.record()
            out = [None] * len(ids)
            if chain_rs is None:
                for k, s in enumerate(seeds[b * batch:b * batch + len(ids)]):
                    key, pos = _state_of(np.random.RandomState(s))
                    fr["key"][k], fr["pos"][k] = key, pos
                res, ms, _ = ops.ground_planes(rows_dev, fr, min_h, max_h, ctx=ctx)
                nxt = rd.submit(load, batches[b + 1]) if b + 1 < len(batches) else None   # host staging slot of b-1 is free
                t["gpu_s"] += ms / 1e3
                for k, i in enumerate(ids):
                    out[k] = _take(res[k], host, offs, k, mats[k], min_h, max_h, np.random.RandomState(seeds[b * batch + k]), t)
            else:
                lo = 0
                res = np.zeros(len(ids), dtype=ops.GP_RESULT)
                first = True
                while lo < len(ids):   # the chain stops at a frame that goes to the host; the rest is called again
                    sub = np.ascontiguousarray(fr[lo:])
                    key, pos = _state_of(chain_rs)
                    sub["key"][0], sub["pos"][0] = key, pos
                    r, ms, _ = ops.ground_planes(rows_dev, sub, min_h, max_h, chain=True, ctx=ctx)
                    if first:
                        nxt = rd.submit(load, batches[b + 1]) if b + 1 < len(batches) else None
                        first = False
                    t["gpu_s"] += ms / 1e3
                    host_at = np.nonzero(r["status"] == ops.GP_HOST)[0]
                    stop = int(host_at[0]) if len(host_at) else len(sub)
                    for k in range(stop):
                        out[lo + k] = _take(r[k], host, offs, lo + k, mats[lo + k], min_h, max_h, None, t)
                    if stop > 0:
                        _set_state(chain_rs, sub[stop - 1]["key"], sub[stop - 1]["pos"])
                    if stop < len(sub):
                        _set_state(chain_rs, sub[stop]["key"], sub[stop]["pos"])   # (the state before that frame)
                        out[lo + stop] = _take(r[stop], host, offs, lo + stop, mats[lo + stop], min_h, max_h, chain_rs, t)
                        stop += 1
                    lo += stop
            t["h2d_s"] += e0.elapsed_time(e1) / 1e3
            t["frames"] += len(ids)
            pending.append(wr.submit(write, [(i, w, h) for i, (w, h) in zip(ids, out)]))
        for p in pending:
            p.result()
    t["wall_s"] = time.perf_counter() - wall0
    if stats is not None:
        stats.update(t)
    return t


def _take(r, host, offs, k, mats, min_h, max_h, rs, t):
    """(w, h) of frame k from its device result; a hand-back is fitted here by the host mirror with `rs`"""
    from . import ops
    st = int(r["status"])
    if st == ops.GP_DEFAULT:
        return W_DEFAULT, H_DEFAULT
    if st == ops.GP_FITTED:
        return r["plane"][:3].copy(), float(r["plane"][3])
    if st == ops.GP_NO_CONSENSUS:
        raise ValueError("RANSAC could not find a valid consensus set. All `max_trials` iterations were "
                         "skipped because each randomly chosen sub-sample failed the passing criteria.")
    assert rs is not None, "a frame went to the host without its generator"
    rows = host[int(offs[k]):int(offs[k + 1])].numpy()
    cand = frame_candidates(rows, mats[0], mats[1], min_h, max_h)
    t["host_fits"] += 1
    w, h, _ = fit_frame_host(cand, rs)
    return w, h


def extract_ransac_host(calib_dir, lidar_dir, planes_dir, min_h=1.5, max_h=2, split_file=None, *, seed=0,
                        global_seed=None):
    """The same files from the host mirror alone (no GPU): the CPU reference of extract_ransac."""
    idx_list = list_frames(lidar_dir, split_file)
    if not osp.isdir(planes_dir):
        os.makedirs(planes_dir, exist_ok=True)
    rs_chain = np.random.RandomState(global_seed) if global_seed is not None else None
    for i in idx_list:
        with open(osp.join(calib_dir, i + ".txt")) as f:
            V2C, R0 = calib_mats(f.read())
        rows = np.fromfile(osp.join(lidar_dir, i + ".bin"), dtype=np.float32).reshape(-1, 4)
        cand = frame_candidates(rows, V2C, R0, min_h, max_h)
        rs = rs_chain if rs_chain is not None else np.random.RandomState(frame_seed(seed, i))
        w, h, _ = fit_frame_host(cand, rs)
        with open(osp.join(planes_dir, i + ".txt"), "w") as f:
            f.write(plane_text(w, h))


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--calib_dir", default="KITTI/object/training/calib")
    p.add_argument("--lidar_dir", default="KITTI/object/training/velodyne")
    p.add_argument("--planes_dir", default="KITTI/object/training/velodyne_planes")
    p.add_argument("--min_h", type=float, default=1.5)
    p.add_argument("--max_h", type=float, default=1.8)
    p.add_argument("--split_file", type=str, default=None)
    p.add_argument("--seed", type=int, default=0, help="frame idx draws from RandomState(seed + int(idx))")
    p.add_argument("--global_seed", type=int, default=None,
                   help="one RandomState(S) consumed in sorted frame order (the reference after np.random.seed(S))")
    p.add_argument("--total_part", type=int, default=1)
    p.add_argument("--part", type=int, default=0)
    p.add_argument("--batch", type=int, default=256, help="frames per GPU call")
    p.add_argument("--readers", type=int, default=8, help="host threads reading .bin files")
    p.add_argument("--overwrite", action="store_true", help="run even when planes_dir exists (the reference skips)")
    return p.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    if osp.isdir(a.planes_dir) and not a.overwrite:   # RANSAC.py:83-85
        print(json.dumps({"tool": "ground_planes", "skipped": True, "planes_dir": a.planes_dir}), flush=True)
        return 0
    if a.global_seed is not None and a.total_part > 1:
        print("--global_seed reproduces one sorted run of the reference: use --seed with --total_part", file=sys.stderr)
        return 2
    t = extract_ransac(a.calib_dir, a.lidar_dir, a.planes_dir, a.min_h, a.max_h, a.split_file, seed=a.seed,
                       global_seed=a.global_seed, total_part=a.total_part, part=a.part, batch=a.batch, readers=a.readers)
    wall = max(t["wall_s"], 1e-9)
    print(json.dumps({"tool": "ground_planes", "frames": t["frames"], "frames_per_s": round(t["frames"] / wall, 1),
                      "wall_s": round(wall, 4), "read_s": round(t["read_s"], 4), "h2d_s": round(t["h2d_s"], 4),
                      "gpu_s": round(t["gpu_s"], 4), "write_s": round(t["write_s"], 4), "host_fits": t["host_fits"],
                      "read_mb": round(t["bytes"] / 1e6, 2)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
