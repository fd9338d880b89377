#!/usr/bin/env python
"""bench.py -- BASELINE.json's headline metric on synthetic Lyft-shape input.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

With --gpus N > 1 and no launcher in the environment the script re-executes itself under
`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1` (one rank
per GPU, RCCL); under a launcher it reads RANK / LOCAL_RANK / WORLD_SIZE as usual and REFUSES to run
when WORLD_SIZE != --gpus.  Every rank feeds its GPU from `--procs` helper processes x `--streams`
threads (the host side of a scan is Python + ~60 HIP calls and saturates one process long before the
GPU; --procs 1 keeps everything in the rank process).  Timing is the rank's: barrier, clock, all
helpers run their share of the K steps and synchronise, barrier, clock; max over ranks.

A "step" is one pass of the whole seed-label hot path over one scan whose inputs are already
resident in HBM -- the live frame and the 10 x 36 history frames sit in the frame store
(modest_amd/frame_store.py) exactly as the CLI keeps them; there is no pre-stacked, pre-transformed
history: PP score (descriptor table -> pose fused into the neighbour count, ~10.8 M history points)
-> RANSAC ground plane -> plane/range mask -> PP-weighted mutual-kNN DBSCAN -> cluster filter ->
closeness box fit -> BEV IoU NMS -> KITTI label text.  value = scans/s over all ranks (weak scaling:
every rank processes K scans of its own); ms_per_step = the timed region's wall time / K.

A plain run sets up, warms up, times the K steps and prints the line (contract fields + `config`).
--dump-outputs DIR also writes what the last timed step computed (the last step of the last helper's share) as
DIR/<name>.npy after the clock: pp_score (N,) float32, cluster_labels (N,) and boxes (k, 8) {t0, t1, t2, l, w, h, ry,
volume} float64, label_fields (k, 14) float64 = the numeric fields of the KITTI label lines; with the same arguments
the inputs are the same seeded synthetic scans from run to run.  Only with --full the JSON line also carries
  roofline     -- the PP neighbour count (the operation SURVEY.md 8d prices at 12*M + 16*N
                  algorithmic bytes per scan; here it is a chain of kernels, so the WHOLE chain is
                  timed with HIP events, not just its largest kernel) against the 8 TB/s HBM3E peak, on a
                  block of scans whose history windows are what data_preprocessing/lyft/split_traintest.py:79-113
                  emits: windows by distance thresholds (repeated frames), traversals accepted per scan (T changes
                  inside the block); `roofline_best_case` = the same measurement on the windows of frames i..i+F-1
                  every timed region runs on (35 of 36 frames shared with the previous scan);
  cpu_baseline -- the oracle (the reference's own scipy/sklearn calls, same threading as the
                  reference: cKDTree single-threaded, sklearn n_jobs=-1) timed on this host on a
                  bounded sample of the same scans, plus `best_effort` (SURVEY 8d baseline B:
                  query_ball_point(workers=-1), one process per scan); rank 0, N=1 only;
  value_with_ingest -- the same pool and the same step, except that every step first brings in the 11 frames a
                  scan of a Lyft shard does not share with its predecessor (pinned host -> device, tile sort),
                  solves the 361 relative poses from the raw pose factors and builds its descriptor table
                  from scratch: `value` without the "already resident and described" head start;
  cli          -- the three product CLIs (pre_compute_pp_score, generate_mask, gen_label_files) on a
                  synthetic KITTI tree with shared history frames, file I/O included; rank 0, N=1;
  steady_state -- the whole helper pool over 24 steps per helper when K gives the helpers fewer (see below);
  parity       -- the measured path against the oracle on the CPU sample's scans.
Without --full these keys are null.
Nothing here reads the reference project's sources.
"""
from __future__ import annotations

import argparse
import gc
import json
import os
import socket
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0     # /opt/skills/guides/MI355X_MICROARCH.md: 8.0 TB/s spec
# Every helper gets at least MIN_STEPS_PER_HELPER steps.  The driver's 20-step run is a 6.5-7.5 ms window whichever way it
# is dealt: few helpers carry long chains of stages 2 + 3 on their host side, many helpers run many small PP blocks one after
# the other on the GPU (a block of 4 / 7 / 10 scans costs 0.74 / 0.79 / 0.90 ms).  Measured with the round-5 kernels, three runs
# each (tools/r05_steps20.sh): 5 x 4 scans 2 620-3 020 scans/s, 4 x 5 2 540-2 770, 3 x 6-7 2 750-3 010, 2 x 10 2 640-2 840.
# A --full run with fewer than STEADY_STEPS_PER_HELPER steps per helper also reports `steady_state`: the whole pool over 24 steps per
# helper, measured after the contract region with its own barrier / synchronise bracket.
MIN_STEPS_PER_HELPER = int(os.environ.get("MODEST_MIN_STEPS_PER_HELPER", "6"))
STEADY_STEPS_PER_HELPER = 24


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=560)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--no-mask-chain", action="store_true",
                    help="A/B: the mask stage scan by scan (modest_mask_stage) instead of one call per chain of --pp-batch scans")
    ap.add_argument("--scans", type=int, default=64,
                    help="resident scans per host process, cycled through: CONSECUTIVE scans of synthetic shards of --shard-scans "
                         "scans each (consecutive scans of a Lyft shard share 35 of their 36 history frames per traversal)")
    ap.add_argument("--shard-scans", type=int, default=32, help="consecutive scans per resident shard")
    ap.add_argument("--pp-batch", type=int, default=32,
                    help="consecutive scans whose PP stage is ONE call (FrameStore.pp_score_batch: modest_pp_score_block for >= 4 "
                         "scans that share their frames, modest_pp_score_frames_batch otherwise); clamped to --shard-scans")
    ap.add_argument("--mask-batch", type=int, default=32,
                    help="scans per chain of stages 2 + 3 (modest_seed_chain).  32 since round 6: with the chain behind one library call the longer "
                         "chain's GPU efficiency reaches `value` (7 200-7 500 against 6 450-6 550 scans/s at 16; round 5 measured no gain: its host "
                         "side held the helper twice as long)")
    ap.add_argument("--no-pp-block", action="store_true",
                    help="A/B: the PP stage through modest_pp_score_frames_batch (every scan streams its own 361 frames) in chains of "
                         "at most 8 scans, never through modest_pp_score_block")
    ap.add_argument("--config", choices=("c3", "c5"), default="c3",
                    help="BASELINE.json configuration: c3 = Lyft shape (30 k live points, 10 traversals x 36 frames); c5 = nuScenes "
                         "shape (35 k points, 20 traversals x 16 frames, remove_center on the history, plane_estimate.max_hs=-1.3, "
                         "image_shape=[900,1600]; README.md:62-70).  c5 sets --n-live / --traversals / --frames")
    ap.add_argument("--n-live", type=int, default=30000)
    ap.add_argument("--traversals", type=int, default=10)
    ap.add_argument("--frames", type=int, default=36)
    ap.add_argument("--cpu-scans", type=int, default=5, help="scans of the CPU baseline sample, timed one by one after one untimed warm-up scan: "
                    "the rate is 1 / their median (BASELINE.md 3; 0 = skip)")
    ap.add_argument("--cpu-best-effort", type=int, default=16,
                    help="scans of the best-effort CPU baseline (one process per scan, workers=-1; 0 = skip)")
    ap.add_argument("--sharing", choices=("best", "realistic"), default="realistic",
                    help="realistic (default): the line's `roofline` is the isolated measurement on a shard whose history windows are chosen "
                         "by the reference's rule (split_traintest.py:79-113; live 8 m/s, history 3-15 m/s at 5 Hz: repeated frames, traversals "
                         "that enter and leave, union ~2.5 x a scan's entries); the windows of frames i..i+F-1 (35 of 36 frames shared: the best "
                         "case) are `roofline_best_case`.  best: only the latter")
    ap.add_argument("--pp-only", action="store_true", help="config 2: PP-score stage only")
    ap.add_argument("--no-prefetch", action="store_true",
                    help="A/B: do not enqueue the next scan's PP stage under the host tail of the current scan's label stage "
                         "(same stream, same context; default on)")
    ap.add_argument("--mask-only", action="store_true",
                    help="diagnostic: stages 2 + 3 only (the PP score of every resident scan is computed once); "
                         "not a BASELINE configuration")
    ap.add_argument("--pp-cus", type=int, default=128,
                    help="with several host processes per GPU: the CU count every process sizes its persistent PP grids "
                         "for (MODEST_NUM_CUS).  Kernels of different processes do run side by side; a PP launch that "
                         "fills all 256 CUs keeps the other processes' small mask-stage kernels waiting (measured: "
                         "1.91 k scans/s at 256, 2.1-2.2 k at 64..192).  0 = all CUs.  The isolated roofline "
                         "measurement always uses a context sized for the whole GPU.")
    ap.add_argument("--procs", type=int, default=8,
                    help="host processes per GPU (per rank).  The host side of a scan is Python + ~60 HIP calls; one "
                         "process saturates at ~350 scans/s on its interpreter lock and HIP runtime locks while the "
                         "GPU is half idle, so every rank feeds its GPU from several helper processes (what the "
                         "reference's own total_part/part split does by hand).  1 = everything in the rank process.")
    ap.add_argument("--streams", type=int, default=1,
                    help="scans in flight per host process: threads, each with its own HIP stream and modest_ctx")
    ap.add_argument("--cli-scans", type=int, default=768,
                    help="live scans of the CLI measurement (0 = skip): the three product CLIs on a synthetic KITTI "
                         "tree, 10 history traversals x 36 frames per scan, frames shared between consecutive scans")
    ap.add_argument("--cli-workers", type=int, default=6,
                    help="worker processes per GPU of the CLI measurement's workers=N legs (profiles/r06_cli_workers_readers.txt: "
                         "5-6 workers x 2 reader threads is where the ingest-bound CLIs peak; 8 lose a fifth to the contention of "
                         "their reads)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything besides the headline figure: steady state, value_with_ingest, the "
                         "isolated PP roofline (best case and realistic windows), the CLI leg, the CPU baselines and the parity "
                         "check against the oracle.  Off: set up, warm up, time --steps steps, print the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (float32 / float64, "
                         "at most 64 MB in all)")
    a = ap.parse_args(argv)
    a.nusc = a.config == "c5"
    if a.nusc:
        a.n_live, a.traversals, a.frames = 35000, 20, 16
    return a


# --------------------------------------------------------------------------- launcher
def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch_command(gpus: int, argv) -> list:
    """The command `python bench.py --gpus N` re-executes itself as when no launcher set WORLD_SIZE."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={gpus}",
            "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__), *argv]


def maybe_relaunch(a, argv) -> None:
    if a.gpus <= 1 or "WORLD_SIZE" in os.environ:
        return
    n_dev = torch.cuda.device_count() if torch.cuda.is_available() else 0
    # MODEST_DIST_BACKEND=gloo: the ranks may SHARE devices (LOCAL_RANK wraps around the visible ones; RCCL refuses two ranks
    # on one device) -- the multi-rank path of this script on a one-GPU box (tests/test_gpu_multirank.py)
    if n_dev < a.gpus and not (os.environ.get("MODEST_DIST_BACKEND") == "gloo" and n_dev >= 1):
        raise SystemExit(f"bench.py --gpus {a.gpus}: only {n_dev} HIP device(s) visible")
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    sys.exit(subprocess.call(launch_command(a.gpus, argv), env=env))


# --------------------------------------------------------------------------- resident inputs
GEN_STRIDE = 1 << 20   # the re-inserted copy of a frame (ingest-inclusive step) alternates between two integer keys


class ResidentShard:
    """S consecutive scans of a shard as the CLI holds them: every frame once in the frame store, a descriptor table
    per scan.  Scan i of the shard looks at frames i .. i+F-1 of every traversal's track (synth.make_shard)."""

    def __init__(self, sh, dev, calib, store, base, nusc=False, realistic=False):
        self.store, self.dev, self.base, self.nusc = store, dev, int(base), bool(nusc)
        self.realistic = bool(realistic)   # windows by the reference's rule: tracks of different lengths, repeated frames
        self.T, self.L = len(sh.tracks), max(len(tr) for tr in sh.tracks)
        self.W, self.gen, self.raw_host, items = {}, {}, {}, []
        for t, tr in enumerate(sh.tracks):
            for j, (raw, W) in enumerate(tr):
                fid = self.base + t * self.L + j
                self.W[fid], self.gen[fid] = W, 0
                items.append((fid, torch.from_numpy(raw).to(dev), W))
        self.scans = []
        for sc in sh.scans:
            lid = self.base + self.T * self.L + sc.index
            self.W[lid], self.gen[lid] = sc.live_W, 0
            items.append((lid, torch.from_numpy(sc.live_raw).to(dev), sc.live_W))
        store.insert_many(items)
        for sc in sh.scans:
            self.scans.append(ResidentScan(self, sh, sc, calib))

    def key(self, fid):
        return fid + GEN_STRIDE * self.gen[fid]


class ResidentScan:
    """One scan of a resident shard.  For the ingest-inclusive step it also keeps, in pinned host memory, the raw frames
    the scan brings in new (the last frame of every traversal's window + the live scan = 11 of its 361) and the raw pose
    factors of all of them."""

    def __init__(self, shard, sh, sc, calib):
        from modest_amd.pre_compute_pp_score import relative_poses
        self.shard, self.calib = shard, calib
        self.live_host = sc.live_raw
        self.live_id = shard.base + shard.T * shard.L + sc.index
        self.live_raw = torch.from_numpy(sc.live_raw).to(shard.dev)   # file order, for stages 2 + 3
        self.N, self.T = int(sc.live_raw.shape[0]), (sc.n_trav if sc.travs is not None else shard.T)   # (the scan's own number of traversals)
        self.hist_ids = [shard.base + t * shard.L + j for t, j in sc.hist]
        self.travs = sc.trav_list()
        self.M = int(sum(len(sh.tracks[t][j][0]) for t, j in sc.hist))   # (history points before remove_center)
        self.rels, self.live_rel, self.A44 = sc.rels, sc.live_rel, sc.world_from_ref
        self.W_stack = np.stack([shard.W[f] for f in self.hist_ids] + [sc.live_W])   # raw pose factors E @ L @ K of all 361 frames
        self.fixed_ego, self.fixed_l2e, self.K = sc.first_pose, sc.l2e, sc.K
        assert np.array_equal(relative_poses(self.fixed_l2e, self.fixed_ego, self.W_stack, self.K)[:-1], self.rels)
        self.desc = None
        if shard.realistic:   # (isolated PP measurement only: no ingest-inclusive step on these)
            self.describe()
            return
        F = len(sc.hist) // shard.T
        # ---- ingest-inclusive step: the scan's 11 "new" frames (last frame of every traversal's window + the live scan)
        self.new_ids = [self.hist_ids[t * F + F - 1] for t in range(shard.T)] + [self.live_id]
        raws = [sh.tracks[t][sc.hist[t * F + F - 1][1]][0] for t in range(shard.T)] + [sc.live_raw]
        self.new_W = np.stack([shard.W[f] for f in self.new_ids])
        self.new_offs = np.cumsum([0] + [len(r) for r in raws])
        self.new_pinned = torch.empty((int(self.new_offs[-1]), 4), dtype=torch.float32, pin_memory=True)
        self.new_pinned.numpy()[:] = np.concatenate(raws)
        self.desc = None
        self.describe()

    @property
    def live_key(self):
        return self.shard.key(self.live_id)

    def describe(self, rels=None):
        """the scan's descriptor table from the store (the frames' current copies)"""
        sh = self.shard
        rl = self.rels if rels is None else rels[:-1]
        lr = self.live_rel if rels is None else rels[-1]
        self.desc = sh.store.describe(self.live_key, lr, [sh.key(f) for f in self.hist_ids], self.travs, rl, sh.nusc)
        return self.desc


class Runner:
    """The pipeline of one host process: resident synthetic shards, `n_threads` worker threads with one HIP stream +
    modest_ctx each.  Steps are numbered globally; step i takes resident scan i mod n, a BLOCK is the steps of one
    multiple of --pp-batch (= consecutive scans of one shard): its PP stage is one call, its stages 2 + 3 run in chains
    of --mask-batch scans."""

    def __init__(self, a, rank, local, slot):
        import threading
        self.slot = int(slot)
        from modest_amd import _lib, config, ops, synth
        from modest_amd.frame_store import FrameStore
        from modest_amd.gen_label_files import gen_label_chain, gen_label_scan
        from modest_amd.generate_mask import generate_mask_chain, generate_mask_scan
        from modest_amd.utils import kitti_util
        self.a, self.ops, self.threading = a, ops, threading
        self._gen_label_scan, self._generate_mask_scan = gen_label_scan, generate_mask_scan
        self._generate_mask_chain = generate_mask_chain
        self._gen_label_chain = gen_label_chain
        _lib.load()
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs an MI355X: the hot path has no CPU fallback")
        self.dev = torch.device("cuda", local)
        torch.cuda.set_device(self.dev)
        self.n_threads = max(1, a.streams)
        if self.n_threads > 1:
            # the worker threads hand the GIL over at their blocking library calls; CPython's default
            # forced-switch interval (5 ms) is longer than a whole step, 0.5 ms measured best (+20 %)
            sys.setswitchinterval(float(os.environ.get("MODEST_SWITCH_INTERVAL", "0.0005")))
        self.streams = [torch.cuda.Stream(device=self.dev) for _ in range(self.n_threads)]
        shared = a.procs > 1 and a.pp_cus > 0 and "MODEST_NUM_CUS" not in os.environ
        if shared:
            os.environ["MODEST_NUM_CUS"] = str(a.pp_cus)
        self.ctxs = [_lib.Context(local) for _ in range(self.n_threads)]
        self.prefetch = not (a.no_prefetch or a.pp_only or a.mask_only)
        self.S = max(1, min(int(a.shard_scans), int(a.scans)))
        self.PB = max(1, min(int(a.pp_batch), self.S))
        while self.S % self.PB:   # blocks never straddle shards
            self.PB -= 1
        self.MB = max(1, int(a.mask_batch))
        self.block = False if a.no_pp_block else None   # None: FrameStore decides (>= 4 scans that share their frames)
        self.mark_batch = [[] for _ in range(self.n_threads)]   # scans per profile mark, per thread
        self.pp_ctxs = self.ctxs
        # the mask stage of a chain runs every scan in its own context (the thread's + MB - 1 more)
        self.chain_ctxs = [[self.ctxs[w]] + [_lib.Context(local) for _ in range(self.MB - 1)] for w in range(self.n_threads)]
        if shared:
            del os.environ["MODEST_NUM_CUS"]
        self._lib, self.local, self.iso_ctx = _lib, local, None
        with tempfile.TemporaryDirectory() as d:
            open(os.path.join(d, "c.txt"), "w").write(synth.CALIB_TXT)
            calib = kitti_util.Calibration(os.path.join(d, "c.txt"))
        nusc = bool(getattr(a, "nusc", False))
        self.margs = config.compose("generate_mask", ["data_root=/unused"] + (["plane_estimate.max_hs=-1.3"] if nusc else []))
        self.largs = config.compose("generate_label_files", ["data_root=/unused"] + (["image_shape=[900,1600]"] if nusc else []))
        self.store = FrameStore(self.dev, 0.3, ctx=self.ctxs[0])
        # as the CLI does (pre_compute_pp_score.py: frame_prealloc_gb): device memory for the frames the ingest-inclusive steps will
        # bring in, taken from the driver in ONE call before any clock (a 256 MB slab on demand every third block otherwise: a
        # hipMalloc under eight processes costs tens of milliseconds -- 97 ms of the 256-step ingest region in round 5's first runs)
        self.store.reserve(float(os.environ.get("MODEST_BENCH_PREALLOC_GB", "3")) * 2 ** 30)
        self.shards, self.scans = [], []
        n_sh = max(1, (int(a.scans) + self.S - 1) // self.S)
        for q in range(n_sh):
            n_sc = min(self.S, int(a.scans) - q * self.S) if a.scans >= self.S else int(a.scans)
            sh = synth.make_shard(n_sc, n_live=a.n_live, n_trav=a.traversals, n_frames=a.frames, seed=scan_seed(rank, slot, q),
                                  x0=30.0 * q, nusc=bool(getattr(a, "nusc", False)))
            rs = ResidentShard(sh, self.dev, calib, self.store, 4096 * 64 * q, nusc)
            self.shards.append(rs)
            self.scans.extend(rs.scans)
            del sh
        self.ingest = False
        self.h_ring = {}   # per thread: two pinned host buffers for the scores of a block (pp_many)
        self.lock = threading.Lock()   # ingest mode re-inserts frames: one block at a time per process
        # every thread (stream + scratch arena + kernel attributes) runs before any clock starts
        self.n_warm = -(-max(a.warmup, 2 * self.n_threads, self.PB * self.n_threads) // self.PB) * self.PB   # whole blocks
        self.run(0, self.n_warm)
        torch.cuda.synchronize()

    def scan_of(self, i):
        return self.scans[i % len(self.scans)]

    def pp_many(self, scs, w):
        """PP stage of the scans of one block: ONE call -> [H]"""
        ctx = self.ctxs[w]
        if getattr(self, "trace", None) is not None:
            t0 = time.perf_counter()
            self.trace, keep = None, self.trace
            try:
                return self.pp_many(scs, w)
            finally:
                self.trace = keep
                keep.append((f"pp[{len(scs)}]", time.perf_counter() - t0))
        # the scores of a block live in ONE device tensor and travel to the host as ONE asynchronous copy into pinned memory
        # right behind the kernels (the host statement of stages 2 + 3 wants them only when the library hands a scan back;
        # the first synchronise of the mask stage is behind this copy): no blocking read-back per scan
        self.mark_batch[w].append(len(scs))
        ns = [int(sc.desc[0]["n"][0]) for sc in scs]
        if len(set(ns)) != 1 or ns[0] == 0:
            return self.store.pp_score_batch([sc.live_key for sc in scs], [sc.desc for sc in scs], scs[0].T, ctx=ctx, block=self.block)
        B, N = len(scs), ns[0]
        Hall = torch.empty((B, N), dtype=torch.float32, device=self.dev)
        Hs = self.store.pp_score_batch([sc.live_key for sc in scs], [sc.desc for sc in scs], scs[0].T, outs=[Hall[i] for i in range(B)],
                                       ctx=ctx, block=self.block)
        ring = self.h_ring.setdefault(w, [None, None, 0])
        k = ring[2] & 1   # two buffers per thread: the next block's scores arrive while this block's are still referenced
        ring[2] += 1
        if ring[k] is None or ring[k].shape[0] < B or ring[k].shape[1] != N:   # (both buffers at once: never inside a clock)
            ring[0] = torch.empty((max(B, self.PB), N), dtype=torch.float32).pin_memory()
            ring[1] = torch.empty((max(B, self.PB), N), dtype=torch.float32).pin_memory()
        ring[k][:B].copy_(Hall, non_blocking=True)
        host = ring[k].numpy()
        for i, H in enumerate(Hs):
            H._host = host[i]
        return Hs

    def _ingest(self, scs, ctx):
        """What the scans of a Lyft shard cost before their kernels can start (consecutive scans share 35 of
        36 frames per traversal): the 11 new frames of every scan travel from pinned host memory to the device and are
        tile-sorted (one device block and ONE sort launch for the whole block of scans), the relative poses of all 361
        frames of every scan are solved from the raw pose factors (get_relative_pose), and the descriptor tables are
        rebuilt from the store -- nothing of a scan's table is reused from a previous step.  A re-inserted frame replaces
        its resident copy for every scan of the shard (the sharing between the scans is that of the CLI)."""
        from modest_amd.pre_compute_pp_score import relative_poses_block
        sh = scs[0].shard
        keys_all, offs, Ws, base = [], [0], [], 0
        # one device staging block per thread (= per stream), kept: a fresh 170 MB tensor per block went to the driver for a new segment
        # every other block -- a hipMalloc inside the clock, tens of milliseconds with eight processes (MODEST_BENCH_TRACE=1:
        # torch_segments_allocated).  Reuse is safe in stream order: the sort that reads the block is enqueued before the next copy into it.
        need = sum(int(sc.new_pinned.shape[0]) for sc in scs)
        stage = getattr(self, "_ingest_stage", None)
        if stage is None:
            stage = self._ingest_stage = {}
        buf = stage.get(id(ctx))
        if buf is None or buf.shape[0] < need:
            buf = stage[id(ctx)] = torch.empty((need + need // 8, 4), dtype=torch.float32, device=self.dev)
        dev = buf[:need]
        old = []
        for sc in scs:
            n = int(sc.new_pinned.shape[0])
            dev[base:base + n].copy_(sc.new_pinned, non_blocking=True)
            for j, fid in enumerate(sc.new_ids):
                old.append(sh.key(fid))
                sh.gen[fid] ^= 1
                keys_all.append(sh.key(fid))
            offs += [base + int(o) for o in sc.new_offs[1:]]
            Ws.append(sc.new_W)
            base += n
        self.store.drop(old)
        self.store.insert_block(keys_all, dev, np.asarray(offs), np.concatenate(Ws), ctx=ctx)
        # every scan of the shard sees the new copies; the block's own scans solve their poses again (a few scans per thread:
        # LAPACK releases the interpreter lock) and their tables come out of ONE gather from the store's slot tables
        rels = relative_poses_block([sc.fixed_l2e for sc in scs], [sc.fixed_ego for sc in scs], [sc.W_stack for sc in scs], scs[0].K)
        descs = self.store.describe_many([sc.live_key for sc in scs], [r[-1] for r in rels], [[sh.key(f) for f in sc.hist_ids] for sc in scs],
                                         [sc.travs for sc in scs], [r[:-1] for r in rels], sh.nusc)
        for sc, d in zip(scs, descs):
            sc.desc = d
        for sc in sh.scans:
            if sc not in scs:
                sc.describe()

    def steps(self, js, w, Hs, after=None):
        """The scans of one chain of stages 2 + 3 on thread w.  Hs: their PP scores (enqueued ahead of time); the mask stage
        of the chain is ONE library call (generate_mask_chain: the mask / graph / DBSCAN block and the cluster statistics as
        one launch per kernel for all of them), boxes and labels go scan by scan; after: called (same stream, same
        context) as soon as the LAST scan has no device work left, i.e. under the host tail of its label stage -- the
        worker enqueues the PP stage of its next block there.  Returns [(H, labels, objs, text)]."""
        a = self.a
        scs = [self.scan_of(i) for i in js]
        if a.pp_only:
            return [(H, None, None, None) for H in Hs]
        # boxes stay (k,8) rows between the stages: the SimpleNamespace objects of the reference exist for its
        # pickle files, which the CLIs write and this in-memory pipeline does not
        items = [dict(ptc=sc.live_host, pp_score=getattr(H, "_host", None) if getattr(H, "_host", None) is not None else H.cpu().numpy(),
                      random_state=np.random.RandomState(i), ptc_dev=sc.live_raw,
                      pp_dev=H) for i, sc, H in zip(js, scs, Hs)]
        tr = getattr(self, "trace", None)
        t0 = time.perf_counter()
        if len(items) > 1 and not a.no_mask_chain:
            res = self._generate_mask_chain(items, scs[0].calib, self.margs, as_rows=True, ctxs=self.chain_ctxs[w][:len(items)],
                                            with_iou=bool(self.largs.nms.enable))
        else:
            res = [self._generate_mask_scan(it["ptc"], it["pp_score"], scs[0].calib, self.margs, random_state=it["random_state"],
                                            ptc_dev=it["ptc_dev"], pp_dev=it["pp_dev"], as_rows=True) for it in items]
        if tr is not None:
            tr.append((f"mask[{len(items)}]", time.perf_counter() - t0))
            t0 = time.perf_counter()
        if len(res) > 1 and not a.no_mask_chain:   # the IoU matrices of the chain's label stage: one launch
            lab = self._gen_label_chain([r[1] for r in res], [sc.calib for sc in scs], self.largs, after_device=after,
                                        ious=[r[3] if len(r) > 3 else None for r in res])
        else:
            lab = [self._gen_label_scan(r[1], sc.calib, self.largs, after_device=after if q == len(res) - 1 else None)
                   for q, (r, sc) in enumerate(zip(res, scs))]
        if tr is not None:
            tr.append((f"label[{len(items)}]", time.perf_counter() - t0))
        return [(H, r[0], r[1], text) for H, r, (text, kept) in zip(Hs, res, lab)]

    def blocks_of(self, lo, hi):
        """steps lo..hi-1 cut at the multiples of the block size -> [[step, ...], ...]"""
        out, i = [], lo
        while i < hi:
            e = min(hi, (i // self.PB + 1) * self.PB)
            out.append(list(range(i, e)))
            i = e
        return out

    def run(self, lo, hi, collect=None, only=None):
        """steps lo..hi-1: the blocks are dealt round-robin to the worker threads; collect: list that receives
        (step, (H, labels, objs, text)) of every step, or of step `only` alone"""
        errs = []
        blocks = self.blocks_of(lo, hi)

        def worker(w):
            try:
                torch.cuda.set_device(self.dev)
                with torch.cuda.stream(self.streams[w]):
                    mine = blocks[w::self.n_threads]
                    Hq = {}

                    def enqueue(bi):   # the PP stage of block bi: one call
                        js = mine[bi]
                        if self.a.mask_only:   # diagnostic: the PP score of a scan is computed once, steps run stages 2 + 3
                            for j in js:
                                sc = self.scan_of(j)
                                if getattr(sc, "_H", None) is None:
                                    sc._H = self.pp_many([sc], w)[0]
                                Hq[j] = sc._H
                            return
                        Hq.update(zip(js, self.pp_many([self.scan_of(j) for j in js], w)))

                    def ingest(bi):   # ingest-inclusive mode: the new frames of block bi (copy + sort + poses + tables)
                        t_in = time.perf_counter()
                        with self.lock:
                            self._ingest([self.scan_of(j) for j in mine[bi]], self.ctxs[w])
                        if getattr(self, "trace", None) is not None:
                            self.trace.append((f"ingest[{len(mine[bi])}]", time.perf_counter() - t_in))

                    for bi, js in enumerate(mine):
                        if js[0] not in Hq:
                            if self.ingest:
                                ingest(bi)
                            enqueue(bi)
                        # like the CLI's ingest thread, the frames of the NEXT block are brought in one block ahead of their
                        # kernels: by the time its PP stage is enqueued the sort has reported every frame's point count
                        if self.ingest and bi + 1 < len(mine):
                            ingest(bi + 1)
                        chains = [js[c:c + self.MB] for c in range(0, len(js), self.MB)]
                        for ci, cj in enumerate(chains):
                            # the next block's PP stage goes out under the label tail of this block's last chain
                            last = ci == len(chains) - 1
                            hook = (lambda b1=bi + 1: enqueue(b1)) if (self.prefetch and last and bi + 1 < len(mine)) else None
                            out = self.steps(cj, w, [Hq.pop(j) for j in cj], after=hook)
                            if collect is not None:
                                collect.extend((j, o) for j, o in zip(cj, out) if only is None or j == only)
                    self.streams[w].synchronize()
            except Exception as e:   # surfaced after join
                errs.append(e)

        if self.n_threads == 1:
            worker(0)
        else:
            th = [self.threading.Thread(target=worker, args=(w,)) for w in range(self.n_threads)]
            for t in th:
                t.start()
            for t in th:
                t.join()
        if errs:
            raise errs[0]

    def rehearse(self, n_steps):
        """Untimed, before the clock: one pass over the SHAPES the timed region will run (its first block and its last,
        possibly partial, one).  A block of fewer than 8 scans takes the per-scan chain, whose scratch arena differs from the
        block path's; an arena that grows inside the timed region costs a device synchronise + hipFree + hipMalloc under
        eight processes (measured: 40 steps in 0.45 s instead of 0.01 s)."""
        if n_steps <= 0 or n_steps in getattr(self, "_rehearsed", set()):
            return
        blocks = self.blocks_of(self.n_warm, self.n_warm + n_steps)
        shapes = {len(b): b for b in blocks}
        for b in shapes.values():
            self.run(b[0], b[-1] + 1)
        torch.cuda.synchronize()
        self._rehearsed = getattr(self, "_rehearsed", set()) | {n_steps}

    def rehearse_ingest(self):
        """Untimed, before the clock of the ingest-inclusive region (like rehearse for the contract region): two blocks per
        thread in that mode (allocator, slab, slot tables, the sort's scratch)."""
        if getattr(self, "_ingest_rehearsed", False):
            return
        self.ingest = True
        self.run(0, 2 * self.PB * self.n_threads)
        torch.cuda.synchronize()
        self.ingest = False
        self._ingest_rehearsed = True

    def timed(self, n_steps, ingest=False, keep_last=False):
        """n_steps steps -> (seconds, HIP-event times of every PP stage launched); keep_last: the last step's
        (H, labels, objs, text) stay in self.last_out"""
        self.ingest = bool(ingest)
        for w, c_ in enumerate(self.pp_ctxs):
            c_.profile_begin(n_steps + 8)
            self.mark_batch[w] = []
        calls0 = (getattr(self.store, "block_calls", 0), getattr(self.store, "chain_calls", 0))
        last = [] if keep_last else None
        t0 = time.perf_counter()
        self.run(self.n_warm, self.n_warm + n_steps, collect=last, only=self.n_warm + n_steps - 1)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        self.last_out = last[-1][1] if last else None
        self.ingest = False
        # which PP path ran INSIDE the clock: calls of modest_pp_score_block / modest_pp_score_frames_batch and their scans
        self.last_paths = dict(block_calls=getattr(self.store, "block_calls", 0) - calls0[0],
                               chain_calls=getattr(self.store, "chain_calls", 0) - calls0[1],
                               scans_per_call=[int(b) for w in range(self.n_threads) for b in self.mark_batch[w]])
        per_scan = []   # a mark brackets the PP stage of a whole block: report it per scan, once per scan
        for w, c_ in enumerate(self.pp_ctxs):
            ms = c_.profile_collect(n_steps + 8)
            sizes = self.mark_batch[w][-len(ms):] if len(ms) else []
            for m, b in zip(ms, sizes):
                per_scan.extend([float(m) / b] * b)
        return dt, np.asarray(per_scan, dtype=np.float32)

    def isolated_pp_ms(self):
        """The PP stage alone on the GPU: one call per block of PB consecutive scans, cycling through all resident shards
        (their block stores + frames exceed the 256 MiB Infinity Cache), HIP events around every call.
        -> (ms per call, scans per call, block path used)"""
        PB, n = self.PB, len(self.scans)
        nb = max(1, n // PB)
        reps = max(6, 3 * nb)
        if self.iso_ctx is None:   # alone on the GPU: grids sized for all CUs
            self.iso_ctx = self._lib.Context(self.local)
        ctx = self.iso_ctx
        calls0 = getattr(self.store, "block_calls", 0)
        ctx.profile_begin(8 * reps + 8)
        with torch.cuda.stream(self.streams[0]):
            for i in range(reps):
                scs = self.scans[(i % nb) * PB:(i % nb) * PB + PB]
                self.store.pp_score_batch([sc.live_key for sc in scs], [sc.desc for sc in scs], scs[0].T, ctx=ctx, block=self.block)
            self.streams[0].synchronize()
        iso = ctx.profile_collect(8 * reps + 8)
        used_block = getattr(self.store, "block_calls", 0) > calls0
        if len(iso) > reps:   # (the per-scan chain splits a call of more than 8 scans into several marks)
            k = len(iso) // reps
            iso = np.asarray(iso[:k * reps]).reshape(reps, k).sum(axis=1)
        return (float(np.mean(iso[2:])), len(scs), used_block) if len(iso) > 2 else None


def realistic_pp(runner):
    """The isolated PP measurement on reference-rule windows: -> dict or None"""
    from modest_amd import synth
    a = runner.a
    PB = runner.PB
    # what a real valid_idx_info.pkl holds (data_preprocessing/lyft/split_traintest.py:79-113): windows by distance thresholds
    # (repeated frames at the fast traversals), and a traversal accepted PER SCAN (closest pose within 3 m, :17,79; two needed, :111)
    # -- tracks enter and leave along the shard, T changes inside the block
    n_tracks = a.traversals + 3
    pres = synth.presence_ramp(PB, n_tracks, t_min=max(2, a.traversals - 3), seed=int(getattr(a, "presence_seed", 5)))
    sh = synth.make_shard_matched(PB, n_live=a.n_live, n_trav=n_tracks, nusc=bool(getattr(a, "nusc", False)), live_speed=8.0,
                                  hist_speeds=(3.0, 15.0), seed=77, presence=pres)
    stats = synth.sharing_stats(sh, PB)
    Ts = [sc.n_trav for sc in sh.scans]
    stats.update(traversals_per_scan_min=int(min(Ts)), traversals_per_scan_max=int(max(Ts)), traversals_per_scan_mean=float(np.mean(Ts)),
                 distinct_traversal_counts=int(len(set(Ts))), tracks=int(n_tracks))
    rs = ResidentShard(sh, runner.dev, runner.scans[0].calib, runner.store, 4096 * 64 * 40, bool(getattr(a, "nusc", False)), realistic=True)
    if runner.iso_ctx is None:
        runner.iso_ctx = runner._lib.Context(runner.local)
    ctx, scs = runner.iso_ctx, rs.scans
    reps = 8
    calls0 = getattr(runner.store, "block_calls", 0)
    ctx.profile_begin(8 * reps + 8)
    with torch.cuda.stream(runner.streams[0]):
        for i in range(reps):
            runner.store.pp_score_batch([sc.live_key for sc in scs], [sc.desc for sc in scs], [sc.T for sc in scs], ctx=ctx, block=runner.block)
        runner.streams[0].synchronize()
    iso = np.asarray(ctx.profile_collect(8 * reps + 8))
    used_block = getattr(runner.store, "block_calls", 0) > calls0
    if len(iso) > reps and len(iso) % reps == 0:
        iso = iso.reshape(reps, -1).sum(axis=1)
    members = float(np.mean([len(sc.hist_ids) for sc in scs]))
    return dict(ms=float(np.mean(iso[2:])), scans=len(scs), block=bool(used_block), sharing=stats, members=members,
                history_points=float(np.mean([sc.M for sc in scs])))


def scan_seed(rank, slot, i):
    return 1000 * rank + 16 * slot + i


def _helper_main(conn, a, rank, local, slot, flag):
    """entry point of a helper process (multiprocessing 'spawn'): pipe protocol
    child -> ('ready', M) ; parent -> ('arm', (n_steps, generation, ingest mode, keep last step)) ; child -> ('armed', None),
    then spins on the shared start flag (all helpers leave the spin within microseconds of each other: a pipe
    message per helper staggers them by ~0.1 ms each, which a 20-step run cannot afford) ;
    child -> ('done', (seconds, kernel_ms)) ; parent -> ('outputs', None) -> child ('outputs', step_arrays of the last step) ;
    parent -> ('iso', None) -> child ('iso', ms) ; parent -> ('exit', None)"""
    try:
        import resource
        t_up = time.perf_counter()
        r = Runner(a, rank, local, slot)
        conn.send(("ready", (r.scans[0].M, time.perf_counter() - t_up, resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0)))
        while True:
            cmd, arg = conn.recv()
            if cmd == "arm":
                n, gen, ingest, keep = arg
                r.rehearse(int(n))
                if ingest:
                    r.rehearse_ingest()
                if not os.environ.get("MODEST_BENCH_GC"):
                    # a generation-2 collection of the interpreter (the process holds its resident shards: millions of objects)
                    # is a 5-10 ms pause -- the length of the driver's whole 20-step window, in which one paused helper
                    # halves the number.  Collected here, outside every clock; the collector is off only while the clock runs.
                    gc.collect()
                    gc.disable()
                conn.send(("armed", None))
                while flag.value != gen:
                    pass
                r.trace = [] if os.environ.get("MODEST_BENCH_TRACE") else None
                seg0 = torch.cuda.memory_stats().get("segment.all.allocated", 0) if r.trace is not None else 0
                dt, kms = r.timed(int(n), ingest=ingest, keep_last=keep)
                if r.trace is not None:
                    r.trace.append(("torch_segments_allocated_x1000", 1.0 * (torch.cuda.memory_stats().get("segment.all.allocated", 0) - seg0)))   # diagnostics: where a helper's share of the timed region went (host wall time)
                    print(f"[helper {slot}] {n} steps {dt * 1e3:.2f} ms: " + " ".join(f"{k} {v * 1e3:.2f}" for k, v in r.trace),
                          file=sys.stderr, flush=True)
                    r.trace = None
                gc.enable()
                conn.send(("done", (dt, kms.tolist(), r.last_paths)))
            elif cmd == "outputs":
                conn.send(("outputs", step_arrays(r.last_out) if r.last_out is not None else None))
            elif cmd == "iso":
                conn.send(("iso", r.isolated_pp_ms()))
            elif cmd == "iso_realistic":
                conn.send(("iso_realistic", realistic_pp(r)))
            else:
                break
    except BaseException as e:   # reported, the parent falls back to the in-process path
        try:
            conn.send(("error", repr(e)))
        except Exception:
            pass


def _split(n, parts):
    return [n // parts + (1 if k < n % parts else 0) for k in range(parts)]


def helper_count(procs: int, steps: int) -> int:
    """Helpers actually used: every one gets at least MIN_STEPS_PER_HELPER steps."""
    return max(1, min(procs, steps // MIN_STEPS_PER_HELPER))


# --------------------------------------------------------------------------- --dump-outputs
DUMP_CAP_BYTES = 64 << 20
LABEL_FIELDS = 14   # "Dynamic -1 -1" + alpha, 2-D box (4), h, w, l, t (3), ry: every field after the class name


def label_fields(text):
    """KITTI label text -> (k, 14) float64, the numeric fields of every line"""
    rows = [[float(v) for v in line.split()[1:]] for line in text.splitlines() if line.strip()]
    return np.asarray(rows, dtype=np.float64).reshape(-1, LABEL_FIELDS)


def step_arrays(out):
    """what a caller of the timed path receives for one scan, (H, labels, objs, text), as float arrays -> {name: array}"""
    H, labels, objs, text = out
    res = {"pp_score": H.detach().cpu().numpy() if torch.is_tensor(H) else np.asarray(H)}
    if labels is not None:   # (--pp-only: the PP score is all the step computes)
        res["cluster_labels"] = np.asarray(labels)
        res["boxes"] = np.asarray(objs).reshape(-1, 8)
        res["label_fields"] = label_fields(text)
    return {k: (v if v.dtype in (np.float32, np.float64) else v.astype(np.float64)) for k, v in res.items()}


def write_outputs(d, arrays, cap=DUMP_CAP_BYTES):
    """DIR/<name>.npy for every array.  Over `cap` bytes in all, the per-point arrays (pp_score, cluster_labels) keep a
    fixed, seeded sample of their points, whose indices are written as point_index."""
    per_point = [k for k in ("pp_score", "cluster_labels") if k in arrays]
    n = len(arrays["pp_score"])
    if sum(v.nbytes for v in arrays.values()) > cap:
        rest = sum(v.nbytes for k, v in arrays.items() if k not in per_point)
        row = 8 + sum(arrays[k].itemsize for k in per_point)   # (+ the float64 point index)
        idx = np.sort(np.random.RandomState(0).choice(n, max(0, min(n, (cap - rest) // row)), replace=False))
        arrays = dict(arrays, point_index=idx.astype(np.float64), **{k: arrays[k][idx] for k in per_point})
    os.makedirs(d, exist_ok=True)
    for k, v in arrays.items():
        np.save(os.path.join(d, k + ".npy"), np.ascontiguousarray(v))
    return sorted(arrays)


# --------------------------------------------------------------------------- CPU baselines
def _cpu_one_scan(args):
    """best-effort CPU worker: one process per scan, multi-threaded neighbour queries"""
    sid, n_live, trav, frames, pp_only, nusc = args
    from modest_amd import synth
    from oracle import labels as ol
    from oracle import mask as om
    from oracle import pp_score as opp
    sh = synth.make_shard(1, n_live=n_live, n_trav=trav, n_frames=frames, seed=sid, nusc=nusc)
    live_xyz, hist = sh.stacked(0)
    live_raw = sh.scans[0].live_raw
    del sh
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "c.txt"), "w").write(synth.CALIB_TXT)
        ocalib = ol.Calibration(os.path.join(d, "c.txt"))
    t0 = time.perf_counter()
    H, _ = opp.pp_score(live_xyz, hist, 0.3, workers=-1)
    if not pp_only:
        cfg = None
        if nusc:
            import copy
            cfg = copy.deepcopy(om.DEFAULT_CFG)
            cfg["plane_estimate"]["max_hs"] = -1.3
        ref = om.generate_mask_scan(live_raw, H, ocalib, cfg=cfg, random_state=np.random.RandomState(0), n_jobs=-1)
        ol.gen_label_scan(ref["objs"], ocalib, **({"image_shape": (900, 1600)} if nusc else {}))
    return t0, time.perf_counter()


def cpu_best_effort(a):
    """SURVEY 8d baseline (B): query_ball_point(workers=-1), sklearn n_jobs=-1, one process per scan,
    all scans at once.  Throughput = scans / (last end - first start of the processing phases)."""
    import multiprocessing as mp
    n = a.cpu_best_effort
    ctx = mp.get_context("spawn")
    with ctx.Pool(processes=n) as pool:
        spans = pool.map(_cpu_one_scan, [(5000 + i, a.n_live, a.traversals, a.frames, a.pp_only, bool(a.nusc)) for i in range(n)])
    t_lo, t_hi = min(s[0] for s in spans), max(s[1] for s in spans)
    return n / (t_hi - t_lo), t_hi - t_lo


# --------------------------------------------------------------------------- CLI measurement
def cli_bench(a, local):
    """The three product CLIs on a synthetic KITTI tree shaped like a Lyft shard: one live sequence
    and 10 history sequences, 36 history frames per traversal per scan, consecutive live scans share
    35 of them.  Everything is included: .bin reads, upload + tile sort of new frames, batched pose
    solves, kernels, .npy/.pkl/.txt writes.  Every CLI runs twice: one process, and `workers=N`
    (N child processes on the GPU; their own loop clocks, i.e. without interpreter start-up)."""
    from modest_amd import gen_label_files, generate_mask, pre_compute_pp_score, synth
    n_scan, F, T, W = int(a.cli_scans), int(a.frames), int(a.traversals), max(2, int(a.cli_workers))
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    out = {}
    with tempfile.TemporaryDirectory(dir=base) as root:
        t0 = time.perf_counter()
        paths = synth.write_kitti_tree(os.path.join(root, "kitti"), os.path.join(root, "meta"), n_seq=T + 1,
                                       n_frames=n_scan + F, n_pts=a.n_live, origins=tuple(range(n_scan)),
                                       hist_frames=F, max_range=80.0)
        out["tree_seconds"] = time.perf_counter() - t0
        data = f"data_root={root}/kitti/training"
        idx = f"data_paths.idx_list={paths['idx_list']}"

        def pp(tag, workers):
            tot = pre_compute_pp_score.main(argv=[data, f"data_paths.track_path={paths['track_path']}",
                                                  f"data_paths.idx_info={paths['idx_info']}", idx,
                                                  f"data_paths.pp_score_path={root}/pp{tag}", f"device={local}",
                                                  f"workers={workers}"])
            return tot["scans"] / tot.get("max_worker_seconds", tot["max_seconds"])

        def mask(tag, workers):
            tot = generate_mask.main(argv=[data, idx, f"data_paths.pp_score_path={root}/pp1",
                                           f"data_paths.seg_save_dst={root}/seg{tag}",
                                           f"data_paths.bbox_info_save_dst={root}/bbox{tag}", f"device={local}",
                                           f"workers={workers}"])
            return tot["scans"] / tot.get("max_worker_seconds", tot["max_seconds"])

        out["pp_scans_per_s"] = pp("1", 1)
        out["mask_scans_per_s"] = mask("1", 1)
        tot = gen_label_files.main(argv=[data, idx, f"data_paths.bbox_info_save_dst={root}/bbox1",
                                         f"data_paths.label_file_save_dst={root}/labels", f"device={local}"])
        out["label_scans_per_s"] = tot["scans"] / tot["max_seconds"]
        out["pipeline_scans_per_s"] = 1.0 / (1.0 / out["pp_scans_per_s"] + 1.0 / out["mask_scans_per_s"]
                                             + 1.0 / out["label_scans_per_s"])
        out["label_files"] = len([f for f in os.listdir(f"{root}/labels") if f.endswith(".txt")])
        out["workers"] = W
        out["pp_scans_per_s_workers"] = pp("W", W)
        out["mask_scans_per_s_workers"] = mask("W", W)
        tot = gen_label_files.main(argv=[data, idx, f"data_paths.bbox_info_save_dst={root}/bboxW",
                                         f"data_paths.label_file_save_dst={root}/labelsW", f"device={local}", f"workers={W}"])
        out["label_scans_per_s_workers"] = tot["scans"] / tot.get("max_worker_seconds", tot["max_seconds"])
        out["pipeline_scans_per_s_workers"] = 1.0 / (1.0 / out["pp_scans_per_s_workers"] + 1.0 / out["mask_scans_per_s_workers"]
                                                     + 1.0 / max(out["label_scans_per_s_workers"], out["label_scans_per_s"]))
        # the fused CLI: the three stages per batch in one process (modest_amd/seed_labels.py), every file of the three CLIs written
        from modest_amd import seed_labels

        def fused(tag, workers):
            tot = seed_labels.main(argv=[data, f"data_paths.track_path={paths['track_path']}", f"data_paths.idx_info={paths['idx_info']}", idx,
                                         f"data_paths.pp_score_path={root}/fpp{tag}", f"data_paths.seg_save_dst={root}/fseg{tag}",
                                         f"data_paths.bbox_info_save_dst={root}/fbbox{tag}", f"data_paths.label_file_save_dst={root}/flabels{tag}",
                                         f"device={local}", f"workers={workers}"])
            return tot["scans"] / tot.get("max_worker_seconds", tot["max_seconds"])

        try:
            out["fused_scans_per_s"] = fused("1", 1)
            out["fused_scans_per_s_workers"] = fused("W", W)
            same = True
            for a_, b_ in (("labels", "flabels1"), ("labels", "flabelsW"), ("seg1", "fseg1"), ("seg1", "fsegW"), ("pp1", "fpp1"), ("pp1", "fppW"),
                           ("bbox1", "fbbox1"), ("bbox1", "fbboxW")):
                for f in os.listdir(f"{root}/{a_}"):
                    if f != "configs.yaml" and open(f"{root}/{a_}/{f}", "rb").read() != open(f"{root}/{b_}/{f}", "rb").read():
                        same = False
            out["fused_outputs_identical"] = same
        except Exception as e:   # noqa: BLE001
            out["fused_error"] = repr(e)
        out["label_files_identical"] = all(open(f"{root}/labels/{f}").read() == open(f"{root}/labelsW/{f}").read()
                                           for f in os.listdir(f"{root}/labels") if f.endswith(".txt"))
        diff = [f for f in sorted(os.listdir(f"{root}/seg1")) if f.endswith(".npy") and
                open(f"{root}/seg1/{f}", "rb").read() != open(f"{root}/segW/{f}", "rb").read()]
        out["workers_outputs_identical"] = not diff
        if diff:
            out["workers_outputs_differing"] = diff[:8]
    out["scans"] = n_scan
    out["note"] = (f"{n_scan} live scans x {T} traversals x {F} frames of {a.n_live} points, one GPU, tree on "
                   + (base or "the default tmp dir") + "; cold: the first scan of a process uploads and sorts all 361 "
                   "frames, later scans 11 new ones; *_workers: max over the workers' own loop clocks; "
                   "pipeline_scans_per_s_workers takes the label stage in whichever mode is faster (it is 0.1 ms of work per scan); "
                   "fused_*: python -m modest_amd.seed_labels, the three stages per batch in one process (per worker), all four output trees "
                   "compared with the separate CLIs' byte for byte")
    return out


def main():
    argv = sys.argv[1:]
    a = parse(argv)
    from modest_amd import dist
    if int(os.environ.get("WORLD_SIZE", "1")) <= 1 and a.gpus <= 1:
        dist.runtime_defaults()   # (before the first HIP call of this process; the helper processes inherit the environment)
    maybe_relaunch(a, argv)
    from modest_amd import ops, synth

    rank, ws, local = dist.init()
    if ws > 1 and torch.cuda.is_available():
        local = local % max(torch.cuda.device_count(), 1)   # (ranks that share a device: MODEST_DIST_BACKEND=gloo)
    # a rank of a multi-GPU run keeps the runtime's own wait mode for itself (RCCL); its helper processes, which do the
    # pipeline's work and are single-rank, poll (dist.runtime_defaults): they inherit the environment as it is from here on
    os.environ.setdefault("HSA_ENABLE_INTERRUPT", "0")
    if ws != a.gpus:
        raise SystemExit(f"bench.py: --gpus {a.gpus} but the launcher started WORLD_SIZE={ws} rank(s); "
                         f"run `python bench.py --gpus {a.gpus}` (it launches its own ranks) or make them agree")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the hot path has no CPU fallback")
    torch.cuda.set_device(torch.device("cuda", local))
    rccl_ws = torch.distributed.get_world_size() if (ws > 1 and torch.distributed.is_initialized()) else 1
    rccl_check = dist.selfcheck()   # backend / world size / ranks counted by an all-reduce of ones (not read from the environment)

    helpers, note, M = [], None, None
    startup = {"helper_seconds": [], "helper_peak_rss_mb": []}
    t_start = time.perf_counter()
    # A rank's helpers cost the host ~6 busy threads each inside the clock (measured: config.host_budget_per_rank -- a polling main
    # thread, the runtime's signal thread, pose / reader / writer threads): 8 ranks x 8 helpers would want ~400 of this host's threads.
    # With several ranks the pool is capped so that all ranks' helpers fit the host's hardware threads.
    if ws > 1 and a.procs > 1:
        fit = max(2, (os.cpu_count() or 64) // (ws * 6))
        if fit < a.procs:
            print(f"[bench] rank {rank}: {a.procs} helper processes x {ws} ranks exceed the host's {os.cpu_count()} threads: {fit} per rank", file=sys.stderr)
            a.procs = fit
    n_procs = helper_count(a.procs, a.steps)
    deal = os.environ.get("MODEST_WINDOW_DEAL")   # (experiments: "8,6,4,2" = the contract region's scans per helper)
    shares = None
    if deal and sum(int(x) for x in deal.split(",")) == a.steps and len(deal.split(",")) <= max(1, a.procs):
        shares = [int(x) for x in deal.split(",")]
        n_procs = len(shares)
    # the helpers beyond the contract region's serve the steady-state region of --full alone: a plain run starts none of them
    n_pool = max(1, a.procs) if a.full else n_procs
    flag = None
    if a.procs > 1:
        import multiprocessing as mp
        ctx = mp.get_context("spawn")
        flag = ctx.Value("i", 0, lock=False)
        try:
            for slot in range(n_pool):
                pc, cc = ctx.Pipe()
                p = ctx.Process(target=_helper_main, args=(cc, a, rank, local, slot, flag), daemon=True)
                p.start()
                helpers.append((p, pc))
            for p, pc in helpers:
                if not pc.poll(900):
                    raise RuntimeError("helper process did not come up")
                tag, msg = pc.recv()
                if tag != "ready":
                    raise RuntimeError(f"helper process failed: {msg}")
                M = int(msg[0])
                startup["helper_seconds"].append(round(float(msg[1]), 2))     # shard generation + upload + warm-up of the helper
                startup["helper_peak_rss_mb"].append(round(float(msg[2]), 1))
        except Exception as e:   # e.g. no semaphores / fork limits on this host: stay inside the rank process
            note = f"helper processes unavailable ({e}); ran in the rank process"
            for p, pc in helpers:
                try:
                    pc.send(("exit", None))
                except Exception:
                    pass
                p.join(5)
                if p.is_alive():
                    p.terminate()
            helpers, n_procs, n_pool = [], 1, 1
            a.streams = max(a.streams, 4)   # threads instead
    runner = Runner(a, rank, local, 0) if not helpers else None
    startup["pool_seconds"] = round(time.perf_counter() - t_start, 2)   # until every helper (or the in-process runner) is ready
    generation = [0]

    def timed_region(active, shares, ingest=False, keep_last=False):
        """barrier + synchronise, the helpers run their shares, synchronise + barrier; rank wall clock.  keep_last: the last
        helper keeps its last step's outputs (('outputs', None) after the region)"""
        for q, ((p, pc), n) in enumerate(zip(active, shares)):
            pc.send(("arm", (n, generation[0] + 1, ingest, keep_last and q == len(active) - 1)))
        for p, pc in active:
            tag, msg = pc.recv()
            if tag != "armed":
                raise RuntimeError(f"helper process failed: {msg}")
        torch.cuda.synchronize()
        dist.barrier()
        t0 = time.perf_counter()
        generation[0] += 1
        flag.value = generation[0]          # every armed helper starts now
        kms, paths = [], []
        for p, pc in active:
            tag, msg = pc.recv()            # a helper synchronises its streams before it answers
            if tag != "done":
                raise RuntimeError(f"helper process failed: {msg}")
            kms.append(np.asarray(msg[1], dtype=np.float32))
            paths.append(msg[2])
        torch.cuda.synchronize()
        dist.barrier()
        timed_region.paths = paths
        return time.perf_counter() - t0, np.concatenate(kms)

    def host_cpu_seconds():
        """user + system seconds of this rank's process and of its helper processes so far"""
        try:
            import psutil
            me = psutil.Process()
            tot = 0.0
            for pr_ in [me] + me.children(recursive=True):
                try:
                    ct = pr_.cpu_times()
                    tot += ct.user + ct.system
                except psutil.Error:
                    pass
            return tot
        except Exception:
            return time.process_time()

    def host_rss_mb():
        try:
            import psutil
            me = psutil.Process()
            return sum(pr_.memory_info().rss for pr_ in [me] + me.children(recursive=True)) / 2 ** 20
        except Exception:
            import resource
            return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0

    cpu0 = host_cpu_seconds()
    dump = bool(a.dump_outputs) and rank == 0
    if helpers:
        dt, kernel_ms = timed_region(helpers[:n_procs], shares or _split(a.steps, n_procs), keep_last=dump)
        paths = timed_region.paths
    else:
        runner.rehearse(a.steps)
        torch.cuda.synchronize()
        dist.barrier()
        t0 = time.perf_counter()
        _, kernel_ms = runner.timed(a.steps, keep_last=dump)
        torch.cuda.synchronize()
        dist.barrier()
        dt = time.perf_counter() - t0
        paths = [runner.last_paths]
    # what a rank costs its host (an 8-GPU node carries 8 of these): busy threads = CPU seconds of the rank process and
    # its helpers inside the contract clock / the clock (a polling helper counts as one whether or not it has work), resident memory
    mine = dict(rank=rank, busy_threads=round((host_cpu_seconds() - cpu0) / max(dt, 1e-9), 2), rss_mb=round(host_rss_mb(), 1),
                processes=1 + len(helpers))
    if dump:   # the last step of the contract region (with helpers: the last step of the last helper's share)
        outputs = None
        if helpers:
            helpers[n_procs - 1][1].send(("outputs", None))
            tag, outputs = helpers[n_procs - 1][1].recv()
            if tag != "outputs":
                raise RuntimeError(f"helper process failed: {outputs}")
        elif runner.last_out is not None:
            outputs = step_arrays(runner.last_out)
        if outputs is None:
            raise RuntimeError("--dump-outputs: the timed region ran no step")
        write_outputs(a.dump_outputs, outputs)
    host_budget = [mine]
    if ws > 1 and torch.distributed.is_initialized():
        host_budget = [None] * ws
        torch.distributed.all_gather_object(host_budget, mine)
    red = dist.reduce_counters(dict(max_seconds=dt, scans=a.steps))
    dt_max, total_scans = red["max_seconds"], red["scans"]
    steady = None
    if a.full and helpers and (n_procs < n_pool or a.steps < STEADY_STEPS_PER_HELPER * n_pool):   # few steps: also the pool's steady state
        n_ss = STEADY_STEPS_PER_HELPER * n_pool
        dt_ss, _ = timed_region(helpers, _split(n_ss, n_pool))
        red_ss = dist.reduce_counters(dict(max_seconds=dt_ss, scans=n_ss))
        steady = {"value": red_ss["scans"] / red_ss["max_seconds"], "unit": "scans/s", "steps": n_ss,
                  "host_processes_per_gpu": n_pool,
                  "note": "same bracket (barrier + synchronise on both sides) as the contract region, run after it"}

    # the same pool, every step bringing in its 11 new frames and building its descriptor table from raw poses
    with_ingest = None
    # (the region's first block has nothing ahead of it: its PP call waits for its own copy + sort behind whatever the other helpers have
    # queued -- 20-25 ms once per helper, MODEST_BENCH_TRACE=1 -- so the region is twice the contract region: four to five blocks per helper)
    n_wi = max(2 * a.steps, STEADY_STEPS_PER_HELPER * n_pool) if helpers else a.steps
    if a.full:
        if helpers:
            dt_wi, _ = timed_region(helpers, _split(n_wi, n_pool), ingest=True)
        else:
            runner.rehearse_ingest()
            torch.cuda.synchronize()
            dist.barrier()
            t0 = time.perf_counter()
            runner.timed(n_wi, ingest=True)
            torch.cuda.synchronize()
            dist.barrier()
            dt_wi = time.perf_counter() - t0
        red_wi = dist.reduce_counters(dict(max_seconds=dt_wi, scans=n_wi))
        with_ingest = {"value": red_wi["scans"] / red_wi["max_seconds"], "unit": "scans/s", "steps": n_wi,
                       "per_step": "11 raw frames (one per traversal + the live scan) pinned host -> device + tile sort "
                                   "(one copy, one launch), get_relative_pose of all 361 frames from the raw pose factors, "
                                   "descriptor table built from the store; then the same pipeline",
                       "new_frame_bytes_per_step": 11 * a.n_live * 16}

    # the same stage with nothing else on the GPU (the timed region has several scans in flight, so its
    # event pairs also see the other scans' kernels): informational, not the reported `achieved`
    iso_ms, iso_B, iso_block, real = None, 1, False, None
    if rank == 0 and a.full:
        if helpers:
            helpers[0][1].send(("iso", None))
            iso = helpers[0][1].recv()[1]
        else:
            iso = runner.isolated_pp_ms()
        if iso:
            iso_ms, iso_B, iso_block = float(iso[0]), int(iso[1]), bool(iso[2])   # ms per call, scans per call, block path
        if a.sharing == "realistic":
            try:
                if helpers:
                    helpers[0][1].send(("iso_realistic", None))
                    real = helpers[0][1].recv()[1]
                else:
                    real = realistic_pp(runner)
            except Exception as e:
                real = {"error": repr(e)}
    for p, pc in helpers:
        pc.send(("exit", None))
    for p, pc in helpers:
        p.join(30)
    n_threads = max(1, a.streams)

    if runner is not None:
        M = runner.scans[0].M
    alg_bytes = 12 * M + 16 * a.n_live
    k_ms = float(np.mean(kernel_ms)) if len(kernel_ms) else None   # None, not NaN: the line must stay strict JSON
    contended = alg_bytes / (k_ms * 1e-3) / 1e9 if k_ms else None
    # top level = the stage alone on the GPU (the figure that follows from profiles/*_pp_only_kernel_stats.csv);
    # the event pairs of the timed region also bracket the other scans' kernels and are reported as `in_pipeline`
    achieved = iso_B * alg_bytes / (iso_ms * 1e-3) / 1e9 if iso_ms else contended
    traffic, traffic_src = None, None
    tnames = (("r06_pp_block_traffic.json", "r05_pp_block_traffic.json", "r05_c5_pp_block_traffic.json", "r04_pp_block_traffic.json") if iso_block else ()) + ("r03_pp_traffic.json", "r02_pp_traffic.json", "r01_pp_traffic.json")
    for tname in tnames:
        tpath = os.path.join(ROOT, "profiles", tname)
        if os.path.exists(tpath):   # PMC counters cannot be read from inside the process: separate rocprofv3 --pmc passes
            tj = json.load(open(tpath))
            if int(tj.get("algorithmic_bytes_per_scan", 0)) == alg_bytes and (iso_block == bool(tj.get("block_path", False))):
                traffic, traffic_src = tj["hbm_bytes_per_scan"] * (iso_B if iso_ms else 1), f"profiles/{tname} (" + tj["source"] + ")"   # per launch, like `achieved`
                break
    pp_B = max(1, min(a.pp_batch, a.shard_scans, a.scans))
    # what ran inside the contract clock (counted by the helpers' frame stores between the two barriers)
    n_block = sum(p["block_calls"] for p in paths)
    n_chain = sum(p["chain_calls"] for p in paths)
    spc = [b for p in paths for b in p["scans_per_call"]]
    pp_path = "block" if n_block and not n_chain else ("chain" if n_chain and not n_block else ("mixed" if n_block else "none"))
    kernel_txt = (f"PP neighbour count of a BLOCK of {iso_B} consecutive scans of a shard, ONE call (modest_pp_score_block): list sizes "
                  "from the frames' tile tables (b4_counts / b4_lists / b4_bases) + ONE pass over the union of the block's frames "
                  f"(b4_scatter: {a.frames} + {iso_B - 1} frames per traversal instead of {iso_B} x {a.frames}) + counting sort of the tile lists by cell "
                  "(b4_seg_*) + per scan: live index on the lattice (b4_live_*, b4_scan_*), plan (b4_plan_*), sort-free join "
                  "(b4_join: records read into registers, the scan's float32 pose applied per record, packed-float pair tests): "
                  "ALL launches of the call, HIP events on the launch stream"
                  if iso_block else
                  f"PP neighbour count, ONE chain of launches for {iso_B} scan(s) (modest_pp_score_frames_batch: every "
                  "kernel takes the scan as blockIdx.y) = live prep (transform + bounding box + clears) + live index "
                  "build (5 launches) + pp3_stream<count> + pp3_scan + pp3_plan + pp3_stream<scatter> + pp3_join: ALL "
                  "launches of the stage, HIP events on the launch stream; the history is read from the frame store "
                  "through the descriptor table (pose fused), not from a stacked copy")
    roofline = {"bound": "hbm",
                "kernel": kernel_txt, "block_path": iso_block,
                "achieved": achieved,
                "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": (achieved / HBM_PEAK_GBPS) if achieved else None,
                "traffic": traffic, "traffic_source": traffic_src,
                "traffic_per_scan": (traffic / (iso_B if iso_ms else 1)) if traffic else None,
                "scans_per_launch": iso_B if iso_ms else 1,
                "algorithmic_bytes_per_launch": (iso_B if iso_ms else 1) * alg_bytes,
                "algorithmic_bytes_per_scan": alg_bytes,
                "kernel_ms": iso_ms if iso_ms else k_ms,
                "kernel_ms_per_scan": (iso_ms / iso_B) if iso_ms else k_ms,
                "measured": (f"HIP events on the launch stream around the call, one call at a time on an otherwise idle GPU, cycling "
                             f"through the {a.scans} resident scans = {max(1, a.scans // max(1, a.shard_scans))} shard(s) of "
                             f"{a.shard_scans} consecutive scans (every shard: {(a.frames + a.shard_scans - 1) * a.traversals} "
                             "history frames; frames + block store of a shard exceed the 256 MiB Infinity Cache), after the timed "
                             "region; algorithmic bytes = 12 B x the 10.8 M history points of EVERY scan + 16 B x its live points, "
                             "whether or not consecutive scans share frames") if iso_ms else "HIP events in the timed region",
                "in_pipeline": {"kernel_ms_per_scan": k_ms, "achieved": contended,
                                "frac": (contended / HBM_PEAK_GBPS) if contended else None,
                                "scans_timed": int(len(kernel_ms)),
                                "scans_per_launch": (float(np.mean(spc)) if spc else None),   # measured: scans per PP call inside the clock
                                "pp_calls": {"modest_pp_score_block": n_block, "modest_pp_score_frames_batch": n_chain},
                                "note": "the same event pairs inside the timed region, divided by the scans of their chain: "
                                        "several chains are in flight on grids sized for part of the GPU, a pair also brackets "
                                        "the other processes' kernels"},
                "isolated": {"kernel_ms": iso_ms, "scans_per_launch": iso_B,
                             "frac": (iso_B * alg_bytes / (iso_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS) if iso_ms else None}}

    roofline["sharing"] = ("best case: windows of frames i..i+F-1, consecutive scans share F-1 of F frames per traversal "
                           "(union of a block of 16 = 1.42 x a scan's frames)")
    roofline_real = None
    if real and "error" not in real:
        alg_r = 12.0 * real["history_points"] + 16 * a.n_live   # (a repeated frame is stacked, and counted, as often as it is listed)
        ach_r = real["scans"] * alg_r / (real["ms"] * 1e-3) / 1e9
        roofline_real = {"bound": "hbm", "achieved": ach_r, "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": ach_r / HBM_PEAK_GBPS,
                         "traffic": None, "block_path": real["block"], "kernel_ms": real["ms"], "scans_per_launch": real["scans"],
                         "kernel_ms_per_scan": real["ms"] / real["scans"], "algorithmic_bytes_per_scan": alg_r,
                         "sharing": dict(real["sharing"], rule="history windows chosen by the reference's rule (data_preprocessing/lyft/"
                                         "split_traintest.py:79-101: closest frame + the first frame beyond 2, 4, ..., 70 m; nuScenes: "
                                         "2, ..., 30 m), live vehicle 8 m/s, history traversals 3-15 m/s at 5 Hz; repeated frames kept"),
                         "measured": "same isolated measurement as `roofline` (one modest_pp_score_block call at a time, HIP events), 8 calls; "
                                     "profiles/r05_sharing_sensitivity.json has the other speed buckets"}
    elif real:
        roofline_real = real
    # The line's `roofline` is the REALISTIC figure: windows chosen as split_traintest.py:79-101 chooses them, repeated
    # frames kept, traversals that enter and leave (T changes inside the block) -- the shape a real valid_idx_info.pkl holds.  The windows
    # of frames i..i+F-1 that every timed region of this file runs on (35 of 36 frames shared: the best case) stay as `roofline_best_case`.
    roofline_best = roofline
    if roofline_real and "error" not in roofline_real:
        tname = "r06_pp_block_traffic_realistic.json"
        tpath = os.path.join(ROOT, "profiles", tname)
        if os.path.exists(tpath) and roofline_real.get("block_path"):
            tj = json.load(open(tpath))
            roofline_real["traffic"] = tj["hbm_bytes_per_scan"] * roofline_real["scans_per_launch"]   # per launch, like `achieved`
            roofline_real["traffic_per_scan"] = tj["hbm_bytes_per_scan"]
            roofline_real["traffic_source"] = f"profiles/{tname} (" + tj["source"] + ")"
        roofline_real["kernel"] = kernel_txt
        roofline_real["algorithmic_bytes_per_launch"] = roofline_real["algorithmic_bytes_per_scan"] * roofline_real["scans_per_launch"]
        roofline = roofline_real
    else:
        roofline = dict(roofline_best, note="the realistic-sharing measurement was not taken (--sharing best, or it failed: see roofline_realistic_error); "
                                            "this is the best-case figure")
    if not a.full:   # (the roofline figures rest on the isolated PP measurements, taken with --full only)
        roofline = roofline_best = roofline_real = None
    cpu_baseline = None
    parity = None
    cli = None
    # the CLI leg first: with the CPU baselines (and the joblib worker processes they leave behind) before it, the first CLI
    # phase came out 3-4x slower in two of about ten default runs; stand-alone runs of the same CLI never did
    if a.full and rank == 0 and ws == 1 and a.cli_scans > 0 and not a.pp_only and not a.nusc:
        try:
            cli = cli_bench(a, local)
        except Exception as e:
            cli = {"error": repr(e)}
    if a.full and rank == 0 and ws == 1 and a.cpu_scans > 0:
        from oracle import labels as ol
        from oracle import mask as om
        from oracle import pp_score as opp
        with tempfile.TemporaryDirectory() as d:
            open(os.path.join(d, "c.txt"), "w").write(synth.CALIB_TXT)
            ocalib = ol.Calibration(os.path.join(d, "c.txt"))
        # the sample = the first scans helper 0 (or the rank process) benchmarked: same generator, same seeds
        n_cpu = min(a.cpu_scans, a.scans, a.shard_scans, max(1, min(a.pp_batch, a.shard_scans, a.scans)))
        # (+ one warm-up scan, the shard's next one: BASELINE.md section 3 -- 1 warm-up + the median of >= 5 scans)
        hsh = synth.make_shard(n_cpu + 1, n_live=a.n_live, n_trav=a.traversals, n_frames=a.frames, seed=scan_seed(rank, 0, 0), nusc=a.nusc)
        ocfg = None
        if a.nusc:
            import copy
            ocfg = copy.deepcopy(om.DEFAULT_CFG)
            ocfg["plane_estimate"]["max_hs"] = -1.3
        stacked = [hsh.stacked(i) for i in range(n_cpu + 1)]
        refs, per_scan = [], []
        for i in [n_cpu] + list(range(n_cpu)):   # (the warm-up scan first, untimed: page cache, thread pools, joblib workers)
            live_xyz, hist = stacked[i]
            t1 = time.perf_counter()
            Href, cref = opp.pp_score(live_xyz, hist, 0.3, workers=1)       # reference: single thread
            ref = None
            if not a.pp_only:
                ref = om.generate_mask_scan(hsh.scans[i].live_raw, Href, ocalib, random_state=np.random.RandomState(i), n_jobs=-1,
                                            **({"cfg": ocfg} if ocfg else {}))
                ref["text"] = ol.gen_label_scan(ref["objs"], ocalib, **({"image_shape": (900, 1600)} if a.nusc else {}))
            if i < n_cpu:
                per_scan.append(time.perf_counter() - t1)
                refs.append((Href, cref, ref))
        tc = float(np.sum(per_scan))
        t_med = float(np.median(per_scan))
        del stacked
        # parity of the measured path against the checker, outside every timed region: the first block of helper 0's first
        # shard (the scans the CPU sample took are its first ones) through ONE PP call, as the timed region runs it
        pa = argparse.Namespace(**vars(a))
        pa.scans, pa.warmup, pa.streams = min(a.shard_scans, a.scans), 0, 1
        pr = Runner(pa, rank, local, 0)
        nblk = pr.PB
        Hgs, cgs = pr.store.pp_score_batch([sc.live_key for sc in pr.scans[:nblk]], [sc.desc for sc in pr.scans[:nblk]],
                                           pr.scans[0].T, ctx=pr.ctxs[0], return_counts=True, block=pr.block)
        Href, cref, ref = refs[0]
        parity = {"pp_counts_equal": bool(all(np.array_equal(cg.cpu().numpy().astype(np.int64), r[1])
                                              for cg, r in zip(cgs, refs))),
                  "pp_max_abs_err": float(max(np.max(np.abs(Hg.cpu().numpy().astype(np.float64) - r[0]))
                                              for Hg, r in zip(Hgs, refs))),
                  "pp_scans_per_call": len(cgs), "pp_scans_checked": n_cpu,
                  "pp_block_path": getattr(pr.store, "block_calls", 0) > 0}
        if ref is not None:
            got = []
            pr.run(0, 1, collect=got)
            _, (_, labels, objs, text) = got[0]
            parity["labels_equal"] = bool(np.array_equal(labels, ref["labels"]))
            parity["n_objs"] = [len(objs), len(ref["objs"])]
            parity["label_text_equal"] = bool(text == ref["text"][0])
        del pr
        cpu_baseline = {"value": 1.0 / t_med, "unit": "scans/s", "cores": os.cpu_count(), "kind": "port",
                        "seconds_per_scan": [round(x, 3) for x in per_scan], "mean_value": n_cpu / tc,
                        "sample": f"median of {n_cpu} of the benchmarked scans timed one by one after one untimed warm-up scan "
                                  f"({'PP stage only' if a.pp_only else 'full pipeline'}); "
                                  "reference threading: cKDTree build+query 1 thread, sklearn n_jobs=-1 on all "
                                  f"{os.cpu_count()} host threads; {tc:.1f} s.  The oracle fills the affinity weights with "
                                  "one vectorised numpy expression where the reference loops over CSR rows in Python "
                                  "(oracle/mask.py:113-121): it is faster than the reference there, i.e. conservative"}
        if a.cpu_best_effort > 0:
            try:
                v, secs = cpu_best_effort(a)
                cpu_baseline["best_effort"] = {
                    "value": v, "unit": "scans/s", "cores": os.cpu_count(),
                    "sample": f"{a.cpu_best_effort} scans of the same generator, one process per scan in parallel, "
                              f"query_ball_point(workers=-1), sklearn n_jobs=-1; {secs:.1f} s"}
            except Exception as e:
                cpu_baseline["best_effort"] = {"error": repr(e)}

    if rank == 0:
        value = total_scans / dt_max
        line = {
            "metric": "LiDAR scans/sec through PP-score+cluster seed-label pipeline",
            "value": value, "unit": "scans/s", "n_gpus": ws, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": dt_max / a.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": (("C2 PP-score only" if a.pp_only else
                                     ("C5 nuScenes-shape stress, full pipeline" if a.nusc else
                                      "C3 full pipeline (PP + RANSAC + DBSCAN + box fit + iou3d NMS + labels)"))
                                    + f", {'nuScenes' if a.nusc else 'Lyft'}-shape: {a.n_live} live pts vs {a.traversals} traversals x "
                                      f"{a.frames} frames = {M} history pts"
                                    + (" (remove_center on the history, max_hs=-1.3, 900x1600)" if a.nusc else "")),
                       "live_points": a.n_live, "history_points": M, "traversals": a.traversals,
                       "frames_per_traversal": a.frames, "radius": 0.3, "scans_per_rank": a.steps,
                       "history_input": "frame store + descriptor table (no stacked history)",
                       "host_processes_per_gpu": n_procs, "threads_per_process": n_threads,
                       "scans_in_flight_per_gpu": n_procs * n_threads, "note": note,
                       "pp_stage_prefetch": (not (a.no_prefetch or a.pp_only or a.mask_only)),
                       "pp_scans_per_call": pp_B, "mask_scans_per_chain": a.mask_batch,
                       "pp_path_in_timed_region": pp_path,
                       "pp_calls_in_timed_region": {"modest_pp_score_block": n_block, "modest_pp_score_frames_batch": n_chain,
                                                    "scans_per_call": spc},
                       "resident_scans_per_process": a.scans, "shard_scans": a.shard_scans,
                       "history_sharing": "consecutive scans of a shard: 35 of 36 frames per traversal shared with the predecessor "
                                          "(data_preprocessing/lyft/split_traintest.py:64,97; SURVEY 8d C4)",
                       "pp_grid_cus_per_process": (a.pp_cus if (a.procs > 1 and a.pp_cus > 0 and not note) else "all"),
                       "startup": startup,
                       "host_budget_per_rank": host_budget,
                       # the process group as it ran (dist.selfcheck: an all-reduce of one 1 per rank): `rccl_world_size` is only set when
                       # the backend IS RCCL ("nccl"); ranks that share one GPU under gloo (tests) report world_size / ranks_seen alone
                       "world_size": rccl_ws, "ranks_seen": rccl_check["ranks_seen"],
                       "process_group_backend": rccl_check["backend"],
                       "rccl_world_size": (rccl_ws if rccl_check["backend"] in ("nccl", "none") else None),
                       "ransac_trial_loops": "host" if os.environ.get("MODEST_RANSAC_HOST") else "device",
                       "runtime_env": {k: os.environ.get(k) for k in ("HSA_ENABLE_INTERRUPT", "HSA_ENABLE_IPC_MODE_LEGACY",
                                                                      "GPU_MAX_HW_QUEUES")},
                       "parallelism": f"scan-sharded x{ws} (no data-path collective)",
                       "full": bool(a.full)},
            "roofline": roofline, "roofline_best_case": roofline_best,
            "roofline_realistic_error": (roofline_real if (roofline_real and "error" in roofline_real) else None),
            "cpu_baseline": cpu_baseline, "parity": parity, "cli": cli, "steady_state": steady,
            "value_with_ingest": with_ingest,
            "speedup_vs_cpu": (value / cpu_baseline["value"]) if cpu_baseline else None,
        }
        print(json.dumps(line), flush=True)
    dist.finalize()


if __name__ == "__main__":
    main()
