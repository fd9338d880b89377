"""Drop-in for OpenPCDet's ``kitti_object_eval_python/eval.py`` (plus the label readers of its ``kitti_common.py``)
with the overlaps and the statistics on the GPU (csrc/kitti_eval.hip).

Same public names and signatures, same result strings (byte for byte) and dicts.  What differs inside:
  * overlaps are computed once per frame as dt x gt blocks (not 50 dense part matrices) and shared by every class,
    difficulty and range bucket; a range bucket marks the boxes outside it ``ignored = -1`` instead of filtering
    copies of the annos (eval.py:816-832: a removed box and an ignored-(-1) box are never matched nor counted);
  * one statistics call per metric runs all configurations (class, difficulty or range, min overlap): pass A, the
    thresholds, pass B and the sums, with one host synchronise;
  * the rotated-polygon buffer holds 24 vertices, so coincident or nested boxes give their true overlap (the
    reference's 8-vertex buffer overflows there);
  * the aos similarity of a frame is summed in gt order from 0, as numba's np.sum does.

``get_coco_eval_result`` raises: the reference's ``do_coco_style_eval`` unpacks 4 of ``do_eval``'s 8 values.
"""
from __future__ import annotations

import bisect
import ctypes as C
import io as sysio
import os
import pathlib
import re

import numpy as np

PAIR_BUDGET = 1 << 25            # dt x gt pairs per batch (MODEST_EVAL_PAIR_BUDGET overrides)
N_SAMPLE_PTS = 41
TMAX = 64                        # threshold slots per configuration in the device tables

CLASS_NAMES = ['car', 'pedestrian', 'cyclist', 'van', 'person_sitting', 'truck', 'dynamic']
MIN_HEIGHT = [40, 25, 25]
MAX_OCCLUSION = [0, 1, 2]
MAX_TRUNCATION = [0.15, 0.3, 0.5]

EVAL_FRAME = np.dtype([("dt_off", "<i8"), ("gt_off", "<i8"), ("pair_off", "<i8"), ("nd", "<i4"), ("ng", "<i4")])
EVAL_CONFIG = np.dtype([("flagset", "<i4"), ("pad", "<i4"), ("min_overlap", "<f8"), ("num_valid_gt", "<i8")])


class _StatsArgs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("frames", "cfg", "dt_score", "dt_bbox", "gt_bbox", "gt_ign", "dt_ign", "gt_dc",
                                          "pair_sim", "tp_scores", "tp_count", "thresholds", "n_thresh", "partial",
                                          "sim_partial")] + \
              [("n_gt", C.c_int64), ("n_dt", C.c_int64), ("n_frames", C.c_int32), ("n_cfg", C.c_int32),
               ("metric", C.c_int32), ("max_nd", C.c_int32)]


# GPU milliseconds of the last calls, by stage (read by the CLI and tools/eval_bench.py)
last_timings = {"overlaps_ms": 0.0, "statistics_ms": 0.0}


def reset_timings():
    last_timings["overlaps_ms"] = 0.0
    last_timings["statistics_ms"] = 0.0


def pair_budget() -> int:
    return max(1, int(os.environ.get("MODEST_EVAL_PAIR_BUDGET", PAIR_BUDGET)))


# --------------------------------------------------------------------------- label readers (kitti_common.py)
_ANNO_KEYS = ('name', 'truncated', 'occluded', 'alpha', 'bbox', 'dimensions', 'location', 'rotation_y')


def _empty_anno():
    # what kitti_common.get_label_anno gives for an empty file: every list is np.array([]) (float64)
    a = {k: np.array([]) for k in _ANNO_KEYS}
    a['bbox'] = a['bbox'].reshape(-1, 4)
    a['dimensions'] = np.array([]).reshape(-1, 3)[:, [2, 0, 1]]
    a['location'] = a['location'].reshape(-1, 3)
    a['rotation_y'] = a['rotation_y'].reshape(-1)
    a['score'] = np.zeros([0])
    return a


def parse_label_texts(texts):
    """label_2 file contents (bytes) -> annos as kitti_common.get_label_anno builds them.  All numbers of all files
    are converted by one numpy call; only the token split runs per file."""
    toks, shapes = [], []
    for t in texts:
        w = t.split()
        nl = t.count(b'\n') + (1 if t and not t.endswith(b'\n') else 0)
        if not w:
            shapes.append((0, 0))
            continue
        ncol = len(t[:t.find(b'\n')].split()) if b'\n' in t else len(w)
        if ncol not in (15, 16) or len(w) != ncol * nl:
            raise ValueError("label file with %d tokens in %d lines: expected 15 or 16 per line" % (len(w), nl))
        toks.extend(w)
        shapes.append((nl, ncol))
    arr = np.array(toks, dtype=object) if toks else np.zeros(0, dtype=object)
    annos, o = [], 0
    # split names from numbers: per file the name is every ncol-th token
    name_mask = np.zeros(len(arr), dtype=bool)
    for nl, ncol in shapes:
        if nl:
            name_mask[o:o + nl * ncol:ncol] = True
            o += nl * ncol
    nums = np.array(arr[~name_mask].tolist(), dtype=np.bytes_).astype(np.float64) if len(arr) else np.zeros(0)
    names = arr[name_mask]
    o_num = o_name = 0
    for nl, ncol in shapes:
        if nl == 0:
            annos.append(_empty_anno())
            continue
        v = nums[o_num:o_num + nl * (ncol - 1)].reshape(nl, ncol - 1)
        a = {'name': np.array([s.decode() for s in names[o_name:o_name + nl]])}
        a['truncated'] = v[:, 0].copy()
        a['occluded'] = v[:, 1].astype(np.int64)
        a['alpha'] = v[:, 2].copy()
        a['bbox'] = v[:, 3:7].copy()
        a['dimensions'] = v[:, 7:10][:, [2, 0, 1]]
        a['location'] = v[:, 10:13].copy()
        a['rotation_y'] = v[:, 13].copy()
        a['score'] = v[:, 14].copy() if ncol == 16 else np.zeros([nl])
        annos.append(a)
        o_num += nl * (ncol - 1)
        o_name += nl
    return annos


def read_files(paths, readers=8):
    """the files' bytes, read by the library's parallel host reader (modest_host_read_files)"""
    from . import _lib
    lib = _lib.load()
    n = len(paths)
    if n == 0:
        return []
    cp = (C.c_char_p * n)(*[str(p).encode() for p in paths])
    sizes = np.zeros(n, dtype=np.uint64)
    need = int(lib.modest_host_read_files(cp, n, None, 0, sizes.ctypes.data, int(readers)))
    if need < 0:
        raise IOError(f"cannot read {paths[-need - 2]}" if need < -1 else "modest_host_read_files: bad arguments")
    buf = np.empty(max(need, int(sizes.sum()), 16), dtype=np.uint8)
    rc = int(lib.modest_host_read_files(cp, n, buf.ctypes.data, buf.nbytes, sizes.ctypes.data, int(readers)))
    if rc != 0:
        raise IOError(f"cannot read {paths[-rc - 2]}" if rc < -1 else "modest_host_read_files failed")
    data = buf.tobytes()
    offs = np.concatenate([[0], np.cumsum(sizes.astype(np.int64))])
    return [data[offs[k]:offs[k + 1]] for k in range(n)]


def get_image_index_str(img_idx):
    return "{:06d}".format(img_idx)


def get_label_anno(label_path):
    return parse_label_texts(read_files([label_path]))[0]


def get_label_annos(label_folder, image_ids=None, readers=8):
    if image_ids is None:
        prog = re.compile(r'^\d{6}.txt$')
        image_ids = sorted(int(p.stem) for p in pathlib.Path(label_folder).glob('*.txt') if prog.match(p.name))
    if not isinstance(image_ids, list):
        image_ids = list(range(image_ids))
    folder = pathlib.Path(label_folder)
    return parse_label_texts(read_files([folder / (get_image_index_str(i) + '.txt') for i in image_ids], readers))


def filter_annos_low_score(image_annos, thresh):
    out = []
    for anno in image_annos:
        keep = np.nonzero(np.asarray(anno['score']) >= thresh)[0]
        out.append({k: anno[k][keep] for k in anno.keys()})
    return out


# --------------------------------------------------------------------------- host restatements of eval.py helpers
def get_thresholds(scores: np.ndarray, num_gt, num_sample_pts=41):
    """eval.py:10-28.  The kept ranks depend only on len(scores) and num_gt, and the skip test is monotone in the rank,
    so each kept rank is found by bisection; the float64 arithmetic is the loop's own."""
    scores.sort()
    scores = scores[::-1]
    return [scores[i] for i in _threshold_ranks(len(scores), num_gt, num_sample_pts)]


def _threshold_ranks(n, num_gt, num_sample_pts=41):
    ranks, cur, start = [], 0, 0

    class _Skip:
        def __getitem__(self, i):
            l_recall = (i + 1) / num_gt
            r_recall = (i + 2) / num_gt if i < n - 1 else l_recall
            return ((r_recall - cur) < (cur - l_recall)) and (i < n - 1)

        def __len__(self):
            return n

    sk = _Skip()
    while start < n:
        i = bisect.bisect_left(_BoolView(sk), True, start, n - 1)
        ranks.append(i)
        cur += 1 / (num_sample_pts - 1.0)
        start = i + 1
    return ranks


class _BoolView:
    """bisect over a monotone predicate: element i is True once skip(i) is False"""

    def __init__(self, sk):
        self.sk = sk

    def __getitem__(self, i):
        return not self.sk[i]

    def __len__(self):
        return len(self.sk)


def clean_data(gt_anno, dt_anno, current_class, difficulty):
    """eval.py:31-86"""
    dc_bboxes, ignored_gt, ignored_dt = [], [], []
    current_cls_name = CLASS_NAMES[current_class].lower()
    num_gt, num_dt = len(gt_anno["name"]), len(dt_anno["name"])
    num_valid_gt = 0
    for i in range(num_gt):
        bbox = gt_anno["bbox"][i]
        gt_name = gt_anno["name"][i].lower()
        height = bbox[3] - bbox[1]
        if gt_name == current_cls_name:
            valid_class = 1
        elif (current_cls_name == "pedestrian" and gt_name == "person_sitting") or \
                (current_cls_name == "car" and gt_name == "van"):
            valid_class = 0
        else:
            valid_class = -1
        ignore = difficulty < 3 and (gt_anno["occluded"][i] > MAX_OCCLUSION[difficulty]
                                     or gt_anno["truncated"][i] > MAX_TRUNCATION[difficulty]
                                     or height <= MIN_HEIGHT[difficulty])
        if valid_class == 1 and not ignore:
            ignored_gt.append(0)
            num_valid_gt += 1
        elif valid_class == 0 or (ignore and valid_class == 1):
            ignored_gt.append(1)
        else:
            ignored_gt.append(-1)
        if gt_anno["name"][i] == "DontCare":
            dc_bboxes.append(gt_anno["bbox"][i])
    for i in range(num_dt):
        valid_class = 1 if dt_anno["name"][i].lower() == current_cls_name else -1
        height = abs(dt_anno["bbox"][i, 3] - dt_anno["bbox"][i, 1])
        if difficulty in (0, 1, 2) and height < MIN_HEIGHT[difficulty]:
            ignored_dt.append(1)
        elif valid_class == 1:
            ignored_dt.append(0)
        else:
            ignored_dt.append(-1)
    return num_valid_gt, ignored_gt, ignored_dt, dc_bboxes


def image_box_overlap(boxes, query_boxes, criterion=-1):
    """eval.py:89-116, vectorised (the same float64 operations per pair)"""
    b = np.asarray(boxes)[:, None, :]
    q = np.asarray(query_boxes)[None, :, :]
    qa = (q[..., 2] - q[..., 0]) * (q[..., 3] - q[..., 1])
    iw = np.minimum(b[..., 2], q[..., 2]) - np.maximum(b[..., 0], q[..., 0])
    ih = np.minimum(b[..., 3], q[..., 3]) - np.maximum(b[..., 1], q[..., 1])
    if criterion == -1:
        ua = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1]) + qa - iw * ih
    elif criterion == 0:
        ua = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1]) + 0 * qa
    elif criterion == 1:
        ua = qa + 0 * b[..., 0]
    else:
        ua = np.ones_like(iw)
    with np.errstate(divide='ignore', invalid='ignore'):
        v = iw * ih / ua
    out = np.zeros((b.shape[0], q.shape[1]), dtype=np.asarray(boxes).dtype)
    m = (iw > 0) & (ih > 0)
    out[m] = v[m]
    return out


def get_split_parts(num, num_part):
    same_part, remain_num = num // num_part, num % num_part
    if same_part == 0:
        return [num]
    return [same_part] * num_part if remain_num == 0 else [same_part] * num_part + [remain_num]


def get_mAP(prec):
    sums = 0
    for i in range(0, prec.shape[-1], 4):
        sums = sums + prec[..., i]
    return sums / 11 * 100


def get_mAP_R40(prec):
    sums = 0
    for i in range(1, prec.shape[-1]):
        sums = sums + prec[..., i]
    return sums / 40 * 100


def print_str(value, *arg, sstream=None):
    if sstream is None:
        sstream = sysio.StringIO()
    sstream.truncate(0)
    sstream.seek(0)
    print(value, *arg, file=sstream)
    return sstream.getvalue()


# --------------------------------------------------------------------------- the device engine
def _device():
    import torch
    from . import _lib
    _lib.load()
    if not torch.cuda.is_available():
        raise _lib.ModestHipError("kitti_eval needs a HIP device: there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _up(a, dtype=None):
    """host array -> device tensor (at least one element, so that every pointer is valid)"""
    import torch
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype=dtype))
    if a.size == 0:
        a = np.zeros(1, dtype=a.dtype)
    return torch.from_numpy(a).to(_device())


def _boxes7(annos):
    if not annos:
        return np.zeros((0, 7))
    loc = np.concatenate([np.asarray(a["location"], dtype=np.float64).reshape(-1, 3) for a in annos], 0)
    dims = np.concatenate([np.asarray(a["dimensions"], dtype=np.float64).reshape(-1, 3) for a in annos], 0)
    rots = np.concatenate([np.asarray(a["rotation_y"], dtype=np.float64).reshape(-1) for a in annos], 0)
    return np.concatenate([loc, dims, rots[:, None]], 1)


def _cat(annos, key, shape):
    if not annos:
        return np.zeros((0,) + shape)
    return np.concatenate([np.asarray(a[key], dtype=np.float64).reshape((-1,) + shape) for a in annos], 0)


def _lower_codes(names_list):
    """per-box lower-cased names as codes into a small vocabulary (np.unique first: one lower() per distinct name)"""
    if not names_list:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), []
    names = np.concatenate([np.asarray(n).astype(str).reshape(-1) for n in names_list])
    uniq, inv = np.unique(names, return_inverse=True)
    lower = [str(u).lower() for u in uniq]
    return inv.reshape(-1), np.array([u == "DontCare" for u in uniq.tolist()], dtype=bool)[inv.reshape(-1)], lower


class EvalSet:
    """gt and dt annos of a list of frames, on the device, with their dt x gt overlaps."""

    def __init__(self, gt_annos, dt_annos):
        assert len(gt_annos) == len(dt_annos)
        import torch
        self.F = F = len(gt_annos)
        ng = np.array([len(a["name"]) for a in gt_annos], dtype=np.int64)
        nd = np.array([len(a["name"]) for a in dt_annos], dtype=np.int64)
        self.frames = np.zeros(F, dtype=EVAL_FRAME)
        self.frames["ng"], self.frames["nd"] = ng, nd
        self.frames["gt_off"] = np.concatenate([[0], np.cumsum(ng)[:-1]]) if F else []
        self.frames["dt_off"] = np.concatenate([[0], np.cumsum(nd)[:-1]]) if F else []
        pairs = nd * ng
        self.frames["pair_off"] = np.concatenate([[0], np.cumsum(pairs)[:-1]]) if F else []
        self.n_gt, self.n_dt, self.n_pairs = int(ng.sum()), int(nd.sum()), int(pairs.sum())
        self.max_nd = int(nd.max()) if F else 0
        from . import _lib
        lim_t, lim_d = C.c_int32(), C.c_int32()
        _lib.check(_lib.load().modest_eval_limits(C.byref(lim_t), C.byref(lim_d)), "modest_eval_limits")
        if self.max_nd > lim_d.value:
            raise ValueError(f"a frame holds {self.max_nd} detections: at most {lim_d.value} per frame are supported")
        # batches of whole frames within the pair budget (a frame larger than the budget is a batch of its own)
        budget, self.batches, b0, acc = pair_budget(), [], 0, 0
        for f in range(F):
            if acc and acc + pairs[f] > budget:
                self.batches.append((b0, f))
                b0, acc = f, 0
            acc += int(pairs[f])
        if F:
            self.batches.append((b0, F))
        # host columns
        self.gt_bbox, self.dt_bbox = _cat(gt_annos, "bbox", (4,)), _cat(dt_annos, "bbox", (4,))
        self.gt_box7, self.dt_box7 = _boxes7(gt_annos), _boxes7(dt_annos)
        self.gt_occ = _cat(gt_annos, "occluded", ())
        self.gt_trunc = _cat(gt_annos, "truncated", ())
        self.gt_alpha, self.dt_alpha = _cat(gt_annos, "alpha", ()), _cat(dt_annos, "alpha", ())
        self.dt_score = _cat(dt_annos, "score", ())
        self.gt_code, self.gt_dontcare, self.gt_vocab = _lower_codes([a["name"] for a in gt_annos])
        self.dt_code, _, self.dt_vocab = _lower_codes([a["name"] for a in dt_annos])
        # device columns
        self.d_frames = _up(self.frames.view(np.uint8))
        self.d_gt7, self.d_dt7 = _up(self.gt_box7, np.float64), _up(self.dt_box7, np.float64)
        self.d_gtbb, self.d_dtbb = _up(self.gt_bbox, np.float64), _up(self.dt_bbox, np.float64)
        self.d_score = _up(self.dt_score, np.float64)
        self._ov = {}            # kind -> device tensor of all pairs (single-batch sets only)
        self._torch = torch

    # ------------------------------------------------------------------ flags (clean_data, filter_det_range)
    def flags(self, rows):
        """rows: [(class index, difficulty, (close, far) or None)] -> gt_ign, dt_ign (int8), dc (uint8), num_valid_gt"""
        S = len(rows)
        gi = np.empty((S, self.n_gt), np.int8)
        di = np.empty((S, self.n_dt), np.int8)
        dc = np.empty((S, self.n_gt), np.uint8)
        nv = np.zeros(S, np.int64)
        gh = self.gt_bbox[:, 3] - self.gt_bbox[:, 1]
        dh = np.abs(self.dt_bbox[:, 3] - self.dt_bbox[:, 1])
        for s, (cls, diff, rng) in enumerate(rows):
            name = CLASS_NAMES[cls].lower()
            gv = np.array([1 if v == name else (0 if (name == "pedestrian" and v == "person_sitting")
                                                or (name == "car" and v == "van") else -1)
                           for v in self.gt_vocab], dtype=np.int8)[self.gt_code] if self.n_gt else np.zeros(0, np.int8)
            if diff < 3:
                ign = (self.gt_occ > MAX_OCCLUSION[diff]) | (self.gt_trunc > MAX_TRUNCATION[diff]) | (gh <= MIN_HEIGHT[diff])
            else:
                ign = np.zeros(self.n_gt, bool)
            g = np.full(self.n_gt, -1, np.int8)
            g[(gv == 0) | (ign & (gv == 1))] = 1
            g[(gv == 1) & ~ign] = 0
            dv = np.array([v == name for v in self.dt_vocab], dtype=bool)[self.dt_code] if self.n_dt else np.zeros(0, bool)
            d = np.where(dv, 0, -1).astype(np.int8)
            if diff in (0, 1, 2):
                d[dh < MIN_HEIGHT[diff]] = 1
            keep_dc = self.gt_dontcare.copy()
            if rng is not None:
                zg, zd = np.abs(self.gt_box7[:, 2]), np.abs(self.dt_box7[:, 2])
                ing, ind = (zg > rng[0]) & (zg <= rng[1]), (zd > rng[0]) & (zd <= rng[1])
                g[~ing] = -1
                keep_dc &= ing
                d[~ind] = -1
            gi[s], di[s], dc[s] = g, d, keep_dc
            nv[s] = int((g == 0).sum())
        return gi, di, dc, nv

    # ------------------------------------------------------------------ overlaps
    def _launch_overlaps(self, kinds, b0, b1, crit=(-1, -1, -1)):
        torch = self._torch
        p0 = int(self.frames["pair_off"][b0]) if b0 < self.F else self.n_pairs
        p1 = int(self.frames["pair_off"][b1]) if b1 < self.F else self.n_pairs
        n = p1 - p0
        dev = self.d_gt7.device
        out = {}
        if "bev" in kinds or "3d" in kinds:
            out["bev"] = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
            out["3d"] = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
        if "img" in kinds:
            out["img"] = torch.empty(max(n, 1), dtype=torch.float64, device=dev)
        if n:
            from . import ops
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.eval_overlaps(self.d_frames, self.F, p0, n, self.d_dt7, self.d_gt7, self.d_dtbb, self.d_gtbb, crit,
                              out.get("bev"), out.get("3d"), out.get("img"))
            e1.record()
            self._events.append(("overlaps_ms", e0, e1))
        return out, p0

    def overlaps(self, kind):
        """all pairs' overlaps of one kind ('img', 'bev', '3d') as a device tensor (computed once)"""
        if kind not in self._ov:
            self._events = getattr(self, "_events", [])
            kinds = ("img",) if kind == "img" else ("bev", "3d")
            out, _ = self._launch_overlaps(kinds, 0, self.F)
            self._ov.update(out)
        return self._ov[kind]

    def _pair_sim(self, b0, b1):
        fr = self.frames[b0:b1]
        sizes = (fr["nd"].astype(np.int64) * fr["ng"])
        if sizes.sum() == 0:
            return _up(np.zeros(1))
        fid = np.repeat(np.arange(len(fr)), sizes)
        q = np.arange(int(sizes.sum()), dtype=np.int64) - np.repeat(fr["pair_off"] - fr["pair_off"][0], sizes)
        ngr = fr["ng"][fid].astype(np.int64)
        j = fr["dt_off"][fid] + q // ngr
        i = fr["gt_off"][fid] + q % ngr
        return _up((1.0 + np.cos(self.gt_alpha[i] - self.dt_alpha[j])) / 2.0)

    # ------------------------------------------------------------------ statistics
    def statistics(self, metric, rows, configs, compute_aos=False):
        """configs: [(row, min_overlap)] -> pr (C, 64, 4) float64 (tp, fp, fn, similarity), n_thresh (C,)"""
        from . import ops
        torch = self._torch
        Cn = len(configs)
        self._events = getattr(self, "_events", [])
        if self.F == 0 or Cn == 0:
            return np.zeros((Cn, TMAX, 4)), np.zeros(Cn, np.int64)
        gi, di, dc, nv = self.flags(rows)
        cfg = np.zeros(Cn, dtype=EVAL_CONFIG)
        cfg["flagset"] = [r for r, _ in configs]
        cfg["min_overlap"] = [float(m) for _, m in configs]
        cfg["num_valid_gt"] = nv[cfg["flagset"]]
        dev = self.d_gt7.device
        d_cfg, d_gi, d_di = _up(cfg.view(np.uint8)), _up(gi), _up(di)
        d_dc = _up(dc) if metric == 0 else None
        aos = bool(compute_aos) and metric == 0
        tp_scores = torch.full((Cn, max(self.n_gt, 1)), -np.inf, dtype=torch.float64, device=dev)
        tp_count = torch.zeros(Cn, dtype=torch.int32, device=dev)
        thresholds = torch.zeros((Cn, TMAX), dtype=torch.float64, device=dev)
        n_thresh = torch.zeros(Cn, dtype=torch.int32, device=dev)
        partial = torch.empty((Cn, TMAX, self.F, 4), dtype=torch.int32, device=dev)
        sim_partial = torch.empty((Cn, TMAX, self.F), dtype=torch.float64, device=dev) if aos else None
        pr = torch.zeros((Cn, TMAX, 4), dtype=torch.float64, device=dev)
        a = _StatsArgs(frames=self.d_frames.data_ptr(), cfg=d_cfg.data_ptr(), dt_score=self.d_score.data_ptr(),
                       dt_bbox=self.d_dtbb.data_ptr(), gt_bbox=self.d_gtbb.data_ptr(), gt_ign=d_gi.data_ptr(),
                       dt_ign=d_di.data_ptr(), gt_dc=d_dc.data_ptr() if d_dc is not None else None, pair_sim=None,
                       tp_scores=tp_scores.data_ptr(), tp_count=tp_count.data_ptr(), thresholds=thresholds.data_ptr(),
                       n_thresh=n_thresh.data_ptr(), partial=partial.data_ptr(),
                       sim_partial=sim_partial.data_ptr() if aos else None, n_gt=self.n_gt, n_dt=self.n_dt,
                       n_frames=self.F, n_cfg=Cn, metric=int(metric), max_nd=self.max_nd)
        kind = {0: "img", 1: "bev", 2: "3d"}[metric]
        single = len(self.batches) == 1

        def batch_overlaps(b0, b1):
            if single:
                return self.overlaps(kind), 0
            out, p0 = self._launch_overlaps(("img",) if metric == 0 else ("bev", "3d"), b0, b1)
            return out[kind], p0

        def stats(stage, b0=0, b1=0, ov=None, p0=0, sorted_=None, pr_=None):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.eval_statistics(stage, a, b0, b1, ov, p0, sorted_, pr_)
            e1.record()
            self._events.append(("statistics_ms", e0, e1))

        for b0, b1 in self.batches:                                   # pass A
            ov, p0 = batch_overlaps(b0, b1)
            stats(0, b0, b1, ov, p0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        srt = torch.sort(tp_scores, dim=1, descending=True).values.contiguous()
        e1.record()
        self._events.append(("statistics_ms", e0, e1))
        stats(1, sorted_=srt)                             # thresholds
        for b0, b1 in self.batches:                                   # pass B
            ov, p0 = batch_overlaps(b0, b1)
            if aos:
                ps = self._pair_sim(b0, b1)
                a.pair_sim = ps.data_ptr()
            stats(2, b0, b1, ov, p0)
        stats(3, pr_=pr)                                  # sums
        out = torch.cat([pr.reshape(-1), n_thresh.to(torch.float64)]).cpu().numpy()   # the one synchronise
        for key, x0, x1 in self._events:
            last_timings[key] += x0.elapsed_time(x1)
        self._events = []
        nt = out[Cn * TMAX * 4:].astype(np.int64)
        if (nt > N_SAMPLE_PTS).any() or (nt < 0).any():
            raise IndexError("get_thresholds kept more than 41 thresholds: eval.py's precision table holds 41")
        return out[:Cn * TMAX * 4].reshape(Cn, TMAX, 4), nt


def _curves(pr, nt, compute_aos):
    """eval.py:540-550 for one configuration"""
    recall, precision, aos = np.zeros(N_SAMPLE_PTS), np.zeros(N_SAMPLE_PTS), np.zeros(N_SAMPLE_PTS)
    n = int(nt)
    with np.errstate(divide='ignore', invalid='ignore'):
        for i in range(n):
            recall[i] = pr[i, 0] / (pr[i, 0] + pr[i, 2])
            precision[i] = pr[i, 0] / (pr[i, 0] + pr[i, 1])
            if compute_aos:
                aos[i] = pr[i, 3] / (pr[i, 0] + pr[i, 1])
        for i in range(n):
            precision[i] = np.max(precision[i:], axis=-1)
            if compute_aos:
                aos[i] = np.max(aos[i:], axis=-1)
    return recall, precision, aos


def _eval_grid(es, metric, classes, buckets, min_overlaps, compute_aos):
    """eval_class over a grid: classes x buckets (difficulty, range or None) x min overlaps -> arrays
    [num_class, num_bucket, num_minoverlap, 41] of recall, precision and aos."""
    rows, configs, index = [], [], []
    for m, cls in enumerate(classes):
        for l, (diff, rng) in enumerate(buckets):
            rows.append((cls, diff, rng))
            for k, mo in enumerate(min_overlaps[:, metric, m]):
                configs.append((len(rows) - 1, mo))
                index.append((m, l, k))
    shape = (len(classes), len(buckets), min_overlaps.shape[0], N_SAMPLE_PTS)
    recall, precision, aos = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    pr, nt = es.statistics(metric, rows, configs, compute_aos)
    for c, (m, l, k) in enumerate(index):
        recall[m, l, k], precision[m, l, k], aos[m, l, k] = _curves(pr[c], nt[c], compute_aos)
    return {"recall": recall, "precision": precision, "orientation": aos}


# --------------------------------------------------------------------------- public eval.py interface
def eval_class(gt_annos, dt_annos, current_classes, difficultys, metric, min_overlaps, compute_aos=False,
               num_parts=100):
    """eval.py:452-556 (num_parts only shaped the reference's dense parts)"""
    assert len(gt_annos) == len(dt_annos)
    if metric not in (0, 1, 2):
        raise ValueError("unknown metric")
    es = EvalSet(gt_annos, dt_annos)
    return _eval_grid(es, metric, list(current_classes), [(d, None) for d in difficultys], np.asarray(min_overlaps),
                      compute_aos)


def _do_eval_set(es, current_classes, min_overlaps, compute_aos, buckets, PR_detail_dict, metrics=(0, 1, 2)):
    res = {}
    for metric in metrics:
        res[metric] = _eval_grid(es, metric, current_classes, buckets, min_overlaps, compute_aos if metric == 0 else False)
    if PR_detail_dict is not None:
        if 0 in res:
            PR_detail_dict['bbox'] = res[0]['precision']
            if compute_aos:
                PR_detail_dict['aos'] = res[0]['orientation']
        PR_detail_dict['bev'] = res[1]['precision']
        PR_detail_dict['bev_recall'] = res[1]['recall']
        PR_detail_dict['3d'] = res[2]['precision']
        PR_detail_dict['3d_recall'] = res[2]['recall']
    return res


def do_eval(gt_annos, dt_annos, current_classes, min_overlaps, compute_aos=False, difficultys=(0, 1, 2),
            PR_detail_dict=None):
    """eval.py:582-623"""
    es = EvalSet(gt_annos, dt_annos)
    res = _do_eval_set(es, list(current_classes), np.asarray(min_overlaps), compute_aos,
                       [(d, None) for d in difficultys], PR_detail_dict)
    mAP_aos = mAP_aos_R40 = None
    if compute_aos:
        mAP_aos, mAP_aos_R40 = get_mAP(res[0]["orientation"]), get_mAP_R40(res[0]["orientation"])
    return (get_mAP(res[0]["precision"]), get_mAP(res[1]["precision"]), get_mAP(res[2]["precision"]), mAP_aos,
            get_mAP_R40(res[0]["precision"]), get_mAP_R40(res[1]["precision"]), get_mAP_R40(res[2]["precision"]),
            mAP_aos_R40)


def _compute_aos(dt_annos):
    for anno in dt_annos:
        if anno['alpha'].shape[0] != 0:
            return bool(anno['alpha'][0] != -10)
    return False


def get_official_eval_result(gt_annos, dt_annos, current_classes, PR_detail_dict=None):
    """eval.py:644-751"""
    overlap_0_7 = np.array([[0.7, 0.5, 0.5, 0.7, 0.5, 0.7], [0.7, 0.5, 0.5, 0.7, 0.5, 0.7],
                            [0.7, 0.5, 0.5, 0.7, 0.5, 0.7]])
    overlap_0_5 = np.array([[0.7, 0.5, 0.5, 0.7, 0.5, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25, 0.5],
                            [0.5, 0.25, 0.25, 0.5, 0.25, 0.5]])
    min_overlaps = np.stack([overlap_0_7, overlap_0_5], axis=0)
    class_to_name = {0: 'Car', 1: 'Pedestrian', 2: 'Cyclist', 3: 'Van', 4: 'Person_sitting', 5: 'Truck'}
    name_to_class = {v: n for n, v in class_to_name.items()}
    if not isinstance(current_classes, (list, tuple)):
        current_classes = [current_classes]
    current_classes = [name_to_class[c] if isinstance(c, str) else c for c in current_classes]
    min_overlaps = min_overlaps[:, :, current_classes]
    result = ''
    compute_aos = _compute_aos(dt_annos)
    mAPbbox, mAPbev, mAP3d, mAPaos, mAPbbox_R40, mAPbev_R40, mAP3d_R40, mAPaos_R40 = do_eval(
        gt_annos, dt_annos, current_classes, min_overlaps, compute_aos, PR_detail_dict=PR_detail_dict)
    ret_dict = {}
    for j, curcls in enumerate(current_classes):
        name = class_to_name[curcls]
        for i in range(min_overlaps.shape[0]):
            ov = "{:.2f}, {:.2f}, {:.2f}:".format(*min_overlaps[i, :, j])
            result += print_str(f"{name} AP@" + ov)
            result += print_str(f"bbox AP:{mAPbbox[j, 0, i]:.4f}, {mAPbbox[j, 1, i]:.4f}, {mAPbbox[j, 2, i]:.4f}")
            result += print_str(f"bev  AP:{mAPbev[j, 0, i]:.4f}, {mAPbev[j, 1, i]:.4f}, {mAPbev[j, 2, i]:.4f}")
            result += print_str(f"3d   AP:{mAP3d[j, 0, i]:.4f}, {mAP3d[j, 1, i]:.4f}, {mAP3d[j, 2, i]:.4f}")
            if compute_aos:
                result += print_str(f"aos  AP:{mAPaos[j, 0, i]:.2f}, {mAPaos[j, 1, i]:.2f}, {mAPaos[j, 2, i]:.2f}")
            result += print_str(f"{name} AP_R40@" + ov)
            result += print_str(f"bbox AP:{mAPbbox_R40[j, 0, i]:.4f}, {mAPbbox_R40[j, 1, i]:.4f}, "
                                f"{mAPbbox_R40[j, 2, i]:.4f}")
            result += print_str(f"bev  AP:{mAPbev_R40[j, 0, i]:.4f}, {mAPbev_R40[j, 1, i]:.4f}, "
                                f"{mAPbev_R40[j, 2, i]:.4f}")
            result += print_str(f"3d   AP:{mAP3d_R40[j, 0, i]:.4f}, {mAP3d_R40[j, 1, i]:.4f}, "
                                f"{mAP3d_R40[j, 2, i]:.4f}")
            if compute_aos:
                result += print_str(f"aos  AP:{mAPaos_R40[j, 0, i]:.2f}, {mAPaos_R40[j, 1, i]:.2f}, "
                                    f"{mAPaos_R40[j, 2, i]:.2f}")
                if i == 0:
                    ret_dict['%s_aos/easy_R40' % name] = mAPaos_R40[j, 0, 0]
                    ret_dict['%s_aos/moderate_R40' % name] = mAPaos_R40[j, 1, 0]
                    ret_dict['%s_aos/hard_R40' % name] = mAPaos_R40[j, 2, 0]
            if i == 0:
                for tag, arr in (("3d", mAP3d_R40), ("bev", mAPbev_R40), ("image", mAPbbox_R40)):
                    ret_dict['%s_%s/easy_R40' % (name, tag)] = arr[j, 0, 0]
                    ret_dict['%s_%s/moderate_R40' % (name, tag)] = arr[j, 1, 0]
                    ret_dict['%s_%s/hard_R40' % (name, tag)] = arr[j, 2, 0]
    return result, ret_dict


def get_coco_eval_result(gt_annos, dt_annos, current_classes):
    raise NotImplementedError(
        "COCO-style AP is broken in the reference: do_coco_style_eval unpacks 4 of do_eval's 8 return values")


def filter_det_range(dets, close, far):
    """eval.py:816-832 (kept for callers; the range eval itself marks boxes ignored instead)"""
    from copy import deepcopy
    dets = deepcopy(dets)
    if dets['location'].shape[0] == 0:
        return dets
    valid_idx = (np.abs(dets['location'][:, 2]) > close) * (np.abs(dets['location'][:, 2]) <= far)
    for k in dets:
        if k in ('frame_id', 'gt_boxes_lidar'):
            continue
        dets[k] = dets[k][valid_idx]
    return dets


def get_range_eval_result(gt_annos, dt_annos, current_classes, PR_detail_dict=None, ranges=(0, 30, 50, 80)):
    """eval.py:834-927: every range bucket in one statistics call per metric, over overlaps computed once"""
    overlap_0_7 = np.array([[0.7, 0.5, 0.5, 0.7, 0.5, 0.7, 0.5], [0.7, 0.5, 0.5, 0.7, 0.5, 0.7, 0.5],
                            [0.7, 0.5, 0.5, 0.7, 0.5, 0.7, 0.5]])
    overlap_0_5 = np.array([[0.7, 0.5, 0.5, 0.7, 0.5, 0.5, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25, 0.5, 0.25],
                            [0.5, 0.25, 0.25, 0.5, 0.25, 0.5, 0.25]])
    min_overlaps = np.stack([overlap_0_7, overlap_0_5], axis=0)
    class_to_name = {0: 'Car', 1: 'Pedestrian', 2: 'Cyclist', 3: 'Van', 4: 'Person_sitting', 5: 'Truck', 6: 'Dynamic'}
    name_to_class = {v: n for n, v in class_to_name.items()}
    if not isinstance(current_classes, (list, tuple)):
        current_classes = [current_classes]
    current_classes = [name_to_class[c] if isinstance(c, str) else c for c in current_classes]
    min_overlaps = min_overlaps[:, :, current_classes]
    compute_aos = _compute_aos(dt_annos)
    ret_dict = {}
    range_pairs = [(ranges[i], ranges[i + 1]) for i in range(len(ranges) - 1)]
    range_pairs.append([ranges[0], ranges[-1]])
    es = EvalSet(gt_annos, dt_annos)
    buckets = [(3, (s, e)) for s, e in range_pairs]
    res = {metric: _eval_grid(es, metric, current_classes, buckets, min_overlaps, False) for metric in (1, 2)}
    if PR_detail_dict is not None:
        # what the last range pair's do_eval leaves in it
        last = buckets[-1:]
        r0 = _eval_grid(es, 0, current_classes, last, min_overlaps, compute_aos)
        PR_detail_dict['bbox'] = r0['precision']
        if compute_aos:
            PR_detail_dict['aos'] = r0['orientation']
        PR_detail_dict['bev'] = res[1]['precision'][:, -1:]
        PR_detail_dict['bev_recall'] = res[1]['recall'][:, -1:]
        PR_detail_dict['3d'] = res[2]['precision'][:, -1:]
        PR_detail_dict['3d_recall'] = res[2]['recall'][:, -1:]
    for r, (range_s, range_e) in enumerate(range_pairs):
        mAPbev_R40 = get_mAP_R40(res[1]['precision'][:, r:r + 1])
        mAP3d_R40 = get_mAP_R40(res[2]['precision'][:, r:r + 1])
        for j, curcls in enumerate(current_classes):
            n = class_to_name[curcls]
            ret_dict[f'{n}_3d_iou0.7/{range_s:02d}-{range_e:02d}_R40'] = mAP3d_R40[j, 0, 0]
            ret_dict[f'{n}_3d_iou0.5/{range_s:02d}-{range_e:02d}_R40'] = mAP3d_R40[j, 0, 1]
            ret_dict[f'{n}_bev_iou0.7/{range_s:02d}-{range_e:02d}_R40'] = mAPbev_R40[j, 0, 0]
            ret_dict[f'{n}_bev_iou0.5/{range_s:02d}-{range_e:02d}_R40'] = mAPbev_R40[j, 0, 1]
    return _range_result_string(ret_dict, current_classes, class_to_name, range_pairs), ret_dict


def _range_result_string(ret_dict, current_classes, class_to_name, range_pairs):
    result = ''
    for curcls in current_classes:
        n = class_to_name[curcls]
        col = [f"{s:02d}-{e:02d}_R40" for s, e in range_pairs]
        bev07 = [ret_dict[f'{n}_bev_iou0.7/{c}'] for c in col]
        threeD07 = [ret_dict[f'{n}_3d_iou0.7/{c}'] for c in col]
        bev05 = [ret_dict[f'{n}_bev_iou0.5/{c}'] for c in col]
        threeD05 = [ret_dict[f'{n}_3d_iou0.5/{c}'] for c in col]
        head = "RANGE " + "  ".join([f"{s:02d}-{e:02d} " for s, e in range_pairs]) + "\n"
        result += f"{n} IoU 0.5:\n" + head
        result += "BEV:  " + ", ".join([f"{x:6.3f}" for x in bev07]) + "\n"
        result += "3D :  " + ", ".join([f"{x:6.3f}" for x in threeD07]) + "\n"
        result += f"{n} IoU 0.25:\n" + head
        result += "BEV:  " + ", ".join([f"{x:6.3f}" for x in bev05]) + "\n"
        result += "3D :  " + ", ".join([f"{x:6.3f}" for x in threeD05]) + "\n"
        result += f"{n} IoU 0.7:\n"
        result += ", ".join([f"{x:3.1f} / {y:3.1f}" for x, y in zip(bev07, threeD07)]) + "\n"
        result += f"{n} IoU 0.5:\n"
        result += ", ".join([f"{x:3.1f} / {y:3.1f}" for x, y in zip(bev05, threeD05)]) + "\n\n"
    return result


# --------------------------------------------------------------------------- device-backed overlap helpers
def _dense(boxes7_dt, boxes7_gt, kind, crit):
    """one 'frame' holding every (box, query box) pair"""
    N, K = len(boxes7_dt), len(boxes7_gt)
    dt = {"name": np.zeros(N, dtype="<U1"), "location": boxes7_dt[:, :3], "dimensions": boxes7_dt[:, 3:6],
          "rotation_y": boxes7_dt[:, 6], "bbox": np.zeros((N, 4)), "alpha": np.zeros(N), "score": np.zeros(N)}
    gt = {"name": np.zeros(K, dtype="<U1"), "location": boxes7_gt[:, :3], "dimensions": boxes7_gt[:, 3:6],
          "rotation_y": boxes7_gt[:, 6], "bbox": np.zeros((K, 4)), "alpha": np.zeros(K), "occluded": np.zeros(K),
          "truncated": np.zeros(K)}
    es = EvalSet([gt], [dt])
    es._events = []
    out, _ = es._launch_overlaps((kind,), 0, 1, crit)
    return out[kind][:N * K].cpu().numpy().reshape(N, K)


def _as7(b5):
    b5 = np.asarray(b5, dtype=np.float32).astype(np.float64).reshape(-1, 5)
    b7 = np.zeros((len(b5), 7))
    b7[:, [0, 2, 3, 5, 6]] = b5
    return b7


def rotate_iou_gpu_eval(boxes, query_boxes, criterion=-1, device_id=0):
    """rotate_iou.py:296-330: (N, K) float32, devRotateIoUEval(query_boxes[k], boxes[n], criterion)"""
    N, K = len(boxes), len(query_boxes)
    if N == 0 or K == 0:
        return np.zeros((N, K), dtype=np.float32)
    return _dense(_as7(boxes), _as7(query_boxes), "bev", (criterion, -1, -1))


def bev_box_overlap(boxes, qboxes, criterion=-1):
    return rotate_iou_gpu_eval(boxes, qboxes, criterion)


def d3_box_overlap(boxes, qboxes, criterion=-1):
    """eval.py:124-157: float32 like the reference's rinc"""
    boxes, qboxes = np.asarray(boxes, dtype=np.float64), np.asarray(qboxes, dtype=np.float64)
    if len(boxes) == 0 or len(qboxes) == 0:
        return np.zeros((len(boxes), len(qboxes)), dtype=np.float32)
    return _dense(boxes, qboxes, "3d", (-1, criterion, -1))


def calculate_iou_partly(gt_annos, dt_annos, metric, num_parts=50):
    """eval.py:343-417 (dense part matrices, as the reference returns them)"""
    assert len(gt_annos) == len(dt_annos)
    total_dt_num = np.stack([len(a["name"]) for a in dt_annos], 0)
    total_gt_num = np.stack([len(a["name"]) for a in gt_annos], 0)
    split_parts = get_split_parts(len(gt_annos), num_parts)
    parted_overlaps, example_idx = [], 0
    for num_part in split_parts:
        g, d = gt_annos[example_idx:example_idx + num_part], dt_annos[example_idx:example_idx + num_part]
        if metric == 0:
            part = image_box_overlap(_cat(g, "bbox", (4,)), _cat(d, "bbox", (4,)))
        elif metric == 1:
            gb, db = _boxes7(g), _boxes7(d)
            part = bev_box_overlap(gb[:, [0, 2, 3, 5, 6]], db[:, [0, 2, 3, 5, 6]]).astype(np.float64)
        elif metric == 2:
            part = d3_box_overlap(_boxes7(g), _boxes7(d)).astype(np.float64)
        else:
            raise ValueError("unknown metric")
        parted_overlaps.append(part)
        example_idx += num_part
    overlaps, example_idx = [], 0
    for j, num_part in enumerate(split_parts):
        gi = di = 0
        for i in range(num_part):
            gn, dn = total_gt_num[example_idx + i], total_dt_num[example_idx + i]
            overlaps.append(parted_overlaps[j][gi:gi + gn, di:di + dn])
            gi += gn
            di += dn
        example_idx += num_part
    return overlaps, parted_overlaps, total_gt_num, total_dt_num


def frame_overlaps(gt_annos, dt_annos):
    """per frame, the (dt, gt) blocks of BEV IoU and 3-D IoU (float64 of the float32 values eval.py stores)"""
    es = EvalSet(gt_annos, dt_annos)
    bev = es.overlaps("bev")[:es.n_pairs].cpu().numpy().astype(np.float64)
    d3 = es.overlaps("3d")[:es.n_pairs].cpu().numpy().astype(np.float64)
    out = []
    for f in es.frames:
        s, n = int(f["pair_off"]), int(f["nd"]) * int(f["ng"])
        out.append((bev[s:s + n].reshape(f["nd"], f["ng"]), d3[s:s + n].reshape(f["nd"], f["ng"])))
    return out
