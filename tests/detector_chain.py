"""The detector ops chained, each fed by the op before it (not a test module; tests/test_detector_chain_cpu.py and
tests/test_gpu_detector_chain.py import it): the two scenes, the stand-in heads with every drop-in bound by its module's own
``bind()``, the stand-ins for the networks, the reference of every stage -- the restatement that stage's own test uses, applied
to host arrays -- the free-running chains of restatements alone, and the three round trips with their derived bounds.

Chain A is an anchor detector (PointPillars / SECOND head): assign_targets -> get_loss -> generate_predicted_boxes ->
post_processing.  Chain B is PointRCNN: a training step (point targets, point loss, point decoding, proposals, RoI targets,
RoI point pooling, RoI loss) and a test-time forward (proposals, RoI decoding, post-processing) on the same heads.

A stand-in for a network is a host function of the previous stage's host copy: the targets plus seeded noise, and seeded
logits that favour the true class.  So a chain is a deterministic function of its scene, and a reference function called
twice on the same bytes is computed once (``memo``).

The round-trip bounds count roundings, u = 2^-24 each, in the operation order DESIGN.md sections 7i, 7l, 7n and 7s state; a
function with a one-ulp budget (sqrt, log, exp, sin, cos, atan2) counts 2 u, as tests/box_decode_seq.py budgets them:
    diag = sqrt(dx^2 + dy^2)           u + u for the squares and their sum under the root -> u, plus the root's 2 u    = 3 u
    x (anchor, point)  encode (xg - xa) / diag: u + 3 u + u = 5 u; decode t diag + xa: 3 u + u = 4 u of |xg - xa|, u |xg|
                       => 9 u |xg - xa| + u |xg|;  y alike
    z                  encode (zg - za) / dza: 2 u; decode t dza + za: u of |zg - za|, u |zg|   => 3 u |zg - za| + u |zg|
    sizes              log(dg / da): u from the quotient, 2 u |t| from the log; exp(t): the error of t plus 2 u; times da: u
                       => (4 + 2 |t|) u dg
    heading (anchor)   (rg - ra) + ra: u |rg - ra| + u |rg|
    heading (point)    atan2(sin rg, cos rg): the two values 2 u each, through atan2 4 u |sin cos| <= 2 u, atan2's own 2 u pi
                       => (2 + 2 pi) u, modulo 2 pi
    x (RoI), L = |xg - xr| + |yg - yr|: into the roi's frame (section 7n): the differences u L, ry = r mod 2 pi moves the
                       angle by up to 2 pi u (2 pi u L), cos and sin 2 u L, the products u L, their sum u L: (5 + 2 pi) u L
                       in x and in y, both of which the turn back mixes: 2 (5 + 2 pi) u L.  The float64 encode rounds once
                       (u) and the decode's t diag adds 4 u, on |x'| + |y'| <= sqrt 2 L: 5 sqrt 2 u L; the turn back's cos
                       and sin 2 sqrt 2 u L, its products sqrt 2 u L, its sum u L; then + xr: u |xg|
                       => (2 (5 + 2 pi) + 8 sqrt 2 + 1) u L + u |xg| < 36 u L + u |xg|;  y alike;  z as above
    heading (RoI)      ry 2 pi u; g - ry u (|g| + 2 pi); its remainder 2 pi u; the turn by pi 2.5 pi u, the shift by 2 pi pi u;
                       the decode's sum u (pi / 2 + |r|)  => (10 pi + |g| + |r|) u, modulo pi
each times 1.01 for the second-order terms.
"""
import functools
import hashlib
import types

import numpy as np

import anchor_loss_seq as al
import anchor_targets_seq as at
import box_decode_seq as bd
import point_loss_seq as pl
import point_targets_seq as pt
import post_process_seq as pp
import proposals_seq as ps
import roi_loss_seq as rl
import roi_targets_seq as rt
import roipool_seq as rp

F = np.float32
U = 2.0 ** -24
SLACK = 1.01
TWO_PI = 2 * np.pi


# ---------------------------------------------------------------------------------------------------- computed once
_memo = {}


def _digest(v, h):
    if isinstance(v, np.ndarray):
        h.update(str((v.dtype, v.shape)).encode())
        h.update(np.ascontiguousarray(v).tobytes())
    elif isinstance(v, dict):
        for k in sorted(v):
            h.update(str(k).encode())
            _digest(v[k], h)
    elif isinstance(v, (list, tuple)):
        for x in v:
            _digest(x, h)
    else:
        h.update(repr(v).encode())


def memo(fn):
    """a reference function of host arrays: the same bytes in, the result computed once and left unchanged"""
    @functools.wraps(fn)
    def wrapped(*args):
        h = hashlib.sha1(fn.__name__.encode())
        _digest(args, h)
        key = h.digest()
        if key not in _memo:
            _memo[key] = fn(*args)
        return _memo[key]
    return wrapped


# ---------------------------------------------------------------------------------------------------- chain A: the scene
MEAN_SIZE = ((3.9, 1.6, 1.56), (0.8, 0.6, 1.73), (1.76, 0.6, 1.73))
CLASS_NAMES = ["Car", "Pedestrian", "Cyclist"]
A_GRID = (12, 8)                       # nx, ny: 8 x 12 cells


def _anchor_class(name, size, bottom, matched, unmatched, rotations):
    return dict(class_name=name, anchor_sizes=[list(size)], anchor_rotations=list(rotations), anchor_bottom_heights=[bottom],
                align_center=False, matched_threshold=matched, unmatched_threshold=unmatched, grid_size=list(A_GRID))


# three classes of different sizes, z centres AND rotations: a swap of two classes' anchors changes every stage
A_CFG = dict(anchor_range=[0, -10.5, -3, 33, 10.5, 1], use_multihead=False, code_size=7, sincos=False, class_names=CLASS_NAMES,
             classes=[_anchor_class("Car", MEAN_SIZE[0], -1.78, 0.6, 0.45, (0.0, 1.57)),
                      _anchor_class("Pedestrian", MEAN_SIZE[1], -0.6, 0.5, 0.35, (0.8, 2.37)),
                      _anchor_class("Cyclist", MEAN_SIZE[2], -0.9, 0.5, 0.35, (-0.8, 0.77))])
A_COUNTS = (5, 0, 8)
A_B, A_N = 3, A_GRID[0] * A_GRID[1] * 6
A_LOSS = al.base_cfg(B=A_B, N=A_N, num_class=3, code=7, bins=2, beta=1.0 / 9.0, dir_offset=0.78539, cls_weight=1.0, loc_weight=2.0,
                     dir_weight=0.2)
A_DIR_LIMIT_OFFSET = 0.0
A_POST = dict(NMS_TYPE="nms_gpu", NMS_THRESH=0.01, NMS_PRE_MAXSIZE=4096, NMS_POST_MAXSIZE=500, RECALL_THRESH_LIST=[0.3, 0.5, 0.7],
              SCORE_THRESH=0.1, OUTPUT_RAW_SCORE=False)


@functools.lru_cache(maxsize=None)
def a_anchors():
    """the list of per-class (1, 8, 12, 1, 2, 7) arrays, as a head holds them"""
    anchors = at.make_anchors(A_CFG)
    assert all(a.shape == (1, A_GRID[1], A_GRID[0], 1, 2, 7) for a in anchors) and A_N == 576
    for a in anchors:
        a.setflags(write=False)
    return anchors


def a_flat():
    """(576, 7): the three tensors joined along the sizes axis and flattened, as the reference's heads do"""
    return bd.flat_anchors(a_anchors())


@functools.lru_cache(maxsize=None)
def scene_a():
    """gt_boxes (3, 8, 8): 5, 0 and 8 gts, zero-padded to 8 rows; each gt a moved and resized copy of an anchor of its class"""
    rs = np.random.RandomState(11)
    gt = np.zeros((A_B, max(A_COUNTS), 8), dtype=F)
    taken = set()
    for b, n in enumerate(A_COUNTS):
        for j in range(n):
            ci = (j + b) % 3
            flat = at.flatten(a_anchors()[ci], False)
            while True:
                k = int(rs.randint(len(flat)))
                if (b, k // 2) not in taken:
                    break
            taken.add((b, k // 2))
            a = flat[k]
            size = a[3:6] * rs.uniform(0.85, 1.2, 3)
            gt[b, j] = [a[0] + rs.normal(0, 0.2) * a[3], a[1] + rs.normal(0, 0.2) * a[4], a[2] + rs.normal(0, 0.1), *size,
                        a[6] + rs.normal(0, 0.2) + np.pi * rs.randint(-1, 2), ci + 1]
    gt.setflags(write=False)
    return gt


def net_anchor(labels, targets, seed=21):
    """the stand-in for an anchor head's network -> {"cls" (B, N, 3), "box" (B, N, 7), "dir" (B, N, 2)} float32: the targets
    plus noise, logits that favour the label's class and the target's direction bin.  Row i of a sample is row i of the labels:
    the predictions of a head are a view(B, -1, K) of (B, H, W, A K)"""
    rs = np.random.RandomState(seed)
    labels, targets = np.asarray(labels).astype(np.int64), np.asarray(targets, dtype=F)
    B, N = labels.shape
    box = (targets.astype(np.float64) + rs.normal(0, 0.03, targets.shape)).astype(F)
    cls = rs.normal(-3.0, 1.0, (B, N, 3))
    pos = labels > 0
    b, i = np.nonzero(pos)
    cls[b, i, np.clip(labels[b, i] - 1, 0, 2)] += 7.0
    rot = targets[..., 6].astype(np.float64) + a_flat()[None, :, 6]
    val = rot - A_LOSS["dir_offset"]
    lim = val - np.floor(val / TWO_PI) * TWO_PI
    bins = np.clip(np.floor(lim / np.pi), 0, 1).astype(np.int64)
    dirl = rs.normal(0.0, 1.0, (B, N, 2))
    dirl[b, i, bins[b, i]] += 3.0
    return {"cls": cls.astype(F), "box": box, "dir": dirl.astype(F)}


def a_layout(x):
    """(B, N, K) -> (B, H, W, A K), the shape a head's convolution leaves"""
    return np.ascontiguousarray(x).reshape(x.shape[0], A_GRID[1], A_GRID[0], 6 * x.shape[2])


# ---------------------------------------------------------------------------------------------------- chain A: the stages
@memo
def ref_a_targets(gt):
    details = []
    out = at.assign(A_CFG, a_anchors(), gt, details)
    return out, details


def a_loss_inputs(preds, labels, targets):
    return {"cls": np.asarray(preds["cls"], F).reshape(A_B, A_N, 3), "box": np.asarray(preds["box"], F).reshape(A_B, A_N, 7),
            "dir": None if preds.get("dir") is None else np.asarray(preds["dir"], F).reshape(A_B, A_N, 2),
            "labels": np.asarray(labels), "tg": np.asarray(targets, F), "anchors": a_flat(), "cw": np.ones(7, dtype=F)}


@memo
def ref_a_loss(inp, bins):
    """-> (restatement, exact()'s pairs) of the anchor loss on these inputs"""
    cfg = dict(A_LOSS, bins=bins)
    ours, dec = al._evaluate(inp, cfg, None)
    return ours, al.exact(inp, cfg, dec)


@memo
def ref_a_decode(box, dirp):
    return bd.anchor_decode(np.asarray(box, F).reshape(A_B, A_N, 7), a_flat(), None if dirp is None else np.asarray(dirp, F).reshape(A_B, A_N, 2),
                            A_LOSS["dir_offset"], A_DIR_LIMIT_OFFSET)


@memo
def ref_a_post(box, cls, gt):
    return pp.post_process(box, cls, A_B, A_POST["NMS_PRE_MAXSIZE"], A_POST["NMS_POST_MAXSIZE"], A_POST["NMS_THRESH"], rotated=True,
                           score_thresh=A_POST["SCORE_THRESH"], normalized=False, gt_boxes=gt, recall_thresh=A_POST["RECALL_THRESH_LIST"])


def free_chain_a():
    """the restatements alone, from the scene -> every stage's result"""
    gt = scene_a()
    targets, details = ref_a_targets(gt)
    preds = net_anchor(targets["box_cls_labels"], targets["box_reg_targets"])
    loss, _ = ref_a_loss(a_loss_inputs(preds, targets["box_cls_labels"], targets["box_reg_targets"]), 2)
    boxes = ref_a_decode(preds["box"], preds["dir"])
    final = ref_a_post(boxes, preds["cls"], gt)
    return dict(gt=gt, targets=targets, details=details, preds=preds, loss=loss, boxes=boxes, final=final)


def matched_gt_a(details, gt):
    """(B, N, 8): per output row the gt its anchor is matched to (the argmax of its IoUs), in the row order of the labels"""
    fm = a_anchors()[0].shape[:3]
    out = []
    for b, info in enumerate(details):
        per = []
        for ci, d in enumerate(info):
            n = len(d["anchors"])
            rows = np.zeros((n, 8), dtype=F)
            if "arg" in d:
                rows = np.asarray(gt[b], F)[d["rows"][d["arg"]]]
            per.append(rows.reshape(*fm, -1, 8))
        out.append(np.concatenate(per, axis=-2).reshape(-1, 8))
    return np.stack(out)


# ---------------------------------------------------------------------------------------------------- the round trips
def _residual_bound(g, a_xyz, a_size):
    """the bounds of centre and size for an encode against (a_xyz, a_size) and the decode against the same: (n, 6)"""
    g, a_xyz, a_size = (np.asarray(v, F).astype(np.float64) for v in (g, a_xyz, a_size))
    out = np.zeros((len(g), 6))
    for k in (0, 1):
        out[:, k] = 9 * U * np.abs(g[:, k] - a_xyz[:, k]) + U * np.abs(g[:, k])
    out[:, 2] = 3 * U * np.abs(g[:, 2] - a_xyz[:, 2]) + U * np.abs(g[:, 2])
    t = np.abs(np.log(g[:, 3:6] / a_size))
    out[:, 3:6] = (4 + 2 * t) * U * g[:, 3:6]
    return out


def round_trip_report(what, decoded, gt, bound, period):
    """decoded (n, 7) float32 against the gts (n, >= 7) they must give back, inside bound (n, 7); the heading modulo `period`.
    The bound must say something: below 1e-3 of the gt's smallest size.  -> text of the rows outside, '' if none"""
    dec, g = np.asarray(decoded, F).astype(np.float64), np.asarray(gt, F).astype(np.float64)[:, :7]
    bound = np.asarray(bound) * SLACK + 2.0 ** -149
    assert len(dec) and dec.shape == g.shape == bound.shape, (what, dec.shape, g.shape, bound.shape)
    smallest = g[:, 3:6].min(axis=1)
    assert (bound.max(axis=1) < 1e-3 * smallest).all(), f"{what}: the bound says nothing: {bound.max()} against sizes from {smallest.min()}"
    err = np.abs(dec - g)
    d = err[:, 6] % period
    err[:, 6] = np.minimum(d, period - d)
    bad = ~(err <= bound)
    return "\n".join(f"{what}: row {i} column {k}: decoded {dec[i, k]!r}, the gt has {g[i, k]!r}, bound {bound[i, k]!r}"
                     for i, k in np.argwhere(bad)[:8])


def anchor_round_trip(decoded, labels, matched):
    """decoded (B, N, 7) = anchor_decode(box_reg_targets): every positive row gives back its matched gt"""
    pos = np.asarray(labels) > 0
    g = matched[pos]
    a = np.broadcast_to(a_flat()[None], (A_B, A_N, 7))[pos].astype(np.float64)
    bound = np.zeros((len(g), 7))
    bound[:, :6] = _residual_bound(g, a[:, 0:3], a[:, 3:6])
    g6 = g[:, 6].astype(np.float64)
    bound[:, 6] = U * np.abs(g6 - a[:, 6]) + U * np.abs(g6)
    return round_trip_report("anchor round trip", np.asarray(decoded)[pos], g, bound, TWO_PI)


def point_round_trip(decoded, labels, points, gt, idx):
    """decoded (N, 7) = point_decode(point_box_labels, one-hot logits): every foreground point gives back the gt box that
    holds it (idx, sample from the batch column)"""
    fg = np.asarray(labels) > 0
    k = pt.sample_of(points, gt.shape[0])
    g = np.asarray(gt, F)[k[fg], idx[fg]]
    mean = np.asarray(MEAN_SIZE, F)[g[:, 7].astype(np.int64) - 1]
    bound = np.zeros((len(g), 7))
    bound[:, :6] = _residual_bound(g, np.asarray(points, F)[fg, 1:4], mean)
    bound[:, 6] = (2 + TWO_PI) * U
    return round_trip_report("point round trip", np.asarray(decoded)[fg], g, bound, TWO_PI)


def roi_encode64(gt_of_rois, rois):
    """the residual encode of canonical gts (.., >= 7) against their rois centred at zero with heading zero, in float64,
    rounded once to float32 -> (.., 7)"""
    g, r = np.asarray(gt_of_rois, F).astype(np.float64), np.asarray(rois, F).astype(np.float64)
    ca, ga = np.maximum(r[..., 3:6], float(F(1e-5))), np.maximum(g[..., 3:6], float(F(1e-5)))
    diag = np.sqrt(ca[..., 0] ** 2 + ca[..., 1] ** 2)
    t = np.concatenate([g[..., 0:1] / diag[..., None], g[..., 1:2] / diag[..., None], g[..., 2:3] / ca[..., 2:3], np.log(ga / ca),
                        g[..., 6:7]], axis=-1)
    return t.astype(F)


def roi_round_trip(decoded, targets):
    """decoded (B M, 7) = roi_decode(rois, roi_encode64(gt_of_rois, rois)): the rows with reg_valid_mask == 1 give back centre
    and size of gt_of_rois_src, and its heading modulo pi where the canonical heading lies strictly inside (-pi/2, pi/2)"""
    valid = np.asarray(targets["reg_valid_mask"]).reshape(-1) == 1
    g = np.asarray(targets["gt_of_rois_src"], F).reshape(valid.size, -1)[valid]
    r = np.asarray(targets["rois"], F).reshape(valid.size, -1)[valid].astype(np.float64)
    canon = np.asarray(targets["gt_of_rois"], F).reshape(valid.size, -1)[valid, 6]
    g64 = g.astype(np.float64)
    bound = np.zeros((len(g), 7))
    bound[:, :6] = _residual_bound(g, r[:, 0:3], np.maximum(r[:, 3:6], 1e-5))
    L = np.abs(g64[:, 0] - r[:, 0]) + np.abs(g64[:, 1] - r[:, 1])
    for k in (0, 1):
        bound[:, k] = 36 * U * L + U * np.abs(g64[:, k])
    inside = (canon > -rt.HALF_PI) & (canon < rt.HALF_PI)
    assert inside.any()
    bound[:, 6] = np.where(inside, (10 * np.pi + np.abs(g64[:, 6]) + np.abs(r[:, 6])) * U, np.inf)
    return round_trip_report("RoI round trip", np.asarray(decoded, F).reshape(valid.size, -1)[valid][:, :7], g, bound, np.pi)


# ---------------------------------------------------------------------------------------------------- chain B: the scenes
B_TARGET = dict(ROI_PER_IMAGE=32, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True, CLS_SCORE_TYPE="cls", CLS_FG_THRESH=0.6,
                CLS_BG_THRESH=0.45, CLS_BG_THRESH_LO=0.1, HARD_BG_RATIO=0.8, REG_FG_THRESH=0.55)
B_TRAIN_NMS = dict(NMS_TYPE="nms_gpu", MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=256, NMS_POST_MAXSIZE=64, NMS_THRESH=0.8)
B_TEST_NMS = dict(NMS_TYPE="nms_gpu", MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=256, NMS_POST_MAXSIZE=32, NMS_THRESH=0.85)
B_POST = dict(NMS_TYPE="nms_gpu", NMS_THRESH=0.1, NMS_PRE_MAXSIZE=4096, NMS_POST_MAXSIZE=100, RECALL_THRESH_LIST=[0.3, 0.5, 0.7],
              SCORE_THRESH=0.1, OUTPUT_RAW_SCORE=False)
B_POINT_LOSS = dict(head="PointHeadBox", num_class=3, code=8, beta=1.0 / 9.0, cls_weight=1.0, box_weight=1.0)
B_ROI_LOSS = dict(code=7, gt_cols=8, corner=True, beta=1.0 / 9.0, cls_weight=1.0, reg_weight=1.0, corner_weight=1.0)
POOL_POINTS, POOL_EXTRA = 64, 1.0
EXTEND = (0.2, 0.2, 0.2)
# variant -> (points per sample, gts per sample, ROI_PER_IMAGE, seed): 0 the scene, 1 fewer points but more samples and rois
B_VARIANTS = {0: ((1500, 1100, 900), (6, 1, 0), 32, 5), 1: ((420, 380, 300, 260), (3, 2, 0, 1), 64, 6)}
SEEDS = (1234, 4321)                  # numpy's and torch's global generators before the RoI draws


@functools.lru_cache(maxsize=None)
def scene_b(variant=0):
    """-> dict(points (N, 4) [sample, x, y, z], gt_boxes (B, G, 8), counts, target_cfg): per gt points on the box's faces and
    inside it (foreground), points just outside a face (inside the enlarged box only: ignored) and ground clutter"""
    counts, gts, per_image, seed = B_VARIANTS[variant]
    rs = np.random.RandomState(seed)
    B, G = len(counts), max(gts)
    gt = np.zeros((B, G, 8), dtype=F)
    chunks = []
    for b, (n, k) in enumerate(zip(counts, gts)):
        for j in range(k):
            ci = (j + b) % 3
            size = np.asarray(MEAN_SIZE[ci]) * rs.uniform(0.9, 1.15, 3)
            gt[b, j] = [8.0 + 9.0 * (j % 3) + rs.uniform(-1, 1), -9.0 + 9.0 * (j // 3) + rs.uniform(-1, 1), rs.uniform(-1.0, -0.6), *size,
                        rs.uniform(-3.2, 3.2), ci + 1]
        pts = np.zeros((n, 3))
        pts[:, 0], pts[:, 1], pts[:, 2] = rs.uniform(0, 36, n), rs.uniform(-16, 12, n), -1.75 + rs.normal(0, 0.05, n)
        n_fg, n_ring = (int(0.2 * n), int(0.08 * n)) if k else (0, 0)
        for i in range(n_fg + n_ring):
            g = gt[b, i % k].astype(np.float64)
            local = rs.uniform(-0.48, 0.48, 3) * g[3:6]
            face = rs.randint(3)
            if i < n_fg:
                if rs.uniform() < 0.7:
                    local[face] = rs.choice((-0.49, 0.49)) * g[3 + face]             # on a face, inside
            else:
                local[face] = rs.choice((-1, 1)) * (0.5 * g[3 + face] + 0.05)      # past a face, inside the enlarged box
            c, s = np.cos(g[6]), np.sin(g[6])
            pts[i] = [g[0] + local[0] * c - local[1] * s, g[1] + local[0] * s + local[1] * c, g[2] + local[2]]
        pts = pts[rs.permutation(n)]
        chunks.append(np.concatenate([np.full((n, 1), float(b)), pts], axis=1))
    points = np.concatenate(chunks).astype(F)
    points.setflags(write=False), gt.setflags(write=False)
    return dict(points=points, gt_boxes=gt, counts=counts, B=B, target_cfg=dict(B_TARGET, ROI_PER_IMAGE=per_image))


def mean_size():
    return np.asarray(MEAN_SIZE, dtype=F)


def extend_of(gt):
    return pt.enlarge(gt, EXTEND)


def net_point(labels, box_labels, seed=31):
    """the stand-in for the point head's network -> {"cls" (N, 3), "box" (N, 8)} float32: logits that favour the label's class
    (an ignored point a little), the box labels plus noise, small on most rows and large on one in four"""
    rs = np.random.RandomState(seed)
    labels, box_labels = np.asarray(labels).astype(np.int64), np.asarray(box_labels, F)
    N = len(labels)
    cls = rs.normal(-2.0, 1.5, (N, 3))
    fg = np.flatnonzero(labels > 0)
    cls[fg, np.clip(labels[fg] - 1, 0, 2)] += 6.0
    cls[labels < 0] += 1.0
    sigma = np.where(rs.uniform(size=(N, 1)) < 0.25, 0.2, 0.02)
    box = (box_labels.astype(np.float64) + rs.normal(0, 1.0, (N, 8)) * sigma).astype(F)
    return {"cls": cls.astype(F), "box": box}


def net_roi(targets, seed=41):
    """the stand-in for the RoI head's network in training -> {"cls" (B M, 1), "reg" (B M, 7)} float32: logits that favour the
    classification label, on the rows that regress the float64 encode of their gt plus noise, elsewhere noise"""
    rs = np.random.RandomState(seed)
    labels = np.asarray(targets["rcnn_cls_labels"]).astype(np.float64).reshape(-1)
    valid = np.asarray(targets["reg_valid_mask"]).reshape(-1) > 0
    code = roi_encode64(targets["gt_of_rois"], targets["rois"]).reshape(len(labels), 7).astype(np.float64)
    noise = rs.normal(0, 0.05, (len(labels), 7))
    reg = np.where(valid[:, None], code + noise, noise).astype(F)
    cls = (np.where(labels >= 0, 4.0 * labels - 2.0, 0.0) + rs.normal(0, 1.0, len(labels))).astype(F)
    return {"cls": cls.reshape(-1, 1), "reg": reg}


def net_rcnn_test(rois, roi_scores, seed=51):
    """the stand-in for the RoI head's network at test time -> {"cls" (B M, 1), "reg" (B M, 7)} float32"""
    rs = np.random.RandomState(seed)
    scores = np.asarray(roi_scores, F).astype(np.float64).reshape(-1)
    cls = (0.8 * scores - 1.0 + rs.normal(0, 0.5, len(scores))).astype(F)
    return {"cls": cls.reshape(-1, 1), "reg": rs.normal(0, 0.04, (len(scores), 7)).astype(F)}


# ---------------------------------------------------------------------------------------------------- chain B: the stages
@memo
def ref_b_point_targets(points, gt, ext):
    member = pt.membership(points, gt, ext)
    return pt.assign(points, gt, ext, 3, mean_size(), want_box=True, member=member), member


def point_loss_cfg(rows):
    return pl.base_cfg(B=1, N=int(rows), **B_POINT_LOSS)


@memo
def ref_b_point_loss(inp):
    cfg = point_loss_cfg(len(inp["labels"]))
    ours, dec = pl._evaluate(inp, cfg, None)
    return ours, pl.exact(inp, cfg, dec)


def point_loss_inputs(preds, labels, box_labels):
    return {"cls": np.asarray(preds["cls"], F), "labels": np.asarray(labels), "box": np.asarray(preds["box"], F),
            "box_t": np.asarray(box_labels, F), "cw": np.ones(8, dtype=F)}


@memo
def ref_b_point_decode(box, xyz, cls):
    return bd.point_decode(box, xyz, cls, mean_size())


@memo
def ref_b_proposals(box, cls, batch_index, B, post, thresh):
    return ps.proposals(box, cls, B, B_TRAIN_NMS["NMS_PRE_MAXSIZE"], post, thresh, True, batch_index)


def seed_draws():
    import torch
    np.random.seed(SEEDS[0])
    torch.manual_seed(SEEDS[1])


@memo
def ref_b_roi_targets(rois, scores, labels, gt, cfg):
    """the restatement under the seeds the device call ran under (tests/roi_targets_cases.py:seeded_draws)"""
    seed_draws()
    details = {}
    return rt.assign_targets(rois, scores, labels, gt, cfg, rt.reference_draws, details=details), details


@memo
def ref_b_pool(xyz, boxes, feat):
    """one sample: xyz (n, 3), boxes (M, 7), feat (n, C) -> (pooled (1, M, 64, 3 + C), flag (1, M)) from zero-filled outputs"""
    large = rp.enlarge(np.asarray(boxes, F)[None, :, :7], (POOL_EXTRA,) * 3)
    M, C = len(boxes), feat.shape[1]
    return rp.roipoint_pool3d(np.asarray(xyz, F)[None], large, np.asarray(feat, F)[None], POOL_POINTS,
                              np.zeros((1, M, POOL_POINTS, 3 + C), F), np.zeros((1, M), np.int32))


def roi_loss_cfg(targets):
    B, M = np.asarray(targets["reg_valid_mask"]).shape
    soft = np.asarray(targets["rcnn_cls_labels"]).dtype == np.float32
    return rl.base_cfg(B=B, M=M, labels="iou" if soft else "cls", label_dtype="float32" if soft else "int64", **B_ROI_LOSS)


def roi_loss_inputs(preds, targets):
    R = np.asarray(targets["reg_valid_mask"]).size
    return {"cls": np.asarray(preds["cls"], F).reshape(R), "reg": np.asarray(preds["reg"], F).reshape(R, 7),
            "labels": np.asarray(targets["rcnn_cls_labels"]).reshape(R), "mask": np.asarray(targets["reg_valid_mask"]).reshape(R),
            "gt": np.asarray(targets["gt_of_rois"], F).reshape(R, -1), "src": np.asarray(targets["gt_of_rois_src"], F).reshape(R, -1),
            "rois": np.asarray(targets["rois"], F).reshape(R, 7), "cw": np.ones(7, dtype=F)}


@memo
def ref_b_roi_loss(inp, B, M):
    soft = inp["labels"].dtype == np.float32
    cfg = rl.base_cfg(B=B, M=M, labels="iou" if soft else "cls", label_dtype="float32" if soft else "int64", **B_ROI_LOSS)
    ours, dec = rl._evaluate(inp, cfg, None)
    return ours, rl.exact(inp, cfg, dec)


@memo
def ref_b_roi_decode(rois, reg):
    return bd.roi_decode(rois, reg).reshape(np.shape(rois))


@memo
def ref_b_post(box, cls, labels, gt, rois, B):
    return pp.post_process(box, cls, B, B_POST["NMS_PRE_MAXSIZE"], B_POST["NMS_POST_MAXSIZE"], B_POST["NMS_THRESH"], rotated=True,
                           score_thresh=B_POST["SCORE_THRESH"], normalized=False, labels=labels, gt_boxes=gt, rois=rois,
                           recall_thresh=B_POST["RECALL_THRESH_LIST"])


def offsets_of(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def free_chain_b(variant=0, score_type="cls"):
    """the restatements alone, from the scene -> every stage's result of the training step and of the test-time forward"""
    sc = scene_b(variant)
    points, gt, B = sc["points"], sc["gt_boxes"], sc["B"]
    cfg = dict(sc["target_cfg"], CLS_SCORE_TYPE=score_type)
    ext = extend_of(gt)
    ptargets, member = ref_b_point_targets(points, gt, ext)
    ppreds = net_point(ptargets["point_cls_labels"], ptargets["point_box_labels"])
    ploss, _ = ref_b_point_loss(point_loss_inputs(ppreds, ptargets["point_cls_labels"], ptargets["point_box_labels"]))
    pboxes = ref_b_point_decode(ppreds["box"], points[:, 1:4], ppreds["cls"])
    props = ref_b_proposals(pboxes, ppreds["cls"], points[:, 0], B, B_TRAIN_NMS["NMS_POST_MAXSIZE"], B_TRAIN_NMS["NMS_THRESH"])
    rtargets, rdetails = ref_b_roi_targets(props[0], props[1], props[2], gt, cfg)
    off = offsets_of(sc["counts"])
    pooled = [ref_b_pool(points[off[b]:off[b + 1], 1:4], rtargets["rois"][b], ppreds["cls"][off[b]:off[b + 1]]) for b in range(B)]
    rpreds = net_roi(rtargets)
    rloss, _ = ref_b_roi_loss(roi_loss_inputs(rpreds, rtargets), B, cfg["ROI_PER_IMAGE"])
    tprops = ref_b_proposals(pboxes, ppreds["cls"], points[:, 0], B, B_TEST_NMS["NMS_POST_MAXSIZE"], B_TEST_NMS["NMS_THRESH"])
    tpreds = net_rcnn_test(tprops[0], tprops[1])
    tboxes = ref_b_roi_decode(tprops[0], tpreds["reg"])
    final = ref_b_post(tboxes, tpreds["cls"].reshape(B, -1, 1), tprops[2], gt, tprops[0], B)
    return dict(scene=sc, cfg=cfg, ext=ext, ptargets=ptargets, member=member, ppreds=ppreds, ploss=ploss, pboxes=pboxes, props=props,
                rtargets=rtargets, rdetails=rdetails, pooled=pooled, rpreds=rpreds, rloss=rloss, tprops=tprops, tpreds=tpreds,
                tboxes=tboxes, final=final)


# ---------------------------------------------------------------------------------------------------- the stand-in heads
class Cfg(dict):
    """a dict with attribute access (what the reference's EasyDict gives its classes)"""
    __getattr__ = dict.__getitem__


@functools.lru_cache(maxsize=None)
def head_classes():
    """the four stand-in classes, each named as the reference's class and bound ONCE by every drop-in module that applies"""
    from modest_amd.utils import (anchor_head_loss, box_decode, point_head_loss, point_head_targets, post_processing, proposal_layer,
                                  roi_head_loss, roi_targets)
    anchor = type("AnchorHeadTemplate", (), {})
    anchor_head_loss.bind(anchor), box_decode.bind(anchor)
    point = type("PointHeadBox", (), {})
    point_head_targets.bind(point), point_head_loss.bind(point), box_decode.bind(point, "PointHeadTemplate")
    roi = type("RoIHeadTemplate", (), {})
    proposal_layer.bind(roi), roi_targets.bind(roi), roi_head_loss.bind(roi), box_decode.bind(roi)
    detector = post_processing.bind(type("Detector3DTemplate", (), {}))
    return types.SimpleNamespace(anchor=anchor, point=point, roi=roi, detector=detector)


def anchor_head(device, anchors=None):
    """the anchor head: model_cfg, box_coder, the loss stubs, num_class, the list of per-class anchor tensors and the drop-in
    assigner as target_assigner"""
    import torch
    from modest_amd.utils import target_assigner
    head = head_classes().anchor()
    head.model_cfg = al.model_cfg(A_LOSS, DIR_LIMIT_OFFSET=A_DIR_LIMIT_OFFSET)
    head.num_class, head.num_anchors_per_location, head.use_multihead = 3, 6, False
    head.box_coder = bd.coder_stub("ResidualCoder", code_size=7, encode_angle_by_sincos=False)
    head.anchors = [torch.from_numpy(np.array(a)).to(device) for a in (a_anchors() if anchors is None else anchors)]
    head.cls_loss_func = al.loss_stub("SigmoidFocalClassificationLoss", alpha=al.ALPHA, gamma=al.GAMMA)
    head.reg_loss_func = al.loss_stub("WeightedSmoothL1Loss", beta=A_LOSS["beta"], code_weights=torch.ones(7, device=device))
    head.dir_loss_func = al.loss_stub("WeightedCrossEntropyLoss")
    head.target_assigner = target_assigner.AxisAlignedTargetAssigner(at.model_cfg(A_CFG), CLASS_NAMES, head.box_coder)
    head.forward_ret_dict = {}
    return head


def point_head(device):
    import torch
    head = head_classes().point()
    head.model_cfg = pl.model_cfg(pl.base_cfg(B=1, N=1, **B_POINT_LOSS))
    head.num_class = 3
    head.box_coder = bd.coder_stub("PointResidualCoder", code_size=8, use_mean_size=True, mean_size=torch.from_numpy(mean_size()).to(device))
    head.cls_loss_func = pl.loss_stub("SigmoidFocalClassificationLoss", alpha=pl.ALPHA, gamma=pl.GAMMA)
    head.reg_loss_func = pl.loss_stub("WeightedSmoothL1Loss", beta=B_POINT_LOSS["beta"], code_weights=torch.ones(8, device=device))
    head.forward_ret_dict = {}
    return head


def roi_head(device, target_cfg):
    import torch
    head = head_classes().roi()
    head.model_cfg = rl.model_cfg(rl.base_cfg(B=1, M=1, **B_ROI_LOSS))
    head.model_cfg["TARGET_CONFIG"] = Cfg(target_cfg)
    head.num_class = 3
    head.box_coder = bd.coder_stub("ResidualCoder", code_size=7, encode_angle_by_sincos=False)
    head.reg_loss_func = rl.loss_stub("WeightedSmoothL1Loss", beta=B_ROI_LOSS["beta"], code_weights=torch.ones(7, device=device))
    head.forward_ret_dict = {}
    return head


def detector(post):
    det = head_classes().detector()
    nms = Cfg(MULTI_CLASSES_NMS=False, **{k: post[k] for k in ("NMS_TYPE", "NMS_THRESH", "NMS_PRE_MAXSIZE", "NMS_POST_MAXSIZE")})
    det.model_cfg = Cfg(POST_PROCESSING=Cfg(NMS_CONFIG=nms, RECALL_THRESH_LIST=list(post["RECALL_THRESH_LIST"]),
                                            SCORE_THRESH=post["SCORE_THRESH"], OUTPUT_RAW_SCORE=post["OUTPUT_RAW_SCORE"]))
    det.num_class = 3
    return det
