"""numpy restatement of ``roipoint_pool3d_cuda.forward`` and ``roiaware_pool3d_cuda.points_in_boxes_gpu`` under the
contract of DESIGN.md section 7e (not a test module; tests/test_roipool_cpu.py, tests/test_gpu_roipool.py and
tools/make_golden_roipool.py import it).

The predicate, box [cx, cy, cz, dx, dy, dz, rz]:
  * outside if float64(|z - cz|) > float64(dz) / 2.0, the difference in float32, strict;
  * cosa / sina = float32(np.cos / np.sin of float64(-rz));
  * lx = sx * cosa + sy * (-sina), ly = sx * sina + sy * cosa in float32 (numpy does not fuse);
  * inside if float64(|lx|) < float64(dx) / 2.0 + float64(float32(1e-5)) and the same for ly / dy, strict.
NaN decides through these comparisons as written.
"""
import numpy as np

MARGIN = np.float64(np.float32(1e-5))


def cos_sin_f32(rz):
    a = -np.asarray(rz, dtype=np.float32).astype(np.float64)
    return np.cos(a).astype(np.float32), np.sin(a).astype(np.float32)


def inside_mask(pts, boxes):
    """pts (N, 3), boxes (M, 7) float32 -> (M, N) bool"""
    p = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3)
    bx = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 7)
    out = np.zeros((len(bx), len(p)), dtype=bool)
    if out.size == 0:
        return out
    cosa, sina = cos_sin_f32(bx[:, 6])
    x, y, z = p[None, :, 0], p[None, :, 1], p[None, :, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        zout = np.abs(z - bx[:, None, 2]).astype(np.float64) > bx[:, None, 5].astype(np.float64) / 2.0
        sx, sy = x - bx[:, None, 0], y - bx[:, None, 1]
        lx = sx * cosa[:, None] + sy * (-sina)[:, None]
        ly = sx * sina[:, None] + sy * cosa[:, None]
        assert lx.dtype == np.float32 and ly.dtype == np.float32
        inx = np.abs(lx).astype(np.float64) < bx[:, None, 3].astype(np.float64) / 2.0 + MARGIN
        iny = np.abs(ly).astype(np.float64) < bx[:, None, 4].astype(np.float64) / 2.0 + MARGIN
    return ~zout & inx & iny


def points_in_boxes(boxes, pts, given=None):
    """boxes (B, M, 7), pts (B, N, 3) -> (B, N) int32: the lowest index of a box holding the point, else as given (-1)"""
    B, N = pts.shape[0], pts.shape[1]
    out = np.full((B, N), -1, dtype=np.int32) if given is None else np.array(given, dtype=np.int32)
    if boxes.shape[1] == 0 or N == 0:
        return out
    for b in range(B):
        m = inside_mask(pts[b], boxes[b])
        hit = m.any(axis=0)
        out[b, hit] = m.argmax(axis=0)[hit]
    return out


def roipoint_pool3d(xyz, boxes, feat, s, pooled_given, flag_given):
    """xyz (B, N, 3), boxes (B, M, 7), feat (B, N, C), pooled_given (B, M, s, 3 + C), flag_given (B, M) int32
    -> (pooled, flag), copies"""
    B, N = xyz.shape[0], xyz.shape[1]
    M = boxes.shape[1]
    pooled = np.array(pooled_given, dtype=np.float32)
    flag = np.array(flag_given, dtype=np.int32)
    rows_all = np.concatenate([np.asarray(xyz, dtype=np.float32), np.asarray(feat, dtype=np.float32).reshape(B, N, -1)],
                              axis=2)
    for b in range(B):
        mask = inside_mask(xyz[b], boxes[b]) if N else np.zeros((M, 0), dtype=bool)
        for i in range(M):
            idx = np.flatnonzero(mask[i])[:s]
            cnt = len(idx)
            if cnt == 0:
                flag[b, i] = 1
                continue
            if flag_given[b, i] != 0:
                continue
            pooled[b, i] = rows_all[b, idx[np.arange(s) % cnt]]
    return pooled, flag


def inside_counts(xyz, boxes):
    """(B, M) number of inside points, uncapped"""
    return np.stack([inside_mask(xyz[b], boxes[b]).sum(axis=1) for b in range(xyz.shape[0])])


def enlarge(boxes, extra):
    """boxes (..., 7) with dx, dy, dz grown by extra (3,) in float32 (box_utils.enlarge_box3d)"""
    out = np.array(boxes, dtype=np.float32)
    out[..., 3:6] = out[..., 3:6] + np.asarray(extra, dtype=np.float32)
    return out


# ---- the detector's shapes (tests/test_gpu_roipool.py and tools/roipool_bench.py) ----------------------------------------
def synthetic_scans():
    """B = 2 clouds of 12 288 points sampled WITH repetition from synthetic Lyft-shape scans, 130 feature channels, and
    the scans' objects as boxes [cx, cy, cz, dx, dy, dz, rz] in the clouds' frame: (xyz, feat, [objects of cloud 0, 1])"""
    from modest_amd import synth
    rs = np.random.RandomState(17)
    clouds, objs = [], []
    for sid in (11, 12):
        sc = synth.make_scan(sid, n_live=9000 if sid == 11 else 30000, n_trav=1, n_frames=1, n_per_frame=2000)
        xyz = sc.live_xyz
        clouds.append(xyz[rs.choice(len(xyz), 12288, replace=True)])
        mob = synth.make_mobiles(sid, 5.0 * sid % 200.0)
        world = synth.make_world(0)
        near = world.boxes[np.abs(world.boxes[:, 0] - 5.0 * sid % 200.0) < 40.0]
        obj = np.concatenate([mob, near])
        to_ref = np.linalg.inv(sc.world_from_ref)
        ctr = (np.c_[obj[:, :3], np.ones(len(obj))] @ to_ref.T)[:, :3]
        x_axis = to_ref[:3, 0]                       # the world's x axis in the clouds' frame gives the heading
        rz = np.full(len(obj), np.arctan2(x_axis[1], x_axis[0]))
        objs.append(np.c_[ctr, obj[:, 3:6], rz].astype(np.float32))
    xyz = np.ascontiguousarray(np.stack(clouds), dtype=np.float32)
    feat = rs.randn(2, 12288, 130).astype(np.float32)
    assert all(len(np.unique(xyz[b], axis=0)) < 12288 for b in range(2))
    return xyz, feat, objs


def synthetic_rois(rs, objs, m):
    """m boxes per cloud: the objects, jittered copies of them, a few far from any point and a few large ones"""
    out = np.zeros((2, m, 7), dtype=np.float32)
    for b in range(2):
        o = objs[b]
        pick = o[rs.randint(0, len(o), m)].astype(np.float64)
        pick[:, :3] += rs.normal(0, 0.4, (m, 3)) * (rs.rand(m, 1) < 0.8)
        pick[:, 3:6] *= rs.uniform(0.8, 1.4, (m, 3))
        pick[:, 6] += rs.normal(0, 0.3, m) + np.pi * rs.randint(-2, 3, m)
        pick[: len(o)] = o[:m][: len(o)]                          # the objects themselves first
        pick[-8:-4, :2] += 500.0                                  # far from any point
        pick[-4:, 3:6] = rs.uniform(15, 40, (4, 3))               # large
        out[b] = pick
    return out


def gt_boxes(rs, objs, m=40, n_gt=(23, 31)):
    """(2, m, 7) gt boxes as OpenPCDet batches them: n_gt real ones per cloud, the rest zero rows"""
    boxes = np.zeros((2, m, 7), dtype=np.float32)
    for b, k in enumerate(n_gt):
        boxes[b, :k] = synthetic_rois(rs, objs, m)[b, :k]
    return boxes


# ---- what the fixture must contain (tools/make_golden_roipool.py and tests/test_roipool_cpu.py assert every entry) ----
def f32_bound_wrong(dx):
    """True if the float32 sum dx * 0.5f + 1e-5f lies below the double bound float64(dx) / 2.0 + float64(1e-5f)"""
    dx = np.float32(dx)
    return np.float64(dx * np.float32(0.5) + np.float32(1e-5)) < np.float64(dx) / 2.0 + MARGIN


def fixture_cases(rec):
    """name -> bool for every case the fixture promises, read from its recorded arrays alone"""
    got = {}
    scenes = [k[:-4] for k in rec if k.endswith("_xyz")]
    cnts, firsts, lasts, tails, Ns, Cs, Ss = set(), set(), set(), False, set(), set(), set()
    rel = set()
    shared = zface = side_in = side_out = wrong = preset = False
    zero_after = zero_alone = nan_pt = nan_box = sentinel_kept = False
    for sc in scenes:
        xyz, boxes, feat = rec[sc + "_xyz"], rec[sc + "_boxes"], rec[sc + "_feat"]
        s = int(rec[sc + "_s"])
        flag0, flag1 = rec[sc + "_flag_given"], rec[sc + "_flag"]
        pooled0, pooled1 = rec[sc + "_pooled_given"], rec[sc + "_pooled"]
        box_idx = rec[sc + "_box_idx"]
        B, N = xyz.shape[:2]
        Ns.add(N), Cs.add(feat.shape[2]), Ss.add(s)
        got["B2"] = got.get("B2", True) and B == 2
        nan_pt |= bool(np.isnan(xyz).any())
        nan_box |= bool(np.isnan(boxes).any())
        for b in range(B):
            m = inside_mask(xyz[b], boxes[b])
            shared |= bool((m.sum(axis=0) >= 2).any())
            for i in range(boxes.shape[1]):
                idx = np.flatnonzero(m[i])
                c = len(idx)
                cnts.add(c)
                rel.add("0" if c == 0 else "S-1" if c == s - 1 else "S" if c == s else "S+1" if c == s + 1
                        else ">>S" if c >= 4 * s and c > s + 1 else "other")
                bx = boxes[b, i]
                if c:
                    firsts.add(int(idx[0])), lasts.add(int(idx[-1]))
                    firsts.add(int(idx[0]) - N), lasts.add(int(idx[-1]) - N)   # N - 1 is recorded as -1
                    tails |= bool(idx[0] >= N - 64 and N > 64)
                    preset |= bool(flag0[b, i] != 0 and flag1[b, i] == flag0[b, i]
                                   and np.array_equal(pooled0[b, i].view(np.uint32), pooled1[b, i].view(np.uint32)))
                    zd = np.abs(xyz[b, idx, 2] - bx[2]).astype(np.float64)
                    zface |= bool((zd == np.float64(bx[5]) / 2.0).any() and bx[5] > 0)
                else:
                    sentinel_kept |= bool(flag1[b, i] == 1 and np.array_equal(pooled0[b, i].view(np.uint32),
                                                                              pooled1[b, i].view(np.uint32)))
                if bx[6] == 0 and bx[0] == 0 and bx[1] == 0 and bx[3] > 0:
                    D = np.float64(bx[3]) / 2.0 + MARGIN
                    up = np.float32(D) if np.float64(np.float32(D)) >= D else np.nextafter(np.float32(D), np.float32(np.inf))
                    dn = np.nextafter(up, np.float32(-np.inf))
                    zok = ~(np.abs(xyz[b, :, 2] - bx[2]).astype(np.float64) > np.float64(bx[5]) / 2.0)
                    yok = np.abs(xyz[b, :, 1]) < 0.25 * bx[4]
                    ax = np.abs(xyz[b, :, 0])
                    side_in |= bool((zok & yok & (ax == dn) & m[i]).any())
                    side_out |= bool((zok & yok & (ax == up) & ~m[i]).any())
                    if f32_bound_wrong(bx[3]):
                        f32sum = bx[3] * np.float32(0.5) + np.float32(1e-5)
                        wrong |= bool((zok & yok & (ax == f32sum) & m[i]).any())
                if not bx.any():
                    at0 = np.flatnonzero(m[i])
                    for k in at0:
                        earlier = m[:i, k].any()
                        zero_after |= bool(earlier and box_idx[b, k] < i)
                        zero_alone |= bool(not earlier and box_idx[b, k] == i)
    got.update({
        "cnt 0": "0" in rel, "cnt 1": 1 in cnts, "cnt 2": 2 in cnts, "cnt S-1": "S-1" in rel, "cnt S": "S" in rel,
        "cnt S+1": "S+1" in rel, "cnt >> S": ">>S" in rel,
        "edge indices": all((k in firsts) or (k in lasts) for k in (0, 63, 64, 255, 256, -1)),
        "all inside points in the last 64": tails, "shared points": shared, "z face": zface,
        "one float inside a side face": side_in, "one float outside a side face": side_out,
        "a bound float32 gets wrong": wrong, "pre-set flag on a non-empty box": preset,
        "zero box behind a box that holds the origin": zero_after, "zero box alone at the origin": zero_alone,
        "NaN point": nan_pt, "NaN box": nan_box, "C = 0, 1, 5": Cs >= {0, 1, 5}, "S = 1, 16, 37": Ss >= {1, 16, 37},
        "N not a multiple of 64": any(n % 64 for n in Ns), "sentinel rows of an empty box": sentinel_kept,
    })
    return got
