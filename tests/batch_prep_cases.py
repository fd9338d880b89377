"""Hand-built cases of training-batch preparation for tests/test_batch_prep_cpu.py and tests/test_gpu_batch_prep.py, in the
form tests/batch_prep_seq.py reads.  case(name) is cached and read-only; want(name) is the restatement's stage 1 on it."""
import functools

import numpy as np

import batch_prep_seq as seq

F32 = np.float32
RANGE = (-75.2, -75.2, -2.0, 75.2, 75.2, 4.0)
EXTRA = (0.2, 0.2, 0.2)
ALL_STEPS = ("flip_x", "flip_y", "rotation", "scaling")
TILE = 1024


def database(rng, objects=20, features=4):
    counts = rng.integers(5, 31, objects)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    pts = np.zeros((off[-1], features), F32)
    pts[:, :3] = rng.uniform(-1, 1, (off[-1], 3)) * np.array([2.0, 0.9, 0.8])
    pts[:, 3:] = rng.uniform(0, 1, (off[-1], features - 3))
    return pts.astype(F32), off


def draws(rng, angle=None, scale=None, flip_x=None, flip_y=None):
    import torch
    a = float(rng.uniform(-np.pi / 4, np.pi / 4)) if angle is None else float(angle)
    t = torch.from_numpy(np.array([a])).float()
    return {"flip_x": bool(rng.integers(2)) if flip_x is None else flip_x, "flip_y": bool(rng.integers(2)) if flip_y is None else flip_y,
            "angle": a, "cos": float(torch.cos(t)[0]), "sin": float(torch.sin(t)[0]),
            "scale": float(rng.uniform(0.95, 1.05)) if scale is None else float(scale)}


def boxes(rng, n, spread=60.0, z=(-1.0, 1.0)):
    return np.c_[rng.uniform(-spread, spread, n), rng.uniform(-spread, spread, n), rng.uniform(z[0], z[1], n), rng.uniform(2.5, 5.0, n),
                 rng.uniform(1.5, 2.2, n), rng.uniform(1.4, 2.0, n), rng.uniform(-3.3, 3.3, n)].astype(F32).reshape(n, 7)


def scene(rng, n, features=4, spread=85.0):
    p = np.zeros((n, features), F32)
    p[:, 0:2] = rng.uniform(-spread, spread, (n, 2))
    p[:, 2] = rng.uniform(-2, 2, n)
    p[:, 3:] = rng.uniform(0, 1, (n, features - 3))
    return p.astype(F32)


def sample(rng, n_points, n_gt, n_cand, objects, features=4, groups=2, spread=60.0, **kw):
    gt = boxes(rng, n_gt, spread)
    cand = boxes(rng, n_cand, spread)
    pts = scene(rng, n_points, features)
    if n_cand and n_points >= 8 * n_cand:          # scene points inside every candidate's box: the removal has work
        for j in range(n_cand):
            pts[8 * j:8 * j + 8, :3] = cand[j, :3] + rng.uniform(-0.4, 0.4, (8, 3)).astype(F32)
    s = {"points": pts, "n_points": n_points, "gt_boxes": gt, "gt_classes": rng.integers(0, 4, n_gt), "cand_boxes": cand,
         "cand_classes": np.sort(rng.integers(1, groups + 1, n_cand)), "cand_objects": rng.integers(0, objects, n_cand),
         "mv_height": rng.uniform(-0.5, 0.5, n_cand), "cand_z": (cand[:, 2].astype(np.float64) - rng.uniform(-0.5, 0.5, n_cand)).astype(F32)}
    s["cand_groups"] = s["cand_classes"].copy()
    s.update(draws(rng, **kw))
    return s


def base(rng, samples, db, steps=ALL_STEPS, road_plane=True, **kw):
    c = {"F": db[0].shape[1], "range": np.asarray(RANGE, F32), "extra": np.asarray(EXTRA, F32), "road_plane": road_plane,
         "steps": list(steps), "want_near": True, "remove_outside": True, "min_corners": 1, "db_points": db[0], "db_offsets": db[1],
         "samples": samples}
    c.update(kw)
    return c


def _sizes():
    """scene sizes around the tile and the wavefront; candidates in every other sample, so that the seam between the object
    rows and the scene rows falls inside a tile, and a sample of more than one tile"""
    rng = np.random.default_rng(11)
    db = database(rng)
    ns = [0, 1, 255, 256, 257, 600, TILE - 1, TILE, TILE + 1, 2 * TILE + 77]
    return base(rng, [sample(rng, n, 6, 5 if k % 2 else 0, 20, spread=30.0) for k, n in enumerate(ns)], db)


def _faces():
    """no augmentor: a point exactly on each x / y face (kept) and one float32 step outside (dropped); NaN and infinite
    coordinates; a scene point on each face of a kept candidate's enlarged box"""
    rng = np.random.default_rng(12)
    db = database(rng)
    r = np.asarray(RANGE, F32)
    up, dn = (lambda v: np.nextafter(F32(v), F32(np.inf))), (lambda v: np.nextafter(F32(v), F32(-np.inf)))
    rows = [(r[0], 0, 0), (dn(r[0]), 0, 0), (r[3], 0, 0), (up(r[3]), 0, 0), (0, r[1], 0), (0, dn(r[1]), 0), (0, r[4], 0), (0, up(r[4]), 0),
            (r[3], r[4], 50), (np.nan, 0, 0), (0, np.nan, 0), (30, 1, np.nan), (np.inf, 0, 0), (0, -np.inf, 0), (2, 2, np.inf)]
    cand = np.array([[0, 0, 0, 4, 2, 1.5, 0]], F32)            # centred on the origin: a point's own x is its local x
    big = cand[0, 3:6] + np.asarray(EXTRA, F32)
    tx, ty = seq.f32_up(np.float64(big[0]) / 2 + seq.MARGIN), seq.f32_up(np.float64(big[1]) / 2 + seq.MARGIN)
    tz = seq.f32_down(np.float64(big[2]) / 2)
    for sgn in (1, -1):
        rows += [(sgn * tx, 0, 0), (sgn * dn(tx), 0, 0), (0, sgn * ty, 0), (0, sgn * dn(ty), 0), (0, 0, sgn * tz), (0, 0, sgn * up(tz))]
    pts = np.zeros((len(rows), 4), F32)
    pts[:, :3] = np.array(rows, F32)
    pts[:, 3] = np.arange(len(rows))
    s = {"points": pts, "n_points": len(pts), "gt_boxes": np.zeros((0, 7), F32), "gt_classes": np.zeros(0, int), "cand_boxes": cand,
         "cand_classes": np.array([1]), "cand_groups": np.array([1]), "cand_objects": np.array([3]), "mv_height": np.zeros(1),
         "cand_z": cand[:, 2].copy()}
    s.update(draws(rng))
    gone = sample(rng, 40, 2, 0, 20)
    gone["points"][:, 0] = 200.0                               # every point of this sample is outside
    return base(rng, [s, gone], db, steps=(), road_plane=False)


def _collisions():
    """two class groups: candidates 0 / 1 overlap only each other (both go); 2 touches gt 0 along an edge; 3 is free and kept;
    group 2: 4 lies on the kept 3 (goes), 5 on the dropped 0 (stays), 6 on a gt of a name outside class_names (goes), 7 has
    zero size, 8 a class outside class_names; a sample without gts, and one without gts and with one candidate"""
    rng = np.random.default_rng(13)
    db = database(rng)
    gt = np.array([[10, 0, 0, 4, 2, 1.5, 0], [-20, 10, 0, 4, 2, 1.5, 0.3], [30, 30, 0, 4, 2, 1.5, 7.0], [0, -40, 0, 4, 2, 1.5, -7.5],
                   [50, -50, 0, 4, 2, 1.5, np.pi], [-50, -50, 0, 4, 2, 1.5, -np.pi]], F32)
    cand = np.array([[0, 20, 0, 4, 2, 1.5, 0.2], [1, 20.5, 0, 4, 2, 1.5, -0.4], [14, 0, 0, 4, 2, 1.5, 0], [40, 0, 0, 4, 2, 1.5, 1.0],
                     [40.5, 0.2, 0, 3, 2, 1.5, 2.0], [0.2, 20.1, 0, 3, 1.8, 1.5, 0.1], [-20, 10, 0, 3, 2, 1.5, 0], [20, -20, 0, 0, 0, 0, 0],
                     [-60, 60, 0, 4, 2, 1.5, 0.5]], F32)
    s = {"points": scene(rng, 300), "n_points": 300, "gt_boxes": gt, "gt_classes": np.array([1, 0, 2, 1, 3, 1]), "cand_boxes": cand,
         "cand_classes": np.array([1, 1, 1, 1, 2, 2, 2, 2, 0]), "cand_groups": np.array([1, 1, 1, 1, 2, 2, 2, 2, 2]),
         "cand_objects": np.arange(9), "mv_height": rng.uniform(-0.5, 0.5, 9), "cand_z": rng.uniform(-1, 1, 9).astype(F32)}
    s.update(draws(rng))
    nogt = sample(rng, 200, 0, 6, 20, spread=8.0)
    one = sample(rng, 100, 0, 1, 20)
    return base(rng, [s, nogt, one], db)


def _corners(min_corners):
    """gts against the x1 face and the z1 face: all corners inside; four inside (heading 0, centred on the face); three inside
    (turned by pi / 4 with one corner beyond the face, the top above z1); none"""
    rng = np.random.default_rng(14)
    db = database(rng)
    x1, z1 = RANGE[3], RANGE[5]
    gt = np.array([[0, 0, 0, 4, 2, 1.5, 0.3], [x1, 0, 0, 4, 2, 1.5, 0], [x1 - 1.2, 20, z1, 2, 2, 1.0, np.pi / 4], [x1 + 10, 0, 0, 4, 2, 1.5, 0]], F32)
    s = {"points": scene(rng, 64), "n_points": 64, "gt_boxes": gt, "gt_classes": np.array([1, 1, 1, 1])}
    s.update(draws(rng))
    return base(rng, [s], db, steps=(), road_plane=False, min_corners=min_corners)


def _limit(n):
    rng = np.random.default_rng(15)
    db = database(rng)
    s = sample(rng, 50, n - 200, 200, 20, spread=70.0)
    return base(rng, [s], db)


def _features(f):
    rng = np.random.default_rng(16 + f)
    db = database(rng, features=f)
    return base(rng, [sample(rng, 700, 8, 10, 20, features=f, spread=40.0) for _ in range(3)], db, steps=("scaling", "rotation", "flip_y", "flip_x"))


def _far():
    """PointRCNN's sample_points: a sample with few far points, one with mostly far points, one below NUM_POINTS"""
    rng = np.random.default_rng(17)
    db = database(rng)
    near = sample(rng, 900, 5, 6, 20, spread=30.0)
    near["points"][:, :2] *= F32(0.45)
    near["points"][:40, 0] = F32(60.0)
    far = sample(rng, 900, 5, 0, 20)
    far["points"][:, 0] = np.abs(far["points"][:, 0]) * F32(0.3) + F32(45.0)
    few = sample(rng, 100, 3, 0, 20, spread=30.0)
    few["points"][:, :2] *= F32(0.5)
    return base(rng, [near, far, few], db)


def workload(B=4, n=120_000, n_gt=30, n_cand=40):
    rng = np.random.default_rng(18)
    db = database(rng, objects=200)
    return base(rng, [sample(rng, n, n_gt, n_cand, 200, spread=70.0) for _ in range(B)], db)


CASES = {"sizes": _sizes, "faces": _faces, "collisions": _collisions, "corners min 1": lambda: _corners(1), "corners min 4": lambda: _corners(4),
         "limit": lambda: _limit(512), "5 features": lambda: _features(5), "8 features": lambda: _features(8), "far": _far,
         "no road plane": lambda: dict(_sizes(), road_plane=False), "rotation only": lambda: dict(_collisions(), steps=["rotation"])}


def _freeze(c):
    for v in list(c.values()) + [x for s in c["samples"] for x in s.values()]:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    for s in c["samples"]:
        s.setdefault("cand_boxes", np.zeros((0, 7), F32))
        for k in ("cand_classes", "cand_groups", "cand_objects"):
            s.setdefault(k, np.zeros(0, np.int64))
        s.setdefault("mv_height", np.zeros(0))
        s.setdefault("cand_z", np.zeros(0, F32))
    return _freeze(c)


@functools.lru_cache(maxsize=None)
def want(name):
    return seq.stage1(case(name))


# stage 2: (processors of the restatement, num_points / shuffle of ops.batch_prep_order_draws)
ORDERS = {"sample 400": ([("sample_points", 400)], 400, False), "sample 400 then shuffle": ([("sample_points", 400), ("shuffle_points",)], 400, True),
          "shuffle only": ([("shuffle_points",)], None, True), "sample -1": ([("sample_points", -1)], -1, False),
          "nothing": ([], None, False),
          "shuffle then sample 400": ([("shuffle_points",), ("sample_points", 400)], 400, True, True)}       # shuffle_first


# ------------------------------------------------------------------------------------------- the module: a database on disk
CLASS_NAMES = ["Car", "Pedestrian", "Cyclist"]


COLLIDING = {"Car": [[10, 10, -1, 4, 2, 1.5, 0.3], [30, 0, -1, 4, 2, 1.5, 0]],              # the second lies on the scene's gt at (33, 0)
             "Pedestrian": [[10.3, 10.1, -1, 0.8, 0.8, 1.7, 0.1], [28.5, 0, -1, 0.8, 0.8, 1.7, 0]],   # on the kept Car, on the dropped Car
             "Cyclist": [[-40, -40, -1, 1.8, 0.8, 1.7, 1.0]], "Van": []}


def write_database(root, seed=21, per_class=(7, 5, 12), given=None):
    """a gt database as create_groundtruth_database leaves it: <root>/gt_database/*.bin and <root>/dbinfos.pkl
    -> the infos {class: [info]}.  given: {class: boxes} instead of drawn boxes (every object then passes the PREPARE filters)"""
    import os
    import pickle
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "gt_database"), exist_ok=True)
    infos = {}
    for name, n in zip(CLASS_NAMES + ["Van"], tuple(per_class) + (2,)):
        infos[name] = []
        bx = boxes(rng, n, spread=55.0)
        if given is not None:
            bx = np.asarray(given[name], F32).reshape(-1, 7)
            n = len(bx)
        for i in range(n):
            k = int(rng.integers(3, 31)) if given is None else int(rng.integers(6, 31))
            pts = np.c_[rng.uniform(-1, 1, (k, 3)) * np.array([2.0, 0.9, 0.8]), rng.uniform(0, 1, (k, 1))].astype(F32)
            path = f"gt_database/{name}_{i}.bin"
            pts.tofile(os.path.join(root, path))
            infos[name].append({"name": name, "path": path, "box3d_lidar": bx[i], "num_points_in_gt": k, "difficulty": int(rng.integers(-1, 3)) if given is None else 0})
    with open(os.path.join(root, "dbinfos.pkl"), "wb") as f:
        pickle.dump(infos, f)
    return infos


def dataset_cfg(processors="pointrcnn", limit_whole_scene=False, scale=(0.95, 1.05), flips=("x",), road_plane=True, num_points=512,
                sample_groups=("Car:5", "Pedestrian:4", "Van:3", "Cyclist:4")):
    sampler = {"NAME": "gt_sampling", "USE_ROAD_PLANE": road_plane, "DB_INFO_PATH": ["dbinfos.pkl"],
               "PREPARE": {"filter_by_min_points": ["Car:5", "Pedestrian:5", "Cyclist:5"], "filter_by_difficulty": [-1]},
               "SAMPLE_GROUPS": list(sample_groups), "NUM_POINT_FEATURES": 4, "DATABASE_WITH_FAKELIDAR": False,
               "REMOVE_EXTRA_WIDTH": [0.0, 0.0, 0.0], "LIMIT_WHOLE_SCENE": limit_whole_scene}
    aug = [sampler, {"NAME": "random_world_flip", "ALONG_AXIS_LIST": list(flips)},
           {"NAME": "random_world_rotation", "WORLD_ROT_ANGLE": [-0.78539816, 0.78539816]},
           {"NAME": "random_world_scaling", "WORLD_SCALE_RANGE": list(scale)}]
    proc = [{"NAME": "mask_points_and_boxes_outside_range", "REMOVE_OUTSIDE_BOXES": True}]
    if processors in ("pointrcnn", "shuffle first"):
        proc += [{"NAME": "sample_points", "NUM_POINTS": {"train": num_points, "test": num_points}},
                 {"NAME": "shuffle_points", "SHUFFLE_ENABLED": {"train": True, "test": False}}]
        if processors == "shuffle first":
            proc[1], proc[2] = proc[2], proc[1]
    elif processors == "pillars":
        proc += [{"NAME": "shuffle_points", "SHUFFLE_ENABLED": {"train": True, "test": False}},
                 {"NAME": "transform_points_to_voxels", "VOXEL_SIZE": [0.8, 0.8, 6.0], "MAX_POINTS_PER_VOXEL": 8,
                  "MAX_NUMBER_OF_VOXELS": {"train": 4000, "test": 4000}}]
    return {"POINT_CLOUD_RANGE": list(RANGE), "DATA_AUGMENTOR": {"DISABLE_AUG_LIST": ["placeholder"], "AUG_CONFIG_LIST": aug},
            "POINT_FEATURE_ENCODING": {"encoding_type": "absolute_coordinates_encoding", "used_feature_list": ["x", "y", "z", "intensity"],
                                       "src_feature_list": ["x", "y", "z", "intensity"]},
            "DATA_PROCESSOR": proc}


V2C = np.array([[7.5e-3, -0.99997, -6.2e-4, -4.1e-3], [1.48e-2, 7.3e-4, -0.99989, -7.6e-2], [0.99986, 7.5e-3, 1.48e-2, -0.272]], F32)
R0 = np.array([[0.99992, 9.8e-3, -7.4e-3], [-9.9e-3, 0.99994, -4.3e-3], [7.4e-3, 4.4e-3, 0.99996]], F32)


def raw_batch(B=3, n=700, seed=22):
    rng = np.random.default_rng(seed)
    names = np.array(CLASS_NAMES + ["Van"])
    out = {"points": [], "gt_boxes": [], "gt_classes": [], "gt_names": [], "road_plane": [], "V2C": [], "R0": [], "batch_size": B,
           "frame_id": np.array([f"{i:06d}" for i in range(B)]), "raw_batch": True}
    for b in range(B):
        g = int(rng.integers(2, 7)) if b != 1 else 0
        nm = names[rng.integers(0, 4, g)]
        out["points"].append(scene(rng, n + 13 * b))
        out["gt_boxes"].append(boxes(rng, g, spread=50.0))
        out["gt_names"].append(nm)
        out["gt_classes"].append(np.array([CLASS_NAMES.index(x) + 1 if x in CLASS_NAMES else 0 for x in nm], np.int64))
        out["road_plane"].append(np.array([0.01, -0.999, 0.02, 1.65 + 0.01 * b]))
        out["V2C"].append(V2C)
        out["R0"].append(R0)
    return out


# ------------------------------------------------------------------- the recording of the reference's own three classes
GOLD = __import__("os").path.join(__import__("os").path.dirname(__import__("os").path.abspath(__file__)), "golden", "batch_prep.npz")


@functools.lru_cache(maxsize=None)
def golden():
    """(arrays, meta) of tests/golden/batch_prep.npz (tools/make_golden_batch_prep.py)"""
    import json
    g = np.load(GOLD)
    return g, json.loads(str(g["meta"]))


def write_golden_database(root, prefix="db"):
    """a recorded database (a scene's meta names its prefix under "db") back on disk, as the reference read it"""
    import os
    import pickle
    g, _ = golden()
    g = {key[len(prefix) + 1:]: g[key] for key in g.files if key.startswith(prefix + "_")}
    g = {"db_" + key: v for key, v in g.items()}
    os.makedirs(os.path.join(root, "gt_database"), exist_ok=True)
    off = np.concatenate([[0], np.cumsum(g["db_counts"])])
    infos, seen = {}, {}
    for i, name in enumerate(g["db_names"]):
        name = str(name)
        k = seen[name] = seen.get(name, -1) + 1
        path = f"gt_database/{name}_{k}.bin"
        g["db_points"][off[i]:off[i + 1]].astype(F32).tofile(os.path.join(root, path))
        infos.setdefault(name, []).append({"name": name, "path": path, "box3d_lidar": g["db_boxes"][i], "num_points_in_gt": int(g["db_counts"][i]),
                                           "difficulty": int(g["db_difficulty"][i])})
    with open(os.path.join(root, "dbinfos.pkl"), "wb") as f:
        pickle.dump(infos, f)


def golden_samples(k):
    """scene k -> (meta, [raw sample as collate_raw stacks it, B = 1], [(recorded points, recorded gt_boxes)])"""
    g, meta = golden()
    m = meta["scenes"][k]
    raws, recs = [], []
    for b in range(m["B"]):
        names = g[f"s{k}_{b}_gt_names"].astype(str)
        cls = np.array([CLASS_NAMES.index(x) + 1 if x in CLASS_NAMES else 0 for x in names], np.int64)
        raws.append({"points": [g[f"s{k}_{b}_points"]], "gt_boxes": [g[f"s{k}_{b}_gt_boxes"]], "gt_names": [names], "gt_classes": [cls],
                     "road_plane": [g[f"s{k}_{b}_road_plane"]], "V2C": [g[f"s{k}_{b}_V2C"]], "R0": [g[f"s{k}_{b}_R0"]], "batch_size": 1,
                     "frame_id": np.array([f"{b:06d}"]), "raw_batch": True})
        recs.append((g[f"s{k}_{b}_out_points"], g[f"s{k}_{b}_out_gt_boxes"]))
    return m, raws, recs


def within_contract(got_points, got_gt, rec_points, rec_gt, st, rows):
    """The contract against the recording.  Bit for bit: number and order, z, the features, box z / dx / dy / dz, heading and
    class.  x and y of points and of box centres: OUR values lie within the derived float32 bound (seq.exact_xy) of the exact
    rotation and scaling of the same float32 inputs by the same float32 c, s and scale, and the RECORDED values satisfy the same
    bound.  st: the restatement's stage of the sample, rows: the order its stage 2 left."""
    if got_points.shape != rec_points.shape or got_gt.shape != rec_gt.shape:
        return False
    ok = seq.same_bits(got_points[:, 2:], rec_points[:, 2:]) and seq.same_bits(got_gt[:, 2:], rec_gt[:, 2:])
    e, b = st["exact_xy"][rows], st["bound_xy"][rows]
    for v, ex, bd in ((got_points, e, b), (rec_points, e, b), (got_gt, st["gt_exact_xy"], st["gt_bound_xy"]),
                      (rec_gt, st["gt_exact_xy"], st["gt_bound_xy"])):
        ok = ok and v[:, :2].shape == ex.shape and bool((np.abs(v[:, :2].astype(np.float64) - ex) <= bd).all())
    return ok


def error_over_bound(points, gt, st, rows):
    """largest |value - exact| / bound over x and y of the points and of the box centres (a figure to print, no yardstick)"""
    r = [np.abs(points[:, :2].astype(np.float64) - st["exact_xy"][rows]) / st["bound_xy"][rows],
         np.abs(gt[:, :2].astype(np.float64) - st["gt_exact_xy"]) / st["gt_bound_xy"]]
    return float(max(x.max() if x.size else 0.0 for x in r))


def restate_scene(k, root):
    """the restatement from the seed alone: the module's host plan and the stage-2 draws on one generator, sample by sample as
    the reference draws -> [(points (n, F), gt (m, 8), the stage-1 dict, the rows stage 2 left)]"""
    from modest_amd.utils import batch_prep as bp
    m, raws, _ = golden_samples(k)
    cfg = m["cfg"]
    write_golden_database(str(root), m["db"])
    twin = bp.BatchPrepOnDevice(cfg, CLASS_NAMES, root, device="cpu",
                                database=bp.GtDatabaseOnDevice(root, cfg["DATA_AUGMENTOR"]["AUG_CONFIG_LIST"][0], CLASS_NAMES, device="cpu"))
    procs = ([("sample_points", twin.num_points)] if twin.num_points is not None else []) + ([("shuffle_points",)] if twin.shuffle else [])
    rs = np.random.RandomState(m["seed"])
    out = []
    for raw in raws:
        r = {key: raw[key][0] for key in ("points", "gt_boxes", "gt_classes", "gt_names", "road_plane", "V2C", "R0")}
        s = dict(twin.plan_sample(r, rs), points=r["points"])
        c = {"F": 4, "range": twin.range, "extra": np.asarray(twin.extra, F32), "road_plane": twin.road_plane, "steps": twin.steps,
             "want_near": True, "remove_outside": twin.remove_outside, "min_corners": twin.min_corners,
             "db_points": twin.database.points.numpy(), "db_offsets": twin.database.offsets, "samples": [s]}
        st = seq.stage1_sample(c, s)
        rows = seq.order_rows([st], procs[::-1] if twin.shuffle_first else procs, rs)[0]
        out.append((st["points"][rows], st["gt"], st, rows))
    return out
