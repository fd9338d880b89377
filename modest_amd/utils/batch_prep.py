"""Training-batch preparation on the device: from a collated batch of RAW training
samples -- after ``get_lidar`` / FOV filtering, before any augmentation -- to the model's inputs, ``points`` (N, 1 + F) with
the batch index in column 0 and ``gt_boxes`` (B, Gmax, 8), the tensors ``prepare_data`` + ``collate_batch`` +
``load_data_to_gpu`` deliver.

  GtDatabaseOnDevice   the gt database of ``gt_sampling`` read once and packed into one device tensor; the sampler's state
  plan_sample          the host's part of a sample: the sampler's candidates, the road plane, the augmentors' draws
  raw_prepare_data     ``DatasetTemplate.prepare_data`` that stops after the point feature encoder (training mode)
  collate_raw          ``DatasetTemplate.collate_batch`` for such samples
  BatchPrepOnDevice    raw batch -> batch_dict: one host plan, ``ops.batch_prep_stage1`` (the batch's one synchronise), the
                       host's stage-2 draws from the counts, ``ops.batch_prep_order``; then ``VoxelizeOnDevice`` where the
                       config has ``transform_points_to_voxels``

Draw order: for samples 0 .. B - 1 all stage-1 draws (per class group in config order the sampler's permutation when due, then
flips, angle, scale in the augmentors' order), then, behind the synchronise, for samples 0 .. B - 1 the stage-2 draws
(sample_points, shuffle_points).  With B = 1 that is the reference's order on one generator.
"""
import pickle
from pathlib import Path

import numpy as np
import torch

from .. import ops

AUGMENTORS = ("gt_sampling", "random_world_flip", "random_world_rotation", "random_world_scaling")
PROCESSORS = ("mask_points_and_boxes_outside_range", "sample_points", "shuffle_points", "transform_points_to_voxels",
              "calculate_grid_size")
RAW_KEY = "raw_batch"


def _get(cfg, name, *default):
    return ops._cfg_get(cfg, name, *default)


class GtDatabaseOnDevice:
    """``DataBaseSampler.__init__`` (database_sampler.py:10-77) with every surviving object's points on the device.
    db_infos[class]: the reference's lists, in its order and of its length after PREPARE; boxes[class] (n, 7) float32;
    first[class]: the class's first object in `offsets` (objects + 1,) int64, the rows of `points` (rows, F) float32."""

    def __init__(self, root_path, sampler_cfg, class_names, device=None, readers=8):
        for flag in ("DATABASE_WITH_FAKELIDAR", "DEBUG"):
            if _get(sampler_cfg, flag, False):
                raise NotImplementedError(f"gt_sampling with {flag} is not provided")
        self.root_path = Path(root_path)
        self.class_names = list(class_names)
        self.features = int(_get(sampler_cfg, "NUM_POINT_FEATURES"))
        self.db_infos = {c: [] for c in self.class_names}
        for p in _get(sampler_cfg, "DB_INFO_PATH"):
            with open(str(self.root_path.resolve() / p), "rb") as f:
                infos = pickle.load(f)
            for c in self.class_names:
                self.db_infos[c].extend(infos[c])
        prepare = _get(sampler_cfg, "PREPARE", {})
        for func_name in (prepare if isinstance(prepare, dict) else vars(prepare)):
            val = _get(prepare, func_name)
            if func_name == "filter_by_min_points":
                self._filter_by_min_points(val)
            elif func_name == "filter_by_difficulty":
                self.db_infos = {k: [i for i in v if i["difficulty"] not in val] for k, v in self.db_infos.items()}
            else:
                raise NotImplementedError(f"gt_sampling PREPARE step {func_name!r} is not provided")
        self.limit_whole_scene = bool(_get(sampler_cfg, "LIMIT_WHOLE_SCENE", False))
        self.sample_groups, self.sample_class_num = {}, {}
        for x in _get(sampler_cfg, "SAMPLE_GROUPS"):
            name, num = x.split(":")
            if name not in self.class_names:
                continue
            self.sample_class_num[name] = num
            self.sample_groups[name] = {"sample_num": num, "pointer": len(self.db_infos[name]),
                                        "indices": np.arange(len(self.db_infos[name]))}
        self.first, self.boxes, paths = {}, {}, []
        for c in self.class_names:
            self.first[c] = len(paths)
            infos = self.db_infos[c]
            bx = np.stack([np.asarray(i["box3d_lidar"]) for i in infos], axis=0) if infos else np.zeros((0, 7))
            if bx.shape[1] > 7:
                raise NotImplementedError(f"database boxes of {c} have {bx.shape[1]} columns: boxes with more than 7 columns (the "
                                          f"velocity columns) are not provided")
            self.boxes[c] = bx.astype(np.float32)
            paths.extend(str(self.root_path / i["path"]) for i in infos)
        from ..kitti_eval import read_files
        blobs = read_files(paths, readers)          # every object's file once (modest_host_read_files)
        row = 4 * self.features
        for p, b in zip(paths, blobs):
            if len(b) % row:
                raise ValueError(f"{p}: {len(b)} bytes are no rows of {self.features} float32")
        self.offsets = np.concatenate([[0], np.cumsum([len(b) // row for b in blobs])]).astype(np.int64)
        host = np.frombuffer(b"".join(blobs), dtype=np.float32).reshape(-1, self.features) if blobs else np.zeros((0, self.features), np.float32)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.points = torch.from_numpy(host.copy()).to(self.device)

    def _filter_by_min_points(self, min_gt_points_list):
        for name_num in min_gt_points_list:
            name, min_num = name_num.split(":")
            if int(min_num) > 0 and name in self.db_infos:
                self.db_infos[name] = [i for i in self.db_infos[name] if i["num_points_in_gt"] >= int(min_num)]

    def sample_with_fixed_number(self, class_name, npr):
        """database_sampler.py:79-96 -> the slots drawn in the class's list"""
        g = self.sample_groups[class_name]
        sample_num, pointer, indices = int(g["sample_num"]), g["pointer"], g["indices"]
        if pointer >= len(self.db_infos[class_name]):
            indices = npr.permutation(len(self.db_infos[class_name]))
            pointer = 0
        slots = np.asarray(indices[pointer: pointer + sample_num], np.int64)
        g["pointer"], g["indices"] = pointer + sample_num, indices
        return slots

    def candidates(self, gt_names, npr):
        """the sampler's draws for one sample (database_sampler.py:183-190), the groups in config order
        -> cand_boxes (C, 7) float32, cand_classes, cand_groups, cand_objects (C,)"""
        gt_names = np.asarray(gt_names).astype(str)
        boxes, cls, grp, obj = [], [], [], []
        for k, (name, g) in enumerate(self.sample_groups.items()):
            if self.limit_whole_scene:
                g["sample_num"] = str(int(self.sample_class_num[name]) - int(np.sum(name == gt_names)))
            if int(g["sample_num"]) > 0:
                slots = self.sample_with_fixed_number(name, npr)
                if len(slots) == 0:
                    raise ValueError(f"gt_sampling: the database holds no object of {name} (the reference fails on np.stack)")
                boxes.append(self.boxes[name][slots])
                cls.append(np.full(len(slots), self.class_names.index(name) + 1, np.int64))
                grp.append(np.full(len(slots), k, np.int64))
                obj.append(self.first[name] + slots)
        cat = lambda parts, empty: np.concatenate(parts, axis=0) if parts else empty   # noqa: E731
        return {"cand_boxes": cat(boxes, np.zeros((0, 7), np.float32)), "cand_classes": cat(cls, np.zeros(0, np.int64)),
                "cand_groups": cat(grp, np.zeros(0, np.int64)), "cand_objects": cat(obj, np.zeros(0, np.int64))}


def put_boxes_on_road_planes(boxes, road_plane, V2C, R0):
    """database_sampler.py:99-116 over calibration_kitti.py:50-73, the reference's numpy expressions -> (lowered z float32,
    mv_height float64); evaluated for all candidates (a row of the small products does not depend on the other rows)"""
    boxes = np.asarray(boxes, np.float32)
    V2C, R0 = np.asarray(V2C), np.asarray(R0)
    a, b, c, d = road_plane
    hom = np.hstack((boxes[:, 0:3], np.ones((len(boxes), 1), dtype=np.float32)))
    center_cam = np.dot(hom, np.dot(V2C.T, R0.T))
    cur_height_cam = (-d - a * center_cam[:, 0] - c * center_cam[:, 2]) / b
    center_cam[:, 1] = cur_height_cam
    rect_hom = np.hstack((center_cam, np.ones((len(boxes), 1), dtype=np.float32)))
    R0_ext = np.hstack((R0, np.zeros((3, 1), dtype=np.float32)))
    R0_ext = np.vstack((R0_ext, np.zeros((1, 4), dtype=np.float32)))
    R0_ext[3, 3] = 1
    V2C_ext = np.vstack((V2C, np.zeros((1, 4), dtype=np.float32)))
    V2C_ext[3, 3] = 1
    cur_lidar_height = np.dot(rect_hom, np.linalg.inv(np.dot(R0_ext, V2C_ext).T))[:, 2]
    mv_height = boxes[:, 2] - boxes[:, 5] / 2 - cur_lidar_height
    z = boxes[:, 2].copy()
    z -= mv_height
    return z.astype(np.float32), np.asarray(mv_height, np.float64)


def _enabled(cfg_list, disabled=()):
    return [c for c in cfg_list if _get(c, "NAME") not in disabled]


class BatchPrepOnDevice:
    """raw batch -> batch_dict on the device; keeps its grow-only workspace, pinned table and staging buffers between batches"""

    def __init__(self, dataset_cfg, class_names, root_path, training=True, device=None, database=None):
        if not training:
            raise NotImplementedError("BatchPrepOnDevice in test mode is not provided (raw_prepare_data calls the reference there)")
        self.class_names = list(class_names)
        self.range = np.asarray(_get(dataset_cfg, "POINT_CLOUD_RANGE"), dtype=np.float32)
        enc = _get(dataset_cfg, "POINT_FEATURE_ENCODING")
        if _get(enc, "encoding_type", "absolute_coordinates_encoding") != "absolute_coordinates_encoding":
            raise NotImplementedError("a point feature encoding other than absolute_coordinates_encoding is not provided")
        used = list(_get(enc, "used_feature_list"))
        if used[:3] != ["x", "y", "z"]:
            raise NotImplementedError("use_lead_xyz false (used_feature_list not led by x, y, z) is not provided")
        self.features = len(used)
        aug = _get(dataset_cfg, "DATA_AUGMENTOR")
        self.steps, self.draws, self.sampler_cfg = [], [], None
        for k, cfg in enumerate(_enabled(_get(aug, "AUG_CONFIG_LIST"), _get(aug, "DISABLE_AUG_LIST", ()))):
            name = _get(cfg, "NAME")
            if name not in AUGMENTORS:
                raise NotImplementedError(f"augmentor {name!r} is not provided: {AUGMENTORS}")
            if name == "gt_sampling":
                if k != 0 or self.sampler_cfg is not None:
                    raise NotImplementedError("gt_sampling anywhere but first among the augmentors is not provided")
                self.sampler_cfg = cfg
            elif name == "random_world_flip":
                for axis in _get(cfg, "ALONG_AXIS_LIST"):
                    if axis not in ("x", "y"):
                        raise ValueError(f"random_world_flip along {axis!r}")
                    self.steps.append("flip_" + axis)
                    self.draws.append(("flip_" + axis,))
            elif name == "random_world_rotation":
                r = _get(cfg, "WORLD_ROT_ANGLE")
                r = list(r) if isinstance(r, (list, tuple)) else [-r, r]
                self.steps.append("rotation")
                self.draws.append(("rotation", float(r[0]), float(r[1])))
            else:
                lo, hi = _get(cfg, "WORLD_SCALE_RANGE")
                if hi - lo >= 1e-3:             # a narrower range is neither drawn nor applied (augmentor_utils.py:72)
                    self.steps.append("scaling")
                    self.draws.append(("scaling", float(lo), float(hi)))
        self.num_points, self.shuffle, self.shuffle_first, self.voxelize = None, False, False, None
        self.remove_outside, self.min_corners, seen = False, 1, []
        for cfg in _get(dataset_cfg, "DATA_PROCESSOR"):
            name = _get(cfg, "NAME")
            if name not in PROCESSORS:
                raise NotImplementedError(f"data processor {name!r} is not provided: {PROCESSORS}")
            if name in seen:
                raise NotImplementedError(f"data processor {name!r} twice is not provided")
            if name == "mask_points_and_boxes_outside_range":
                if seen:
                    raise NotImplementedError("mask_points_and_boxes_outside_range anywhere but first is not provided")
                self.remove_outside = bool(_get(cfg, "REMOVE_OUTSIDE_BOXES"))
                self.min_corners = int(_get(cfg, "min_num_corners", 1))
            elif name == "sample_points":
                self.shuffle_first = "shuffle_points" in seen     # the device then rebuilds the near / far lists in shuffled order
                self.num_points = int(_get(_get(cfg, "NUM_POINTS"), "train"))
            elif name == "shuffle_points":
                self.shuffle = bool(_get(_get(cfg, "SHUFFLE_ENABLED"), "train"))
            elif name == "transform_points_to_voxels":
                from .voxelize import VoxelizeOnDevice
                self.voxelize = VoxelizeOnDevice(_get(cfg, "VOXEL_SIZE"), self.range, _get(cfg, "MAX_POINTS_PER_VOXEL"),
                                                 dict(_get(cfg, "MAX_NUMBER_OF_VOXELS")))
                self.voxelize.train()
            seen.append(name)
        if "mask_points_and_boxes_outside_range" not in seen:
            raise NotImplementedError("a DATA_PROCESSOR without mask_points_and_boxes_outside_range is not provided")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.database = database
        self.road_plane, self.extra = False, (0.0, 0.0, 0.0)
        if self.sampler_cfg is not None:
            if self.database is None:
                self.database = GtDatabaseOnDevice(root_path, self.sampler_cfg, self.class_names, self.device)
            if self.database.features != self.features:
                raise ValueError(f"NUM_POINT_FEATURES = {self.database.features}, the points have {self.features}")
            self.road_plane = bool(_get(self.sampler_cfg, "USE_ROAD_PLANE", False))
            self.extra = tuple(float(v) for v in _get(self.sampler_cfg, "REMOVE_EXTRA_WIDTH"))
        self._workspace = self._table = self._staging = self._staging2 = self._scan = None
        self._no_db = None

    def plan_sample(self, raw, npr):
        """the host's part of one sample, its stage-1 draws made on `npr` in the reference's order"""
        gt = np.asarray(raw["gt_boxes"], np.float32)
        s = {"n_points": len(raw["points"]), "gt_boxes": gt, "gt_classes": np.asarray(raw["gt_classes"], np.int64)}
        if self.sampler_cfg is not None:
            names = np.array([self.class_names[c - 1] if c > 0 else "\0" for c in s["gt_classes"]], dtype=object).astype(str) \
                if "gt_names" not in raw else raw["gt_names"]
            s.update(self.database.candidates(names, npr))
            if self.road_plane:
                s["cand_z"], s["mv_height"] = put_boxes_on_road_planes(s["cand_boxes"], raw["road_plane"], raw["V2C"], raw["R0"]) \
                    if len(s["cand_boxes"]) else (np.zeros(0, np.float32), np.zeros(0))
        for d in self.draws:
            if d[0] in ("flip_x", "flip_y"):
                s[d[0]] = bool(npr.choice([False, True], replace=False, p=[0.5, 0.5]))
            elif d[0] == "rotation":
                s["angle"] = npr.uniform(d[1], d[2])
                t = torch.from_numpy(np.array([s["angle"]])).float()          # as rotate_points_along_z takes them
                s["cos"], s["sin"] = float(torch.cos(t)[0]), float(torch.sin(t)[0])
            else:
                s["scale"] = npr.uniform(d[1], d[2])
        return s

    def __call__(self, raw_batch, np_random=None):
        npr = np.random if np_random is None else np_random
        B = int(raw_batch["batch_size"])
        raws = [{k: raw_batch[k][b] for k in ("points", "gt_boxes", "gt_classes", "road_plane", "V2C", "R0", "gt_names")
                 if k in raw_batch} for b in range(B)]
        for r in raws:
            if np.asarray(r["points"]).ndim != 2 or np.asarray(r["points"]).shape[1] != self.features:
                raise ValueError(f"raw points {np.asarray(r['points']).shape} must be (n, {self.features})")
        samples = [self.plan_sample(r, npr) for r in raws]
        if self.database is not None:
            offsets, db = self.database.offsets, self.database.points
        else:
            if self._no_db is None:
                self._no_db = torch.zeros((0, self.features), dtype=torch.float32, device=self.device)
            offsets, db = np.zeros(1, np.int64), self._no_db
        plan = ops.batch_prep_plan(samples, offsets, self.features, self.steps, self.road_plane)
        n = sum(len(r["points"]) for r in raws)
        if self._scan is None or self._scan.shape[0] < n:              # grow-only pinned rows for the raw scans
            self._scan = torch.empty((max(n + n // 8, 1024), self.features), dtype=torch.float32).pin_memory()
        host, at = self._scan.numpy(), 0
        for r in raws:
            host[at:at + len(r["points"])] = r["points"]
            at += len(r["points"])
        scene = self._scan[:n].to(self.device, non_blocking=True)
        st, self._staging = ops.batch_prep_stage1(plan, scene, db, self.range, remove_extra_width=self.extra,
                                                  want_near=self.num_points is not None, remove_outside_boxes=self.remove_outside,
                                                  min_num_corners=self.min_corners, workspace=self._workspace, table=self._table,
                                                  staging=self._staging)
        self._workspace, self._table = st.workspace, st.table_pinned
        if self.shuffle_first:
            picks, rows, perm = ops.batch_prep_order_draws(st.table, self.num_points, self.shuffle, npr, shuffle_first=True)
        else:
            (picks, rows), perm = ops.batch_prep_order_draws(st.table, self.num_points, self.shuffle, npr), None
        points, self._staging2 = ops.batch_prep_order(st, picks, perm=perm, staging=self._staging2)
        gmax = int(st.table[:, 2].max()) if B else 0
        batch = {k: v for k, v in raw_batch.items() if k not in ("points", "gt_boxes", "gt_classes", "road_plane", "V2C", "R0", "gt_names",
                                                                 RAW_KEY)}
        batch["points"] = points
        batch["gt_boxes"] = st.gt_boxes[:, :gmax].contiguous()
        batch["batch_size"] = B
        batch["empty_samples"] = [int(b) for b in np.nonzero(st.table[:, 2] == 0)[0]]
        batch["batch_prep_table"] = st.table
        if self.voxelize is not None:
            batch = self.voxelize(batch)
        return batch


def raw_prepare_data(dataset, data_dict):
    """``DatasetTemplate.prepare_data`` for the device path: in training mode only the point feature encoder runs, and the
    sample keeps what the device needs; in test mode the method this one replaced is called"""
    if not dataset.training:
        return dataset._modest_prepare_data(data_dict)
    assert "gt_boxes" in data_dict, "gt_boxes should be provided for training"
    gt = np.asarray(data_dict["gt_boxes"], np.float32)
    if gt.ndim == 2 and gt.shape[1] > 7:
        raise NotImplementedError(f"gt_boxes with {gt.shape[1]} columns: boxes with more than 7 columns (the velocity columns) are "
                                  f"not provided")
    names = np.asarray(data_dict["gt_names"]).astype(str)
    d = dataset.point_feature_encoder.forward({"points": data_dict["points"]})
    if not d.get("use_lead_xyz", True):
        raise NotImplementedError("use_lead_xyz false is not provided")
    out = {"points": np.asarray(d["points"], np.float32), "gt_boxes": gt.reshape(-1, 7),
           "gt_classes": np.array([dataset.class_names.index(n) + 1 if n in dataset.class_names else 0 for n in names], np.int64),
           "gt_names": names, "frame_id": data_dict.get("frame_id")}
    if "road_plane" in data_dict:
        out["road_plane"] = np.asarray(data_dict["road_plane"])
    if "calib" in data_dict:
        out["V2C"], out["R0"] = np.asarray(data_dict["calib"].V2C), np.asarray(data_dict["calib"].R0)
    return out


def collate_raw(batch_list, _unused=False):
    """``DatasetTemplate.collate_batch`` for raw samples: lists per key, frame_id as an array, and the mark that makes
    ``load_data_to_gpu`` hand the batch to ``BatchPrepOnDevice``"""
    if not batch_list or "gt_classes" not in batch_list[0]:
        raise ValueError("collate_raw takes the samples of raw_prepare_data in training mode")
    ret = {k: [s[k] for s in batch_list] for k in batch_list[0] if k != "frame_id"}
    ret["frame_id"] = np.array([s.get("frame_id") for s in batch_list])
    ret["batch_size"] = len(batch_list)
    ret[RAW_KEY] = True
    return ret


def bind(dataset_template, models_module):
    """DatasetTemplate.prepare_data := raw_prepare_data, DatasetTemplate.collate_batch := collate_raw (in test mode both call
    what they replaced) and pcdet.models.load_data_to_gpu := a version that runs a raw batch through `BatchPrepOnDevice`
    (built on first use from ``load_data_to_gpu.dataset``, which the training script sets) and hands any other batch to the
    original.  Idempotent."""
    if getattr(dataset_template.prepare_data, "_modest", False):
        return
    dataset_template._modest_prepare_data = dataset_template.prepare_data
    dataset_template._modest_collate_batch = dataset_template.__dict__.get("collate_batch", staticmethod(dataset_template.collate_batch))
    original_load = models_module.load_data_to_gpu

    def prepare_data(self, data_dict):
        return raw_prepare_data(self, data_dict)

    def collate_batch(batch_list, _unused=False):
        if batch_list and "gt_classes" in batch_list[0]:
            return collate_raw(batch_list)
        return dataset_template._modest_collate_batch(batch_list, _unused)

    def load_data_to_gpu(batch_dict):
        if not batch_dict.get(RAW_KEY, False):
            return original_load(batch_dict)
        ds = getattr(load_data_to_gpu, "dataset", None)
        if ds is None:
            raise RuntimeError("a raw batch needs load_data_to_gpu.dataset = the training dataset (its config, class names and root)")
        prep = getattr(ds, "_modest_batch_prep", None)       # kept on the dataset: it lives and dies with it
        if prep is None:
            prep = ds._modest_batch_prep = BatchPrepOnDevice(ds.dataset_cfg, ds.class_names, ds.root_path, training=True)
        out = prep(batch_dict)
        batch_dict.clear()
        batch_dict.update(out)

    prepare_data._modest = True
    load_data_to_gpu._modest_original = original_load
    dataset_template.prepare_data = prepare_data
    dataset_template.collate_batch = staticmethod(collate_batch)
    models_module.load_data_to_gpu = load_data_to_gpu


def unbind(dataset_template, models_module):
    """put back the three attributes `bind` set"""
    if not getattr(dataset_template.prepare_data, "_modest", False):
        return
    dataset_template.prepare_data = dataset_template._modest_prepare_data
    dataset_template.collate_batch = dataset_template.__dict__["_modest_collate_batch"]
    models_module.load_data_to_gpu = models_module.load_data_to_gpu._modest_original
    del dataset_template._modest_prepare_data, dataset_template._modest_collate_batch
