"""CPU: the restatement of the RoI target assignment (tests/roi_targets_seq.py) against the fixture recorded from the
reference's own assign_targets (tests/golden/roi_targets.npz), its faulty variants, the draws, the case registry's own
conditions, the binding and the refusals that need no device."""
import importlib.util
import inspect
import os
import sys
import types

import numpy as np
import pytest
import torch

import roi_targets_cases as cases
import roi_targets_seq as seq

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "roi_targets.npz")


@pytest.fixture(scope="module")
def rec():
    return dict(np.load(GOLD))


def test_fixture_scenes(rec):
    assert seq.scenes(rec) == ["cls", "roi_iou", "any_class"] and os.path.getsize(GOLD) <= 64 * 1024
    cfg = seq.scene_inputs(rec, "cls")[0]
    assert (cfg["REG_FG_THRESH"], cfg["CLS_FG_THRESH"], cfg["CLS_BG_THRESH"], cfg["CLS_BG_THRESH_LO"], cfg["HARD_BG_RATIO"],
            cfg["FG_RATIO"], cfg["ROI_PER_IMAGE"]) == (0.55, 0.6, 0.45, 0.1, 0.8, 0.5, 16)
    gt = seq.scene_inputs(rec, "cls")[5]
    assert len(gt) == 4 and not gt[3].any() and len({seq.trim(g) for g in gt}) == 4      # another trailing count each
    cfg, _, rois, _, labels, gt = seq.scene_inputs(rec, "roi_iou")
    assert cfg["CLS_SCORE_TYPE"] == "roi_iou" and cfg["ROI_PER_IMAGE"] > rois.shape[1] and set(np.unique(gt[..., -1])) >= {1, 2, 3}
    assert (labels == 7).any() and not (gt[..., -1] == 7).any()                            # a roi class without a gt
    assert seq.scene_inputs(rec, "any_class")[0]["SAMPLE_ROI_BY_EACH_CLASS"] is False


@pytest.mark.parametrize("name", ["cls", "roi_iou", "any_class"])
def test_restatement_reproduces_the_fixture_from_the_seeds(rec, name):
    """bit for bit, all eight outputs: the draws consume numpy's and torch's generators exactly as the reference does"""
    cfg, seeds, rois, scores, labels, gt = seq.scene_inputs(rec, name)
    np.random.seed(seeds[0])
    torch.manual_seed(seeds[1])
    details = {}
    ours = seq.assign_targets(rois, scores, labels, gt, cfg, details=details)
    want = seq.recorded(rec, name)
    assert seq.same(ours, want), "\n".join(seq.describe(ours, want))
    assert list(ours) == list(seq.KEYS)
    # the same picks from private generators in the same state, through the library's own draw function
    from modest_amd import ops
    rs, gen = np.random.RandomState(seeds[0]), torch.Generator().manual_seed(seeds[1])
    for b in range(len(rois)):
        assert np.array_equal(ops.roi_target_draws(details["counts"][b], cfg, rs, gen, sample=b), details["picks"][b])
    if name == "cls":
        c = details["counts"]
        assert c[0].all() and c[1, 0] and c[1, 1] and not c[1, 2] and not c[2, 0] and not c[2, 2] and not c[3, :2].any()


def test_forward_is_the_seven_keys(rec):
    cfg, seeds, rois, scores, labels, gt = seq.scene_inputs(rec, "cls")
    np.random.seed(seeds[0])
    torch.manual_seed(seeds[1])
    out = seq.forward(rois, scores, labels, gt, cfg)
    want = seq.recorded(rec, "cls")
    assert list(out) == list(seq.KEYS[:7]) and np.array_equal(out["gt_of_rois"], want["gt_of_rois_src"])


@pytest.mark.parametrize("fault", sorted(seq.FAULTS))
def test_each_fault_changes_its_case(fault):
    name = seq.FAULTS[fault]
    c = cases.case(name)
    want, d0 = cases.expected(name)
    d1 = {}
    got = seq.assign_targets(c["rois"], c["roi_scores"], c["roi_labels"], c["gt_boxes"], c["cfg"], cases.seeded_draws(c),
                             fault=fault, details=d1)
    same_found = all(np.array_equal(a[1], b[1]) and all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))
                     for a, b in zip(d0["found"], d1["found"]))
    assert not (seq.same(got, want) and same_found), fault


def test_equivalent_variants_change_nothing():
    for fault, name in seq.EQUIVALENT.items():
        c = cases.case(name)
        got = seq.assign_targets(c["rois"], c["roi_scores"], c["roi_labels"], c["gt_boxes"], c["cfg"], cases.seeded_draws(c), fault=fault)
        assert seq.same(got, cases.expected(name)[0]), fault


def test_registry_conditions():
    assert cases.T == 64 and cases.WG == 512
    for n in ("rois_1", "rois_63", "rois_64", "rois_65", "rois_511", "rois_512", "rois_513", "rois_1000", "gts_1", "gts_63", "gts_64",
              "gts_65", "gts_129", "gt_trailing_0", "gt_trailing_1", "gt_trailing_40", "batch_1", "batch_3", "batch_300"):
        assert n in cases.NAMES, n
    assert {cases.case(n)["cfg"]["ROI_PER_IMAGE"] for n in ("m_1", "m_128", "m_512")} == {1, 128, 512}
    for name in cases.NAMES:
        c = cases.case(name)
        if c["raises"]:
            with pytest.raises(c["raises"], match="FG=0, BG=0"):
                cases.expected(name)
            continue
        out, d = cases.expected(name)
        by_class = c["cfg"].get("SAMPLE_ROI_BY_EACH_CLASS", False)
        for b in range(len(c["rois"])):
            best, at, lists = d["found"][b]
            if c["finite"] and name != "duplicated_gts":       # no positive maximum attained twice
                n = seq.trim(c["gt_boxes"][b])
                valid = c["gt_boxes"][b][:n]
                iou = seq.iou3d(c["rois"][b][:, :7], valid[:, :7])
                comp = (c["roi_labels"][b][:, None] == valid[None, :, -1].astype(np.int64)) if by_class else np.ones(iou.shape, bool)
                assert not ((((iou == best[:, None]) & comp).sum(1) > 1) & (best > 0)).any(), (name, b)
            if c["branches"]:
                assert tuple(k for k, l in zip(cases.KINDS, lists) if len(l)) == c["branches"][b], (name, b)
    assert min(min(len(l) for l in f[2] if len(l)) for n in ("one_fg", "fg_only", "one_hard", "one_easy")
               for f in cases.expected(n)[1]["found"]) == 1
    d = cases.expected("duplicated_gts")[1]
    assert any((f[0] > 0).any() for f in d["found"])
    d = cases.expected("cls_fg_below_reg_fg")[1]
    assert all(len(np.intersect1d(f[2][0], f[2][1])) for f in d["found"])       # fg and hard overlap
    d = cases.expected("nonfinite")[1]
    assert np.isnan(d["found"][0][0]).any() and d["counts"][0].sum() > 0
    assert seq.trim(cases.case("gt_zero_between")["gt_boxes"][0]) == 6 and seq.trim(cases.case("gts_zero_box")["gt_boxes"][0]) == 1
    for name, key in (("thresh_at_fg", "REG_FG_THRESH"), ("thresh_at_cls_fg", "CLS_FG_THRESH"), ("thresh_at_lo", "CLS_BG_THRESH_LO")):
        c = cases.case(name)
        r, v = c["chosen"]
        assert np.float32(c["cfg"][key]) == np.float32(v) == cases.expected(name)[1]["found"][0][0][r]
    # the label thresholds tell > from >= only in a slot that holds the chosen roi: it is among the picks, and its slot
    # has what the strict comparison gives
    for name, key, field, strict in (("thresh_at_fg", "REG_FG_THRESH", "reg_valid_mask", 0),
                                     ("thresh_at_reg_fg", "REG_FG_THRESH", "reg_valid_mask", 0),
                                     ("thresh_at_cls_fg", "CLS_FG_THRESH", "rcnn_cls_labels", 0),     # >= would give 1
                                     ("thresh_at_cls_bg", "CLS_BG_THRESH", "rcnn_cls_labels", 0)):    # >= would give -1
        c = cases.case(name)
        r, v = c["chosen"]
        out, d = cases.expected(name)
        assert np.float32(c["cfg"][key]) == d["found"][0][0][r]
        picked = np.array([d["found"][0][2][lid][pos] for lid, pos in d["picks"][0]])
        slots = np.flatnonzero(picked == r)
        assert len(slots), (name, "the roi at the threshold is not sampled")
        assert (out["gt_iou_of_rois"][0, slots] == np.float32(v)).all() and (out[field][0, slots] == strict).all(), name


def test_registry_headings_need_no_row_taken_out():
    """The GPU test takes out rows whose double cos / sin the device rounds to another float32 than the host's libm.  Two
    checks that need no device say that the registry has no such row.  (1) torch's CPU double cos / sin, another
    implementation than libm's, rounded once, equal libm's on every roi heading, remainder(ry, 2 pi) and gt heading and
    their negatives.  (2) Every libm value lies farther from the two float32 rounding boundaries next to it than 4 units
    in its last place as a double; libm's error is below 1, so any double cos / sin with an error below 3 such units
    rounds to the same float32.  The chance of a heading that near a boundary is 4 * 2^-29 a value."""
    import math
    vals = []
    for name in cases.NAMES:
        c = cases.case(name)
        ry = c["rois"][..., 6]
        vals += [ry.reshape(-1), seq.rem(ry, seq.TWO_PI).reshape(-1), c["gt_boxes"][..., 6].reshape(-1)]
    h = np.unique(np.concatenate(vals).astype(np.float32))
    h = h[np.isfinite(h)].astype(np.float64)
    assert len(h) > 10000
    differ = close = 0
    for fn, tfn in ((math.cos, torch.cos), (math.sin, torch.sin)):
        for v in (h, -h):
            libm = np.array([fn(x) for x in v])
            differ += int((tfn(torch.from_numpy(v)).float().numpy() != libm.astype(np.float32)).sum())
            f = libm.astype(np.float32)
            mid = [(f.astype(np.float64) + np.nextafter(f, np.float32(s) * np.float32(np.inf)).astype(np.float64)) / 2 for s in (-1, 1)]
            margin = np.minimum(np.abs(libm - mid[0]), np.abs(libm - mid[1]))
            close += int((margin <= 4 * np.spacing(np.abs(libm))).sum())
    print(f"headings of the registry: {len(h)}; torch's CPU trig differs from libm's on {differ}; within 4 ulp of a boundary: {close}")
    assert differ == 0 and close == 0


def test_bind_roi_targets():
    from modest_amd.utils import pcdet_bind
    from modest_amd.utils import roi_targets as rt
    name = "pcdet.models.roi_heads.roi_head_template"
    assert pcdet_bind.ROI_TARGETS_NAME == name
    assert list(inspect.signature(pcdet_bind.install).parameters)[-1] == "proposal_layer"
    assert not inspect.signature(pcdet_bind.bind_roi_targets).parameters
    names = list(pcdet_bind.SHIMS) + list(pcdet_bind.STAND_INS) + ["spconv.utils", name]
    saved = {k: sys.modules.get(k) for k in names}
    try:
        for k in names:
            sys.modules.pop(k, None)
        if importlib.util.find_spec("pcdet") is None:
            assert pcdet_bind.bind_roi_targets() is None and name not in sys.modules
        before = sorted(pcdet_bind.install())
        fake = types.ModuleType(name)
        fake.RoIHeadTemplate = type("RoIHeadTemplate", (), {"assign_targets": lambda self, d: "reference",
                                                            "proposal_layer": lambda self, d, c: "reference"})
        sub = type("PointRCNNHead", (fake.RoIHeadTemplate,), {})
        sys.modules[name] = fake
        assert sub().assign_targets({}) == "reference"
        assert pcdet_bind.bind_roi_targets() is fake and pcdet_bind.bind_roi_targets() is fake       # idempotent
        assert fake.RoIHeadTemplate.assign_targets is rt.assign_targets and sub.assign_targets is rt.assign_targets
        assert sub().proposal_layer({}, None) == "reference"                                           # nothing else is touched
        assert sorted(pcdet_bind.install()) == before                                                  # install's keys stay
        sys.modules[name] = types.ModuleType(name)                                                     # a module without the class
        assert pcdet_bind.bind_roi_targets() is None
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_bind_is_inherited():
    from modest_amd.utils import roi_targets as rt
    base = type("Head", (), {})
    sub = type("Sub", (base,), {})
    assert rt.bind(base) is base and sub.assign_targets is rt.assign_targets
    assert rt.KEYS == seq.KEYS


def test_library_constants():
    from modest_amd import ops
    from modest_amd.utils import roi_targets as rt
    assert ops.roi_targets_gt_tile() == rt.GT_TILE
    # 20 bytes a roi and 12 a sample, each of the six arrays rounded up to 256
    up = lambda v: (v + 255) & ~255      # noqa: E731
    for B, N in ((1, 1), (4, 512), (300, 8), (1, 1000)):
        assert ops.roi_targets_workspace_bytes(B, N) == up(12 * B) + 5 * up(4 * B * N)
        off = np.full(6, -1, np.int64)
        assert ops.load().modest_roi_targets_workspace_offsets(B, N, off.ctypes.data) == 0
        assert off[0] == 0 and (np.diff(off) >= np.array([12 * B] + [4 * B * N] * 4)).all() \
            and off[5] + 4 * B * N <= ops.roi_targets_workspace_bytes(B, N) and not (off % 8).any()
    assert ops.load().modest_roi_targets_workspace_offsets(1, 1, None) != 0


def test_host_tensors_and_limits_raise_before_anything_is_launched():
    from modest_amd import ops
    from modest_amd.utils import roi_targets as rt
    c = cases.case("rois_1")
    t = {k: torch.from_numpy(c[k].copy()) for k in ("rois", "roi_scores", "roi_labels", "gt_boxes")}
    with pytest.raises(ValueError, match="device"):
        ops.roi_targets(t["rois"], t["roi_scores"], t["roi_labels"], t["gt_boxes"], c["cfg"])
    head = rt.bind(type("Head", (), {}))()
    head.model_cfg = {"TARGET_CONFIG": c["cfg"]}
    with pytest.raises(ValueError, match="device"):
        head.assign_targets(dict(batch_size=2, **t))
    with pytest.raises(ValueError, match=str(rt.COLS_MAX)):
        ops.roi_targets_limits(2, rt.COLS_MAX + 1, 16)
    ops.roi_targets_limits(rt.BATCH_MAX, rt.COLS_MAX, 1)
    with pytest.raises(ValueError, match=str(rt.BATCH_MAX)):
        ops.roi_targets_limits(rt.BATCH_MAX + 1, 7, 16)
    with pytest.raises(ValueError, match="ROI_PER_IMAGE"):
        ops.roi_targets_limits(2, 7, 0)
    with pytest.raises(ValueError, match=str(2 ** 31 - 1)):
        ops.roi_targets_limits(65535, 7, 16, n_rois=32769)
    ops.roi_targets_limits(65535, 7, 16, n_rois=32768)
    # the library refuses the same before it launches: it needs no device for that
    lib = ops.load()
    assert lib.modest_roi_targets_workspace_bytes(rt.BATCH_MAX + 1, 8) < 0 and lib.modest_roi_targets_workspace_bytes(65535, 32769) < 0
    for args, word in (((rt.BATCH_MAX + 1, 8, 4, None, 7), b"65535"), ((2, 8, 4, None, 4097), b"4096"), ((65535, 32769, 4, None, 7), b"2^31 - 1")):
        rc = lib.modest_roi_targets_match(*args, None, None, 8, 8, 1, 0.5, 0.1, 0.5, 1, None, 0, None, None)
        assert rc != 0 and b"requirement failed" in lib.modest_last_error() and word in lib.modest_last_error()
    rc = lib.modest_roi_targets_sample(2, 8, 4, 0, None, None, 7, None, None, None, 8, 8, 1, 0.5, 0.6, 0.4, 0.2, 0, None, 0,
                                       None, None, None, None, None, None, None, None, None)
    assert rc != 0 and b"ROI_PER_IMAGE" in lib.modest_last_error()


def test_unknown_score_type_and_config_forms():
    from modest_amd import ops
    from modest_amd.utils import roi_targets as rt
    cfg = dict(cases.POINTRCNN, CLS_SCORE_TYPE="raw_roi_iou")
    with pytest.raises(NotImplementedError):
        seq.assign_targets(np.zeros((1, 1, 7), np.float32), np.zeros((1, 1), np.float32), np.zeros((1, 1), np.int64),
                           np.zeros((1, 1, 8), np.float32), cfg)
    ns = types.SimpleNamespace(**cases.POINTRCNN)
    assert ops._cfg_get(ns, "ROI_PER_IMAGE") == ops._cfg_get(cases.POINTRCNN, "ROI_PER_IMAGE") == 16
    assert ops._cfg_get(types.SimpleNamespace(), "SAMPLE_ROI_BY_EACH_CLASS", False) is False
    layer = types.SimpleNamespace(roi_sampler_cfg=ns)
    assert rt._config(types.SimpleNamespace(proposal_target_layer=layer)) is ns and rt._config(layer) is ns
    assert rt._config(types.SimpleNamespace(model_cfg=types.SimpleNamespace(TARGET_CONFIG=ns))) is ns
    with pytest.raises(NotImplementedError, match="sample 3: FG=0, BG=0"):
        ops.roi_target_draws((0, 0, 0), cases.POINTRCNN, sample=3)
