"""The edge cases of the RoI-head loss: the smallest shapes that cross each constant and each branch
of csrc/roi_loss.hip, as configs of tests/roi_loss_seq.py (not a test module; tests/test_roi_loss_cpu.py runs them through the
restatement and exact(), tests/test_gpu_roi_loss.py through the kernels)."""
from roi_loss_seq import EDGE, base_cfg as c
from roi_loss_seq import edge_scene_cfgs

CASES = {
    # R = 1, around a wavefront (64), around the workgroup (256) and four workgroups and a bit
    "r1": c(B=1, M=1, samples=["allfg"], seed=201),
    "r1_nofg": c(B=1, M=1, samples=["nofg"], seed=202),
    "r63": c(B=1, M=63, seed=203),
    "r64": c(B=1, M=64, seed=204),
    "r65": c(B=1, M=65, seed=205),
    "r255": c(B=1, M=255, seed=206),
    "r256": c(B=1, M=256, seed=207),
    "r257": c(B=1, M=257, seed=208),
    "r1040": c(B=1, M=1040, seed=209),
    # 2049 workgroups: rl_finish keeps 8 rows of 256 partials in flight, so lane 0 alone makes a second trip, whose other 7
    # rows are past the end; code 7, the corner term off
    "finish2049": c(B=1, M=2048 * 256 + 1, corner=False, seed=228),
    # B = 3: a sample without foreground, one all foreground, one all ignored; and nothing valid anywhere (max(., 1) twice)
    "b3": c(B=3, M=100, samples=["nofg", "allfg", "ignore"], seed=210),
    "all_ignored": c(B=2, M=70, samples=["ignore", "ignore"], seed=211),
    # code = 8, 9 and 16: the extra columns take part in the smooth L1 and get nothing from the corner term
    "code8": c(B=1, M=130, code=8, seed=212, code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.5]),
    "code9": c(B=1, M=130, code=9, seed=213, code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2]),
    "code16": c(B=1, M=130, code=16, seed=214, code_weights=[1.0] * 7 + [0.1 * k for k in range(1, 10)]),
    # the corner term off; unequal weights; beta = 0 (L1)
    "nocorner": c(B=2, M=130, corner=False, seed=215),
    "weights": c(B=2, M=130, cls_weight=1.5, reg_weight=0.75, corner_weight=2.0, seed=216),
    "l1": c(B=1, M=130, beta=0.0, seed=217),
    # int32, int64 and float labels; int32 and int64 masks
    "labels_int32": c(B=2, M=130, label_dtype="int32", mask_dtype="int32", seed=218),
    "labels_int64": c(B=2, M=130, label_dtype="int64", mask_dtype="int64", seed=219),
    "labels_float": c(B=2, M=130, labels="iou", mask_dtype="int32", seed=220),
    "labels_hard_float": c(B=2, M=130, labels="cls", label_dtype="float32", seed=221),
    # the specials of the edge scene, with the logit of -100 against labels above 0; a min tie; mask values 2 and -1
    "edge": c(B=1, M=257, labels="iou", seed=222, specials=list(EDGE)),
    "edge_hard": c(B=2, M=130, labels="cls", seed=223, specials=list(EDGE)),
    "tie": c(B=1, M=130, seed=224, specials=["tie"]),
    "tie_zero": c(B=1, M=130, labels="iou", seed=225, specials=["tie", "zero_distance", "mask_values"]),
    # gt_of_rois / gt_of_rois_src with a class column behind the code: read through the row stride
    "strided": c(B=2, M=130, gt_cols=8, seed=226),
    "strided_code9": c(B=1, M=130, code=9, gt_cols=12, seed=227, code_weights=[1.0] * 7 + [0.5, 0.25]),
}
# non-finite and huge values on foreground rows, with and without the corner term: the configs of the recorded
# tests/golden/roi_loss_edges.npz
CASES.update(edge_scene_cfgs())
# ... and what is not recorded: -88.9 against a label of 1 (a float32 sigmoid evaluated as 1 / (1 + exp(-x)) is exactly 0 there,
# the contract's is not) and a NaN logit (the reference's binary_cross_entropy raises)
CASES["extreme_sigmoid"] = c(B=1, M=130, seed=57, corner=False, specials=["extreme"])
CASES["nan_cls"] = c(B=1, M=130, seed=58, specials=["nan_cls"])
# the cases that may hold a NaN, and the outputs that hold it: no other output of these and no output of another case does
MAY_HOLD_NAN = {"nonfinite": ("table", "grad_reg"), "nonfinite_inf": ("grad_reg",), "nonfinite_l1": ("table",),
                "nonfinite_corner": ("table", "grad_reg"), "extreme": ("grad_reg",), "extreme_corner": ("grad_reg",),
                "extreme_sigmoid": ("grad_reg",), "nan_cls": ("table", "grad_cls")}
