"""The edge cases of the point-head loss: the smallest shapes that cross each constant and each branch
of csrc/point_loss.hip, as configs of tests/point_loss_seq.py (not a test module; tests/test_point_loss_cpu.py runs them through
the restatement and exact(), tests/test_gpu_point_loss.py through the kernels)."""
from point_loss_seq import EDGE, base_cfg as c
from point_loss_seq import edge_scene_cfgs

PART, BOX, SIMPLE = "PointIntraPartOffsetHead", "PointHeadBox", "PointHeadSimple"

CASES = {
    # N = 1, around a wavefront (64), around the workgroup (256), and 257 workgroups: pl_finish reads a second partial per lane
    "n1": c(head=PART, B=1, N=1, samples=["all"], seed=301),
    "n1_nopos": c(head=PART, B=1, N=1, samples=["none"], seed=302),
    "n63": c(head=PART, B=1, N=63, num_class=3, seed=303),
    "n64": c(head=BOX, B=1, N=64, seed=304),
    "n65": c(head=PART, B=1, N=65, seed=305),
    "n255": c(head=BOX, B=1, N=255, num_class=3, seed=306),
    "n256": c(head=PART, B=1, N=256, seed=307),
    "n257": c(head=PART, B=1, N=257, num_class=3, seed=308),
    "n65537": c(head=PART, B=1, N=65537, pos=0.03, seed=309),
    # 2049 workgroups: pl_finish keeps 8 rows of 256 partials in flight, so lane 0 alone makes a second trip, whose other 7
    # rows are past the end; the cls term only, one class
    "finish2049": c(head=SIMPLE, B=1, N=2048 * 256 + 1, pos=0.03, seed=329),
    # each combination of terms
    "cls": c(head=SIMPLE, B=2, N=130, num_class=3, seed=310),
    "cls_box": c(head=BOX, B=2, N=130, num_class=3, seed=311),
    "cls_part": c(head=PART, box_layers=False, B=2, N=130, num_class=3, seed=312),
    "cls_part_box": c(head=PART, B=2, N=130, num_class=3, seed=313),
    # C = 32 (C = 1 and 3 above); code 7 and 16 (8 above)
    "c32": c(head=BOX, B=1, N=130, num_class=32, pos=0.4, seed=314),
    "code7": c(head=BOX, B=1, N=130, code=7, seed=315),
    "code16": c(head=PART, B=1, N=130, code=16, seed=316, code_weights=[0.1 * k for k in range(1, 17)]),
    # no positive anywhere (max(P, 1) three times), all positive, all ignored, positives in one sample only of a stacked batch
    "nopos": c(head=PART, B=2, N=130, samples=["none", "none"], seed=317),
    "allpos": c(head=PART, B=2, N=70, num_class=3, samples=["all", "all"], seed=318),
    "all_ignored": c(head=PART, B=2, N=70, samples=["ignore", "ignore"], seed=319),
    "one_sample": c(head=PART, B=3, N=100, num_class=3, samples=["none", "all", "ignore"], seed=320),
    "b2_uneven": c(head=BOX, B=2, N=130, num_class=3, samples=["mixed", "none"], pos=0.3, seed=321),
    # int32 labels (int64 above); beta = 0 (plain |d|); unequal code weights and loss weights
    "labels_int32": c(head=PART, B=2, N=130, num_class=3, int64=False, seed=322),
    "l1": c(head=BOX, B=1, N=130, beta=0.0, seed=323),
    "weights": c(head=PART, B=2, N=130, num_class=3, cls_weight=1.5, part_weight=0.75, box_weight=2.0, seed=324,
                 code_weights=[1.0, 1.0, 1.0, 0.5, 0.5, 0.5, 2.0, 0.2]),
    # the specials of the edge scene with +-100 against part labels above 0; part labels at 1 + 2^-23 and -2^-24; a label above
    # num_class; NaN and infinite part and box values in rows that are not positive
    "edge": c(head=PART, B=1, N=257, num_class=3, seed=325, specials=list(EDGE)),
    "edge_box": c(head=BOX, B=2, N=130, seed=326, specials=list(EDGE)),
    "outside": c(head=PART, B=2, N=130, num_class=3, seed=327, specials=["part_outside", "label_above", "nonfinite_off"]),
    "outside_c1": c(head=BOX, B=1, N=130, num_class=1, seed=328, specials=["label_above", "nonfinite_off"]),
}
# non-finite and huge values on positive rows: the configs of the recorded tests/golden/point_loss_edges.npz
CASES.update(edge_scene_cfgs())
# ... and what is not recorded: -88.9 against a part label above 0 (a float32 sigmoid evaluated as 1 / (1 + exp(-x)) is exactly 0
# there, the contract's is not) and a NaN part logit (the reference's binary_cross_entropy raises)
CASES["extreme_sigmoid"] = c(head=PART, B=1, N=130, num_class=3, seed=66, specials=["extreme"])
CASES["nan_part"] = c(head=PART, B=1, N=130, num_class=3, seed=67, specials=["nan_part"])
# the cases that may hold a NaN, and the outputs that hold it: no other output of these and no output of another case does
MAY_HOLD_NAN = {"nonfinite": ("table", "grad_cls", "grad_box"), "nonfinite_inf": ("grad_box",), "nonfinite_l1": ("table",),
                "extreme": ("grad_box",), "extreme_box": ("grad_box",), "extreme_sigmoid": ("grad_box",),
                "nan_part": ("table", "grad_part")}
