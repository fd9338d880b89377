"""The edge cases of the anchor-head loss: the smallest shapes that cross each constant of
csrc/anchor_loss.hip, as configs of tests/anchor_loss_seq.py (not a test module; tests/test_anchor_loss_cpu.py runs them
through the restatement and exact(), tests/test_gpu_anchor_loss.py through the kernels)."""
from anchor_loss_seq import base_cfg as c
from anchor_loss_seq import edge_scene_cfgs

CASES = {
    # N one row short of, at, one past and four times the workgroup (256), and below one
    "n70": c(B=1, N=70, seed=101, pos=0.2),
    "n255": c(B=1, N=255, seed=102),
    "n256": c(B=1, N=256, seed=103),
    "n257": c(B=1, N=257, seed=104),
    "n1040": c(B=1, N=1040, seed=105),
    # B = 3: a sample without positives (max(cnt, 1)), one all positive, one all -1
    "b3": c(B=3, N=257, samples=["none", "all", "ignore"], seed=106),
    "b3_mixed": c(B=3, N=300, samples=["mixed", "none", "mixed"], seed=107),
    # C = 1 with labels 1 and 3 (class-agnostic), then 3 and 10
    "c1": c(B=2, N=257, num_class=1, label_max=3, seed=108, pos=0.1),
    "c3": c(B=2, N=257, num_class=3, seed=109, pos=0.1),
    "c10": c(B=1, N=257, num_class=10, seed=110, pos=0.1),
    # code = 7, 8 and 9
    "code8": c(B=1, N=257, code=8, seed=111, pos=0.1, code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.5]),
    "code9": c(B=1, N=257, code=9, seed=112, pos=0.1, code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2]),
    # no direction head; bins = 2 and 4; dir_offset 0 and 0.78539
    "nodir": c(B=2, N=257, bins=0, seed=113, pos=0.1),
    "bins4": c(B=1, N=257, bins=4, dir_offset=0.0, seed=114, pos=0.3),
    "bins2_off0": c(B=1, N=257, bins=2, dir_offset=0.0, seed=115, pos=0.3),
    # logits of exactly +0 and -0, +-30 and +-100; |d| == beta and d == 0; a NaN in a target's column 2, and in column 6
    "logits": c(B=2, N=257, seed=116, specials=["logits", "beta", "nan2"]),
    "logits_c1": c(B=1, N=70, num_class=1, seed=117, specials=["logits"]),
    "nan6": c(B=2, N=70, seed=118, specials=["nan6"]),
    # beta = 0 (L1), int64 labels, a label above num_class (no fault, no contribution to the classification target)
    "l1": c(B=1, N=257, beta=0.0, seed=119, pos=0.1),
    "int64": c(B=2, N=257, int64=True, seed=120, pos=0.1),
    "label_above": c(B=1, N=257, seed=121, specials=["label_above"]),
    "label_above_int64": c(B=1, N=257, int64=True, label_max=9, seed=122, pos=0.1),
    # labels no 32-bit cast keeps: 2^32 + 1 (truncated: class 1), 2^31, -2^40 and INT64_MIN (truncated: background 0); int32 -7
    "labels_wide": c(B=1, N=257, int64=True, seed=126, specials=["labels_wide"]),
    "labels_wide_int32": c(B=1, N=257, seed=127, specials=["labels_wide"]),
}
# headings at every bin edge, saturating and infinite direction logits, non-finite and huge values, the head's real layout:
# then al_finish past one row of 256 partials and past its first batch of 8 rows: the configs of the recorded
# tests/golden/anchor_loss_edges.npz
CASES.update(edge_scene_cfgs())
# the cases that may hold a NaN, and the outputs that hold it: no other output of these and no output of another case does
MAY_HOLD_NAN = {"nan6": ("losses", "grad_box"), "dir_logits": ("losses", "grad_dir"),
                "nonfinite": ("losses", "grad_cls", "grad_box"), "nonfinite_inf": ("grad_box",),
                "nonfinite_l1": ("losses", "grad_box")}
