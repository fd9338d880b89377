"""CPU: the two numpy restatements of the RoI proposal layer (tests/proposals_seq.py: the oracle's greedy walk, and the
kernel's walk in chunks of 64 against a kept list) agree on every case of tests/proposals_cases.py and reproduce, bit for
bit, what tools/make_golden_proposals.py recorded from the reference's own RoIHeadTemplate.proposal_layer
(tests/golden/proposals.npz).  Every case holds the edge it is named after, every fault the chunked walk can be asked for
shows on a named case, the branches that are not provided raise, the binding is opt-in and leaves the default install()
as it was, the header and its ctypes mirror agree on the new entry, and the walk kernel uses no scratch."""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import pytest

import proposals_cases as cases
import proposals_seq as seq

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "proposals.npz")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def chunked(c, fault=None):
    return seq.proposals_chunked(c["box"], c["cls"], c["B"], c["pre"], c["post"], c["thresh"], c["rotated"], c["batch_index"],
                                 fault=fault)


# ------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("name", list(cases.CASES))
def test_every_case_holds_its_edge_and_both_restatements_agree(name):
    c = cases.case(name)
    st = cases.stats_of(c)
    assert c["present"](c, st), st
    n = c["box"].size // c["box"].shape[-1]
    assert n <= 5614 and c["B"] <= 3 and c["post"] <= 512
    want = cases.want(c)
    assert want[0].shape == (c["B"], c["post"], c["box"].shape[-1]) and want[2].dtype == np.int64 and want[1].dtype == F
    got = chunked(c)
    assert seq.same(got, want), "\n".join(seq.describe(got, want))
    for s, one in enumerate(st):                     # the padding: zeros, zeros and ones
        k = one["kept"]
        assert not want[0][s, k:].any() and not want[1][s, k:].any() and (want[2][s, k:] == 1).all()
        assert (want[2][s, :k] >= 1).all() and (want[2][s, :k] <= c["cls"].shape[-1]).all()


def both(c):
    """stats, and both restatements agreeing on the case; the padding is zeros, zeros and ones (all samples at once)"""
    rows_of = []
    st = cases.stats_of(c, rows_of)
    want = cases.want(c)
    assert want[0].shape == (c["B"], c["post"], c["box"].shape[-1]) and want[2].dtype == np.int64 and want[1].dtype == F
    box, cls, _ = seq._flat(c["box"], c["cls"], c["batch_index"])
    got = seq._assemble(box, cls, c["B"], c["post"], rows_of)            # proposals_chunked, its walk made once
    assert seq.same(got, want), "\n".join(seq.describe(got, want))
    pad = np.arange(c["post"])[None, :] >= np.array([one["kept"] for one in st])[:, None]
    assert not want[0][pad].any() and not want[1][pad].any() and (want[2][pad] == 1).all()
    assert (want[2] >= 1).all() and (want[2] <= c["cls"].shape[-1]).all()
    return st


@pytest.mark.parametrize("name", list(cases.EDGE_CASES))
def test_every_edge_case_holds_its_edge_and_both_restatements_agree(name):
    """the three B = 65535 cases take 5 to 6.5 s each on the build machine (one oracle walk and one chunked walk per
    sample, the padding of all samples at once); candidates() splits their 131 076 rows in 0.1 s, by one mask per sample
    it took 6.7 s each time it was called"""
    c = cases.case(name)
    st = both(c)
    assert c["present"](c, st), st[:3]
    if name in cases.EDGE_DISTINCT:
        assert cases.is_distinct(c)


def test_iou_normal_drops_a_nan_as_fmaxf_does(monkeypatch):
    """the axis-aligned pair test of the chunked walk on non-finite boxes: with np.maximum / np.minimum, which hand a NaN
    on, it keeps other boxes than the C walk of oracle/iou3d_oracle.c (fmaxf / fminf); with np.fmax / np.fmin the same"""
    c = cases.case("non-finite boxes axis-aligned")
    assert seq.same(chunked(c), cases.want(c))
    a = np.array([[0, 0, 0, 2, 2, 1, 0]], F)
    b = np.array([[np.nan, 0, 0, 2, 2, 1, 0], [0, 0, 0, np.nan, 2, 1, 0], [0, 0, 0, np.inf, 2, 1, 0], [0.5, 0, 0, 2, 2, 1, 0]], F)
    # x NaN: fmaxf / fminf leave a's edges, 4 / (4 + 4 - 4); dx NaN: the union is NaN, fmaxf gives 1e-8; dx inf: 4 / inf
    v = seq.iou_normal(a, b)[0]
    assert v[0] == 1 and v[1] > 1e8 and v[2] == 0 and v[3] == F(0.6) and np.isnan(seq.iou_normal(a, b, nan_propagates=True)[0, :2]).all()
    import functools
    monkeypatch.setattr(seq, "iou_normal", functools.partial(seq.iou_normal, nan_propagates=True))
    assert not seq.same(chunked(c), cases.want(c))
    for name in cases.CASES:                       # finite boxes: either form gives the same
        c = cases.case(name)
        if not c["rotated"] and c["B"] == 1:
            assert seq.same(chunked(c), cases.want(c)), name


def test_the_cases_cover_the_list():
    kept = {n: [s["kept"] for s in cases.stats_of(cases.case(n))] for n in ("fewer than POST", "POST inside a chunk", "PRE cuts a tie")}
    assert kept["fewer than POST"] == [44] and kept["POST inside a chunk"] == [100]
    cand = {cases.stats_of(cases.case(n))[0]["candidates"] for n in ("1 row", "63 rows", "64 rows", "65 rows", "129 rows", "1000 rows")}
    assert cand == {1, 63, 64, 65, 129, 1000}
    assert {cases.case(n)["post"] for n in cases.CASES} >= {1, 64, 65, 100, 512}
    assert {cases.case(n)["thresh"] for n in cases.CASES} >= {0.01, 0.7, 0.85}
    assert {cases.case(n)["B"] for n in cases.CASES} == {1, 3}
    assert {cases.case(n)["box"].shape[-1] for n in cases.CASES} == {7, 9} and {cases.case(n)["cls"].shape[-1] for n in cases.CASES} == {1, 3}
    assert {cases.case(n)["rotated"] for n in cases.CASES} == {True, False}
    assert any(cases.case(n)["batch_index"] is None for n in cases.CASES)
    # the stop inside a chunk: survivors were left behind the last one, which is neither first nor last of its chunk
    st = cases.stats_of(cases.case("POST inside a chunk"))[0]
    assert st["left_behind"] and 0 < st["last_in_chunk"] < seq.CHUNK - 1
    # the cut inside a group of equal scores takes the rows of lower index
    c = cases.case("PRE cuts a tie")
    score = c["cls"][:, 0]
    rows = seq.candidates(score, np.zeros(len(score), np.int64), 1, c["pre"])[0]
    tied = np.flatnonzero(score == score[rows[-1]])
    inside = np.intersect1d(tied, rows)
    assert 0 < len(inside) < len(tied) and np.array_equal(inside, tied[:len(inside)])
    # the stacked rows of the dense case give the dense result
    assert seq.same(cases.want(cases.case("dense")), cases.want(cases.case("dense rows stacked")))
    # the strays change nothing
    assert seq.same(cases.want(cases.case("3 samples")), cases.want(cases.case("3 samples and strays")))
    # past every capacity of the kernel
    st = cases.stats_of(cases.case("past every capacity"))
    assert st[0]["kept"] == st[1]["kept"] == 512 > seq.CHUNK * seq.WAVES and st[0]["chunks"] > seq.WAVES and st[2]["candidates"] == 0
    assert (seq.CHUNK, seq.WAVES, seq.POST_MAX, seq.BATCH_MAX) == (64, 4, 1024, 65535)
    text = open(os.path.join(ROOT, "modest_amd", "csrc", "prop_walk.h")).read()     # the one place that holds the walk's figures
    for line in ("constexpr int WK_WAVES = 4;", "constexpr int WK_CHUNK = 64;", "constexpr int WK_POST_MAX = 1024;",
                 "constexpr int WK_MAX_BATCH = 65535;"):
        assert line in text, line
    # the edges: every limit run, the rows all padding, thresholds on both sides of every IoU
    edge = [cases.case(n) for n in cases.EDGE_CASES]
    assert seq.BATCH_MAX in {c["B"] for c in edge} and seq.POST_MAX in {c["post"] for c in edge}
    assert 4096 in {c["box"].shape[-1] for c in edge} and 4096 in {c["cls"].shape[-1] for c in edge}
    assert {0, 1, seq.CHUNK, seq.CHUNK + 1} <= {c["pre"] for c in edge}
    assert any(c["thresh"] < 0 for c in edge) and any(np.isnan(c["thresh"]) for c in edge) and any(np.isposinf(c["thresh"]) for c in edge)
    assert {0.0, 1.0} <= {c["thresh"] for c in edge}
    assert any(c["batch_index"] is None and c["B"] == seq.BATCH_MAX for c in edge)
    assert {c["batch_index"].dtype for c in edge if c["B"] == seq.BATCH_MAX and c["batch_index"] is not None} == {np.dtype(F), np.dtype(np.int64)}
    assert any((c["cls"] < 0).sum() > 100 for c in edge) and any(not np.isfinite(c["box"][..., :7]).all() for c in edge)
    assert seq.same(cases.want(cases.case("B 65535 stacked")), cases.want(cases.case("B 65535 stacked int64")))
    assert seq.same(cases.want(cases.case("B 65535 stacked")), cases.want(cases.case("B 65535 dense")))     # the strays change nothing


# fault -> cases on which the chunked walk, so broken, gives other outputs
SEEN_BY = {
    "first wavefront's share only": ["1000 rows", "POST 512", "past every capacity", "dense", "thresh 0.7 axis-aligned",
                                     "POST 1024 full", "logits", "thresh 0", "non-finite boxes"],
    "chunk not tested against itself": ["63 rows", "64 rows", "exact duplicates", "equal scores", "PRE 64", "PRE 65", "thresh -1",
                                        "thresh 1", "4096 class columns"],
    "suppressed candidates still suppress": ["thresh 0.7", "3 samples", "non-finite boxes axis-aligned"],
    "kept list restarts per chunk": ["129 rows", "1000 rows", "fewer than POST", "3 samples axis-aligned", "logits",
                                     "POST 1024 full", "non-finite boxes axis-aligned", "thresh -1 axis-aligned"],
}
# wrong key -> the case on which the restatement, sorting by it, gives other outputs
KEY_SEEN_BY = {"negatives not inverted": "logits", "-0 below +0": "zeros and denormals", "denormals are zero": "zeros and denormals",
               "NaN last": "NaN scores"}


@pytest.mark.parametrize("fault", list(seq.FAULTS))
def test_every_fault_shows_on_its_cases(fault):
    assert set(SEEN_BY) == set(seq.FAULTS)
    for name in SEEN_BY[fault]:
        c = cases.case(name)
        assert not seq.same(chunked(c, fault), cases.want(c)), (fault, name)


@pytest.mark.parametrize("fault", list(seq.KEY_FAULTS))
def test_every_wrong_key_shows_on_its_case(fault):
    assert set(KEY_SEEN_BY) == set(seq.KEY_FAULTS) and not set(seq.KEY_FAULTS) & set(seq.FAULTS)
    c = cases.case(KEY_SEEN_BY[fault])
    args = (c["box"], c["cls"], c["B"], c["pre"], c["post"], c["thresh"], c["rotated"], c["batch_index"])
    assert seq.same(seq.proposals(*args, key_fault=None), cases.want(c))
    assert not seq.same(seq.proposals(*args, key_fault=fault), cases.want(c)), fault
    with pytest.raises(AssertionError):
        seq.descending_bits(np.zeros(1, F), fault="no such key")


def test_tie_rules():
    cls = np.array([[1, 1, 0], [0, 2, 2], [np.nan, 5, np.nan], [3, np.nan, 9], [-0.0, 0.0, -1]], F)
    score, label = seq.score_label(cls)
    assert label.tolist() == [0, 1, 0, 1, 0] and np.isnan(score[2:4]).all() and score[0] == 1 and score[1] == 2
    s = np.array([0.5, np.nan, np.inf, -np.inf, 0.0, -0.0, 0.5, -1.0, np.nan], F)
    order = np.argsort(seq.descending_bits(s), kind="stable")
    assert order.tolist() == [1, 8, 2, 0, 6, 4, 5, 7, 3]
    smp = seq.sample_of(np.array([0, 1, 2, 3, -1, 0.5, np.nan, np.inf, 1], F), 9, 3)
    assert smp.tolist() == [0, 1, 2, 3, 3, 3, 3, 3, 1]


# ------------------------------------------------------------------------------------------------ the recorded fixture
def test_fixture_is_small_and_holds_its_scenes(gold):
    assert os.path.getsize(GOLD) <= 64 * 1024
    assert seq.scenes(gold) == ["stacked", "dense", "post"]
    cfg, box, cls, bidx = seq.scene_inputs(gold, "stacked")
    assert cfg["batch_size"] == 3 and 250 <= len(box) <= 350 and bidx.dtype == F and int((np.diff(bidx) != 0).sum()) > 100
    cfg, box, cls, bidx = seq.scene_inputs(gold, "dense")
    assert bidx is None and box.shape[0] == cfg["batch_size"] == 2 and box.shape[2] == 9 and cls.shape[2] == 3
    assert cfg["NMS_PRE_MAXSIZE"] < box.shape[1]
    cfg, box, cls, bidx = seq.scene_inputs(gold, "post")
    scores = seq.recorded(gold, "post")[1]
    assert (scores[0] != 0).all() and (scores[1] == 0).any() and (scores[1] != 0).any()
    for name in seq.scenes(gold):        # no order the reference leaves open was recorded
        cfg, box, cls, bidx = seq.scene_inputs(gold, name)
        assert cases.is_distinct(dict(box=box, cls=cls, batch_index=bidx, B=cfg["batch_size"])), name
        assert all(gold[k].dtype.kind in "fiU" for k in gold)          # data only


def test_restatements_reproduce_the_reference(gold):
    for name in seq.scenes(gold):
        cfg, box, cls, bidx = seq.scene_inputs(gold, name)
        ref = seq.recorded(gold, name)
        assert ref[0].dtype == F and ref[1].dtype == F and ref[2].dtype == np.int64
        for fn in (seq.proposals, seq.proposals_chunked):
            ours = fn(box, cls, cfg["batch_size"], cfg["NMS_PRE_MAXSIZE"], cfg["NMS_POST_MAXSIZE"], cfg["NMS_THRESH"],
                      cfg["NMS_TYPE"] == "nms_gpu", bidx)
            assert seq.same(ours, ref), name + "\n" + "\n".join(seq.describe(ours, ref))
        bad = tuple(a.copy() for a in ref)                                # the comparison is not vacuous
        bad[0][0, 0, 0] = np.nextafter(bad[0][0, 0, 0], F(1e9))
        assert not seq.same(bad, ref) and seq.describe(bad, ref)


# ------------------------------------------------------------------------------------------------ the Python side
def stand_in_head():
    from modest_amd.utils import proposal_layer as pl
    return pl.bind(type("RoIHead", (), {}))()


def config(**kw):
    cfg = dict(MULTI_CLASSES_NMS=False, NMS_TYPE="nms_gpu", NMS_PRE_MAXSIZE=9000, NMS_POST_MAXSIZE=100, NMS_THRESH=0.8)
    cfg.update(kw)
    return types.SimpleNamespace(**cfg)


def test_branches_that_are_not_provided_raise(monkeypatch):
    import torch
    from modest_amd import _lib, ops
    from modest_amd.utils import proposal_layer as pl

    def no_load(*a, **k):
        raise AssertionError("the library was opened")
    monkeypatch.setattr(_lib, "load", no_load)
    monkeypatch.setattr(ops, "load", no_load)
    head = stand_in_head()
    d = dict(batch_size=2, batch_box_preds=torch.zeros((2, 5, 7)), batch_cls_preds=torch.zeros((2, 5, 1)))
    with pytest.raises(NotImplementedError):
        head.proposal_layer(dict(d), config(MULTI_CLASSES_NMS=True))
    with pytest.raises(ValueError, match="NMS_TYPE"):
        head.proposal_layer(dict(d), config(NMS_TYPE="nms_cpu"))
    with pytest.raises(ValueError, match=str(pl.POST_MAX)):
        head.proposal_layer(dict(d), config(NMS_POST_MAXSIZE=pl.POST_MAX + 1))
    with pytest.raises(ValueError, match=str(pl.BATCH_MAX)):
        head.proposal_layer(dict(d, batch_size=pl.BATCH_MAX + 1), config())
    with pytest.raises(ValueError, match="device"):                       # CPU tensors: refused before the library is opened
        head.proposal_layer(dict(d), config())
    with pytest.raises(ValueError, match="device"):
        ops.proposals(torch.zeros((5, 7)), torch.zeros((5, 1)), 1, 9000, 100, 0.8, batch_index=torch.zeros(5))
    with pytest.raises(AssertionError):                                   # the reference's: the stacked form is 2-D
        head.proposal_layer(dict(d, batch_index=torch.zeros(10)), config())
    assert (pl.POST_MAX, pl.BATCH_MAX) == (seq.POST_MAX, seq.BATCH_MAX)
    assert head.proposal_layer.__func__ is pl.proposal_layer


def test_binding_is_opt_in():
    from modest_amd.utils import pcdet_bind
    from modest_amd.utils import proposal_layer as pl
    import inspect
    name = "pcdet.models.roi_heads.roi_head_template"
    names = list(pcdet_bind.SHIMS) + list(pcdet_bind.STAND_INS) + ["spconv.utils", name]
    saved = {k: sys.modules.get(k) for k in names}
    params = list(inspect.signature(pcdet_bind.install).parameters.values())
    assert params[-1].name == "proposal_layer" and params[-1].default is False
    try:
        for k in names:
            sys.modules.pop(k, None)
        assert name == pcdet_bind.PROPOSAL_LAYER_NAME and name not in pcdet_bind.SHIMS and name not in pcdet_bind.STAND_INS
        keys = sorted(list(pcdet_bind.SHIMS) + list(pcdet_bind.STAND_INS))
        if importlib.util.find_spec("pcdet") is None:
            # nothing to bind onto: the name is left out, nothing is registered under it
            assert sorted(pcdet_bind.install(proposal_layer=True)) == keys and name not in sys.modules

        def reference_method(self, batch_dict, nms_config):
            return "reference"
        fake = types.ModuleType(name)
        fake.RoIHeadTemplate = type("RoIHeadTemplate", (), {"proposal_layer": reference_method})
        sub = type("PointRCNNHead", (fake.RoIHeadTemplate,), {})
        sys.modules[name] = fake
        for kw in ({}, {"sparse_conv": True}, {"point_targets": True}, {"proposal_layer": False}):   # the default call does what it did
            bound = pcdet_bind.install(**kw)
            assert sorted(bound) == keys, kw
            assert fake.RoIHeadTemplate.proposal_layer is reference_method and sys.modules[name] is fake
        bound = pcdet_bind.install(proposal_layer=True)
        assert sorted(bound) == sorted(keys + [name]) and bound[name] is fake and sys.modules[name] is fake
        assert fake.RoIHeadTemplate.proposal_layer is pl.proposal_layer
        assert sub.proposal_layer is pl.proposal_layer                        # the heads inherit it
        again = pcdet_bind.install(proposal_layer=True)                       # idempotent
        assert sorted(again) == sorted(bound) and all(again[k] is bound[k] for k in bound)
        assert sorted(pcdet_bind.install()) == keys and fake.RoIHeadTemplate.proposal_layer is pl.proposal_layer
        assert sorted(pcdet_bind.install(stand_ins=False, proposal_layer=True)) == sorted(list(pcdet_bind.SHIMS) + [name])
        sys.modules[name] = types.ModuleType(name)                            # a module of that name without the class
        assert name not in pcdet_bind.install(proposal_layer=True)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    assert all(sys.modules.get(k) is v for k, v in saved.items())


# ------------------------------------------------------------------------------------------------ the build
def test_header_ctypes_mirror_and_no_scratch():
    import ctypes as C
    import re
    from modest_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "modest_hip.h")).read(), flags=re.S)
    ctype = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float}
    for fn, count in (("modest_proposals", 19), ("modest_proposals_workspace_bytes", 1)):
        m = re.search(r"\b(int64_t|int)\s+%s\s*\(([^)]*)\)" % fn, src)
        assert m, fn
        args = [a.strip() for a in m.group(2).split(",")]
        want = [_lib.VP if "*" in a else ctype[a.split()[0]] for a in args]
        res, have = _lib.SIGNATURES[fn]
        assert res is ctype[m.group(1)] and have == want and len(want) == count, fn
        assert hasattr(lib, fn)
    # refused arguments launch nothing and need no device; each limit names itself
    call = lambda n=0, b=1, pre=9000, post=100: lib.modest_proposals(n, b, 0, None, 7, None, 1, None, 1, pre, post, 0.8, 1, None, None,  # noqa: E731
                                                                     None, None, 0, None)
    assert call(post=seq.POST_MAX + 1) != 0 and b"1024" in lib.modest_last_error()
    assert call(b=seq.BATCH_MAX + 1) != 0 and b"65535" in lib.modest_last_error()
    assert call(n=-1) != 0 and call(pre=-1) != 0
    assert call(n=5) != 0                       # rows without buffers
    assert call(b=0) == 0 and call(post=0) == 0  # empty outputs: nothing to do
    assert lib.modest_proposals_workspace_bytes(0) > 0 and lib.modest_proposals_workspace_bytes(-1) < 0
    n = 845000                                  # two key and two index buffers and the sort's table: no (n, n / 64) mask
    assert 24 * n <= lib.modest_proposals_workspace_bytes(n) <= 26 * n
    res = json.load(open(os.path.join(os.path.dirname(build.LIB), "kernel_resources.json")))
    mine = {k: v for k, v in res.items() if v.get("file") == "proposals.hip"}
    assert len(mine) == 3 and sum("prop_walk" in k for k in mine) == 2 and sum("rank_keysILb0E" in k for k in mine) == 1
    # no scratch memory: no vector register is spilled (a scalar one may move to a vector lane, which costs no memory)
    assert all(v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 for v in mine.values()), mine
    assert max(v["LDS Size [bytes/block]"] for v in mine.values()) <= 160 * 1024
    text = open(os.path.join(ROOT, "modest_amd", "csrc", "proposals.hip")).read()
    assert "hipMalloc" not in text and "hipMemcpy" not in text and "Synchronize" not in text and "atomic" not in text
    # the IoU device functions are one text, shared with nms_tiles
    assert '#include "iou_bev.h"' in text and '#include "iou_bev.h"' in open(os.path.join(ROOT, "modest_amd", "csrc", "iou3d.hip")).read()
