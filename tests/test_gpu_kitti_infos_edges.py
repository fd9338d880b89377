"""GPU: the dataset-infos kernels (csrc/kitti_infos.hip: infos_count, infos_scan, infos_gather)
against the numpy restatement tests/infos_seq.py on the named cases of tests/infos_cases.py, through ops.infos_count /
st.read() / ops.infos_gather: the FOV flag of every row, the dense database mask BIT FOR BIT (every element, the padding
columns included), db_count, the gathered rows bit for bit (order and the bits of column 3), hull_count, und_n and the
undecided rows as a set (past the capacity: und_n exact, the stored entries distinct members of the set), the reference's
count end to end, and the same bits on a second call.  Then the library driven directly: every box's words are written
into 0x5A-filled buffers, and every refusal by its text, nothing launched."""
import numpy as np
import pytest
import torch

import infos_seq as seq
from infos_cases import CASES, restated
from modest_amd import kitti_infos as ki
from modest_amd import ops

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5A5A5A


def run(case, gpu, want_fov=True):
    """-> dict of numpy outputs of one count + read + gather"""
    fr = case["frames"]
    R, stride = len(case["rows"]), int(fr["n"].max())
    rows = torch.from_numpy(case["rows"]).to(gpu)
    before = rows.clone()
    st = ops.infos_count(rows, R, fr, case["boxes"], pass_boxes=case["pass_boxes"], und_cap=case["und_cap"], want_fov=want_fov,
                         dense_stride=stride)
    assert st.wcount_words == case["wcount_words"]
    hull, und_n, und_idx, db_count = (np.array(a) for a in st.read())
    out = ops.infos_gather(st)
    assert torch.equal(rows.view(torch.int32), before.view(torch.int32))                 # the rows are left untouched
    return dict(hull=hull, und_n=und_n, und_idx=und_idx, db_count=db_count, gathered=out,
                fov=st.fov.cpu().numpy()[:R] if want_fov else None, dense=st.dense.cpu().numpy() if stride else None)


def compare(case, want, got):
    fr, cap = case["frames"], case["und_cap"]
    if got["fov"] is not None:
        assert got["fov"].dtype == np.uint8 and np.array_equal(got["fov"], want["fov"].astype(np.uint8)), np.nonzero(got["fov"] != want["fov"])[0][:8]
    if got["dense"] is not None:
        dense = np.zeros_like(got["dense"])
        for f in range(len(fr)):
            b0, nb, n = int(fr["box_begin"][f]), int(fr["box_count"][f]), int(fr["n"][f])
            dense[b0:b0 + nb, :n] = want["dense"][f]
        bad = np.argwhere(got["dense"] != dense)
        assert not len(bad), ("dense (box, row)", bad[:8].tolist())
    assert np.array_equal(got["db_count"], want["db_count"]), np.nonzero(got["db_count"] != want["db_count"])[0][:8]
    assert got["gathered"].shape == want["gathered"].shape
    bad = np.nonzero((got["gathered"].view(np.uint32) != want["gathered"].view(np.uint32)).any(axis=1))[0]
    assert not len(bad), ("gathered rows", bad[:8].tolist(), got["gathered"][bad[:2]], want["gathered"][bad[:2]])
    assert np.array_equal(got["hull"], want["hull_count"]), [(k, int(got["hull"][k]), int(want["hull_count"][k]))
                                                             for k in np.nonzero(got["hull"] != want["hull_count"])[0][:8]]
    assert np.array_equal(got["und_n"], want["und_n"]), [(k, int(got["und_n"][k]), int(want["und_n"][k]))
                                                         for k in np.nonzero(got["und_n"] != want["und_n"])[0][:8]]
    assert got["und_idx"].shape == (len(case["boxes"]), cap)
    for k, (f, j) in enumerate(seq.box_frame(case)):
        n = int(want["und_n"][k])
        if n <= cap:
            assert sorted(got["und_idx"][k, :n].tolist()) == want["und"][k].tolist(), (k, f, j)
            if want["hull_ref"][k] is not None:          # end to end: the decided rows + the reference's predicate on the undecided ones
                sel = np.sort(got["und_idx"][k, :n])
                extra = int(ki.in_hull(seq.frame_rows(case, f)[sel, :3], case["corners"][f][j]).sum()) if n else 0
                assert int(got["hull"][k]) + extra == want["hull_ref"][k], (k, f, j)
        else:                                            # which rows arrive depends on the order of the atomics
            kept = got["und_idx"][k].tolist()
            assert len(set(kept)) == cap and set(kept) <= set(want["und"][k].tolist()), (k, f, j)


def same_run(a, b):
    for key in ("hull", "und_n", "db_count", "gathered", "fov", "dense"):
        assert (a[key] is None and b[key] is None) or seq.same_bits(a[key], b[key]), key
    for k, n in enumerate(a["und_n"]):
        n = int(n) if n <= a["und_idx"].shape[1] else 0      # (past the capacity the rows that arrive depend on the order of the atomics)
        assert sorted(a["und_idx"][k, :n].tolist()) == sorted(b["und_idx"][k, :n].tolist()), k


def test_chunk_rows_are_the_cases_chunk_rows(gpu):
    assert ops.infos_chunk_rows() == seq.CHUNK and ops.INFOS_MAX_PASS == 256


@pytest.mark.parametrize("name", sorted(CASES))
def test_named_cases(gpu, name, capsys):
    case, want = CASES[name], restated(name)
    got = run(case, gpu)
    compare(case, want, got)
    same_run(got, run(case, gpu))                        # the same bits on a second call
    capsys.readouterr()


def test_without_boxes_and_without_the_flag(gpu):
    """n_boxes == 0 with want_fov (the flags) and without (nothing to do), and a case with boxes run without the flag"""
    case, want = CASES["frames_no_boxes"], restated("frames_no_boxes")
    got = run(case, gpu, want_fov=False)
    assert got["fov"] is None and got["gathered"].shape == (0, 4) and got["hull"].shape == (0,)
    case, want = CASES["frames_seven"], restated("frames_seven")
    got = run(case, gpu, want_fov=False)
    compare(case, want, got)


class Raw:
    """modest_infos_count / modest_infos_gather driven directly, every buffer the test's own"""

    def __init__(self, case, gpu, fill=SENTINEL):
        from modest_amd import _lib
        self.lib = _lib.load()
        self.case = case
        fr, nb = case["frames"], len(case["boxes"])
        self.rows = torch.from_numpy(np.concatenate([case["rows"], np.zeros((4, 4), np.float32)])).to(gpu)
        self.tb = int(self.lib.modest_infos_table_bytes(len(fr), nb))
        self.tables = torch.empty((self.tb + 256,), dtype=torch.uint8, device=gpu)
        assert self.tables.data_ptr() % 256 == 0
        new = lambda n: torch.full((max(n, 1),), fill, dtype=torch.int32, device=gpu)         # noqa: E731
        self.wcount, self.hull, self.und_n, self.db = new(case["wcount_words"]), new(nb), new(nb), new(nb)
        self.und_idx = new(nb * case["und_cap"])
        self.stride = int(fr["n"].max())
        self.dense = torch.zeros((max(nb, 1), max(self.stride, 1)), dtype=torch.int32, device=gpu)
        torch.cuda.synchronize()

    def count(self, **over):
        c = self.case
        a = dict(rows=self.rows.data_ptr(), n_rows=len(c["rows"]), frames=c["frames"].ctypes.data, n_frames=len(c["frames"]),
                 boxes=c["boxes"].ctypes.data, n_boxes=len(c["boxes"]), pass_boxes=c["pass_boxes"], und_cap=c["und_cap"],
                 tables=self.tables.data_ptr(), tables_bytes=self.tb, wcount=self.wcount.data_ptr(), wcount_words=c["wcount_words"],
                 hull=self.hull.data_ptr(), und_n=self.und_n.data_ptr(), und_idx=self.und_idx.data_ptr(), db=self.db.data_ptr(),
                 fov=None, dense=None, dense_stride=0, stream=None)
        assert set(over) <= set(a)
        a.update(over)
        return self.lib.modest_infos_count(*a.values())

    def gather(self, db_count_, base_, out_, total_, **over):
        c = self.case
        base_dev = torch.from_numpy(base_[:-1].copy()).to(self.rows.device)
        a = dict(rows=self.rows.data_ptr(), n_rows=len(c["rows"]), frames=c["frames"].ctypes.data, n_frames=len(c["frames"]),
                 n_boxes=len(c["boxes"]), pass_boxes=c["pass_boxes"], tables=self.tables.data_ptr(), wcount=self.wcount.data_ptr(),
                 wcount_words=c["wcount_words"], base_dev=base_dev.data_ptr(), db_count_host=db_count_.ctypes.data,
                 base_host=base_.ctypes.data, out=out_.data_ptr(), out_rows=total_, stream=None)
        assert set(over) <= set(a)
        a.update(over)
        rc = self.lib.modest_infos_gather(*a.values())
        torch.cuda.synchronize()
        return rc


@pytest.mark.parametrize("name", ["frames_seven", "frames_all_empty", "pass_boxes257_pass1"])
def test_every_box_word_is_written(gpu, name):
    """hull / und_n / db_count filled with 0x5A5A5A5A before the call: every box's words hold the counts afterwards, the
    boxes of frames without rows included"""
    case, want = CASES[name], restated(name)
    raw = Raw(case, gpu)
    assert raw.count() == 0, raw.lib.modest_last_error()
    torch.cuda.synchronize()
    nb = len(case["boxes"])
    assert np.array_equal(raw.hull.cpu().numpy()[:nb], want["hull_count"])
    assert np.array_equal(raw.und_n.cpu().numpy()[:nb], want["und_n"])
    assert np.array_equal(raw.db.cpu().numpy()[:nb], want["db_count"])


def test_every_refusal_of_the_library(gpu):
    case = CASES["frames_seven"]
    raw = Raw(case, gpu, fill=0)
    fr = case["frames"]

    def frames(field, k, value):
        t = fr.copy()
        t[field][k] = value
        return t

    keep = [frames("n", 3, len(case["rows"])), frames("box_begin", 2, 3), frames("cnt_offset", 3, int(fr["cnt_offset"][3]) + 1)]
    nb = len(case["boxes"])
    more = np.concatenate([case["boxes"], case["boxes"][:1]])
    for over, text in ((dict(n_frames=0), b"1..65535 frames per call"),
                       (dict(pass_boxes=0), b"pass_boxes must lie in 1..MODEST_INFOS_MAX_PASS"),
                       (dict(pass_boxes=257), b"pass_boxes must lie in 1..MODEST_INFOS_MAX_PASS"),
                       (dict(frames=keep[0].ctypes.data), b"frame rows outside rows_dev"),
                       (dict(frames=keep[1].ctypes.data), b"boxes must be listed frame after frame"),
                       (dict(frames=keep[2].ctypes.data), b"cnt_offset must be the running sum of chunks * box_count"),
                       (dict(boxes=more.ctypes.data, n_boxes=nb + 1), b"frames do not cover the box table"),
                       (dict(wcount_words=case["wcount_words"] - 1), b"wcount_dev too small"),
                       (dict(dense=raw.dense.data_ptr(), dense_stride=raw.stride - 1), b"dense_stride below a frame's rows"),
                       (dict(rows=raw.rows.data_ptr() + 4), b"rows must be 16-byte and tables 256-byte aligned"),
                       (dict(tables=raw.tables.data_ptr() + 16), b"rows must be 16-byte and tables 256-byte aligned"),
                       (dict(tables_bytes=raw.tb - 1), b"tables_dev too small"),
                       (dict(und_idx=None), b"bad undecided capacity"),
                       (dict(und_cap=-1), b"bad undecided capacity"),
                       (dict(hull=None), b"NULL argument")):
        rc = raw.count(**over)                              # one at a time: the error text is the last call's
        assert rc != 0 and text in raw.lib.modest_last_error(), (over, text, raw.lib.modest_last_error())
    torch.cuda.synchronize()
    assert not raw.hull.cpu().numpy().any() and not raw.db.cpu().numpy().any()       # nothing was launched, nothing written
    # the gather after a good count
    assert raw.count() == 0, raw.lib.modest_last_error()
    torch.cuda.synchronize()
    want = restated("frames_seven")
    db_count = np.ascontiguousarray(raw.db.cpu().numpy()[:nb])
    assert np.array_equal(db_count, want["db_count"])
    base = np.concatenate([[0], np.cumsum(db_count, dtype=np.int64)]).astype(np.int64)
    total = int(base[-1])
    out = torch.full((total, 4), SENTINEL, dtype=torch.int32, device=gpu)
    shifted = base.copy()
    shifted[5] += 1
    negative = db_count.copy()
    negative[5] = -1
    for over, text in ((dict(base_host=shifted.ctypes.data), b"box_base must be the exclusive sum of db_count"),
                       (dict(db_count_host=negative.ctypes.data), b"box_base must be the exclusive sum of db_count"),
                       (dict(out_rows=total - 1), b"out_rows_dev too small"),
                       (dict(out=out.data_ptr() + 4), b"rows must be 16-byte aligned"),
                       (dict(pass_boxes=0), b"pass_boxes must lie in 1..MODEST_INFOS_MAX_PASS")):
        rc = raw.gather(db_count, base, out, total, **over)
        assert rc != 0 and text in raw.lib.modest_last_error(), (over, text, raw.lib.modest_last_error())
    assert (out.cpu().numpy() == SENTINEL).all()                                      # nothing was launched
    assert raw.gather(db_count, base, out, total) == 0, raw.lib.modest_last_error()
    assert seq.same_bits(out.cpu().numpy().view(np.float32), want["gathered"])        # every row is written
