"""GPU: csrc/ground_planes.hip at its hand-back and tie edges, on the frame families of tests/planes_cases.py (what they
hold is pinned without a GPU by tests/test_ground_planes_cases_cpu.py).

Every frame goes through ops.ground_planes and is held to the status planes_cases.expected() predicts from the host
mirror's own operations: candidate count, median and MAD bit for bit against numpy, then for a fit the triplets, trial
count, winner's inlier count, advanced generator and the plane to 1e-12, and for a hand-back the generator
bit for bit as it was handed in (a hand-back at the refit, for a consensus set of one height, has run its trials: their
count, the triplets and the winner's inlier count are held too).  The chained mode, the CLI's driver loop around a mid-batch hand-back and the argument
checks of the entry point follow."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import planes_cases as pc
from tests.planes_cases import DEFAULT, FITTED, HOST, NO_CONSENSUS
from tests.planes_tree import read_planes, write_tree

pytestmark = pytest.mark.gpu


def _table(frames, calibs, states):
    """GP_FRAME rows and the packed rows of a batch; states: one (key, pos) per frame"""
    from modest_amd import ops
    from modest_amd.ground_planes import calib_mats
    fr = np.zeros(len(frames), dtype=ops.GP_FRAME)
    offs = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int64)
    fr["row_offset"], fr["n"] = offs[:-1], np.diff(offs)
    for k, (c, (key, pos)) in enumerate(zip(calibs, states)):
        V2C, R0 = calib_mats(c)
        fr["v2c"][k], fr["r0"][k] = V2C.ravel(), R0.ravel()
        fr["key"][k], fr["pos"][k] = key, pos
    rows = np.concatenate(frames) if len(frames) else np.zeros((0, 4), dtype=np.float32)
    return fr, np.ascontiguousarray(rows, dtype=np.float32)


def _check_frame(name, cand, e, res, fr, fr0, trip):
    """the common assertions for one frame: its GP_RESULT row, its GP_FRAME row after and before the call, its triplets"""
    assert res["n_cand"] == len(cand), name
    if len(cand) > pc.SMALL:
        med = np.median(cand[:, 1])
        assert res["median"] == med and res["mad"] == np.median(np.abs(cand[:, 1] - med)), name        # bit for bit
    assert res["status"] == e.status, (name, int(res["status"]), e.status, int(res["n_trials"]), e.n_trials)
    if e.status == HOST:
        assert fr["pos"] == fr0["pos"] and np.array_equal(fr["key"], fr0["key"]), name
        if e.one_height:            # handed back at the refit: the trials ran, and ran as the mirror's
            f = e.fit
            assert (res["n_trials"], res["n_inliers"]) == (f.n_trials, f.n_inliers), name
            if trip is not None:
                np.testing.assert_array_equal(trip[:f.n_trials], f.triplets, err_msg=name)
                assert (trip[f.n_trials:] == -1).all(), name
        return
    assert fr["pos"] == e.pos and np.array_equal(fr["key"], e.key), name       # advanced by the executed trials
    if e.status == NO_CONSENSUS:
        assert res["n_trials"] == e.n_trials, name
    if e.status == FITTED:
        f = e.fit
        assert (res["n_trials"], res["n_inliers"]) == (f.n_trials, f.n_inliers), name
        if trip is not None:
            np.testing.assert_array_equal(trip[:f.n_trials], f.triplets, err_msg=name)
            assert (trip[f.n_trials:] == -1).all(), name
        np.testing.assert_allclose(res["plane"], pc.plane_of(f), rtol=1e-12, atol=1e-14, err_msg=name)
    if e.status == DEFAULT:
        assert list(res["plane"]) == [0.0, -1.0, 0.0, 1.65]


def _run_family(gpu, family):
    """every frame of a family, one call per (window, max_trials, stop_probability); returns {status: count}"""
    import torch
    from modest_amd import ops
    todo = pc.predict(family)
    groups = {}
    for item in todo:
        c = item[0]
        groups.setdefault((c.window, c.max_trials, c.p), []).append(item)
    seen = {}
    for (window, max_trials, p), items in groups.items():
        fr, rows = _table([c.rows for c, _, _ in items], [c.calib for c, _, _ in items],
                          [pc.state_of(np.random.RandomState(c.seed)) for c, _, _ in items])
        fr0 = fr.copy()
        res, _, trip = ops.ground_planes(torch.from_numpy(rows).to(gpu), fr, window[0], window[1], max_trials=max_trials,
                                         stop_probability=p, return_triplets=True)
        for k, (c, cand, e) in enumerate(items):
            _check_frame(c.name, cand, e, res[k], fr[k], fr0[k], trip[k])
            seen[e.status] = seen.get(e.status, 0) + 1
    return seen


def test_select_and_compaction_at_chunk_edges(gpu):
    """301..1025 candidates of both parities, ragged and full ballots, runs of equal keys across the middle, two different
    middle values, keys equal but for the last byte, a dozen binades, a window below zero: median and MAD as numpy's"""
    seen = _run_family(gpu, "select")
    assert seen == {FITTED: 98}


def test_window_bounds_and_non_finite_rows(gpu):
    assert _run_family(gpu, "window") == {FITTED: 4}


def test_collinear_triplets_hand_back_with_the_generator_restored(gpu):
    """frames next to a handed-back frame in the same batch are fitted as if alone"""
    seen = _run_family(gpu, "dup")
    assert seen[HOST] >= 6 and seen[FITTED] >= 4


def test_zero_threshold_frames(gpu):
    """MAD == 0: |y - pred| <= 0 as numpy rounds pred; one and two trials reach NO_CONSENSUS, the NaN-score accept, the
    refit hand-back and winners of exactly three; the flat set, wherever it wins, is one height and handed back at the refit"""
    seen = _run_family(gpu, "flat")
    assert seen == {NO_CONSENSUS: 9, HOST: 64, FITTED: 17}


@pytest.mark.parametrize("q", pc.QUANTA)
def test_quantised_heights(gpu, q):
    """residual == thr membership (1/64 m: fitted) and equal-nk ties (1/16, 1/8 m: thr == 0, the winner is one height level,
    handed back at the refit with its trials, triplets and inlier count the mirror's)"""
    assert _run_family(gpu, f"quant{q}") == {(FITTED if q == 64 else HOST): len(pc.QUANT_SEEDS[q])}


def test_two_level_frames_decide_their_ties_as_the_mirror(gpu):
    """equal-nk ties between different planes, accepted and passed over (pinned on the CPU): the fitted plane shows which
    trial won, so this is where `nk == n_best && score < score_best` is held on the device"""
    assert _run_family(gpu, "two") == {FITTED: len(pc.TWO_SEEDS)}


def test_parameters(gpu):
    """stop_probability 0 and 1, max_trials 1 / 37 / 256 / 4096 (a second MT19937 refill, the 4096-row triplet table), the
    near-integer trial bounds and their controls"""
    seen = _run_family(gpu, "params")
    assert seen == {FITTED: 27, HOST: 9}       # the near-integer bounds, and the six half-flat frames at their refit


def _walk_chain(frames, seed):
    """the frames of a --global_seed run on one RandomState: [(cand, Expected)], the mirror fitting every hand-back"""
    from modest_amd.utils.ransac import ransac_plane64
    rs = np.random.RandomState(seed)
    out = []
    for rows, calib in frames:
        cand = pc.candidates(rows, calib)
        e = pc.expected(cand, rs)
        out.append((cand, e))
        if e.status == HOST:
            ransac_plane64(cand[:, [0, 2]], cand[:, 1], random_state=rs)
    return out


def test_chained_mode_stops_at_a_mid_batch_hand_back(gpu):
    import torch
    from modest_amd import ops
    frames = pc.chain_frames()
    fr, rows = _table([f for f, _ in frames], [c for _, c in frames],
                      [pc.state_of(np.random.RandomState(pc.CHAIN_SEED))] * len(frames))
    fr0 = fr.copy()
    res, _, trip = ops.ground_planes(torch.from_numpy(rows).to(gpu), fr, *pc.WINDOW, chain=True, return_triplets=True)
    want = _walk_chain(frames, pc.CHAIN_SEED)
    assert [e.status for _, e in want[:3]] == [FITTED, FITTED, HOST] and want[2][1].collinear >= 2
    for k in range(2):
        _check_frame(f"chain-{k}", want[k][0], want[k][1], res[k], fr[k], fr0[k], trip[k])
    # the stopped frame carries the state before it: the one after frame 1
    assert res["status"][2] == HOST and res["n_cand"][2] == len(want[2][0])
    assert fr["pos"][2] == want[1][1].pos and np.array_equal(fr["key"][2], want[1][1].key)
    for k in range(3, len(frames)):
        assert res["status"][k] == HOST and res["n_cand"][k] == len(want[k][0]), k
        assert res["n_trials"][k] == 0 and (trip[k] == -1).all(), k


def _tree(tmp_path, frames):
    names = ["%06d" % k for k in range(len(frames))]
    cd, ld = write_tree(str(tmp_path), names, [f for f, _ in frames], [c for _, c in frames])
    return names, cd, ld


@pytest.mark.parametrize("batch", [4, 256])
def test_driver_loop_around_a_hand_back_writes_the_host_files(gpu, tmp_path, batch):
    """extract_ransac over the chain frames in both RNG modes against extract_ransac_host, byte for byte; host_fits counts
    the predicted hand-backs"""
    from modest_amd.ground_planes import extract_ransac, extract_ransac_host
    frames = pc.chain_frames()
    names, cd, ld = _tree(tmp_path, frames)
    n_host = {"global": sum(e.status == HOST for _, e in _walk_chain(frames, pc.CHAIN_SEED)),
              "frame": sum(pc.expected(pc.candidates(r, c), np.random.RandomState(2 + k)).status == HOST
                           for k, (r, c) in enumerate(frames))}
    assert n_host == {"global": 2, "frame": 2}       # the duplicate frame (a collinear triplet) and the flat one (one height)
    for mode, kw in (("global", dict(global_seed=pc.CHAIN_SEED)), ("frame", dict(seed=2))):
        got, ref, stats = str(tmp_path / ("gpu_" + mode)), str(tmp_path / ("host_" + mode)), {}
        extract_ransac(cd, ld, got, *pc.WINDOW, batch=batch, stats=stats, **kw)
        extract_ransac_host(cd, ld, ref, *pc.WINDOW, **kw)
        assert sorted(os.listdir(got)) == [i + ".txt" for i in names]
        assert read_planes(got, names) == read_planes(ref, names), mode
        assert stats["host_fits"] == n_host[mode] and stats["frames"] == len(frames), (mode, stats)


def test_no_consensus_raises_the_references_error(gpu, tmp_path, monkeypatch):
    """a frame that ends MODEST_GP_NO_CONSENSUS: RANSACRegressor's ValueError.  No frame gets there in 100 trials (a zero
    threshold needs a flat majority, which 100 triplets find), so the driver's device call is held to one trial."""
    import functools
    from modest_amd import ground_planes, ops
    frames = [pc.base_frame(100), pc.flat_frame(1)]
    e = pc.expected(pc.candidates(*frames[1]), np.random.RandomState(1), max_trials=1)
    assert e.status == NO_CONSENSUS
    names, cd, ld = _tree(tmp_path, frames)
    monkeypatch.setattr(ops, "ground_planes", functools.partial(ops.ground_planes, max_trials=1))
    with pytest.raises(ValueError, match="could not find a valid consensus set"):
        ground_planes.extract_ransac(cd, ld, str(tmp_path / "planes"), *pc.WINDOW, seed=0)


def test_entry_point_arguments(gpu):
    import torch
    from modest_amd import _lib, ops
    lib = _lib.load()
    ctx = _lib.default_context(0)
    rows_np, calib = pc.base_frame(0)
    cand = pc.candidates(rows_np, calib)
    rows = torch.from_numpy(rows_np).to(gpu)

    def call(n_frames=1, max_trials=100, chain=0, pos=624, n=len(rows_np), rows_ptr=rows.data_ptr()):
        fr, _ = _table([rows_np], [calib], [pc.state_of(np.random.RandomState(0))])
        fr["pos"], fr["n"] = pos, n
        P = np.zeros((), dtype=ops.GP_PARAMS)
        P["min_h"], P["max_h"], P["stop_probability"], P["max_trials"], P["chain"] = 1.5, 2.5, 0.99, max_trials, chain
        res = np.zeros(1, dtype=ops.GP_RESULT)
        res["status"] = -7
        _lib.check(lib.modest_ground_planes(ctx.handle, rows_ptr, fr.ctypes.data, n_frames, P.ctypes.data, res.ctypes.data,
                                            None, None, torch.cuda.current_stream().cuda_stream), "modest_ground_planes")
        return res[0], fr[0]

    e = pc.expected(cand, np.random.RandomState(0))
    for bad in (dict(n_frames=65536), dict(n_frames=-1), dict(max_trials=0), dict(max_trials=4097), dict(chain=2),
                dict(pos=625), dict(pos=-1), dict(n=-1), dict(rows_ptr=None)):
        with pytest.raises(_lib.ModestHipError):
            call(**bad)
        res, fr = call()                       # ... and a normal call still works
        assert (res["status"], res["n_trials"], res["n_inliers"]) == (FITTED, e.fit.n_trials, e.fit.n_inliers), bad
        assert fr["pos"] == e.pos
    res, _ = call(n_frames=0, rows_ptr=None)   # nothing to do: returns at once, the results untouched
    assert res["status"] == -7
    res, _ = call(n=0, rows_ptr=None)          # no rows needed
    assert (res["status"], res["n_cand"]) == (DEFAULT, 0)


@pytest.mark.parametrize("chain", [False, True])
def test_empty_frames_at_the_first_middle_and_last_position(gpu, chain):
    import torch
    from modest_amd import ops
    empty = np.zeros((0, 4), dtype=np.float32)
    a, b = pc.base_frame(100), pc.base_frame(101)
    frames = [(empty, a[1]), a, (empty, a[1]), b, (empty, b[1])]
    seeds = [pc.CHAIN_SEED] * 5 if chain else [7, 8, 9, 10, 11]
    fr, rows = _table([f for f, _ in frames], [c for _, c in frames], [pc.state_of(np.random.RandomState(s)) for s in seeds])
    fr0 = fr.copy()
    res, _, trip = ops.ground_planes(torch.from_numpy(rows).to(gpu), fr, *pc.WINDOW, chain=chain, return_triplets=True)
    assert list(res["status"]) == [DEFAULT, FITTED, DEFAULT, FITTED, DEFAULT]
    rs = np.random.RandomState(pc.CHAIN_SEED)
    for k, (f, c) in enumerate(frames):
        cand = pc.candidates(f, c)
        e = pc.expected(cand, rs if chain else np.random.RandomState(seeds[k]))
        _check_frame(f"empty-{k}", cand, e, res[k], fr[k], fr0[k], trip[k])
