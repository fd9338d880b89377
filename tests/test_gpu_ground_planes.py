"""GPU: the ground planes of data_preprocessing/RANSAC.py on the device (csrc/ground_planes.hip, modest_amd.ground_planes).

The CLI reproduces the reference's plane files byte for byte in both RNG modes (tests/golden/planes.npz), and the batch
entry point agrees with the float64 host mirror on full-size synthetic frames: candidate counts, MAD bit for bit,
triplets, trial counts, winner's inlier counts, planes to 1e-12."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.planes_tree import TREES, golden, read_planes, tree_frames, write_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cli(*args):
    r = subprocess.run([sys.executable, "-m", "modest_amd.ground_planes", *args], cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("name", TREES)
def test_cli_reproduces_reference_plane_files(gpu, tmp_path, name):
    g = golden()
    names, frames, calibs, (lo, hi) = tree_frames(name)
    cd, ld = write_tree(str(tmp_path), names, frames, calibs)
    for mode, flag in (("global", "--global_seed"), ("frame", "--seed")):
        pd = str(tmp_path / ("planes_" + mode))
        out = _cli("--calib_dir", cd, "--lidar_dir", ld, "--planes_dir", pd, "--min_h", repr(lo), "--max_h", repr(hi), flag, "0",
                   "--batch", "5")
        assert '"frames_per_s"' in out
        got = read_planes(pd, names)
        for i, a, b in zip(names, got, g[f"{name}_{mode}"]):
            assert a == str(b), (name, mode, i)


@pytest.mark.gpu
def test_cli_parts_equal_one_part(gpu, tmp_path):
    names, frames, calibs, (lo, hi) = tree_frames("nusc")
    cd, ld = write_tree(str(tmp_path), names, frames, calibs)
    common = ["--calib_dir", cd, "--lidar_dir", ld, "--min_h", repr(lo), "--max_h", repr(hi), "--seed", "0"]
    _cli(*common, "--planes_dir", str(tmp_path / "one"))
    for p in (0, 1):
        _cli(*common, "--planes_dir", str(tmp_path / "two"), "--total_part", "2", "--part", str(p), "--overwrite")
    assert sorted(os.listdir(tmp_path / "two")) == sorted(i + ".txt" for i in names)
    assert read_planes(str(tmp_path / "two"), names) == read_planes(str(tmp_path / "one"), names)


def _frames_table(frames, calibs, seeds):
    from modest_amd import ops
    from modest_amd.ground_planes import calib_mats
    fr = np.zeros(len(frames), dtype=ops.GP_FRAME)
    offs = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int64)
    fr["row_offset"], fr["n"] = offs[:-1], np.diff(offs)
    for k, (c, s) in enumerate(zip(calibs, seeds)):
        V2C, R0 = calib_mats(c)
        fr["v2c"][k], fr["r0"][k] = V2C.ravel(), R0.ravel()
        st = np.random.RandomState(s).get_state()
        fr["key"][k], fr["pos"][k] = st[1], st[2]
    return fr, offs


@pytest.mark.gpu
def test_trunc_frames_split_at_301_candidates(gpu):
    """5..300 candidates go back to the host (sklearn permutes there), 301 is fitted on the device, < 5 is the default"""
    import torch
    from modest_amd import ops
    g = golden()
    names, frames, calibs, (lo, hi) = tree_frames("trunc")
    fr, offs = _frames_table(frames, calibs, [int(i) for i in names])
    rows = torch.from_numpy(np.concatenate(frames)).to(gpu)
    res, _, _ = ops.ground_planes(rows, fr, lo, hi)
    assert list(res["n_cand"]) == [0, 4, 5, 120, 299, 300, 301]
    assert list(res["status"]) == [ops.GP_DEFAULT] * 2 + [ops.GP_HOST] * 4 + [ops.GP_FITTED]
    st = g["trunc_frame_stats"][6]
    assert (res["n_cand"][6], res["mad"][6], res["n_trials"][6], res["n_inliers"][6]) == (st[0], st[1], st[2], st[3])
    from modest_amd.ground_planes import plane_text
    assert plane_text(res["plane"][6][:3], res["plane"][6][3]) == str(g["trunc_frame"][6])
    # hand-backs come back with the generator untouched
    for k in range(6):
        assert fr["pos"][k] == np.random.RandomState(int(names[k])).get_state()[2]


@pytest.mark.gpu
def test_batch_matches_host_mirror_on_full_size_frames(gpu):
    import torch
    from modest_amd import ops, synth
    from modest_amd.ground_planes import calib_mats, frame_candidates
    from modest_amd.utils.ransac import ransac_plane64
    rng = np.random.default_rng(2024)
    F = 640
    sizes = rng.integers(30000, 60000, F)
    sizes[[5, 77, 300]] = 0
    sizes[123] = 200000
    frames, calibs = [], []
    for k in range(F):
        tilt = (rng.uniform(-0.004, 0.004), rng.uniform(-0.004, 0.004))
        frames.append(synth.ground_frame(rng, int(sizes[k]), height=2.1 + rng.uniform(-0.1, 0.1), tilt=tilt,
                                         clutter=rng.uniform(0.1, 0.5)))
        calibs.append(synth.ground_calib_txt(k))
    seeds = list(range(1000, 1000 + F))
    fr, offs = _frames_table(frames, calibs, seeds)
    rows = torch.from_numpy(np.concatenate(frames)).to(gpu)
    res, ms, trip = ops.ground_planes(rows, fr, 1.5, 2.5, return_triplets=True)
    assert ms > 0
    mats = [calib_mats(c) for c in calibs[:3]]
    fitted = 0
    sk = None
    try:
        from sklearn.linear_model import RANSACRegressor as sk
    except ImportError:
        pass
    for k in range(F):
        cand = frame_candidates(frames[k], *mats[k % 3], 1.5, 2.5)
        assert res["n_cand"][k] == len(cand), k
        if len(cand) < 5:
            assert res["status"][k] == ops.GP_DEFAULT
            continue
        assert len(cand) > 300
        assert res["status"][k] == ops.GP_FITTED, k
        fitted += 1
        rs = np.random.RandomState(seeds[k])
        fit = ransac_plane64(cand[:, [0, 2]], cand[:, 1], random_state=rs)
        assert res["median"][k] == fit.median and res["mad"][k] == fit.threshold, k       # bit for bit
        assert (res["n_trials"][k], res["n_inliers"][k]) == (fit.n_trials, fit.n_inliers), k
        np.testing.assert_array_equal(trip[k, :fit.n_trials], fit.triplets)
        assert (trip[k, fit.n_trials:] == -1).all()
        st = rs.get_state()
        assert fr["pos"][k] == st[2] and np.array_equal(fr["key"][k], st[1]), k          # the advanced generator
        c0, c1, b = fit.coef[0], fit.coef[1], fit.intercept
        n = np.linalg.norm([c0, -1.0, c1])
        np.testing.assert_allclose(res["plane"][k], [c0 / n, -1 / n, c1 / n, b / n], rtol=1e-12, atol=1e-14)
        if sk is not None and k % 40 == 1:
            reg = sk(random_state=np.random.RandomState(seeds[k])).fit(cand[:, [0, 2]], cand[:, 1])
            assert (reg.n_trials_, int(reg.inlier_mask_.sum())) == (res["n_trials"][k], res["n_inliers"][k])
            e = reg.estimator_
            n2 = np.linalg.norm([e.coef_[0], -1.0, e.coef_[1]])
            np.testing.assert_allclose(res["plane"][k], [e.coef_[0] / n2, -1 / n2, e.coef_[1] / n2, e.intercept_ / n2],
                                       rtol=1e-9, atol=1e-12)
    assert fitted >= F - 3


@pytest.mark.gpu
def test_chained_generator_matches_one_random_state(gpu):
    """chain = 1: frames consume one RandomState in order; the result equals the mirror run frame after frame"""
    import torch
    from modest_amd import ops
    from modest_amd.ground_planes import calib_mats, frame_candidates
    from modest_amd.utils.ransac import ransac_plane64
    names, frames, calibs, (lo, hi) = tree_frames("nusc")
    fr, offs = _frames_table(frames, calibs, [0] * len(frames))
    rows = torch.from_numpy(np.concatenate(frames)).to(gpu)
    res, _, _ = ops.ground_planes(rows, fr, lo, hi, chain=True)
    rs = np.random.RandomState(0)
    for k in range(len(frames)):
        cand = frame_candidates(frames[k], *calib_mats(calibs[k]), lo, hi)
        fit = ransac_plane64(cand[:, [0, 2]], cand[:, 1], random_state=rs)
        assert res["status"][k] == ops.GP_FITTED
        assert (res["n_trials"][k], res["n_inliers"][k]) == (fit.n_trials, fit.n_inliers)
        st = rs.get_state()
        assert fr["pos"][k] == st[2] and np.array_equal(fr["key"][k], st[1])
