"""CPU: the ground planes of data_preprocessing/RANSAC.py (modest_amd.ground_planes) on the host side -- the float64
mirror against the reference's own plane files (tests/golden/planes.npz, tools/make_golden_planes.py) in both RNG
modes, frame listing, skip-if-exists, the file format and the --seed mode's independence of the other frames."""
import json
import os
from fractions import Fraction

import numpy as np
import pytest

from tests.planes_tree import TREES, golden, read_planes, tree_frames, write_tree


def _mirror(name, mode):
    from modest_amd.ground_planes import calib_mats, fit_frame_host, frame_candidates, plane_text
    names, frames, calibs, (lo, hi) = tree_frames(name)
    chain = np.random.RandomState(0)
    texts, stats = [], []
    for i, f, c in zip(names, frames, calibs):
        V2C, R0 = calib_mats(c)
        cand = frame_candidates(f, V2C, R0, lo, hi)
        rs = chain if mode == "global" else np.random.RandomState(int(i))
        w, h, fit = fit_frame_host(cand, rs)
        texts.append(plane_text(w, h))
        stats.append([-1.0] * 4 if fit is None else [len(cand), fit.threshold, fit.n_trials, fit.n_inliers])
    return texts, np.array(stats)


@pytest.mark.parametrize("mode", ["global", "frame"])
@pytest.mark.parametrize("name", TREES)
def test_host_mirror_reproduces_reference_plane_files(name, mode):
    g = golden()
    texts, stats = _mirror(name, mode)
    assert texts == [str(t) for t in g[f"{name}_{mode}"]]
    ref = g[f"{name}_{mode}_stats"]
    np.testing.assert_array_equal(stats[:, [0, 2, 3]], ref[:, [0, 2, 3]])   # n_cand, n_trials, winner's inliers
    np.testing.assert_array_equal(stats[:, 1], ref[:, 1])                   # the MAD threshold, bit for bit


def test_fixture_covers_both_sides_of_the_sampling_line():
    g = golden()
    assert list(g["trunc_global_stats"][:, 0]) == [-1, -1, 5, 120, 299, 300, 301]
    assert all(t.endswith("0.000000e+00 -1.000000e+00 0.000000e+00 1.650000e+00") for t in g["lyft_a_global"])
    assert (g["nusc_global_stats"][:, 0] > 2000).all() and (g["lyft_b_global_stats"][:, 0] > 2000).all()
    tilt = [float(str(t).split("\n")[-1].split()[0]) for t in g["tilt_global"]]
    assert max(abs(v) for v in tilt) > 0.02   # rolled / pitched frames: not (0, -1, 0)


def test_extract_ransac_host_writes_the_reference_tree(tmp_path):
    from modest_amd.ground_planes import extract_ransac_host
    names, frames, calibs, (lo, hi) = tree_frames("trunc")
    cd, ld = write_tree(str(tmp_path), names, frames, calibs)
    for mode in ("global", "frame"):
        pd = str(tmp_path / ("planes_" + mode))
        extract_ransac_host(cd, ld, pd, lo, hi, global_seed=0 if mode == "global" else None)
        assert sorted(os.listdir(pd)) == [i + ".txt" for i in names]
        assert read_planes(pd, names) == [str(t) for t in golden()[f"trunc_{mode}"]]


def test_plane_text_format():
    from modest_amd.ground_planes import H_DEFAULT, W_DEFAULT, plane_from_fit, plane_text
    assert plane_text(W_DEFAULT, H_DEFAULT) == "# Plane\nWidth 4\nHeight 1\n0.000000e+00 -1.000000e+00 0.000000e+00 1.650000e+00"
    w, h = plane_from_fit(0.01, -0.002, 1.7)
    n = np.sqrt(0.01 ** 2 + 1 + 0.002 ** 2)
    assert np.allclose(w, [0.01 / n, -1 / n, -0.002 / n], rtol=1e-15) and abs(h - 1.7 / n) < 1e-15
    assert plane_text(w, h) == "# Plane\nWidth 4\nHeight 1\n" + "{:e} {:e} {:e} {:e}".format(w[0], w[1], w[2], h)
    assert not plane_text(w, h).endswith("\n")


def test_frame_listing_like_the_reference(tmp_path):
    from modest_amd.ground_planes import list_frames
    for n in ("000010", "000002", "000007"):
        (tmp_path / (n + ".bin")).write_bytes(b"")
    (tmp_path / "000003.txt").write_bytes(b"")
    (tmp_path / "notes.bin.bak").write_bytes(b"")
    assert list_frames(str(tmp_path)) == ["000002", "000007", "000010"]
    split = tmp_path / "split.txt"
    split.write_text("000010\n000002  \n\n7\n 000007\n")   # "\n" is dropped, "7\n" (two characters) is kept
    assert list_frames(str(tmp_path), str(split)) == ["000002", "000007", "000010", "7"]
    split.write_text("000010\n\n000002")
    assert list_frames(str(tmp_path), str(split)) == ["000002", "000010"]


def test_cli_skips_an_existing_planes_dir(tmp_path, capsys):
    from modest_amd import ground_planes
    pd = tmp_path / "planes"
    pd.mkdir()
    (pd / "keep.txt").write_text("x")
    assert ground_planes.main(["--calib_dir", "/nonexistent", "--lidar_dir", "/nonexistent", "--planes_dir", str(pd)]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["skipped"] is True
    assert os.listdir(pd) == ["keep.txt"]
    a = ground_planes.parse_args([])
    assert (a.min_h, a.max_h, a.seed, a.global_seed, a.overwrite) == (1.5, 1.8, 0, None, False)
    assert ground_planes.main(["--planes_dir", str(tmp_path / "new"), "--global_seed", "0", "--total_part", "2"]) == 2


def test_seed_mode_needs_integer_names():
    from modest_amd.ground_planes import frame_seed
    assert frame_seed(5, "000012") == 17
    with pytest.raises(ValueError, match="--global_seed"):
        frame_seed(0, "scene-0001_cam")


def test_seed_mode_plane_does_not_depend_on_other_frames(tmp_path):
    from modest_amd.ground_planes import extract_ransac_host
    names, frames, calibs, (lo, hi) = tree_frames("nusc")
    cd, ld = write_tree(str(tmp_path), names[:6], frames[:6], calibs[:6])
    extract_ransac_host(cd, ld, str(tmp_path / "all"), lo, hi, seed=3)
    split = tmp_path / "split.txt"
    split.write_text("000004\n000001\n")
    extract_ransac_host(cd, ld, str(tmp_path / "two"), lo, hi, split_file=str(split), seed=3)
    assert read_planes(str(tmp_path / "two"), ["000001", "000004"]) == read_planes(str(tmp_path / "all"), ["000001", "000004"])
    # ... and differs from another seed
    extract_ransac_host(cd, ld, str(tmp_path / "other"), lo, hi, split_file=str(split), seed=4)
    assert read_planes(str(tmp_path / "other"), ["000001"]) != read_planes(str(tmp_path / "all"), ["000001"])


def test_numpy_prediction_rounding_is_the_device_statement():
    """ground_planes.hip: gp_pred rounds X @ coef as numpy's dgemv does for (n,2) rows: fma(x, c0, z * c1)"""
    rng = np.random.default_rng(0)
    X = np.ascontiguousarray(rng.normal(size=(400, 2)) * 20)
    c = np.array([-1.234567e-3, 3.21e-3])
    got = X @ c
    want = [float(Fraction(x) * Fraction(c[0]) + Fraction(float(z * c[1]))) for x, z in X]
    assert np.array_equal(got, np.array(want))


def test_host_mirror_matches_sklearn_when_available():
    sk = pytest.importorskip("sklearn.linear_model")
    from modest_amd.utils.ransac import ransac_plane64
    rng = np.random.default_rng(7)
    for n in (5, 40, 299, 300, 301, 5000):
        X = np.stack([rng.uniform(-20, 20, n), rng.uniform(-10, 70, n)], 1)
        y = 1.6 + 0.01 * X[:, 0] - 0.003 * X[:, 1] + rng.normal(0, 0.02, n)
        out = rng.random(n) < 0.3
        y[out] = rng.uniform(1.3, 2.0, out.sum())
        a, b = np.random.RandomState(n), np.random.RandomState(n)
        reg = sk.RANSACRegressor(random_state=a).fit(X, y)
        fit = ransac_plane64(X, y, random_state=b)
        assert (reg.n_trials_, int(reg.inlier_mask_.sum())) == (fit.n_trials, fit.n_inliers)
        np.testing.assert_allclose(fit.coef, reg.estimator_.coef_, rtol=1e-9, atol=1e-12)
        assert abs(fit.intercept - reg.estimator_.intercept_) < 1e-9
        assert a.get_state()[2] == b.get_state()[2] and np.array_equal(a.get_state()[1], b.get_state()[1])
