"""CPU: bench.py's launcher logic (the driver calls `python bench.py --gpus N` with no launcher)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_helper_count_keeps_a_minimum_of_steps_per_helper():
    import bench
    assert bench.MIN_STEPS_PER_HELPER >= 2
    n20 = bench.helper_count(8, 20)                # the driver's 20-step run: the whole pool, 2-3 steps each
    assert n20 == min(8, 20 // bench.MIN_STEPS_PER_HELPER)
    assert bench.helper_count(8, 560) == 8
    assert bench.helper_count(8, 3) == max(1, 3 // bench.MIN_STEPS_PER_HELPER)
    assert bench.helper_count(1, 560) == 1
    assert sum(bench._split(20, n20)) == 20 and min(bench._split(20, n20)) >= bench.MIN_STEPS_PER_HELPER


def test_launch_command_is_one_rank_per_gpu_on_localhost():
    import bench
    cmd = bench.launch_command(4, ["--gpus", "4", "--steps", "20", "--warmup", "5"])
    assert cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-6:] == ["--gpus", "4", "--steps", "20", "--warmup", "5"]
    assert os.path.basename(cmd[-7]) == "bench.py"


def test_plain_run_is_the_default_and_full_is_an_option():
    import bench
    a = bench.parse(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert a.full is False and a.dump_outputs is None and a.steps == 20 and a.warmup == 5
    a = bench.parse(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"


def test_dump_outputs_arrays_are_float_and_capped(tmp_path):
    """--dump-outputs: what one step hands back, as float32 / float64 .npy files; over the cap a fixed, seeded sample of the points."""
    import numpy as np
    import torch
    import bench
    text = ("Dynamic -1 -1 -1.5708 100.0000 150.0000 200.0000 250.0000 1.5000 1.8000 4.2000 1.0000 1.6000 20.0000 0.0000\n"
            "Dynamic -1 -1 0.1000 10.0000 15.0000 20.0000 25.0000 1.0000 0.5000 0.7000 -3.0000 1.2000 9.5000 0.2500")
    lf = bench.label_fields(text)
    assert lf.dtype == np.float64 and lf.shape == (2, bench.LABEL_FIELDS) and lf[0, 0] == -1 and lf[1, -1] == 0.25
    assert bench.label_fields("").shape == (0, bench.LABEL_FIELDS)
    n = 5000
    H = torch.linspace(0, 1, n, dtype=torch.float32)
    labels = np.arange(n, dtype=np.int64) % 7
    rows = np.random.RandomState(1).rand(2, 8)
    arrays = bench.step_arrays((H, labels, rows, text))
    assert sorted(arrays) == ["boxes", "cluster_labels", "label_fields", "pp_score"]
    assert all(v.dtype in (np.float32, np.float64) for v in arrays.values())
    assert arrays["pp_score"].dtype == np.float32 and np.array_equal(arrays["cluster_labels"], labels)
    assert bench.step_arrays((H, None, None, None)).keys() == {"pp_score"}   # --pp-only
    names = bench.write_outputs(str(tmp_path / "all"), arrays)
    assert names == sorted(arrays)
    assert np.array_equal(np.load(tmp_path / "all" / "pp_score.npy"), H.numpy())
    cap = 30000   # bytes: fewer than the 5000 points' 60 000
    bench.write_outputs(str(tmp_path / "s1"), arrays, cap=cap)
    bench.write_outputs(str(tmp_path / "s2"), arrays, cap=cap)
    files = sorted(p.name for p in (tmp_path / "s1").iterdir())
    assert files == ["boxes.npy", "cluster_labels.npy", "label_fields.npy", "point_index.npy", "pp_score.npy"]
    assert sum(np.load(tmp_path / "s1" / f).nbytes for f in files) <= cap
    idx = np.load(tmp_path / "s1" / "point_index.npy").astype(np.int64)
    assert len(idx) > 0 and np.array_equal(np.load(tmp_path / "s1" / "pp_score.npy"), H.numpy()[idx])
    assert all(np.array_equal(np.load(tmp_path / "s1" / f), np.load(tmp_path / "s2" / f)) for f in files)


def test_world_size_mismatch_fails_loudly():
    """Under a launcher that started the wrong number of ranks the bench refuses to run (round 1: it
    silently measured one GPU)."""
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], env=env, capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0
    assert "--gpus 2" in r.stderr and "WORLD_SIZE=1" in r.stderr


def test_more_gpus_than_devices_fails_loudly():
    """No launcher and fewer devices than --gpus: an error, not a one-GPU run."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "64"], env=env, capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0 and "HIP device(s) visible" in r.stderr
