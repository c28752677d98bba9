"""`python bench.py --gpus N` started plainly must itself start N ranks: run it with the gloo
backend switch and the stub workload (a torch-only two-layer net: plumbing, no HIP kernels) and read rank 0's line."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*flags):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "2"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *flags], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]                     # ONE JSON line, from rank 0
    return json.loads(lines[0])


def test_gpus_2_starts_two_ranks_by_itself():
    rec = _run("--gpus", "2", "--steps", "3", "--warmup", "1", "--backend", "gloo", "--workload", "stub")
    assert rec["n_gpus"] == 2 and rec["steps"] == 3 and rec["warmup"] == 1
    assert rec["config"]["global_batch"] == 2 and rec["scaling"] == "weak"
    assert rec["value"] > 0 and abs(rec["value"] - 2 * 3 / (rec["ms_per_step"] * 3e-3)) < 1e-6 * rec["value"]


def test_single_rank_plain_start():
    rec = _run("--gpus", "1", "--steps", "2", "--warmup", "0", "--backend", "gloo", "--workload", "stub")
    assert rec["n_gpus"] == 1


def test_dump_outputs_of_the_last_timed_step_repeat_from_run_to_run(tmp_path):
    """--dump-outputs: float32 .npy files of the last timed step (its loss is the line's `loss`), identical for two runs
    with the same arguments; with two ranks only rank 0 writes."""
    import numpy as np
    recs = [_run("--gpus", "1", "--steps", "3", "--warmup", "1", "--backend", "gloo", "--workload", "stub",
                 "--dump-outputs", str(tmp_path / d)) for d in ("a", "b")]
    names = sorted(recs[0]["dump_outputs"]["arrays"])
    assert names == ["grads", "loss", "output", "params"]
    assert recs[0]["dump_outputs"]["params_without_grad"] == []
    assert recs[0]["dump_outputs"]["arrays"]["grads"]["shape"] == recs[0]["dump_outputs"]["arrays"]["params"]["shape"]
    assert sorted(os.listdir(tmp_path / "a")) == sorted(os.listdir(tmp_path / "b")) == [n + ".npy" for n in names]
    for n in names:
        a, b = np.load(tmp_path / "a" / (n + ".npy")), np.load(tmp_path / "b" / (n + ".npy"))
        assert a.dtype == np.float32 and np.array_equal(a, b), n
    assert float(np.load(tmp_path / "a" / "loss.npy")[0]) == recs[0]["loss"]
    rec = _run("--gpus", "2", "--steps", "2", "--warmup", "0", "--backend", "gloo", "--workload", "stub",
               "--dump-outputs", str(tmp_path / "c"))
    assert rec["n_gpus"] == 2 and sorted(rec["dump_outputs"]["arrays"]) == names


def test_dump_outputs_samples_large_arrays_within_64mb(tmp_path):
    """Arrays that do not fit are written as a seeded sample of their own elements, the same one every time, and arrays
    of one size (params / grads) at the same indices."""
    import numpy as np
    import torch

    import bench
    big = torch.arange(12 << 20, dtype=torch.float32)
    arrays = {"loss": torch.tensor([0.5]), "big": big, "bigger": -torch.arange(15 << 20, dtype=torch.float64),
              "big2": 2 * big}
    info = bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 << 20
    assert not info["loss"]["sampled"] and info["big"]["sampled"] and info["bigger"]["sampled"]
    assert np.array_equal(np.load(tmp_path / "a" / "big2.npy"), 2 * np.load(tmp_path / "a" / "big.npy"))
    for n in arrays:
        a = np.load(tmp_path / "a" / (n + ".npy"))
        assert a.dtype == np.float32 and a.size == info[n]["saved"] and np.array_equal(a, np.load(tmp_path / "b" / (n + ".npy")))
    s = np.load(tmp_path / "a" / "big.npy")
    assert np.all(np.diff(s) > 0) and s[0] >= 0 and s[-1] < big.numel()      # distinct elements of `big`, in order


def test_rank_count_mismatch_is_refused():
    """Started by a launcher with a world size other than --gpus: refuse instead of reporting a wrong n_gpus."""
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29533")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--workload",
                        "stub"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "ranks" in (r.stderr + r.stdout)
