"""bench.py's N > 1 path with the real workload: `--gpus 2 --backend gloo` is the rehearsal form (two ranks sharing the
box's one GPU, gloo carrying the gradient buckets): self-launch, PatchParallel with hook-launched exchanges from the
side stream, the timed region's barriers, the per-kernel pass with its collectives, rank 0's line.  And what `--full`
adds to a plain run."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_two_rank_rehearsal_on_one_device():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_PORT="29549")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--workload", "flavr",
                        "--size", "64", "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline", "--kernel-steps", "2"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["n_gpus"] == 2 and rec["steps"] == 3 and rec["scaling"] == "weak"
    assert rec["config"]["global_batch"] == 2 and "REHEARSAL" in rec["config"]["parallelism"]
    assert rec["value"] > 0 and rec["ms_per_step"] > 0
    assert rec["roofline"]["frac"] > 0                          # the per-kernel pass ran on both ranks (it has collectives)


def test_plain_run_leaves_the_cpu_leg_and_the_kernel_pass_to_full():
    """A plain run prints the headline keys and nothing of the two untimed legs; --full adds the CPU oracle leg (with
    its parity line) and the per-kernel pass, and leaves the headline keys as they are."""
    recs = []
    for extra in ([], ["--full", "--cpu-steps", "1", "--kernel-steps", "2"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--size", "32", "--steps", "3",
                            "--warmup", "1", *extra], cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        recs.append(json.loads(lines[0]))
    plain, full = recs
    legs = ("cpu_baseline", "parity_vs_cpu", "roofline", "mfma_kernel_ms_per_step", "kernel_timing")
    assert not [k for k in plain if k in legs or k.startswith("roofline")]
    assert all(k in full for k in legs)
    assert full["parity_vs_cpu"]["fwd_rel"] < 1e-3 and full["roofline"]["frac"] > 0
    for rec in recs:
        assert rec["metric"] == "3D patches/sec (fwd+bwd, 32^3 fp32)" and rec["dtype"] == "f32" and rec["steps"] == 3
        assert rec["unit"] == "patches/s" and rec["higher_is_better"] is True
        assert abs(rec["value"] - 3 / (rec["ms_per_step"] * 3e-3)) < 1e-6 * rec["value"]
    assert abs(plain["loss"] - full["loss"]) <= 1e-5 * abs(plain["loss"])     # same seeds, same timed steps
