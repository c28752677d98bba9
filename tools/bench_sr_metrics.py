"""Achieved bytes / s of the stage-1 validation pass (hip_backend.sr_metrics: rehr_sr_metrics_f32 / _bf16, all four
operands given) against an existing streaming pass of the project over the same number of bytes, rehr_minmax_f32, in
the same process.  Algorithmic bytes: one read of each of the four operands (the tile halos the kernel re-reads and its
few KB of partial sums are not counted).  Time: device events around `--reps` back-to-back calls of the launch layer,
allocation of the outputs included; the three candidates alternate for `--rounds` rounds after a warm-up of each, and
the median round is reported.  The host's enqueue time per call is printed next to it: where it is no smaller than the
event time the figure measures the launches, not the kernel -- the second, larger shape shows the kernel's own rate.

    python tools/bench_sr_metrics.py [--shape 32 4 128 128] [--large 32 16 256 256] [--reps 500] [--rounds 7] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rehrseg_amd import hip_backend as hb  # noqa: E402

PEAK = 6.29e12   # measured copy peak
DEV = "cuda:0"


def timed(fn, reps):
    """-> (device seconds per call, host enqueue seconds per call)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    host = (time.perf_counter() - t0) / reps
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps, host


def measure(shape, reps, rounds):
    g = torch.Generator().manual_seed(0)
    n = int(np.prod(shape))
    tgt = torch.rand(shape, generator=g).to(DEV)
    pred = (tgt + 0.05 * torch.randn(shape, generator=g).to(DEV)).contiguous()
    logits = torch.randn(shape, generator=g).to(DEV)
    seg = (torch.rand(shape, generator=g) > 0.6).float().to(DEV)
    pred_b, logits_b = pred.bfloat16(), logits.bfloat16()
    bytes_f32, bytes_bf16 = 16 * n, 12 * n
    flat = torch.rand(bytes_f32 // 4, generator=g).to(DEV)           # the yardstick streams the fp32 pass's bytes
    mm = hb.minmax_new(flat.device)
    cands = {
        "sr_metrics fp32": (lambda: hb.sr_metrics(pred, tgt, logits, seg), bytes_f32),
        "sr_metrics bf16": (lambda: hb.sr_metrics(pred_b, tgt, logits_b, seg), bytes_bf16),
        "rehr_minmax_f32": (lambda: hb.minmax(flat, mm), bytes_f32),
    }
    for fn, _ in cands.values():
        for _ in range(10):
            fn()
    res = {k: [] for k in cands}
    for _ in range(rounds):
        for k, (fn, _) in cands.items():
            res[k].append(timed(fn, reps))
    lines = [f"shape {tuple(shape)}: {n} voxels, {bytes_f32 / 1e6:.1f} MB (fp32) / {bytes_bf16 / 1e6:.1f} MB (bf16 "
             f"prediction and logits) of algorithmic reads, {reps} calls x {rounds} alternating rounds"]
    rate = {}
    for k, (_, nbytes) in cands.items():
        dev = np.array([r[0] for r in res[k]])
        host = float(np.median([r[1] for r in res[k]]))
        med = float(np.median(dev))
        rate[k] = nbytes / med
        lines.append(f"  {k}: median {med * 1e6:.2f} us / call (min {dev.min() * 1e6:.2f}, max {dev.max() * 1e6:.2f}), "
                     f"host enqueue {host * 1e6:.2f} us / call, {rate[k] / 1e12:.3f} TB/s = {rate[k] / PEAK:.1%} of the "
                     f"copy peak" + ("  [launch-bound: enqueue >= event time]" if host >= 0.95 * med else ""))
    for k in ("sr_metrics fp32", "sr_metrics bf16"):
        lines.append(f"  {k} / rehr_minmax_f32 (bytes per second): {rate[k] / rate['rehr_minmax_f32']:.2f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=4, default=[32, 4, 128, 128])
    ap.add_argument("--large", type=int, nargs=4, default=[32, 16, 256, 256])
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sr_metrics measures on the GPU; there is none here")
    lines = measure(a.shape, a.reps, a.rounds) + measure(a.large, max(a.reps // 10, 10), a.rounds)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
