"""What percentile_normalization costs on handoff-sized volumes (GPU box): one 20 x 455 x 633 and one 80 x 455 x 633
float32 volume resident on the device, each once as Gaussian data and once as clipped Gaussians with 60 % exact zeros.

  1. percentile_normalization on the device tensor (radix select, bounds and the clip / scale pass), and its parts.
  2. The host route it replaces, in the same process: download, the reference's numpy lines, upload.
  3. torch.sort of the same volume on the device (what one order statistic costs by way of a full sort).

Device events around every call, 3 warm-up runs, median (min - max) of --reps runs.  The last lines give the
zero-heavy / Gaussian ratio of the device route.  With --trace N nothing is timed: the device route runs N times on
every volume, for a kernel trace of the process.

    python tools/bench_intensity_norm.py [--reps 20] [--out FILE] [--trace N]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rehrseg_amd import hip_backend as hb  # noqa: E402
from rehrseg_amd.utils import seg_utils as su  # noqa: E402

SHAPES = ((20, 455, 633), (80, 455, 633))
WARMUP = 3


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def timed(fn, reps):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    runs = [event_ms(fn) for _ in range(reps)]
    return [t for t, _ in runs], runs[-1][1]


def fmt(ms):
    return f"{float(np.median(ms)):9.3f} ms  (min {min(ms):.3f}, max {max(ms):.3f})"


def make(shape, kind, seed):
    g = np.random.RandomState(seed)
    n = int(np.prod(shape))
    if kind == "gaussian":
        x = g.standard_normal(n).astype(np.float32) * np.float32(300.0) + np.float32(1000.0)
    else:
        x = np.abs(g.standard_normal(n)).astype(np.float32) * np.float32(300.0)
        x[g.random_sample(n) < 0.6] = 0.0
    return x.reshape((1, 1) + tuple(shape))


def host_route(t):
    """Download, the reference's lines (np.percentile, clip, scale), upload."""
    img = t.cpu().numpy()
    v_min, v_max = np.percentile(img, [0.5, 99.5])
    if v_min < 0:
        v_min = 0
    out = (np.clip(img, v_min, v_max) - v_min) / (v_max - v_min)
    return torch.from_numpy(out.astype(np.float32)).to(t.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", type=int, default=0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"percentile_normalization(p 0.5 / 99.5) of one float32 volume on the device; device events, {WARMUP} "
             f"warm-up runs, median of {args.reps} runs"]
    ratios = []
    for shape in SHAPES:
        med = {}
        for kind in ("gaussian", "zero-heavy"):
            t = torch.from_numpy(make(shape, kind, 1)).to(dev)
            if args.trace:
                for _ in range(args.trace):
                    su.percentile_normalization(t)
                continue
            S = t.numel()
            ranks, frac = hb.percentile_plan(S, (0.5, 99.5))
            ch = t[:, 0]
            ws = hb.order_stats_workspace(1, len(ranks), dev)
            dev_ms, got = timed(lambda: su.percentile_normalization(t), args.reps)
            sel_ms, stats = timed(lambda: hb.order_stats(ch, ranks, workspace=ws), args.reps)
            bounds = hb.percentile_bounds(stats, frac, True)
            app_ms, _ = timed(lambda: hb.intensity_apply(ch, bounds, hb.INTENSITY_PERCENTILE), args.reps)
            host_ms, want = timed(lambda: host_route(t), max(3, args.reps // 4))
            sort_ms, srt = timed(lambda: torch.sort(t.view(-1)).values, args.reps)
            diff = float((got.view(-1) - want.view(-1)).abs().max())
            picked = torch.equal(stats.view(-1), srt[torch.tensor(ranks, device=dev)])
            med[kind] = float(np.median(dev_ms))
            lines += [f"{shape[0]} x {shape[1]} x {shape[2]} ({S / 1e6:.2f} M voxels), {kind}: "
                      f"{float((t == 0).float().mean()) * 100:.1f} % zeros",
                      f"  percentile_normalization, device tensor      {fmt(dev_ms)}",
                      f"    order statistics alone (4 ranks, 9 launches) {fmt(sel_ms)}",
                      f"    clip / scale pass alone                      {fmt(app_ms)}",
                      f"  host route (download, numpy lines, upload)   {fmt(host_ms)}",
                      f"  torch.sort of the volume on the device       {fmt(sort_ms)}",
                      f"  largest |device - host route| {diff:.3e} (the host route computes in numpy's float64); "
                      f"order statistics against the sort: {'equal' if picked else 'DIFFERENT'}"]
        if med:
            ratios.append((shape, med["zero-heavy"] / med["gaussian"]))
    for shape, r in ratios:
        lines.append(f"zero-heavy / Gaussian, device route, {shape[0]} x {shape[1]} x {shape[2]}: {r:.2f}")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out and not args.trace:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
