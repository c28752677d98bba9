"""What sample_class_locations costs on handoff-sized label volumes (GPU box): one 20 x 455 x 633 and one
80 x 455 x 633 uint8 volume resident on the device, each with about 0.1 % and about 10 % foreground.

  1. sample_class_locations on the device tensor (count, scan, select for 10 000 fractions, one download of the
     table), and the three launches of hip_backend.class_locations alone.
  2. The host route it replaces, in the same process: download of the label volume, np.flatnonzero, the same picks.

Device events around every call, 3 warm-up runs, median (min - max) of --reps runs; the two routes' tables are
compared.  No ratio is fixed in advance: the file holds what the run showed.

    python tools/bench_class_locations.py [--reps 20] [--out FILE]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rehrseg_amd import hip_backend as hb  # noqa: E402
from rehrseg_amd.utils import seg_utils as su  # noqa: E402

SHAPES = ((20, 455, 633), (80, 455, 633))
FRACTIONS = (0.001, 0.1)
WARMUP, SAMPLES, SEED = 3, 10000, 0


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


def host_route(t, u):
    """Download, np.flatnonzero, the picks of the same ranks, coordinates."""
    lab = t.cpu().numpy()
    at = np.flatnonzero(lab.reshape(-1) == 1)
    picks = at[(u.astype(np.uint64) * np.uint64(at.size)) >> np.uint64(32)]
    return np.stack(np.unravel_index(picks, lab.shape), axis=1).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    u = np.random.default_rng(SEED).integers(0, 2**32, SAMPLES, dtype=np.uint32)
    u_dev = torch.from_numpy(u.view(np.int32)).to(dev)
    lines = [f"sample_class_locations(classes=(1,), n={SAMPLES}) of one uint8 label volume on the device; device events, "
             f"{WARMUP} warm-up runs, median of {args.reps} runs"]
    for shape in SHAPES:
        for frac in FRACTIONS:
            lab = (np.random.default_rng(1).random(shape) < frac).astype(np.uint8)
            t = torch.from_numpy(lab).to(dev)
            ws = hb.class_locations_workspace(t.numel(), dev)
            dev_ms, got = timed(lambda: su.sample_class_locations(t, (1,), SAMPLES, SEED), args.reps)
            ker_ms, _ = timed(lambda: hb.class_locations(t, 1, u_dev, workspace=ws), args.reps)
            host_ms, want = timed(lambda: host_route(t, u), max(3, args.reps // 4))
            same = np.array_equal(got[1], want)
            lines += [f"{shape[0]} x {shape[1]} x {shape[2]} ({t.numel() / 1e6:.2f} M voxels), "
                      f"{float(lab.mean()) * 100:.2f} % foreground",
                      f"  sample_class_locations, device tensor         {fmt(dev_ms)}",
                      f"    count, scan and select alone (3 launches)     {fmt(ker_ms)}",
                      f"  host route (download, np.flatnonzero, picks)  {fmt(host_ms)}",
                      f"  tables of the two routes: {'equal' if same else 'DIFFERENT'}"]
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
