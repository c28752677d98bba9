"""Deep supervision at the reference's stage-2 lattice: one launch for all levels against a launch per level (GPU box).

    python tools/bench_ds.py [--json out.json] [--rounds 7]

Lattice 2 x 2 x 16 x 320 x 384 (batch, classes, z, y, x), the reference's six scales, its weights (the sixth is 0, so
five levels are weighted), with an uncertainty map per level.  Timed, alternating within every round so that drifting
clocks hit all of them alike (HIP events on the launch stream, 20 calls after 3 warm-ups, per call including the
host's descriptor work):

  pyramid        hb.label_pyramid: the five resized levels of one (2, 1, 16, 320, 384) map in one launch
  pyramid_loop   the same levels from hb.axis_resample, one launch per axis that changes
  ds_fwd         hb.seg_loss_ds_fwd: one memset + one launch
  ds_bwd         hb.seg_loss_ds_bwd: one launch (and the five gradient buffers)
  loop_fwd       hb.seg_loss_fwd per weighted level: five memsets + five launches
  loop_bwd       hb.seg_loss_bwd per weighted level: five launches

Per row: the median over the rounds, the smallest and largest round, the algorithmic bytes (every operand read or
written once) and the resulting share of the 8 TB/s spec / 6.29 TB/s measured-copy peaks of MI355X_MICROARCH.md."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from rehrseg_amd import hip_backend as hb  # noqa: E402
from rehrseg_amd.utils import augment as A  # noqa: E402
from rehrseg_amd.utils import seg_utils as su  # noqa: E402

dev = torch.device("cuda:0")
N, C, LATTICE = 2, 2, (16, 320, 384)


def timed(fn, reps=20):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    weights = su._build_loss(True).weight_factors
    extents = A.pyramid_extents(LATTICE, A.DEEP_SUPERVISION_SCALES)
    live = [l for l, w in enumerate(weights) if w != 0]
    g = torch.Generator(device="cpu").manual_seed(0)
    label = torch.randint(0, C, (N, 1) + LATTICE, generator=g).float().to(dev)
    unc = (1 - torch.rand((N, 1) + LATTICE, generator=g) * 0.99).to(dev)
    step = A.DownsampleSegForDSTransform2(A.DEEP_SUPERVISION_SCALES, 0)
    labels, uncs = step.pyramid(label), step.pyramid(unc)
    logits = [torch.randn((N, C) + e, generator=g).to(dev).contiguous(memory_format=torch.channels_last_3d)
              for e in extents]
    S = [e[0] * e[1] * e[2] for e in extents]
    ts = [t.reshape(N, s) for t, s in zip(labels, S)]
    us = [u.reshape(N, s) for u, s in zip(uncs, S)]
    go = torch.ones(1, device=dev)
    stats = hb.seg_loss_ds_fwd(logits, ts, us, weights)
    stats1 = [hb.seg_loss_fwd(logits[l], ts[l], us[l]) for l in live]
    work = [l for l in range(len(extents)) if extents[l] != LATTICE]
    tabs = [tuple(A._cached_index(n, m, dev) for n, m in zip(LATTICE, extents[l])) for l in work]
    src = label.contiguous()

    def pyramid_loop():
        for l in work:
            v = src
            for axis, (n, m) in enumerate(zip(LATTICE, extents[l])):
                if n != m:
                    v = hb.axis_resample(v, 2 + axis, *A._cached_taps(A.zoom_nearest_matrix, (n, m), dev), validated=True)

    voxels = sum(N * S[l] for l in live)
    pyr_bytes = sum(2 * 4 * N * S[l] for l in work)             # one gathered read and one write per output voxel
    calls = {
        "pyramid": (pyr_bytes, lambda: hb.label_pyramid(src, [extents[l] for l in work], tabs)),
        "pyramid_loop": (pyr_bytes, pyramid_loop),
        "ds_fwd": (voxels * (4 * C + 8), lambda: hb.seg_loss_ds_fwd(logits, ts, us, weights)),
        "loop_fwd": (voxels * (4 * C + 8), lambda: [hb.seg_loss_fwd(logits[l], ts[l], us[l]) for l in live]),
        "ds_bwd": (voxels * (8 * C + 8),
                   lambda: hb.seg_loss_ds_bwd(logits, ts, us, weights, stats, 1.0, 1.0, 1e-5, False, go)),
        "loop_bwd": (voxels * (8 * C + 8),
                     lambda: [hb.seg_loss_bwd(logits[l], ts[l], us[l], st, 1.0, 1.0, 1e-5, False, go)
                              for l, st in zip(live, stats1)]),
    }
    times = {k: [] for k in calls}
    for _ in range(args.rounds):
        for k, (_, fn) in calls.items():
            times[k].append(timed(fn))
    rows = []
    for k, (nbytes, _) in calls.items():
        t = statistics.median(times[k])
        rows.append({"call": k, "us_median": t * 1e6, "us_min": min(times[k]) * 1e6, "us_max": max(times[k]) * 1e6,
                     "algorithmic_bytes": nbytes, "TBps": nbytes / t / 1e12, "frac_of_8TBps": nbytes / t / 8e12,
                     "frac_of_6p29": nbytes / t / 6.29e12})
        print(f"{k:14s} {t * 1e6:8.1f} us (rounds {min(times[k]) * 1e6:.1f} .. {max(times[k]) * 1e6:.1f})  "
              f"{nbytes / 1e6:7.1f} MB  {nbytes / t / 1e12:5.2f} TB/s ({nbytes / t / 8e12:5.1%} of 8 TB/s)", flush=True)
    if args.json:
        json.dump({"lattice": [N, C, *LATTICE], "extents": extents, "weights": list(weights), "rounds": args.rounds,
                   "rows": rows}, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
