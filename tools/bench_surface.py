"""What the boundary metrics add to a validation case (GPU box): evaluate_case with surface=False and surface=True on
one 1 x 16 x 320 x 384 case -- one [16, 320, 384] tile x 8 mirrorings of the cfg-4 student plan of tools/bench_eval.py,
random init, fp32 -- alternating the two in one process, device events around every call, warm-up first, median of
--reps runs.  Then the surface work alone on the two maps of that case, stage by stage (the distance kernels, torch's
sort, the reduction), and surface_distance_metrics on two offset ellipsoids of the same lattice.

    python tools/bench_surface.py [--reps 11] [--out FILE]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rehrseg_amd import hip_backend as hb  # noqa: E402
from rehrseg_amd.utils import seg_utils as su  # noqa: E402
from tools.bench_eval import student  # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def ellipsoid(shape, centre, radii):
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    return (((z - centre[0]) / radii[0]) ** 2 + ((y - centre[1]) / radii[1]) ** 2 +
            ((x - centre[2]) / radii[2]) ** 2) <= 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    shape, sp, patch = (16, 320, 384), (5.0, 0.5, 0.5), [16, 320, 384]
    rng = np.random.RandomState(0)
    img = rng.randint(0, 1000, size=(1,) + shape).astype(np.float32)
    label = ellipsoid(shape, (9, 170, 200), (5.5, 70, 70)).astype(np.float32)[None]
    net = student(dev)
    runs = {False: lambda: su.evaluate_case(net, img, label, 4.0, patch),
            True: lambda: su.evaluate_case(net, img, label, 4.0, patch, surface=True, spacing=sp)}
    for _ in range(2):
        for flag in (False, True):
            runs[flag]()
    torch.cuda.synchronize()
    ms = {False: [], True: []}
    for _ in range(args.reps):
        for flag in (False, True):
            t, out = event_ms(runs[flag])
            ms[flag].append(t)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    lines = [f"evaluate_case, 1 x 16 x 320 x 384, tile {patch} x 8 mirrorings, cfg-4 student, fp32, device events, "
             f"median of {args.reps} alternating runs after 2 warm-up runs each:",
             f"  surface=False  {med[False]:9.3f} ms  (min {min(ms[False]):.3f}, max {max(ms[False]):.3f})",
             f"  surface=True   {med[True]:9.3f} ms  (min {min(ms[True]):.3f}, max {max(ms[True]):.3f})",
             f"  difference     {med[True] - med[False]:9.3f} ms = {100 * (med[True] - med[False]) / med[False]:.2f} % "
             f"of the case",
             f"  surface of that case: {out[4]}"]

    # the surface work alone, on the maps of that case
    pred = torch.from_numpy(out[0]).to(dev)
    gt = torch.from_numpy(label[0].astype(np.uint8)).to(dev)
    stage = {"distance kernels (surface, W, H, D + gather)": [], "torch.sort of 2 N floats": [],
             "reduction (2 kernels)": []}
    for rep in range(args.reps + 2):
        buf = torch.zeros(5, dtype=torch.int64, device=dev)
        t0, (dist, ws) = event_ms(lambda: hb.seg_surface_distances(pred, gt, sp, buf[3:5]))
        t1, srt = event_ms(lambda: torch.sort(dist.view(-1)).values)
        t2, _ = event_ms(lambda: hb.seg_surface_reduce(dist, srt, buf[3:5], buf[0:3], ws))
        if rep >= 2:
            for k, t in zip(stage, (t0, t1, t2)):
                stage[k].append(t)
    lines.append(f"surface work alone on those two maps (N = {pred.numel()}), each stage between its own events:")
    lines += [f"  {k:46s} {float(np.median(v)):8.3f} ms" for k, v in stage.items()]

    P = torch.from_numpy(ellipsoid(shape, (7.5, 150, 180), (6, 60, 80))).to(dev)
    G = torch.from_numpy(ellipsoid(shape, (9, 170, 200), (5.5, 70, 70))).to(dev)
    ts = [event_ms(lambda: su.surface_distance_metrics(P, G, sp)) for _ in range(args.reps + 2)][2:]
    lines.append(f"surface_distance_metrics on two device-resident ellipsoids of that lattice: "
                 f"{float(np.median([t for t, _ in ts])):.3f} ms  {ts[-1][1]}")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
