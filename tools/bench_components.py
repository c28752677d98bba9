"""What the lesion-wise scores cost on the stage-2 lattice (GPU box): a (16, 320, 384) map, RandomState(1).rand < 0.3
(336 components at connectivity 26, 121212 at 6), against the same map moved by (1, 2, 3) voxels.

  1. evaluate_case with components=False and components=True through a pointwise device-only toy network, whose
     prediction is that map, so that the network does not dominate; alternating in one process.
  2. lesion_metrics on the two device-resident maps alone, host sync included.
  3. The host route it replaces, in the same process: download both maps, two scipy.ndimage.label calls and the numpy
     bookkeeping for the same eight integers.

Device events around every call, 3 warm-up runs, median (min - max) of --reps runs.  With --trace N nothing is timed:
lesion_metrics runs N times at each connectivity, for a kernel trace of the process.

    python tools/bench_components.py [--reps 20] [--out FILE] [--trace N]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from scipy import ndimage as ndi  # noqa: E402

from rehrseg_amd.utils import seg_utils as su  # noqa: E402

SHAPE = (16, 320, 384)
WARMUP = 3


class PointToy(torch.nn.Module):
    """Class 1 wherever the normalised image is positive; device ops only."""

    def __init__(self, sep):
        super().__init__()
        self.sep = sep

    def forward(self, x):
        lr = torch.cat([torch.zeros_like(x), x], 1)
        return lr, torch.repeat_interleave(lr, self.sep, dim=2)


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


def host_route(pred, gt, connectivity):
    """The eight integers of lesion_metrics from two device maps by way of the host."""
    st = ndi.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity])
    P, G = pred.cpu().numpy() != 0, gt.cpu().numpy() != 0
    lp, n_p = ndi.label(P, st)
    lg, n_g = ndi.label(G, st)
    both = P & G
    size_p, size_g = np.bincount(lp.ravel(), minlength=n_p + 1)[1:], np.bincount(lg.ravel(), minlength=n_g + 1)[1:]
    best = int(np.argmax(size_p)) + 1 if n_p else 0      # the first of equal sizes: scipy numbers in raster order
    return [n_p, n_g, len(np.unique(lp[both])), len(np.unique(lg[both])), int(size_p.max()) if n_p else 0,
            int(size_g.max()) if n_g else 0, int(((lp == best) & both).sum()), int(G.sum())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", type=int, default=0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    mask = np.random.RandomState(1).rand(*SHAPE) < 0.3
    moved = np.zeros_like(mask)
    moved[1:, 2:, 3:] = mask[:-1, :-2, :-3]
    pred, gt = torch.from_numpy(mask).to(dev), torch.from_numpy(moved).to(dev)
    if args.trace:
        for conn in (26, 6):
            for _ in range(args.trace):
                su.lesion_metrics(pred, gt, conn)
        return

    lines = [f"stage-2 lattice {SHAPE}, RandomState(1).rand < 0.3 against itself moved by (1, 2, 3); device events, "
             f"{WARMUP} warm-up runs, median of {args.reps} runs"]
    img, label = mask.astype(np.float32)[None], moved.astype(np.float32)[None]
    net, patch = PointToy(4).to(dev), list(SHAPE)
    for conn in (26, 6):
        runs = {False: lambda: su.evaluate_case(net, img, label, 4, patch, device=dev),
                True: lambda: su.evaluate_case(net, img, label, 4, patch, device=dev, components=True,
                                               connectivity=conn)}
        for _ in range(WARMUP):
            for flag in (False, True):
                runs[flag]()
        torch.cuda.synchronize()
        ms = {False: [], True: []}
        for _ in range(args.reps):
            for flag in (False, True):
                t, out = event_ms(runs[flag])
                ms[flag].append(t)
        assert np.array_equal(out[0] != 0, mask), "the toy network's prediction is the map"
        dev_ms, got = timed(lambda: su.lesion_metrics(pred, gt, conn), args.reps)
        host_ms, want = timed(lambda: host_route(pred, gt, conn), args.reps)
        vals = [got[k] for k in ("n_pred", "n_gt", "tp_pred", "tp_gt", "largest_pred", "largest_gt")]
        vals += [got["dice_largest_terms"][0], got["dice_largest_terms"][2]]
        assert out[4] == got, "evaluate_case and lesion_metrics agree"
        med = {k: float(np.median(v)) for k, v in ms.items()}
        lines += [f"connectivity {conn}: {got['n_pred']} / {got['n_gt']} components",
                  f"  evaluate_case, pointwise toy network, one tile x 8 mirrorings:",
                  f"    components=False               {fmt(ms[False])}",
                  f"    components=True                {fmt(ms[True])}",
                  f"    difference                     {med[True] - med[False]:9.3f} ms",
                  f"  lesion_metrics, device tensors   {fmt(dev_ms)}",
                  f"  host route (download, 2 x scipy.ndimage.label, numpy) {fmt(host_ms)}",
                  f"  the eight integers: device {vals}, host {want}: {'equal' if vals == want else 'DIFFERENT'}"]
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
