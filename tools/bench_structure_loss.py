"""Times the fused stage-1 structure loss (models.losses.StructureLoss over csrc/sr_losses.hip) on the device.

  1. forward + backward of the fused loss against the same loss composed from plain torch ops on the GPU (F.conv2d
     windows, autograd), at (32, 1, 4, 96, 96) -- the stage-1 training batch -- and (4, 1, 4, 32, 32);
  2. train_sr_step on the reference's stage-1 shape (UNet_3D_3D(2, 'unet_18', 4, 4, use_uncertainty), 32 x 2 x 4 x 96 x 96)
     with torch.nn.L1Loss against the same step with StructureLoss(l1=1, ssim=1, sobel=1).

Device events around runs of back-to-back calls, the candidates alternating round by round; median and range over the
rounds.  Writes what it prints to --out (default profiles/structure_loss_bench.txt).  Needs an MI355X: no fallback."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rehrseg_amd import hip_backend as hb  # noqa: E402
from rehrseg_amd.models.FLAVR.FLAVR_arch import UNet_3D_3D  # noqa: E402
from rehrseg_amd.models.losses import StructureLoss  # noqa: E402
from rehrseg_amd.train_steps import train_sr_step  # noqa: E402
from rehrseg_amd.utils.seg_utils import BCEDiceLoss  # noqa: E402

DEV = "cuda:0"


class TorchStructureLoss(torch.nn.Module):
    """The definition of DESIGN section 3.18 in plain torch ops (the yardstick of this tool, not product code)."""

    def __init__(self, l1, l2, ssim, sobel, data_range=1.0):
        super().__init__()
        self.w = (l1, l2, ssim, sobel)
        k = torch.arange(11, dtype=torch.float64) - 5
        g = torch.exp(-k * k / (2 * 1.5 ** 2))
        self.register_buffer("g", (g / g.sum()).float())
        kx = torch.tensor([[-1.0, 0.0, 1.0], [-2.0, 0.0, 2.0], [-1.0, 0.0, 1.0]]) / 8
        self.register_buffer("k", torch.stack((kx, kx.t())).view(2, 1, 3, 3))
        self.C1, self.C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2

    def forward(self, input, target):
        l1, l2, ssim, sobel = self.w
        H, W = input.shape[-2:]
        x, y = input.reshape(-1, 1, H, W), target.reshape(-1, 1, H, W)
        loss = 0.0
        if l1:
            loss = loss + l1 * (x - y).abs().mean()
        if l2:
            loss = loss + l2 * ((x - y) ** 2).mean()
        if ssim:
            def win(f):
                return F.conv2d(F.conv2d(f, self.g.view(1, 1, 1, 11)), self.g.view(1, 1, 11, 1))
            mx, my = win(x), win(y)
            sxx, syy, sxy = win(x * x) - mx * mx, win(y * y) - my * my, win(x * y) - mx * my
            S = ((2 * mx * my + self.C1) * (2 * sxy + self.C2)) / ((mx * mx + my * my + self.C1) * (sxx + syy + self.C2))
            loss = loss + ssim * (1 - S.mean())
        if sobel:
            def mag(f):
                r = F.conv2d(F.pad(f, (1, 1, 1, 1), mode="replicate"), self.k)
                return torch.sqrt(r[:, 0:1] ** 2 + r[:, 1:2] ** 2 + 1e-6)
            loss = loss + sobel * (mag(x) - mag(y)).abs().mean()
        return loss


def timed(fn, calls):
    """Milliseconds per call of `calls` back-to-back calls, by device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def alternate(candidates, calls, rounds, warmup):
    """{name: [ms per call, one per round]}; the candidates take turns within every round."""
    for fn in candidates.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in candidates}
    for _ in range(rounds):
        for name, fn in candidates.items():
            times[name].append(timed(fn, calls))
    return times


def fmt(ts, unit=1e3, what="us"):
    return f"{statistics.median(ts) * unit:9.1f} {what}  (min {min(ts) * unit:.1f}, max {max(ts) * unit:.1f})"


def bench_loss(shape, weights, say, calls, rounds):
    g = torch.Generator().manual_seed(1)
    t = torch.rand(shape, generator=g)
    p = (t + 0.05 * torch.randn(shape, generator=g)).to(DEV)
    t = t.to(DEV)
    # the network's output as the step sees it: channel 0 of a channels-last (N, 2, D, H, W) tensor
    net = torch.cat((p, torch.zeros_like(p)), 1).contiguous(memory_format=torch.channels_last_3d).requires_grad_()
    fused, plain = StructureLoss(*weights), TorchStructureLoss(*weights).to(DEV)

    def run(fn):
        def call():
            net.grad = None
            fn(net[:, 0:1], t).backward()
        return call

    run(fused)()
    gf, lf = net.grad.clone(), float(fused(net[:, 0:1], t).detach())
    run(plain)()
    gp, lp = net.grad.clone(), float(plain(net[:, 0:1], t).detach())
    times = alternate({"fused": run(fused), "torch": run(plain)}, calls, rounds, 5)
    fwd = alternate({"fused": lambda: fused(net[:, 0:1].detach(), t), "torch": lambda: plain(net[:, 0:1].detach(), t)},
                    calls, rounds, 5)
    view, go = net[:, 0:1].detach(), torch.ones(1, device=DEV)
    fields = hb.structure_loss_fwd(view, t, weights)[2]
    bwd = alternate({"fused": lambda: hb.structure_loss_bwd(view, t, weights, fields, go)}, calls, rounds, 5)
    V = p.numel()
    say(f"{tuple(shape)}, weights (l1, l2, ssim, sobel) = {weights}: {V} pixels, {8 * V / 1e6:.2f} MB of operands")
    say(f"  fused  forward + backward   {fmt(times['fused'])}")
    say(f"  torch  forward + backward   {fmt(times['torch'])}   "
        f"torch / fused {statistics.median(times['torch']) / statistics.median(times['fused']):.2f}")
    say(f"  fused  forward alone        {fmt(fwd['fused'])}")
    say(f"  torch  forward alone        {fmt(fwd['torch'])}   "
        f"torch / fused {statistics.median(fwd['torch']) / statistics.median(fwd['fused']):.2f}")
    say(f"  fused  backward alone       {fmt(bwd['fused'])}   (the launch layer; autograd adds the scatter of the "
        f"channel's gradient into the network output's)")
    say(f"  value fused {lf:.7f} torch {lp:.7f}; largest |gradient difference| {float((gf - gp).abs().max()):.3e} "
        f"of max |gradient| {float(gp.abs().max()):.3e}")


def bench_step(say, calls, rounds, batch):
    g = torch.Generator().manual_seed(0)
    x = torch.rand(batch, 2, 4, 96, 96, generator=g).to(DEV)
    hr = torch.rand(batch, 2, 16, 96, 96, generator=g)
    hr[:, 1:] = (hr[:, 1:] > 0.5).float()
    hr = hr.to(DEV)
    bd = BCEDiceLoss(1.0, 1.0)
    steps = {}
    for name, loss_obj in (("L1Loss", torch.nn.L1Loss()), ("StructureLoss", StructureLoss(l1=1.0, ssim=1.0, sobel=1.0))):
        torch.manual_seed(0)
        model = UNet_3D_3D(2, "unet_18", 4, 4, use_uncertainty=True).to(DEV)
        opt = torch.optim.Adam(model.parameters(), lr=5e-4, betas=(0.9, 0.99), fused=True)
        steps[name] = (lambda m=model, o=opt, l=loss_obj: train_sr_step(m, o, None, x.clone(), hr, l, bd, 4.0, 4, True))
    times = alternate(steps, calls, rounds, 3)
    say(f"train_sr_step, UNet_3D_3D(2, 'unet_18', 4, 4, use_uncertainty), {batch} x 2 x 4 x 96 x 96, fp32, Adam; the loss "
        f"object is applied twice per step (image pair, uncertainty pair)")
    for name in steps:
        say(f"  loss_obj = {name:14s} {fmt(times[name], 1.0, 'ms')}")
    d = statistics.median(times["StructureLoss"]) - statistics.median(times["L1Loss"])
    say(f"  StructureLoss(l1=1, ssim=1, sobel=1) - L1Loss: {d * 1e3:+.0f} us per step (difference of the medians)")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "structure_loss_bench.txt"))
    ap.add_argument("--calls", type=int, default=50, help="back-to-back calls per timed run of the loss")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--step-calls", type=int, default=5, help="train_sr_step calls per timed run")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_structure_loss.py measures on an MI355X; there is no device here")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"fused structure loss against its composition from torch ops, {torch.cuda.get_device_name(0)}; device events, "
        f"{args.calls} back-to-back calls per run, candidates alternating for {args.rounds} rounds, median (min, max)")
    for shape in ((32, 1, 4, 96, 96), (4, 1, 4, 32, 32)):
        for weights in ((1.0, 0.0, 1.0, 1.0), (1.0, 0.0, 0.0, 1.0)):
            bench_loss(shape, weights, say, args.calls, args.rounds)
    if not args.no_step:
        bench_step(say, args.step_calls, args.rounds, args.batch)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
