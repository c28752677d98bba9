"""The top-k cross-entropy + Dice loss forward + backward on the device (GPU box).

    python tools/bench_topk_loss.py [--json out.json] [--rounds 7] [--out profiles/topk_loss_bench.txt]

Shapes (batch, classes, z, y, x): the reference's stage-2 lattice 2 x 2 x 16 x 320 x 384 without and with an
uncertainty map (the loss map is then 2 x 2 x S), and the HR logits 2 x 2 x 128^3.  Per shape three losses, value and
logit gradient each call (HIP events on the launch stream, 10 calls after 3 warm-ups, alternating within every round so
that drifting clocks hit all of them alike):

  fused_topk     DC_and_topk_loss(k=10) through its fused node: rehr_seg_topk_{fwd,bwd}_f32
  fused_plain    DC_and_weighted_CE_loss through its fused node (rehr_seg_loss_{fwd,bwd}_f32): what selection adds
  torch_topk     DC_and_topk_loss's torch composition on the device (softmax, loss map, torch.topk, scatter): what a
                 user would otherwise write

and the forward's and backward's halves of fused_topk through the launch layer.  Per row: the median over the rounds,
the smallest and largest round, and for the fused rows the algorithmic bytes (every operand read or written once per
pass that touches it) with the resulting share of the 8 TB/s spec peak of MI355X_MICROARCH.md.  Before timing, the fused
value is compared with the torch composition's on the same inputs."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from rehrseg_amd import hip_backend as hb  # noqa: E402
from rehrseg_amd import ops  # noqa: E402
from rehrseg_amd.utils import seg_utils as su  # noqa: E402

dev = torch.device("cuda:0")
CASES = [("stage2", (2, 2, 16, 320, 384), False), ("stage2+unc", (2, 2, 16, 320, 384), True),
         ("hr128", (2, 2, 128, 128, 128), False)]
K_PERCENT = 10


def timed(fn, reps=10):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


def topk_bytes(N, C, S, with_unc):
    """(forward, backward) bytes: the logits pass (logits, labels, uncertainty in; the map out), five reads of the map
    by the select (four histogram passes, of which the later ones read every element and count few) and the count pass;
    backward the logits pass again with the map in and the gradient out."""
    M = (N * N if with_unc else N) * S
    voxel_in = N * S * (4 * C + 4) + (N * S * 4 if with_unc else 0)
    return voxel_in + 4 * M + 5 * 4 * M, voxel_in + 4 * M + N * S * 4 * C


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    lines, rows = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for name, shape, with_unc in CASES:
        N, C, D, H, W = shape
        S = D * H * W
        g = torch.Generator(device="cpu").manual_seed(0)
        logits = ops.to_cl((torch.randn(shape, generator=g) * 2).to(dev)).requires_grad_(True)
        target = torch.randint(0, C, (N, 1, D, H, W), generator=g).float().to(dev)
        unc = (1 - torch.rand((N, 1, D, H, W), generator=g) * 0.99).to(dev) if with_unc else None
        topk, plain = su._build_loss(topk=K_PERCENT), su._build_loss()
        M = (N * N if with_unc else N) * S
        K = int(M * K_PERCENT / 100)

        def torch_topk():
            x = logits
            ce = topk.ce(x, target[:, 0], unc)
            return ce + topk.dc(x, target)

        def fwd_bwd(loss_fn):
            def run():
                logits.grad = None
                loss_fn().backward()
            return run

        a, b = topk(logits, target, unc), torch_topk()
        assert type(a.grad_fn).__name__ == "_FusedDCTopKBackward" and type(b.grad_fn).__name__ != "_FusedDCTopKBackward"
        say(f"{name}: {shape} uncertainty={with_unc}  M={M} K={K}  fused value {float(a):.7f}  torch value {float(b):.7f}")
        assert abs(float(a) - float(b)) <= 1e-4 * abs(float(b))
        t2, u2 = target.reshape(N, S), (None if unc is None else unc.reshape(N, S))
        lg = logits.detach()
        stats, ws = hb.seg_topk_fwd(lg, t2, u2, K)
        go = torch.ones(1, device=dev)
        fb, bb = topk_bytes(N, C, S, with_unc)
        calls = {
            "fused_topk": (fb + bb, fwd_bwd(lambda: topk(logits, target, unc))),
            "fused_plain": (2 * (N * S * (4 * C + 4) + (N * S * 4 if with_unc else 0)) + N * S * 4 * C,
                            fwd_bwd(lambda: plain(logits, target, unc))),
            "torch_topk": (None, fwd_bwd(torch_topk)),
            "topk_fwd_only": (fb, lambda: hb.seg_topk_fwd(lg, t2, u2, K, ws)),
            "topk_bwd_only": (bb, lambda: hb.seg_topk_bwd(lg, t2, u2, K, stats, ws, 1.0, 1.0, 1e-5, False, go)),
            "select_only": (5 * 4 * M, lambda: hb.order_stats(hb.seg_topk_map(ws, N, S, with_unc).view(1, M), [M - K])),
        }
        times = {k: [] for k in calls}
        for _ in range(args.rounds):
            for k, (_, fn) in calls.items():
                times[k].append(timed(fn))
        med = {k: statistics.median(v) for k, v in times.items()}
        for k, (nbytes, _) in calls.items():
            t = med[k]
            extra = "" if nbytes is None else f"  {nbytes / 1e6:7.1f} MB  {nbytes / t / 1e12:5.2f} TB/s ({nbytes / t / 8e12:5.1%} of 8 TB/s)"
            say(f"  {k:14s} {t * 1e6:9.1f} us (rounds {min(times[k]) * 1e6:.1f} .. {max(times[k]) * 1e6:.1f}){extra}")
            rows.append({"case": name, "call": k, "us_median": t * 1e6, "us_min": min(times[k]) * 1e6,
                         "us_max": max(times[k]) * 1e6, "algorithmic_bytes": nbytes})
        say(f"  fused_topk / fused_plain = {med['fused_topk'] / med['fused_plain']:.2f}    "
            f"torch_topk / fused_topk = {med['torch_topk'] / med['fused_topk']:.2f}")
        del logits, target, unc, stats, ws
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if args.json:
        json.dump({"k_percent": K_PERCENT, "rounds": args.rounds, "rows": rows}, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
