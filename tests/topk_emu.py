"""CPU statement of hip_backend.seg_topk_fwd / seg_topk_bwd (csrc/seg_loss_topk.hip) for host-logic tests: the same
statistics vector, a workspace that carries the loss map to the backward, the threshold and the tie weight read from
the statistics as the device does.  Everything else is tests/emu_backend.py's; install it with ops.set_backend().
`seg_topk_on_host` lets DC_and_topk_loss take its fused node on CPU tensors while this backend is installed."""
import torch

import emu_backend

name = "topk_emu"
seg_topk_on_host = True
SEG_TOPK_STATS = 4
calls = []          # ("fwd" | "bwd", N, C, S, K, with_unc) per call, for the tests that count launches


def __getattr__(attr):
    return getattr(emu_backend, attr)


def _softmax_ce(logits, target):
    N, C = logits.shape[:2]
    x = logits.reshape(N, C, -1)
    p = torch.softmax(x, 1)
    y = torch.zeros_like(p).scatter_(1, target.long().view(N, 1, -1), 1.0)
    ce = -(torch.log_softmax(x, 1) * y).sum(1)
    return p, y, ce


def seg_topk_fwd(logits, target, unc, K, workspace=None):
    N, C = logits.shape[:2]
    S = logits[0, 0].numel()
    assert tuple(target.shape) == (N, S) and (unc is None or tuple(unc.shape) == (N, S)) and 2 <= C <= 4 and N <= 4
    p, y, ce = _softmax_ce(logits, target)
    m = ce if unc is None else unc.to(ce.dtype)[:, None, :] * ce[None, :, :]       # m[a][b][v] = ce[b][v] * u[a][v]
    m = torch.where(m == 0, torch.zeros_like(m), m)                                # zeros enter as +0
    M = m.numel()
    assert 1 <= K <= M
    flat = m.reshape(-1)
    t = torch.sort(flat).values[M - K] if not torch.isnan(flat).any() else flat.new_tensor(float("nan"))
    stats = torch.zeros(N * C * 3 + 1 + SEG_TOPK_STATS, dtype=torch.float64)
    stats[:N * C * 3] = torch.stack([(p * y).sum(2), p.sum(2), y.sum(2)], -1).double().reshape(-1)
    stats[N * C * 3] = (ce.sum(0) * (unc.sum(0) if unc is not None else 1.0)).sum().double()
    stats[N * C * 3 + 1:] = torch.stack([(flat > t).sum().double(), (flat == t).sum().double(),
                                         flat[flat > t].double().sum(), t.double()])
    calls.append(("fwd", N, C, S, K, unc is not None))
    return stats, m.contiguous()


def seg_topk_bwd(logits, target, unc, K, stats, workspace, w_ce, w_dice, smooth, do_bg, grad_out):
    N, C = logits.shape[:2]
    S = logits[0, 0].numel()
    p, y, _ = _softmax_ce(logits, target)
    n_gt, n_eq, _, t = stats[N * C * 3 + 1:].tolist()
    m = workspace
    wtie = (K - n_gt) / n_eq if n_eq > 0 else 0.0
    w = (m > t).to(p.dtype) + (m == t).to(p.dtype) * wtie
    cw = (w if unc is None else (w * unc.to(p.dtype)[:, None, :]).sum(0)) * (w_ce / K)       # (N, S)
    ipg = stats[:N * C * 3].view(N, C, 3)
    I, P, G = ipg[..., 0], ipg[..., 1], ipg[..., 2]
    raw = G + P + smooth
    den = raw.clamp_min(1e-8)
    ncls = C if do_bg else C - 1
    kd = w_dice / (N * ncls)
    on = torch.ones(C, dtype=torch.float64) if do_bg else torch.tensor([0.0] + [1.0] * (C - 1), dtype=torch.float64)
    A = (-kd * 2.0 / den * on).to(p.dtype)[:, :, None]
    B = (kd * (2.0 * I + smooth) / (den * den) * on * (raw >= 1e-8)).to(p.dtype)[:, :, None]
    g = y * A + B
    dot = (g * p).sum(1, keepdim=True)
    dl = grad_out.to(p.dtype).reshape(()) * (cw[:, None, :] * (p - y) + p * (g - dot))
    calls.append(("bwd", N, C, S, K, unc is not None))
    out = torch.empty_like(logits)
    out.copy_(dl.view(logits.shape))
    return out
