"""CPU statement of the stage-1 structure-loss kernels of csrc/sr_losses.hip (test only): rehr_structure_loss_fwd_f32 /
_bwd_f32 in numpy under the kernels' precision contract -- per-pixel terms, window moments, the index, the three SSIM
coefficient fields and the gradient in fp32 (11-tap passes horizontal first, taps in ascending order; numpy rounds each
product and each sum where the kernel fuses them), every sum across pixels in fp64.  The backward pass of the Sobel term
is written in scatter form here (every position hands its nine taps to the clamped neighbours), the kernel gathers.
Everything else is tests/emu_backend.py's; install it with ops.set_backend()."""
import numpy as np
import torch

import emu_backend
from sr_metrics_emu import _ssim_index, _taps

name = "structure_loss_emu"
F32 = np.float32


def __getattr__(attr):
    return getattr(emu_backend, attr)


def _operands(input, target, weights):
    for t in (input, target):
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise TypeError("structure loss: float32 tensors")
    if input.dim() not in (4, 5) or input.shape != target.shape:
        raise ValueError("structure loss: input and target of one shape (N, C, D, H, W) or (N, C, H, W)")
    p, t = input.detach().numpy(), target.detach().numpy()
    if p.ndim == 4:
        p, t = p[:, :, None], t[:, :, None]
    weights = tuple(float(w) for w in weights)
    if weights[2] != 0 and (p.shape[-2] < 11 or p.shape[-1] < 11):
        raise ValueError("structure loss: the SSIM term needs H, W >= 11")
    return p, t, weights


def _sobel(f):
    """gx, gy, G of the float32 array f over its last two axes, replicate padding."""
    q = np.pad(f, [(0, 0)] * (f.ndim - 2) + [(1, 1), (1, 1)], mode="edge")
    H, W = f.shape[-2:]
    a, b, c = q[..., 0:H, 0:W], q[..., 0:H, 1:W + 1], q[..., 0:H, 2:W + 2]
    d, e = q[..., 1:H + 1, 0:W], q[..., 1:H + 1, 2:W + 2]
    g, h, k = q[..., 2:H + 2, 0:W], q[..., 2:H + 2, 1:W + 1], q[..., 2:H + 2, 2:W + 2]
    gx = (((c - a) + F32(2) * (e - d)) + (k - g)) * F32(0.125)
    gy = (((g - a) + F32(2) * (h - b)) + (k - c)) * F32(0.125)
    return gx, gy, np.sqrt((gx * gx + gy * gy) + F32(1e-6))


def _ssim_fields(p, t, data_range):
    """S and the coefficient fields a = dS/dmu_x, b = dS/dE[x^2], c = dS/dE[xy] on the valid positions, fp32."""
    mx, my, A1, A2, B1, B2, S = _ssim_index(p, t, data_range)
    two, one = F32(2), F32(1)
    inv = one / (B1 * B2)
    a = (two * my) * (A2 - A1) * inv - (two * mx) * S * (one / B1 - one / B2)
    b = -S / B2
    c = (two * A1) * inv
    assert S.dtype == a.dtype == b.dtype == c.dtype == np.float32
    return S, np.stack((a, b, c), 3)          # (N, C, D, 3, H - 10, W - 10)


def structure_loss_fwd(input, target, weights, data_range=1.0, need_grad=True):
    p, t, (l1, l2, ssim, sobel) = _operands(input, target, weights)
    N, C, D, H, W = p.shape
    V, M = float(p.size), float(N * C * D * (H - 10) * (W - 10))
    stats = np.zeros((N, 4), np.float64)
    e = p - t
    ax = (1, 2, 3, 4)
    if l1 != 0:
        stats[:, 0] = np.abs(e).astype(np.float64).sum(ax)
    if l2 != 0:
        stats[:, 1] = (e * e).astype(np.float64).sum(ax)
    fields = None
    if ssim != 0:
        S, abc = _ssim_fields(p, t, data_range)
        stats[:, 2] = S.astype(np.float64).sum(ax)
        if need_grad:
            fields = np.zeros((N, C, D, 3, H, W), np.float32)
            fields[..., 5:H - 5, 5:W - 5] = abc
            fields = torch.from_numpy(fields)
    if sobel != 0:
        stats[:, 3] = np.abs(_sobel(p)[2] - _sobel(t)[2]).astype(np.float64).sum(ax)
    s = stats.sum(0)
    loss = 0.0
    if l1 != 0:
        loss += l1 / V * s[0]
    if l2 != 0:
        loss += l2 / V * s[1]
    if ssim != 0:
        loss += ssim * (1.0 - s[2] / M)
    if sobel != 0:
        loss += sobel / V * s[3]
    return torch.tensor(loss, dtype=torch.float32), torch.from_numpy(stats), fields


def _same(f, g):
    """11-tap passes along the last axis, then the one before it, zero outside: the size of f."""
    H, W = f.shape[-2:]
    q = np.pad(f, [(0, 0)] * (f.ndim - 2) + [(5, 5), (5, 5)])
    h = np.zeros(q.shape[:-1] + (W,), np.float32)
    for k in range(11):
        h = h + g[k] * q[..., k:k + W]
    v = np.zeros(f.shape, np.float32)
    for k in range(11):
        v = v + g[k] * h[..., k:k + H, :]
    return v


def structure_loss_bwd(input, target, weights, fields, grad_out, out=None):
    p, t, (l1, l2, ssim, sobel) = _operands(input, target, weights)
    N, C, D, H, W = p.shape
    V, M = float(p.size), float(N * C * D * (H - 10) * (W - 10))
    e = p - t
    g = np.zeros(p.shape, np.float32)
    if l1 != 0:
        g = g + F32(l1 / V) * np.sign(e)
    if l2 != 0:
        g = g + F32(2.0 * l2 / V) * e
    if ssim != 0:
        f = fields.numpy()
        taps = _taps()
        wa, wb, wc = (_same(f[:, :, :, k], taps) for k in range(3))
        g = g + F32(-ssim / M) * ((wa + (F32(2) * p) * wb) + t * wc)
    if sobel != 0:
        gx, gy, gp = _sobel(p)
        s = np.sign(gp - _sobel(t)[2])
        ux, uy = s * gx / gp, s * gy / gp
        acc = np.zeros(p.shape, np.float32)
        ys, xs = np.arange(H), np.arange(W)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                kx, ky = F32((2 - abs(dy)) * dx), F32((2 - abs(dx)) * dy)
                yy, xx = np.clip(ys + dy, 0, H - 1), np.clip(xs + dx, 0, W - 1)
                np.add.at(acc, (Ellipsis, yy[:, None], xx[None, :]), ux * kx + uy * ky)
        g = g + F32(sobel / V) * (acc * F32(0.125))
    g = torch.from_numpy(grad_out.reshape(()).numpy() * g).reshape(input.shape)
    if out is not None:
        out.copy_(g)
        return out
    return g
