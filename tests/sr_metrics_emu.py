"""CPU statement of the stage-1 validation kernel of csrc/sr_metrics.hip (test only): rehr_sr_metrics_f32 / _bf16 in
numpy under the kernel's precision contract -- per-voxel terms, window moments and the index in fp32 (the horizontal
11-tap pass, then the vertical one, taps in ascending order; numpy rounds each product and each sum where the kernel
fuses them), every sum across voxels and positions in fp64.  Everything else is tests/emu_backend.py's; install it with
ops.set_backend()."""
import numpy as np
import torch

import emu_backend

name = "sr_metrics_emu"


def __getattr__(attr):
    return getattr(emu_backend, attr)


def _taps():
    e = np.exp(-((np.arange(11) - 5.0) ** 2) / (2.0 * 1.5 * 1.5))
    return (e / e.sum()).astype(np.float32)


def _window(f, g):
    """Valid 11-tap passes along the last axis, then the one before it, of the float32 array f."""
    H, W = f.shape[-2:]
    h = np.zeros(f.shape[:-1] + (W - 10,), np.float32)
    for k in range(11):
        h = h + g[k] * f[..., k:k + W - 10]
    v = np.zeros(f.shape[:-2] + (H - 10, W - 10), np.float32)
    for k in range(11):
        v = v + g[k] * h[..., k:k + H - 10, :]
    return v


def _ssim_index(p, t, data_range):
    """The window means mu_x, mu_y, the four factors and the index S = (A1 A2) / (B1 B2) on the valid positions of the
    last two axes, fp32: the statement of csrc/ssim_tile.h's ssim_index."""
    g = _taps()
    c1, c2 = np.float32(0.01) * np.float32(data_range), np.float32(0.03) * np.float32(data_range)
    C1, C2 = c1 * c1, c2 * c2
    mx, my, exx, eyy, exy = (_window(f, g) for f in (p, t, p * p, t * t, p * t))
    mxx, myy, mxy = mx * mx, my * my, mx * my
    sxx, syy, sxy = exx - mxx, eyy - myy, exy - mxy
    two = np.float32(2.0)
    A1, A2 = two * mxy + C1, two * sxy + C2
    B1, B2 = (mxx + myy) + C1, (sxx + syy) + C2
    S = (A1 * A2) / (B1 * B2)
    assert S.dtype == np.float32
    return mx, my, A1, A2, B1, B2, S


def sr_metrics(pred, target, seg_logits=None, seg_target=None, data_range=1.0):
    if pred.dtype not in (torch.float32, torch.bfloat16) or target.dtype != torch.float32:
        raise TypeError("pred: float32 or bfloat16 (widened at the load), target: float32")
    p, t = pred.float().numpy(), target.numpy()
    N, D, H, W = p.shape
    out = np.zeros((N, 7), np.float64)
    e = p - t
    out[:, 0] = np.abs(e).astype(np.float64).sum((1, 2, 3))
    out[:, 1] = (e * e).astype(np.float64).sum((1, 2, 3))
    out[:, 2] = _ssim_index(p, t, data_range)[-1].astype(np.float64).sum((1, 2, 3))
    out[:, 3] = D * (H - 10) * (W - 10)
    if seg_logits is not None:
        fp, ft = seg_logits.float().numpy() > 0, seg_target.numpy() > 0.5
        out[:, 4] = (fp & ft).sum((1, 2, 3))
        out[:, 5] = fp.sum((1, 2, 3))
        out[:, 6] = ft.sum((1, 2, 3))
    return torch.from_numpy(out)
