"""CPU statement of the stage-1 -> stage-2 handoff kernels of csrc/sr_volume.hip (test only): the contracts of
rehr_minmax_f32, rehr_sr_window_gather_f32, rehr_sr_volume_scatter_f32, rehr_stage2_prep_f32 and
rehr_stage2_unc_u8_f32 in torch on the CPU with the same fp32 operations, one rounding each.  Everything else
(the network's kernels) is tests/emu_backend.py's; install it with ops.set_backend()."""
import torch

import emu_backend

name = "handoff_emu"


def __getattr__(attr):
    return getattr(emu_backend, attr)


def _encode(f):
    u = f.contiguous().view(torch.int32)
    return torch.where(u < 0, ~u, u | -0x80000000)


def minmax_new(device, pairs=1):
    return torch.tensor([-1, 0] * pairs, dtype=torch.int32)


def minmax_decode(mm):
    return torch.where(mm < 0, mm & 0x7FFFFFFF, ~mm).view(torch.float32)


def _fold(mm, x):
    """atomicMin / atomicMax on the codes, which order as unsigned integers"""
    old = minmax_decode(mm)
    empty = int(mm[0]) == -1 and int(mm[1]) == 0
    lo, hi = x.min(), x.max()
    if not empty:
        lo, hi = torch.minimum(lo, old[0]), torch.maximum(hi, old[1])
    mm.copy_(_encode(torch.stack([lo, hi])))


def minmax(x, out=None):
    out = minmax_new(x.device) if out is None else out
    _fold(out, x.float())
    return out


def sr_window_gather(vol, w0, b):
    X, Y, Z, C = vol.shape
    Xp, Yp = X + (-X) % 16, Y + (-Y) % 16
    out = torch.zeros((b, 4, Xp, Yp, C), dtype=torch.float32)
    zoff = -2 if Z == 2 else -1
    for bi in range(b):
        for s in range(4):
            z = w0 + bi + zoff + s
            if 0 <= z < Z:
                out[bi, s, :X, :Y] = vol[:, :, z]
    return out.permute(0, 4, 1, 2, 3)


def sr_volume_scatter(net, in_minmax, w0, img, seg, out_minmax):
    b, C, n_out = net.shape[:3]
    Zo, Y, X = img.shape
    lo, hi = minmax_decode(in_minmax)
    v = net[:, :, :, :X, :Y].float() * (hi - lo)      # two roundings: the product, then the sum
    v = v + lo
    v = v.permute(1, 0, 2, 4, 3).reshape(C, b * n_out, Y, X)
    sl = slice(w0 * n_out, (w0 + b) * n_out)
    img[sl] = v[0]
    if seg is not None:
        seg[sl] = (v[1] > 0).to(torch.uint8)
    _fold(out_minmax, v[0])


def _norm255(v, mm):
    lo, hi = minmax_decode(mm)
    return ((v - lo) / (hi - lo)) * 255.0


def stage2_prep(img, minmax_codes, taps):
    n = _norm255(img, minmax_codes)
    X, L = img.shape[0], taps.numel()
    left = (L - 1) // 2
    out = torch.zeros_like(n)
    for t in range(L):                                 # ascending taps, product and sum rounded separately
        a, b = max(0, left - t), min(X, X + left - t)  # output rows whose source row x + t - left is inside the axis
        if b > a:
            out[a:b] = out[a:b] + taps[t] * n[a + t - left:b + t - left]
    return out


def stage2_unc_u8(u, minmax_codes):
    q = _norm255(u, minmax_codes) * 255.0
    return (q.to(torch.int32) & 0xFF).to(torch.uint8)
