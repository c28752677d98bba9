"""CPU statement of the stage-1 volume preparation kernels of csrc/stage1_volume.hip (test only): the contracts of
rehr_zoom_depth_f32, rehr_bspline_prefilter_axis_f64acc_f32 and rehr_blur_to_slices_f32 in numpy with the same fp64 /
fp32 operations in the same order, one rounding each -- except the blur, where the kernel fuses each product into its
sum (fmaf) and numpy rounds both.  Everything else is tests/emu_backend.py's; install it with ops.set_backend()."""
import math

import numpy as np
import torch

import emu_backend

name = "stage1_emu"


def __getattr__(attr):
    return getattr(emu_backend, attr)


def prefilter_lines(x):
    """ndimage's cubic spline filter with mirror boundaries along the LAST axis of the float64 array x (ni_splines.c:
    apply_filter, _init_causal_mirror, _init_anticausal_mirror), operation for operation."""
    n = x.shape[-1]
    if n < 2:
        return x.copy()
    z = math.sqrt(3.0) - 2.0
    c = x * ((1.0 - z) * (1.0 - 1.0 / z))
    zn1 = math.pow(z, n - 1)
    v = c[..., 0] + zn1 * c[..., n - 1]
    zi = z
    for i in range(1, n - 1):
        v = v + zi * (c[..., i] + zn1 * c[..., n - 1 - i])
        zi = zi * z
    v = v / (1.0 - zn1 * zn1)
    c[..., 0] = v
    for i in range(1, n):
        v = c[..., i] + z * v
        c[..., i] = v
    v = ((z * c[..., n - 2] + v) * z) / (z * z - 1.0)
    c[..., n - 1] = v
    for i in range(n - 2, -1, -1):
        v = z * (v - c[..., i])
        c[..., i] = v
    return c


def zoom_depth(vol, idx, w, nn):
    v = vol.numpy()
    idx, w, nn = idx.numpy(), w.numpy(), nn.numpy()
    n = v.shape[2]
    c = prefilter_lines(v[..., 0].astype(np.float64))
    ix = np.clip(idx, 0, n - 1)
    t = np.zeros(v.shape[:2] + (idx.shape[0],), np.float64)
    for q in range(4):
        t = t + c[..., ix[:, q]] * w[:, q]
    img = torch.from_numpy(t.astype(np.float32))
    if v.shape[3] == 1:
        return img, None
    lab = v[..., 1][..., np.clip(nn, 0, n - 1)].astype(np.int32).astype(np.uint8)
    lab[..., nn < 0] = 0
    return img, torch.from_numpy(np.ascontiguousarray(lab))


def bspline_prefilter(x, axis):
    a = np.moveaxis(x.numpy().astype(np.float64), axis, -1)
    return torch.from_numpy(np.ascontiguousarray(np.moveaxis(prefilter_lines(a), -1, axis).astype(np.float32)))


def blur_to_slices(img, taps, axis):
    a, k = img.numpy(), taps.numpy()
    A, L = a.shape[axis], k.shape[0]
    left = (L - 1) // 2
    a = np.moveaxis(a, axis, 0)                        # (a, b, z)
    out = np.zeros_like(a)
    for t in range(L):                                 # ascending taps
        lo, hi = max(0, left - t), min(A, A + left - t)
        if hi > lo:
            out[lo:hi] = out[lo:hi] + k[t] * a[lo + t - left:hi + t - left]
    return torch.from_numpy(np.ascontiguousarray(out.transpose(2, 0, 1)))
