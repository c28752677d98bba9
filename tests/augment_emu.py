"""CPU emulation of the augmentation kernels of csrc/augment.hip and of rehr_axis_resample_f32 over the host tap
tables of rehrseg_amd/utils/augment.py (test only): the same tables, the same arithmetic order, numpy float64."""
import numpy as np

from rehrseg_amd.utils import augment as A


def resample(x, axis, m):
    """rehr_axis_resample_f32 with the fp32 tap table of the dense operator m."""
    idx, w = A.dense_to_taps(m)
    x = np.moveaxis(np.asarray(x, np.float64), axis, -1)
    y = np.zeros(x.shape[:-1] + (idx.shape[0],))
    for t in range(idx.shape[1]):
        ok = idx[:, t] >= 0
        y[..., ok] += w[ok, t].astype(np.float64) * x[..., idx[ok, t]]
    return np.moveaxis(y, -1, axis).astype(np.float32)


def _coords(params, in_hw, out_hw):
    p0, p1 = np.meshgrid(np.arange(out_hw[0]) - (out_hw[0] - 1) / 2.0, np.arange(out_hw[1]) - (out_hw[1] - 1) / 2.0,
                         indexing="ij")
    r00, r01, r10, r11, s, c0, c1 = params[:7]
    return (p0 * r00 + p1 * r10) * s + c0, (p0 * r01 + p1 * r11) * s + c1


def warp(src, params, out_hw, label):
    """rehr_aug_warp2d_f32 for one item: src (C, Hi, Wi) (coefficients for the spline mode)."""
    C, Hi, Wi = src.shape
    y, x = _coords(params, (Hi, Wi), out_hw)
    inside = (y >= 0) & (y <= Hi - 1) & (x >= 0) & (x <= Wi - 1)
    fy, fx = np.floor(y).astype(int), np.floor(x).astype(int)
    mi = np.vectorize(A._mirror)
    out = np.zeros((C,) + tuple(out_hw))
    if not label:
        b3 = np.vectorize(A._bspline3)
        for a in range(4):
            wy, ry = b3(y - (fy + a - 1)), mi(fy + a - 1, Hi)
            for e in range(4):
                wx, rx = b3(x - (fx + e - 1)), mi(fx + e - 1, Wi)
                out += (wy * wx)[None] * src[:, ry, rx]
        return np.where(inside[None], out, 0).astype(np.float32)
    ty, tx = y - fy, x - fx
    labs = [src[:, mi(fy + a, Hi), mi(fx + e, Wi)] for a in range(2) for e in range(2)]
    ws = [(1 - ty if a == 0 else ty) * (1 - tx if e == 0 else tx) for a in range(2) for e in range(2)]
    best = np.full(out.shape, -np.inf)
    for k in range(4):
        ind = sum(np.where(labs[m] == labs[k], ws[m][None], 0.0) for m in range(4))
        best = np.where((ind >= 0.5) & (labs[k] > best), labs[k], best)
    return np.where(inside[None] & np.isfinite(best), best, 0).astype(np.float32)


def spatial(img, params, out_hw):
    """prefilter along x then y (rehr_axis_resample_f32), then the spline warp."""
    C, Hi, Wi = img.shape
    c = resample(resample(img, 2, A.prefilter_matrix(Wi)), 1, A.prefilter_matrix(Hi))
    return warp(c, params, out_hw, False)


def blur(x, sigma):
    for axis in range(x.ndim):
        x = resample(x, axis, A.gaussian_matrix(x.shape[axis], sigma))
    return x


def lowres(x, zoom):
    tgt = A.lowres_shape(x.shape, zoom)
    down = x
    for axis in (1, 2):
        down = resample(down, axis, A.zoom_nearest_matrix(x.shape[axis], tgt[axis]))
    up = down
    for axis in (1, 2):
        up = resample(up, axis, A.zoom_cubic_matrix(tgt[axis], x.shape[axis]))
    return np.clip(up, down.min(), down.max())
