"""CPU statement of the boundary-metric calls of csrc/seg_surface.hip (test only): the contracts of
rehr_seg_surface_dist_f32 and rehr_seg_surface_reduce_f64 -- surface bits and counts, three separable min-plus passes
W, H, D, the gather into the 2 x N distance buffer, and the reduction from its ascending sort.  The fields and
distances are fp64 here, the definition in exact terms (for spacings whose squares fp64 holds exactly), so that the
host logic above the calls can be pinned to 1e-12; the kernels' fp32 rounding is checked on the device against
tests/surface_oracle.py.  Everything else is tests/eval_emu.py's; install it with ops.set_backend()."""
import numpy as np
import torch

import eval_emu

name = "surface_emu"


def __getattr__(attr):
    return getattr(eval_emu, attr)


def _surface_bits(m):
    """Foreground voxels with fewer than six foreground face neighbours inside the volume."""
    m = m != 0
    n = np.zeros(m.shape, np.int32)
    for ax in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        n[tuple(lo)] += m[tuple(hi)]
        n[tuple(hi)] += m[tuple(lo)]
    return m & (n < 6)


def _min_plus(f, axis, s):
    """out[i] = min_j (f[j] + ((i - j) * s)^2) along `axis`."""
    n = f.shape[axis]
    f = np.moveaxis(f, axis, -1)
    idx = np.arange(n, dtype=np.float64)
    t = (idx[:, None] - idx[None, :]) * s
    out = (f[..., None, :] + t * t).min(-1)
    return np.moveaxis(out, -1, axis)


def seg_surface_distances(pred, gt, spacing, counts, workspace=None):
    sd, sh, sw = (float(np.float32(s)) for s in spacing)
    bits = [_surface_bits(pred.numpy()), _surface_bits(gt.numpy())]
    fields = []
    for b in bits:
        f = np.where(b, 0.0, np.inf)
        for axis, s in ((2, sw), (1, sh), (0, sd)):
            f = _min_plus(f, axis, s)
        fields.append(np.sqrt(f))
    dist = np.stack([np.where(bits[0], fields[1], np.inf), np.where(bits[1], fields[0], np.inf)]).reshape(2, -1)
    counts[0] += int(bits[0].sum())
    counts[1] += int(bits[1].sum())
    return torch.from_numpy(dist), None


def seg_surface_reduce(dist, dist_sorted, counts, out, workspace):
    n_p, n_g = int(counts[0]), int(counts[1])
    if n_p == 0 or n_g == 0:
        res = [float("nan")] * 3
    else:
        n = n_p + n_g
        v = dist_sorted.double().numpy()
        h = 0.95 * (n - 1)
        k0 = int(np.floor(h))
        t = h - k0
        a, b = v[k0], v[min(k0 + 1, n - 1)]
        hd95 = b - (b - a) * (1.0 - t) if t >= 0.5 else a + (b - a) * t      # numpy's lerp
        d = dist.double()
        sums = [float(row[torch.isfinite(row)].sum()) for row in d]
        res = [v[n - 1], hd95, (sums[0] / n_p + sums[1] / n_g) / 2.0]
    out.copy_(torch.tensor(res, dtype=torch.float64).view(torch.int64))
