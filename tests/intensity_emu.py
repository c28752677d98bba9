"""CPU statement of the intensity-normalisation calls of csrc/intensity_norm.hip (test only): the contracts of
rehr_order_stats_f32 (the same MSD radix select over the order-preserving key, four digits of 8 bits, with numpy's
bincount standing for the histograms), rehr_percentile_f64, rehr_intensity_apply_f32 and rehr_aug_stats_f32 over CPU
tensors.  Everything else is tests/components_emu.py's; install it with ops.set_backend()."""
import numpy as np
import torch

import components_emu

name = "intensity_emu"
INTENSITY_PERCENTILE, INTENSITY_ZEROONE = 0, 1


def __getattr__(attr):
    return getattr(components_emu, attr)


def _items(x):
    """The items of a (B, ...) CPU tensor as flat float32 numpy views (each item is a dense run)."""
    assert x.dtype == torch.float32 and x[0].is_contiguous()
    return [x[b].view(-1).numpy() for b in range(x.shape[0])]


def _select(v, k):
    u = v.view(np.uint32)
    keys = np.where(u >> 31 != 0, ~u, u ^ np.uint32(0x80000000)).astype(np.uint32)
    prefix = 0
    for p in range(4):
        live = keys if p == 0 else keys[(keys >> np.uint32(32 - 8 * p)) == prefix]
        counts = np.bincount((live >> np.uint32(24 - 8 * p)) & np.uint32(0xff), minlength=256)
        incl = np.cumsum(counts)
        d = int(np.searchsorted(incl, k, side="right"))
        k -= int(incl[d] - counts[d])
        prefix = (prefix << 8) | d
    key = np.array([prefix], dtype=np.uint32)
    return np.where(key >> 31 != 0, key ^ np.uint32(0x80000000), ~key).astype(np.uint32).view(np.float32)[0]


def order_stats(x, ranks, out=None, workspace=None):
    rows = []
    for v in _items(x):
        assert all(0 <= int(k) < v.size for k in ranks) and 1 <= len(ranks) <= 8
        rows.append([np.float32(np.nan)] * len(ranks) if np.isnan(v).any() else [_select(v, int(k)) for k in ranks])
    res = torch.from_numpy(np.array(rows, dtype=np.float32))
    if out is not None:
        out.copy_(res)
        return out
    return res


def percentile_bounds(stats, t, strictly_positive=False, out=None):
    st = stats.numpy()
    res = np.empty((st.shape[0], len(t)), np.float64)
    for b in range(st.shape[0]):
        for j, tj in enumerate(t):
            lo, hi = float(st[b, 2 * j]), float(st[b, 2 * j + 1])
            d = hi - lo
            v = hi - d * (1.0 - tj) if tj >= 0.5 else lo + d * tj
            res[b, j] = 0.0 if (j == 0 and strictly_positive and v < 0) else v
    res = torch.from_numpy(res)
    if out is not None:
        out.copy_(res)
        return out
    return res


def intensity_apply(x, bounds, mode, out=None):
    B, S = x.shape[0], x[0].numel()
    if out is None:
        out = torch.empty((B, S), dtype=torch.float32)
    dst = _items(x) if out is x else _items(out.view(B, S))
    for b, (src, d) in enumerate(zip(_items(x), dst)):
        lo, hi = np.float32(float(bounds[b, 0])), np.float32(float(bounds[b, 1]))
        with np.errstate(all="ignore"):
            v = np.minimum(np.maximum(src, lo), hi) if mode == INTENSITY_PERCENTILE else src
            d[:] = (v - lo) / (hi - lo)
    return out


def aug_stats(x, out=None):
    rows = []
    for v in _items(x):
        d = v.astype(np.float64)
        rows.append([d.sum(), (d * d).sum(), np.fmin.reduce(v), np.fmax.reduce(v)])
    res = torch.from_numpy(np.array(rows, dtype=np.float64))
    if out is not None:
        out.copy_(res)
        return out
    return res
