"""CPU statement of the connected-component calls of csrc/seg_components.hip (test only): the contracts of
rehr_seg_cc_roots_i32, rehr_seg_cc_compact_i32 and rehr_seg_cc_lesion_i64 in numpy, without scipy -- the root map as
the fixed point of "take the smallest index among yourself and your neighbours", the labels from the prefix sum of
(roots[v] == v), the eight integers from arrays indexed by root and the packed key of the largest component.
Everything else is tests/surface_emu.py's; install it with ops.set_backend()."""
import itertools

import numpy as np
import torch

import surface_emu

name = "components_emu"


def __getattr__(attr):
    return getattr(surface_emu, attr)


def _offsets(connectivity):
    most = {6: 1, 18: 2, 26: 3}[connectivity]
    return [o for o in itertools.product((-1, 0, 1), repeat=3) if 0 < sum(v != 0 for v in o) <= most]


def _shifted(a, off, fill):
    """b[v] = a[v + off], `fill` where v + off is outside the volume (no wrap-around)."""
    b = np.full_like(a, fill)
    src = tuple(slice(max(o, 0), n + min(o, 0)) for o, n in zip(off, a.shape))
    dst = tuple(slice(max(-o, 0), n + min(-o, 0)) for o, n in zip(off, a.shape))
    b[dst] = a[src]
    return b


def seg_cc_roots(mask, connectivity, workspace=None):
    m = mask.numpy() != 0
    big = m.size
    r = np.where(m, np.arange(m.size, dtype=np.int64).reshape(m.shape), big)
    offs = _offsets(connectivity)
    while True:
        new = r
        for off in offs:
            new = np.minimum(new, _shifted(r, off, big))
        new = np.where(m, new, big)
        if np.array_equal(new, r):
            break
        r = new
    return torch.from_numpy(np.where(m, r, -1).astype(np.int32)), workspace


def seg_cc_compact(roots, count):
    r = roots.numpy().ravel()
    rank = np.cumsum(r == np.arange(r.size), dtype=np.int32)
    count[0] += int(rank[-1])
    return torch.from_numpy(np.where(r >= 0, rank[np.maximum(r, 0)], 0).astype(np.int32).reshape(roots.shape))


def _key(sizes):
    """max over the components of (size << 32) | (0xffffffff - root); 0 without one."""
    at = np.flatnonzero(sizes)
    return int(((sizes[at] << 32) | (0xffffffff - at)).max()) if at.size else 0


def seg_cc_lesion(roots_pred, roots_gt, out, workspace=None):
    rp, rg = roots_pred.numpy().ravel().astype(np.int64), roots_gt.numpy().ravel().astype(np.int64)
    n = rp.size
    both = (rp >= 0) & (rg >= 0)
    size_p, size_g = np.bincount(rp[rp >= 0], minlength=n), np.bincount(rg[rg >= 0], minlength=n)
    ov_p, ov_g = np.bincount(rp[both], minlength=n), np.bincount(rg[both], minlength=n)
    keys = [_key(size_p), _key(size_g)]
    best = 0xffffffff - (keys[0] & 0xffffffff)
    vals = [int((size_p > 0).sum()), int((size_g > 0).sum()), int((ov_p > 0).sum()), int((ov_g > 0).sum()),
            keys[0] >> 32, keys[1] >> 32, int(ov_p[best]) if keys[0] else 0, int((rg >= 0).sum())]
    out += torch.tensor(vals, dtype=torch.int64)
    return torch.tensor(keys, dtype=torch.int64)
