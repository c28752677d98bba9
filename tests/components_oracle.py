"""Yardstick of the connected-component calls (test only; independent of the kernels and of their emulation): pure
numpy plus scipy.ndimage.label with generate_binary_structure(3, 1 | 2 | 3) for connectivity 6 | 18 | 26.

From scipy's partition: the root map (the smallest linear index of every component, -1 at background), the labels
renumbered by root (scipy's own order is not relied on), the largest component under the tie rule (the smaller root
among equal sizes), the eight integers of rehr_seg_cc_lesion_i64 and the dict of lesion_metrics.
Also the masks of the test cases, shared by the CPU and the GPU tests."""
import functools
import math

import numpy as np
from scipy import ndimage as ndi

import surface_oracle as so

CONNECTIVITIES = (6, 18, 26)


def structure(connectivity):
    return ndi.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity])


def _label(mask, connectivity):
    """(scipy's labels flattened, n, first[k] = the smallest linear index of label k; first[0] unused)."""
    lab, n = ndi.label(np.asarray(mask) != 0, structure(connectivity))
    flat = lab.ravel()
    first = np.full(n + 1, flat.size, np.int64)
    idx = np.arange(flat.size - 1, -1, -1)
    first[flat[::-1]] = idx                 # a repeated index keeps the last value assigned: the smallest position
    return flat, n, first


def roots(mask, connectivity):
    flat, _, first = _label(mask, connectivity)
    return np.where(flat > 0, first[flat], -1).astype(np.int32).reshape(np.shape(mask))


def labels(mask, connectivity):
    """(labels int32, n): component k is the one with the k-th smallest root."""
    flat, n, first = _label(mask, connectivity)
    order = np.argsort(first[1:], kind="stable")
    renumber = np.zeros(n + 1, np.int32)
    renumber[1 + order] = np.arange(1, n + 1, dtype=np.int32)
    return renumber[flat].reshape(np.shape(mask)), n


def _largest(flat, n, first):
    """(scipy label of the largest component, its size); the smaller root among equal sizes; (0, 0) if there is none."""
    if n == 0:
        return 0, 0
    sizes = np.bincount(flat, minlength=n + 1)[1:]
    tied = np.flatnonzero(sizes == sizes.max())
    best = int(tied[np.argmin(first[1 + tied])])
    return best + 1, int(sizes[best])


def n_largest_ties(mask, connectivity):
    """How many components share the largest size."""
    flat, n, _ = _label(mask, connectivity)
    sizes = np.bincount(flat, minlength=n + 1)[1:]
    return int((sizes == sizes.max()).sum()) if n else 0


def keep_largest(mask, connectivity):
    flat, n, first = _label(mask, connectivity)
    best, _ = _largest(flat, n, first)
    return ((flat == best) & (flat > 0)).astype(np.uint8).reshape(np.shape(mask))


def eight(pred, gt, connectivity):
    P, G = (np.asarray(pred) != 0).ravel(), (np.asarray(gt) != 0).ravel()
    fp_, n_p, first_p = _label(pred, connectivity)
    fg_, n_g, first_g = _label(gt, connectivity)
    best_p, size_p = _largest(fp_, n_p, first_p)
    _, size_g = _largest(fg_, n_g, first_g)
    return [n_p, n_g, len(np.unique(fp_[P & G])), len(np.unique(fg_[P & G])), size_p, size_g,
            int(((fp_ == best_p) & P & G).sum()), int(G.sum())]


def lesion_dict(vals):
    n_pred, n_gt, tp_pred, tp_gt, largest_pred, largest_gt, inter, sum_gt = (int(v) for v in vals)
    p = tp_pred / n_pred if n_pred else math.nan
    r = tp_gt / n_gt if n_gt else math.nan
    if math.isnan(p) or math.isnan(r):
        f1 = math.nan
    elif p + r == 0:
        f1 = 0.0
    else:
        f1 = 2 * p * r / (p + r)
    smooth = 1e-5                              # calculate_dice's
    return {"n_pred": n_pred, "n_gt": n_gt, "tp_pred": tp_pred, "tp_gt": tp_gt, "fp": n_pred - tp_pred,
            "fn": n_gt - tp_gt, "largest_pred": largest_pred, "largest_gt": largest_gt, "precision": p, "recall": r,
            "f1": f1, "dice_largest": (2.0 * inter + smooth) / (largest_pred + sum_gt + smooth),
            "dice_largest_terms": (inter, largest_pred, sum_gt)}


def same_dict(got, want):
    """Exact equality, NaN equal to NaN."""
    if set(got) != set(want):
        return False
    for k, w in want.items():
        g = got[k]
        if isinstance(w, float):
            if not isinstance(g, float) or not (g == w or (math.isnan(g) and math.isnan(w))):
                return False
        elif type(g) is not type(w) or g != w:
            return False
    return True


# ----------------------------------------------------------------------------- the cases
def _points(shape, *voxels):
    m = np.zeros(shape, bool)
    for v in voxels:
        m[v] = True
    return m


def _snake():
    """One voxel wide: every second row of every second slice in full, joined at alternating ends and, through the
    slice between, from the last row of one slice to the same row of the next."""
    D, H, W = 5, 9, 67
    m = np.zeros((D, H, W), bool)
    cur = 0                                    # the x at which the path enters a row
    for k, z in enumerate(range(0, D, 2)):
        ys = list(range(0, H, 2))
        if k % 2:
            ys.reverse()
        for j, y in enumerate(ys):
            m[z, y, :] = True
            cur = W - 1 - cur                  # it leaves at the other end
            if j + 1 < len(ys):
                m[z, (y + ys[j + 1]) // 2, cur] = True
        if z + 2 < D:
            m[z + 1, ys[-1], cur] = True
    return m


def _comb(mirror):
    m = np.zeros((3, 8, 67), bool)
    m[:, :, ::2] = True                        # teeth: planes of constant x, two apart
    m[-1, -1, :] = True                        # they meet in the last row of the last slice only
    return m[::-1, ::-1, :].copy() if mirror else m


def _lesion_maps():
    """(pred, gt) on (6, 40, 48): six label lesions; a thin predicted bar bridges two of them, two more are hit by
    a blob of their own, two are missed, and the largest predicted blob is a false alarm."""
    shape = (6, 40, 48)
    e = functools.partial(so.ellipsoid, shape)
    gt = (e((2.5, 8, 8), (1.5, 4, 4)) | e((2.5, 8, 20), (1.5, 4, 4)) | e((3, 28, 10), (2, 5, 5)) |
          e((1, 30, 36), (1, 3, 3)) | e((4, 16, 40), (1, 2, 2)) | e((3, 20, 30), (1.5, 3, 3)))
    pred = (e((2.5, 8, 14), (1.2, 2.5, 11)) | e((3, 29, 11), (2, 4, 4)) | e((3, 20, 31), (1, 2, 2)) |
            e((4, 33, 26), (1.9, 6, 8)))
    return pred, gt


@functools.lru_cache(maxsize=None)
def case(name):
    """The mask of a named case (read-only)."""
    if name.startswith("noise_"):
        m = np.random.RandomState(5).rand(6, 20, 67) < float(name[6:])
    elif name == "checkerboard":
        m = np.indices((4, 6, 10)).sum(0) % 2 == 0
    elif name == "corners":
        m = _points((3, 4, 5), (0, 1, 3), (1, 2, 2))
    elif name == "edges":
        m = _points((3, 4, 5), (1, 1, 1), (1, 2, 2))
    elif name == "no_wrap":
        m = _points((3, 4, 5), (0, 1, 4), (0, 2, 0), (1, 3, 2), (2, 0, 2))
    elif name == "snake":
        m = _snake()
    elif name == "late_join":
        m = _comb(False)
    elif name == "late_join_mirror":
        m = _comb(True)
    elif name == "full":
        m = np.ones((6, 20, 24), bool)
    elif name == "empty":
        m = np.zeros((6, 20, 24), bool)
    elif name == "one_slice":
        m = np.random.RandomState(6).rand(1, 33, 40) < 0.5
    elif name == "one_row":
        m = np.random.RandomState(7).rand(1, 1, 130) < 0.7
    elif name == "one_column":
        m = np.random.RandomState(8).rand(7, 5, 1) < 0.6
    elif name == "wide":
        m = np.random.RandomState(9).rand(3, 5, 130) < 0.6
    elif name == "lesions_pred":
        m = _lesion_maps()[0]
    elif name == "lesions_gt":
        m = _lesion_maps()[1]
    elif name == "lattice":
        m = np.random.RandomState(1).rand(16, 320, 384) < 0.3
    else:
        raise KeyError(name)
    m = np.ascontiguousarray(m)
    m.setflags(write=False)
    return m


SMALL = ("noise_0.1", "noise_0.3", "noise_0.6", "checkerboard", "corners", "edges", "no_wrap", "snake", "late_join",
         "late_join_mirror", "full", "empty", "one_slice", "one_row", "one_column", "wide", "lesions_pred",
         "lesions_gt")


def partner(name):
    """The second map of a case's lesion statistics: the label of `lesions`, else the mask moved by (1, 2, 3) voxels
    with zeros moved in, which overlaps some components and misses others."""
    if name == "lesions_pred":
        return case("lesions_gt")
    if name == "lesions_gt":
        return case("lesions_pred")
    m = case(name)
    g = np.zeros_like(m)
    d, h, w = (min(s, n - 1) for s, n in zip((1, 2, 3), m.shape))
    g[d:, h:, w:] = m[:m.shape[0] - d, :m.shape[1] - h, :m.shape[2] - w]
    return g


@functools.lru_cache(maxsize=None)
def expected(name, connectivity):
    """{'roots', 'labels', 'n', 'keep', 'eight', 'dict'} of a case, computed once."""
    m, g = case(name), partner(name)
    lab, n = labels(m, connectivity)
    vals = eight(m, g, connectivity)
    return {"roots": roots(m, connectivity), "labels": lab, "n": n, "keep": keep_largest(m, connectivity),
            "eight": vals, "dict": lesion_dict(vals)}
