"""The device contract of csrc/intensity_norm.hip in numpy, without the product code (test only):

  order_stats      np.sort of every item, the values at the ranks; an item with a NaN gives NaN in every rank
  plan             numpy.percentile's virtual index h = q / 100 * (S - 1) in Python floats: k0, k1, t
  percentiles      the two-sided lerp of sorted[k0], sorted[k1] in fp64 (Python floats: no contraction)
  percentile_norm  (min(max(x, lo), hi) - lo) / (hi - lo) in float32 with the fp64 bounds rounded to float32
  zeroone          (x - min) / (max - min) in float32

and the named cases of the GPU tests: the smallest shapes at which each step of the radix select can go wrong."""
import math

import numpy as np

SIZES = (1, 2, 3, 63, 64, 65, 255, 257, 4099, 65537)
Q_SETS = ([0.5, 99.5], [0.0, 100.0], [5.0, 95.0], [33.3, 66.7])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_order_stats(got, want):
    """uint32 bit patterns, -0 and +0 alike."""
    g, w = bits(got).copy(), bits(want).copy()
    g[g == 0x80000000] = 0
    w[w == 0x80000000] = 0
    return g.shape == w.shape and np.array_equal(g, w)


def same_values(got, want):
    """Bit patterns of two float32 or float64 arrays, with every NaN alike (a NaN's payload and sign are no part of the
    contract: 0 / 0 is 0xffc00000 on one machine and 0x7fc00000 on another)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    u = np.uint32 if got.dtype == np.float32 else np.uint64
    ng, nw = np.isnan(got), np.isnan(want)
    return np.array_equal(ng, nw) and np.array_equal(got.view(u)[~ng], want.view(u)[~nw])


def order_stats(x, ranks):
    x = np.asarray(x, dtype=np.float32)
    x = x.reshape(x.shape[0], -1)
    out = np.sort(x, axis=1)[:, list(ranks)]
    out[np.isnan(x).any(axis=1)] = np.nan
    return out


def plan(S, q):
    ranks, ts = [], []
    for p in q:
        h = (float(p) / 100.0) * (S - 1)
        k0 = int(math.floor(h))
        ranks += [k0, min(k0 + 1, S - 1)]
        ts.append(h - k0)
    return ranks, ts


def percentiles(x, q, strictly_positive=False):
    """float64 (B, len(q)); with strictly_positive a negative first column becomes 0."""
    x = np.asarray(x, dtype=np.float32)
    x = x.reshape(x.shape[0], -1)
    ranks, ts = plan(x.shape[1], q)
    st = order_stats(x, ranks)
    out = np.empty((x.shape[0], len(ts)), np.float64)
    for b in range(x.shape[0]):
        for j, t in enumerate(ts):
            lo, hi = float(st[b, 2 * j]), float(st[b, 2 * j + 1])
            d = hi - lo
            v = hi - d * (1.0 - t) if t >= 0.5 else lo + d * t
            if j == 0 and strictly_positive and v < 0:
                v = 0.0
            out[b, j] = v
    return out


def _apply(x, lo, hi, clip):
    lo, hi = np.float32(lo), np.float32(hi)
    with np.errstate(all="ignore"):
        v = np.minimum(np.maximum(x, lo), hi) if clip else x
        return ((v - lo) / (hi - lo)).astype(np.float32)


def percentile_norm(x, p_min=0.5, p_max=99.5, strictly_positive=True):
    """x (B, ...) float32 -> float32 of the same shape, every item with its own bounds."""
    x = np.asarray(x, dtype=np.float32)
    bounds = percentiles(x, [p_min, p_max], strictly_positive)
    return np.stack([_apply(x[b], bounds[b, 0], bounds[b, 1], True) for b in range(x.shape[0])])


def zeroone(x):
    x = np.asarray(x, dtype=np.float32)
    return np.stack([_apply(x[b], x[b].min(), x[b].max(), False) for b in range(x.shape[0])])


# ----------------------------------------------------------------------------- data
def gaussian(S, seed):
    return np.random.RandomState(seed).randn(S).astype(np.float32)


def zero_heavy(S, seed, frac=0.6):
    """Clipped Gaussians with `frac` exact zeros and a heavy right tail, as an MRI volume with its background."""
    g = np.random.RandomState(seed)
    x = np.abs(g.randn(S)).astype(np.float32) * np.float32(300.0)
    x[g.rand(S) < 0.01] *= np.float32(8.0)
    x[g.rand(S) < frac] = 0.0
    return x


def integers(S, seed):
    return np.random.RandomState(seed).randint(-20, 200, size=S).astype(np.float32)


def size_ranks(S):
    return [min(max(k, 0), S - 1) for k in (0, S // 2, S - 2, S - 1)]


def key_to_float(keys):
    """The float whose order-preserving key is `keys`: negatives have all bits flipped, the rest the sign bit."""
    keys = np.asarray(keys, dtype=np.uint32)
    b = np.where(keys >> 31 != 0, keys ^ np.uint32(0x80000000), ~keys)
    return b.astype(np.uint32).view(np.float32)


def _digits_to_key(digits, widths):
    key, used = 0, 0
    for d, w in zip(digits, widths):
        used += w
        key |= d << (32 - used)
    return key


def prefix_collisions(widths):
    """(x, ranks, pairs): eight keys built from the digit fields of `widths` (8/8/8/8 or 11/11/10) among 500 others.
    pairs: (0, 1) share digit 0 and differ in digit 1; (2, 3) share digits 0, 1 and differ in digit 2; (4, 5) differ in
    the last digit only; (6, 7) differ in digit 0 already.  ranks[i] is the place of key i in the sorted array."""
    top = 0xC0 if widths[0] == 8 else 0x600          # positive floats around 2..4: no NaN pattern
    n = len(widths)
    last = [3] * n
    fields = [[top, 1] + [5] * (n - 2), [top, 2] + [5] * (n - 2),
              [top + 1, 7, 1] + [5] * (n - 3), [top + 1, 7, 2] + [5] * (n - 3),
              [top + 2] + last[1:-1] + [1], [top + 2] + last[1:-1] + [2],
              [top + 3] + [9] * (n - 1), [top + 4] + [9] * (n - 1)]
    keys = np.array([_digits_to_key(f, widths) for f in fields], dtype=np.uint32)
    g = np.random.RandomState(11 + widths[0])
    filler = (np.uint32(top) << np.uint32(32 - widths[0])) + g.randint(0, 5 << (32 - widths[0]), size=500).astype(np.uint32)
    filler = filler[~np.isin(filler, keys)]
    allk = np.concatenate([keys, filler])
    g.shuffle(allk)
    srt = np.sort(allk)
    ranks = [int(np.searchsorted(srt, k)) for k in keys]
    x = key_to_float(allk)
    assert not np.isnan(x).any() and len(set(ranks)) == 8
    return x[None], ranks, ((0, 1), (2, 3), (4, 5), (6, 7))


def step_case(S, q, extra):
    """k0 (+ extra) zeros followed by ones, k0 the percentile's lower index: with extra = 1 sorted[k0] = 0 and
    sorted[k0 + 1] = 1 straddle the step, with extra = 0 both lie on the ones."""
    ranks, _ = plan(S, [q])
    x = np.ones(S, np.float32)
    x[:ranks[0] + extra] = 0.0
    np.random.RandomState(5).shuffle(x)
    return x[None], ranks


def order_cases():
    """name -> (x (B, S) float32, ranks)."""
    cases = {}
    for S in SIZES:
        cases[f"size_{S}"] = (gaussian(S, S)[None], size_ranks(S))
    cases["three_items_4099"] = (np.stack([gaussian(4099, 1), zero_heavy(4099, 2), integers(4099, 3)]), size_ranks(4099))
    g = np.random.RandomState(4)
    cases["last_digit"] = ((np.float32(1.0) + g.randint(0, 1024, size=4099).astype(np.float32) * np.float32(2.0 ** -23))[None],
                           [0, 1, 1000, 2049, 3000, 4000, 4097, 4098])
    e = np.arange(-126, 128).astype(np.float64)
    spread = np.concatenate([2.0 ** e, -(2.0 ** e), [0.0, -0.0, np.inf, -np.inf]]).astype(np.float32)
    den = np.array([1, 2, 0x7fffff, 0x80000001, 0x807fffff], dtype=np.uint32).view(np.float32)
    spread = np.concatenate([spread, den])
    g.shuffle(spread)
    n = spread.size
    cases["first_digit"] = (spread[None], [0, 1, n // 4, n // 2 - 1, n // 2 + 2, 3 * n // 4, n - 2, n - 1])
    cases["constant"] = (np.full((1, 4099), 3.5, np.float32), size_ranks(4099))
    for q in (0.5, 99.5):
        for extra in (0, 1):
            cases[f"step_q{q}_{extra}"] = step_case(4099, q, extra)
    z = zero_heavy(4099, 6)
    nz = int((z == 0).sum())
    cases["ties"] = (z[None], [0, nz // 2, nz - 1, nz, nz + 1])
    cases["all_negative"] = (-np.abs(gaussian(4099, 7))[None] - np.float32(0.25), size_ranks(4099))
    cases["mixed_sign"] = (gaussian(4099, 8)[None] * np.float32(50.0), [0, 20, 2049, 4078, 4098])
    x = np.stack([gaussian(4099, 9), zero_heavy(4099, 10), integers(4099, 11)])
    x[1, 1234] = np.nan
    cases["nan_item"] = (x, size_ranks(4099))
    for widths in ((8, 8, 8, 8), (11, 11, 10)):
        x, ranks, _ = prefix_collisions(widths)
        cases[f"prefix_{widths[0]}bit"] = (x, ranks)
    return cases


def volume_case(shape=(20, 455, 633), seed=12):
    """One volume-shaped item of clipped Gaussians with 60 % exact zeros, (1, 1, D, H, W)."""
    S = int(np.prod(shape))
    return zero_heavy(S, seed).reshape((1, 1) + tuple(shape))
