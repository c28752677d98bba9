"""Shared by tests/test_sr_metrics_cpu.py and tests/test_sr_metrics_gpu.py: the seeded inputs, the fp64 oracle of the
stage-1 validation metrics (the definition of include/rehrseg_hip.h written with scipy.ndimage.correlate1d over the
whole slice, cropped to the valid region; it shares no code with tests/sr_metrics_emu.py), the fp32 torch composition
that serves as the SSIM yardstick, and the comparison under the tolerances below.

  sum_abs, sum_sq   relative error <= 5e-7 against fp64: two fp32 roundings per voxel term (2 * 2^-24 = 1.2e-7), fp64
                    accumulation; the factor 4 covers the bf16 widening and the order of the partial sums.  More than
                    that means a sum was kept in fp32 somewhere.
  counts, ssim_cnt  exact.
  ssim              d32 = the distance of the formula evaluated with fp32 torch ops on the CPU from the fp64 oracle on
                    the same input (largest over the samples); the code under test must stay within max(4 d32, 1e-6)
                    of the oracle: 4 for another summation order inside the window and fused multiply-adds, the floor
                    for inputs where d32 happens to be near zero.
"""
import numpy as np
import torch
from scipy import ndimage

KINDS = ("a", "b", "c", "d")
SMALL_SHAPES = [(3, 1, 11, 11), (2, 3, 45, 37), (1, 2, 70, 67)]
REL_SUMS = 5e-7
SSIM_FLOOR = 1e-6


def gaussian64():
    e = np.exp(-((np.arange(11) - 5.0) ** 2) / (2.0 * 1.5 ** 2))
    return e / e.sum()


def make_case(kind, shape, seed=0):
    """-> pred, target, seg_logits, seg_target (float32 numpy, `shape`), data_range."""
    rng = np.random.RandomState(1000 * (KINDS.index(kind) + 1) + seed + sum(shape))
    if kind in ("a", "d"):
        t = rng.rand(*shape)
    elif kind == "b":
        t = ndimage.uniform_filter(rng.rand(*shape), size=(1, 1, 9, 9), mode="reflect")
    else:
        t = np.full(shape, 0.7)
    p = t + 0.05 * rng.randn(*shape)
    rng_ = 1.0
    if kind == "d":
        p, t, rng_ = 100.0 * p + 1000.0, 100.0 * t + 1000.0, 100.0
    logits = rng.randn(*shape)
    seg = (rng.rand(*shape) > 0.6).astype(np.float32)
    return p.astype(np.float32), t.astype(np.float32), logits.astype(np.float32), seg, rng_


def oracle(pred, target, seg_logits=None, seg_target=None, data_range=1.0):
    """(N, 7) float64 from float arrays (their values taken as they are, in fp64), the counts exact integers."""
    p, t = np.asarray(pred, np.float64), np.asarray(target, np.float64)
    N, D, H, W = p.shape
    g = gaussian64()

    def win(f):
        f = ndimage.correlate1d(ndimage.correlate1d(f, g, axis=-1, mode="constant"), g, axis=-2, mode="constant")
        return f[..., 5:H - 5, 5:W - 5]

    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mx, my = win(p), win(t)
    sxx, syy, sxy = win(p * p) - mx * mx, win(t * t) - my * my, win(p * t) - mx * my
    S = ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2))
    out = np.zeros((N, 7), np.float64)
    out[:, 0] = np.abs(p - t).sum((1, 2, 3))
    out[:, 1] = ((p - t) ** 2).sum((1, 2, 3))
    out[:, 2] = S.sum((1, 2, 3))
    out[:, 3] = D * (H - 10) * (W - 10)
    if seg_logits is not None:
        fp, ft = np.asarray(seg_logits) > 0, np.asarray(seg_target) > 0.5
        out[:, 4] = np.count_nonzero(fp & ft, axis=(1, 2, 3))
        out[:, 5] = np.count_nonzero(fp, axis=(1, 2, 3))
        out[:, 6] = np.count_nonzero(ft, axis=(1, 2, 3))
    return out


def ssim_torch_fp32(pred, target, data_range=1.0):
    """The per-sample mean SSIM index from plain fp32 torch ops on the CPU (the yardstick, not the code under test)."""
    p, t = torch.as_tensor(pred, dtype=torch.float32), torch.as_tensor(target, dtype=torch.float32)
    N, D, H, W = p.shape
    g = torch.tensor(gaussian64(), dtype=torch.float32)

    def win(f):
        f = torch.nn.functional.conv2d(f.reshape(N * D, 1, H, W), g.view(1, 1, 1, 11))
        return torch.nn.functional.conv2d(f, g.view(1, 1, 11, 1)).reshape(N, -1)

    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mx, my = win(p), win(t)
    sxx, syy, sxy = win(p * p) - mx * mx, win(t * t) - my * my, win(p * t) - mx * my
    S = ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2))
    assert S.dtype == torch.float32
    return S.double().mean(1).numpy()


def check_stats(label, got, pred, target, seg_logits, seg_target, data_range):
    """got: the (N, 7) stats of the code under test for these inputs (pred as the code saw it, e.g. after bf16)."""
    got = np.asarray(got, np.float64)
    want = oracle(pred, target, seg_logits, seg_target, data_range)
    assert got.shape == want.shape, (got.shape, want.shape)
    rel = np.abs(got[:, :2] - want[:, :2]) / np.maximum(np.abs(want[:, :2]), 1e-300)
    rel[want[:, :2] == 0] = np.abs(got[:, :2])[want[:, :2] == 0]
    ssim64 = want[:, 2] / want[:, 3]
    d32 = float(np.abs(ssim_torch_fp32(pred, target, data_range) - ssim64).max())
    dist = float(np.abs(got[:, 2] / got[:, 3] - ssim64).max())
    print(f"{label}: ssim {ssim64.min():.4f}..{ssim64.max():.4f}  d32 {d32:.3e}  distance {dist:.3e}  "
          f"bound {max(4 * d32, SSIM_FLOOR):.3e}  sums rel {rel.max():.3e}")
    assert rel.max() <= REL_SUMS, (label, rel)
    assert np.array_equal(got[:, 3:], want[:, 3:]), (label, got[:, 3:], want[:, 3:])
    assert dist <= max(4 * d32, SSIM_FLOOR), (label, dist, d32)
    return d32, dist
