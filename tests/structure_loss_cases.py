"""Shared by tests/test_structure_loss_cpu.py and tests/test_structure_loss_gpu.py: the seeded inputs, the fp64 oracle of
the stage-1 structure loss (the definition of include/rehrseg_hip.h written with torch conv2d in float64 and autograd
for the gradient; it shares no code with tests/structure_loss_emu.py or the kernels), the same formulas in float32 as the
yardstick, and the comparison under the bars below.

    loss = l1 mean|p - t| + l2 mean (p - t)^2 + ssim (1 - mean S) + sobel mean|G(p) - G(t)|

d32 is the distance of the same formulas in float32 torch ops (CPU) from the fp64 oracle on the same input: one number
per case for the value, one per element for the gradient.  A float32 statement is not unique: the 11x11 window sum can
be taken rows first, columns first or as one 2-D correlation, and each order draws its own rounding error, which for
one case may by chance be several times smaller than for the next.  d32 is therefore the LARGEST distance over these
three orders (ORDERS), so that it measures the error of float32 rather than one draw of it.  The code under test must
stay within max(4 d32, floor) of the oracle, the factor 4 as in tests/sr_metrics_cases.py (another summation order inside
the window, fused multiply-adds).

  value floor     REL_SUMS (5e-7) relative on each of the three mean terms (two fp32 roundings per voxel term, fp64
                  accumulation, one rounding of the result to fp32) plus SSIM_FLOOR (1e-6) per unit of the ssim weight:
                  the floors tests/sr_metrics_cases.py derives for the same sums and the same index.
  gradient floor  the gradient of the SSIM term at a pixel is the sum of three window-filtered fields that cancel to a
                  few parts in a thousand (a shift of the image changes no variance), so its float32 error is a
                  heavy-tailed draw per element: d32_j is near zero for some elements of every case and several times
                  its root mean square for others, and the code under test, which rounds in its own order, has its
                  outliers at other elements.  A bar of 4 d32_j at the element cannot hold whatever the code does (the
                  CPU statement, whose error has the same mean square as the yardstick's, misses it at a few elements
                  of most cases).  The floor is therefore the yardstick's largest error over the elements of the case
                  under the same factor, and never less than SSIM_FLOOR relative to the largest gradient element of the
                  oracle (the floor of the index, a quantity of magnitude 1, carried over to the gradient's magnitude):
                      floor = max(4 max_j d32_j, 1e-6 max_j |g64_j|),   bar_j = max(4 d32_j, floor) = floor.
                  A misplaced halo, tap or tile edge moves elements by a large fraction of max|g|, five orders above
                  this.  Nothing in the bars comes from the code under test.
"""
import numpy as np
import torch
import torch.nn.functional as F

import sr_metrics_cases as sc

KINDS = sc.KINDS
# the smallest shapes at which the kernels can go wrong
SHAPES = [(1, 1, 1, 11, 11),     # one valid window, every pixel a border for Sobel
          (2, 1, 3, 12, 43),     # W crosses a 32-tile with both halos
          (1, 2, 2, 45, 37),
          (1, 1, 1, 70, 67)]     # crosses 64
ROW_SHAPE = (1, 1, 2, 1, 5)      # ssim = 0 only: Sobel on a one-row slice
TERMS = {"l1": (1.0, 0.0, 0.0, 0.0), "l2": (0.0, 1.0, 0.0, 0.0), "ssim": (0.0, 0.0, 1.0, 0.0),
         "sobel": (0.0, 0.0, 0.0, 1.0), "all": (1.0, 0.5, 0.7, 1.3)}
GRAD_FLOOR = sc.SSIM_FLOOR
ORDERS = ("hv", "vh", "2d")     # float32 statements of the window sum


def make_case(kind, shape, seed=0):
    """-> pred, target (float32 numpy, `shape` = (N, C, D, H, W)), data_range: the input kinds (a)-(d) of
    tests/sr_metrics_cases.py."""
    N, C, D, H, W = shape
    p, t, _, _, rng = sc.make_case(kind, (N * C, D, H, W), seed)
    return p.reshape(shape), t.reshape(shape), rng


def _loss(p, t, weights, data_range, order="hv"):
    """The definition in torch ops of p's dtype; p, t: (N, C, D, H, W).  order: how the window sum is associated."""
    l1, l2, ssim, sobel = weights
    H, W = p.shape[-2:]
    dt = p.dtype
    x, y = p.reshape(-1, 1, H, W), t.reshape(-1, 1, H, W)
    loss = torch.zeros((), dtype=dt)
    if l1 != 0:
        loss = loss + l1 * (x - y).abs().mean()
    if l2 != 0:
        loss = loss + l2 * ((x - y) ** 2).mean()
    if ssim != 0:
        g = torch.tensor(sc.gaussian64(), dtype=dt)

        def win(f):
            if order == "hv":
                return F.conv2d(F.conv2d(f, g.view(1, 1, 1, 11)), g.view(1, 1, 11, 1))
            if order == "vh":
                return F.conv2d(F.conv2d(f, g.view(1, 1, 11, 1)), g.view(1, 1, 1, 11))
            return F.conv2d(f, torch.outer(g, g).view(1, 1, 11, 11))

        C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
        mx, my = win(x), win(y)
        sxx, syy, sxy = win(x * x) - mx * mx, win(y * y) - my * my, win(x * y) - mx * my
        S = ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2))
        loss = loss + ssim * (1 - S.mean())
    if sobel != 0:
        kx = torch.tensor([[-1.0, 0.0, 1.0], [-2.0, 0.0, 2.0], [-1.0, 0.0, 1.0]], dtype=dt) / 8
        k = torch.stack((kx, kx.t())).view(2, 1, 3, 3)

        def mag(f):
            r = F.conv2d(F.pad(f, (1, 1, 1, 1), mode="replicate"), k)
            return torch.sqrt(r[:, 0:1] ** 2 + r[:, 1:2] ** 2 + 1e-6)

        loss = loss + sobel * (mag(x) - mag(y)).abs().mean()
    return loss


def evaluate(pred, target, weights, data_range=1.0, dtype=torch.float64, order="hv"):
    """-> (value: float, gradient: float64 numpy of pred's shape) of the definition evaluated in `dtype` on the CPU."""
    p = torch.from_numpy(np.array(pred)).to(dtype).requires_grad_()
    t = torch.from_numpy(np.array(target)).to(dtype)
    loss = _loss(p, t, weights, data_range, order)
    assert loss.dtype == dtype
    loss.backward()
    return float(loss.detach()), p.grad.double().numpy()


def yardstick(pred, target, weights, data_range=1.0):
    """-> (value64, grad64, d32 of the value, d32 per element of the gradient): the oracle and the largest distance of
    the float32 statements from it."""
    v64, g64 = evaluate(pred, target, weights, data_range, torch.float64)
    dv32, d32 = 0.0, np.zeros(g64.shape)
    for order in (ORDERS if weights[2] != 0 else ORDERS[:1]):
        v32, g32 = evaluate(pred, target, weights, data_range, torch.float32, order)
        dv32, d32 = max(dv32, abs(v32 - v64)), np.maximum(d32, np.abs(g32 - g64))
    return v64, g64, dv32, d32


_REFS = {}


def reference(kind, shape, term):
    """(pred, target, data_range, yardstick(...)) of a seeded case, computed once and shared (read-only arrays)."""
    key = (kind, tuple(shape), term)
    if key not in _REFS:
        p, t, rng = make_case(kind, shape)
        ref = yardstick(p, t, TERMS[term], rng)
        for a in (p, t, ref[1], ref[3]):
            a.setflags(write=False)
        _REFS[key] = (p, t, rng, ref)
    return _REFS[key]


def value_floor(pred, target, weights, data_range):
    """REL_SUMS on the three mean terms as the oracle has them, SSIM_FLOOR per unit of the ssim weight."""
    parts = [abs(evaluate(pred, target, tuple(w if i == k else 0.0 for i in range(4)), data_range)[0])
             for k, w in enumerate(weights) if k != 2 and w != 0]
    return sc.REL_SUMS * sum(parts) + sc.SSIM_FLOOR * abs(weights[2])


def check(label, value, grad, pred, target, weights, data_range, ref=None):
    """value, grad: the code under test's loss and d loss / d pred for these inputs.  -> the measured distances."""
    v64, g64, dv32, d32 = ref if ref is not None else yardstick(pred, target, weights, data_range)
    grad = np.asarray(grad, np.float64)
    assert grad.shape == g64.shape, (grad.shape, g64.shape)
    dv = abs(float(value) - v64)
    vbar = max(4 * dv32, value_floor(pred, target, weights, data_range))
    rms = float(np.sqrt(np.mean(d32 ** 2)))
    gmax = float(np.abs(g64).max())
    bar = np.maximum(4 * d32, max(4 * float(d32.max()), GRAD_FLOOR * gmax))
    dist = np.abs(grad - g64)
    worst = int(np.argmax(dist - bar))
    print(f"{label}: value {v64:.6g}  d32 {dv32:.3e}  distance {dv:.3e}  bound {vbar:.3e} | gradient max|g| {gmax:.3e}  "
          f"d32 max {d32.max():.3e} rms {rms:.3e}  distance max {dist.max():.3e} rms {np.sqrt(np.mean(dist ** 2)):.3e}  "
          f"worst element: distance {dist.flat[worst]:.3e} bound {bar.flat[worst]:.3e}")
    assert np.isfinite(grad).all() and np.isfinite(value), label
    assert dv <= vbar, (label, dv, vbar)
    assert (dist <= bar).all(), (label, float(dist.flat[worst]), float(bar.flat[worst]))
    return dv32, dv, float(d32.max()), float(dist.max())
