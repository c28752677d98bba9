"""The loss and distillation kernels at the shapes where their launch geometry changes, each against the torch
composition the project owns, evaluated on the CPU in fp64 with autograd.

  kernel                                   reference                                   what the shapes reach
  seg_loss_{fwd,bwd}_kernel<2,3,4>         seg_utils.DC_and_weighted_CE_loss           N = 1..9 around SL_MAXN = 4 (grid.y > 1, a last
   (csrc/seg_loss.hip)                      (RobustCrossEntropyLoss + SoftDiceLoss)     chunk of 1 or 2 samples, the uncertainty sum over
                                                                                        ALL samples), do_bg, smooth, both weights, S = 189
                                                                                        (under one block), S = 526 683 (grid-stride, odd),
                                                                                        saturated logits, an absent class with the clipped
                                                                                        denominator, a channel slice as logits
  bce_dice_{fwd,bwd}_kernel                seg_utils.BCEDiceLoss                       S > 256 * 256 and odd (grid-stride), the clamped
                                                                                        denominator next to a saturated channel
  quad_maxpool_{fwd,bwd}_kernel            nn.MaxPool2d((H/2, W/2), ceil_mode=True)    ties (first maximum), constant planes, NaN, C that
   (csrc/elementwise.hip)                                                               does not divide 256, C > 256, 1-element windows
  cosdist_{stats,bwd}_kernel               the un-fused branch of                      N * S > 65536 (grid-stride backward), N = 1 and 3
                                            seg_model.cosine_distance_loss              (1024 / N block split), an all-zero voxel

Every test asserts that the device call went through the fused autograd node: a fallback to torch ops cannot pass.

Bars are those of tests/test_seg_loss_gpu.py and tests/test_kernels_gpu.py: DC+CE value 1e-5 * max(1, |ref|), gradient
1e-4 * max |ref gradient|; BCE+Dice value 1e-6 * |ref|, gradient 1e-5 * max |ref gradient|; max-pool exact; cosine distance
value 1e-6 * max(1, |ref|), gradient 1e-4 * max |ref gradient|.  Saturated logits only (|x| up to ~100, where the kernels'
__expf / __logf and the formula itself lose digits): the bar is the larger of the one above and 4 x the error of the same
torch composition evaluated in fp32 on the CPU against the fp64 one, on the same inputs -- the fp32 composition is the
error floor of the formula, the factor 4 covers the fast intrinsics and the summation order.  Every comparison prints
"name measured / bar" before it asserts.
"""
import pytest
import torch
import torch.nn.functional as F

from rehrseg_amd.models import seg_model as sm
from rehrseg_amd.utils import seg_utils as su

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _mk(*shape, seed):
    return torch.randn(*shape, generator=_gen(seed), dtype=torch.float32)


def _close(name, err, bar):
    print(f"{name}: {err:.3e} / {bar:.3e}")
    assert err <= bar, f"{name}: error {err:.3e} > bar {bar:.3e}"


def _fused(t, node):
    """`t` came out of the autograd node `node` (a torch.autograd.Function of the package), not out of torch ops."""
    assert t.grad_fn is not None and type(t.grad_fn).__name__ == node.__name__ + "Backward", \
        f"not the fused path: {type(t.grad_fn).__name__}"


def _bar(name, err, bar, floor32=None):
    """Assert err <= bar, or <= max(bar, 4 * floor32) where the fp32-composition rule applies (both printed)."""
    if floor32 is None:
        return _close(name, err, bar)
    print(f"{name}: {err:.3e} / max(bar {bar:.3e}, 4 x fp32 composition {floor32:.3e})")
    assert err <= max(bar, 4.0 * floor32), \
        f"{name}: error {err:.3e} > max(bar {bar:.3e}, 4 x fp32 composition error {floor32:.3e})"


# ----------------------------------------------------------------------------- 1. DC + weighted CE
UP = 3.0   # upstream gradient: goes through the device scalar


def _dcce(do_bg=False, smooth=1e-5, w_ce=1, w_dice=1):
    return su.DC_and_weighted_CE_loss({"batch_dice": False, "smooth": smooth, "do_bg": do_bg, "ddp": False},
                                      {"reduction": "none"}, weight_ce=w_ce, weight_dice=w_dice, ignore_label=None,
                                      dice_class=su.SoftDiceLoss)


def _composition(mod, full, pick, target, unc, dtype):
    """The torch composition on the CPU (CPU tensors never take the fused path): value, d value / d full."""
    x = full.detach().to(dtype).requires_grad_(True)
    val = mod(pick(x), target.to(dtype), None if unc is None else unc.to(dtype))
    assert val.dtype == dtype
    (val * UP).backward()
    return val.detach().double(), x.grad.double() / UP


def _check_dcce(name, cfg, full, target, unc, pick=lambda t: t, saturated=False):
    dev = _dev()
    rv, rg = _composition(_dcce(**cfg), full, pick, target, unc, torch.float64)
    assert torch.isfinite(rv) and bool(torch.isfinite(rg).all())
    fv = fg = None
    if saturated:
        v32, g32 = _composition(_dcce(**cfg), full, pick, target, unc, torch.float32)
        fv, fg = abs(float(v32 - rv)), float((g32 - rg).abs().max())
    mod = _dcce(**cfg)
    x = full.to(dev).requires_grad_(True)
    lg, tg, ug = pick(x), target.to(dev), None if unc is None else unc.to(dev)
    assert mod._fusable(lg, tg, ug)
    val = mod(lg, tg, ug)
    _fused(val, su._FusedDCCE)
    (val * UP).backward()
    got = x.grad.double().cpu() / UP
    _bar(f"dcce {name} value", abs(float(val.detach()) - float(rv)), 1e-5 * max(1.0, abs(float(rv))), fv)
    _bar(f"dcce {name} gradient", float((got - rg).abs().max()), 1e-4 * float(rg.abs().max()), fg)


def _unc(N, dims, g):
    return 1.0 - torch.randint(0, 256, (N, 1) + dims, generator=g).float() / 255.0 * 0.99


def _seg_cases():
    """(C, N, uncertainty, do_bg, smooth, weight_ce, weight_dice).  SL_MAXN = 4 samples per block row: N = 5, 6, 9 leave a
    last chunk of 1, 2, 1 samples at b0 = 4 / 8, and with an uncertainty map every chunk pairs with the sum over all N."""
    cases = []
    for C in (2, 3, 4):
        cases += [(C, N, True, False, 1e-5, 1, 1) for N in (5, 6, 9)]
        cases += [(C, 1, False, True, 1.0, 0.3, 2.0), (C, 1, True, False, 1e-5, 1, 1),
                  (C, 4, False, False, 1e-5, 1, 1), (C, 4, True, True, 1.0, 0.3, 2.0),
                  (C, 5, False, True, 1e-5, 1, 1), (C, 6, False, False, 1.0, 0.3, 2.0),
                  (C, 9, False, True, 1.0, 1, 1), (C, 9, True, True, 1e-5, 0.3, 2.0)]
    return cases


def _seg_id(c):
    return f"C{c[0]}-N{c[1]}-{'unc' if c[2] else 'nounc'}-{'bg' if c[3] else 'nobg'}-s{c[4]:g}-w{c[5]:g}_{c[6]:g}"


@pytest.mark.parametrize("case", _seg_cases(), ids=_seg_id)
def test_dc_ce_classes_batch_background(case):
    """S = 3 * 7 * 9 = 189: less than one block, not a multiple of the wave."""
    C, N, with_unc, do_bg, smooth, w_ce, w_dice = case
    dims = (3, 7, 9)
    g = _gen(1000 + 16 * C + N)
    logits = torch.randn((N, C) + dims, generator=g) * 2.0
    target = torch.randint(0, C, (N, 1) + dims, generator=g).float()
    unc = _unc(N, dims, g) if with_unc else None
    _check_dcce(_seg_id(case), dict(do_bg=do_bg, smooth=smooth, w_ce=w_ce, w_dice=w_dice), logits, target, unc)


def test_dc_ce_grid_stride():
    """S = 3 * 419 * 419 = 526 683 > 2048 blocks x 256 threads, odd: 2395 threads take a second voxel."""
    dims = (3, 419, 419)
    g = _gen(1101)
    logits = torch.randn((2, 2) + dims, generator=g) * 2.0
    target = torch.randint(0, 2, (2, 1) + dims, generator=g).float()
    _check_dcce("grid-stride", {}, logits, target, _unc(2, dims, g))


def _saturated_inputs(seed):
    dims = (3, 7, 9)
    g = _gen(seed)
    logits = torch.randn((6, 4) + dims, generator=g) * 30.0
    target = torch.randint(0, 3, (6, 1) + dims, generator=g).float()
    return logits, target, _unc(6, dims, g)


def test_dc_ce_saturated_logits():
    """Logits ~N(0, 30): softmax differences far into the tails of __expf, cross-entropies of tens."""
    logits, target, unc = _saturated_inputs(1102)
    _check_dcce("saturated", {}, logits, target, unc, saturated=True)


def test_dc_ce_absent_class_clipped_denominator():
    """Class 3 is in no target and its logit is -200 everywhere: with do_bg and smooth = 0, G + P + smooth < 1e-8 on
    every sample, the denominator is clipped and only the numerator's term of the Dice gradient remains (cB = 0)."""
    logits, target, unc = _saturated_inputs(1103)
    logits[:, 3] = -200.0
    cfg = dict(do_bg=True, smooth=0.0)
    sp = torch.softmax(logits.double(), 1)[:, 3].sum((1, 2, 3))
    assert float(sp.max()) < 1e-8 and not bool((target == 3).any())     # the clip branch, on every sample
    _check_dcce("absent class", cfg, logits, target, unc, saturated=True)


def test_dc_ce_non_contiguous_logits():
    """Logits that are a channel slice of a wider tensor; the gradient is compared on the whole tensor."""
    dims = (3, 7, 9)
    g = _gen(1104)
    full = torch.randn((5, 5) + dims, generator=g) * 2.0
    target = torch.randint(0, 3, (5, 1) + dims, generator=g).float()
    _check_dcce("channel slice", {}, full, target, _unc(5, dims, g), pick=lambda t: t[:, 1:4])


# ----------------------------------------------------------------------------- 2. BCE + Dice
ALPHA, BETA = 0.7, 1.3


def _bce_composition(x, t, dtype):
    xr = x.detach().to(dtype).requires_grad_(True)
    val = su.BCEDiceLoss(ALPHA, BETA)(xr, t.to(dtype))
    assert val.dtype == dtype
    (val * UP).backward()
    return val.detach().double(), xr.grad.double() / UP


def _check_bce(name, x, t, saturated_channels=()):
    """The gradient is compared per channel against that channel's own largest reference magnitude."""
    dev = _dev()
    rv, rg = _bce_composition(x, t, torch.float64)
    assert torch.isfinite(rv) and bool(torch.isfinite(rg).all())
    if saturated_channels:
        v32, g32 = _bce_composition(x, t, torch.float32)
    xg = x.to(dev).requires_grad_(True)
    val = su.BCEDiceLoss(ALPHA, BETA)(xg, t.to(dev))
    _fused(val, su._FusedBCEDice)
    (val * UP).backward()
    got = xg.grad.double().cpu() / UP
    _bar(f"bce {name} value", abs(float(val.detach()) - float(rv)), 1e-6 * abs(float(rv)),
         abs(float(v32 - rv)) if saturated_channels else None)
    for c in range(x.shape[1]):
        floor = float((g32[:, c] - rg[:, c]).abs().max()) if c in saturated_channels else None
        _bar(f"bce {name} gradient of channel {c}", float((got[:, c] - rg[:, c]).abs().max()),
             1e-5 * float(rg[:, c].abs().max()), floor)


@pytest.mark.parametrize("N,C,dims", [(1, 1, (1, 1, 70001)), (2, 3, (3, 151, 151))], ids=["S70001", "S68403"])
def test_bce_dice_grid_stride(N, C, dims):
    """S > 256 blocks x 256 threads and odd: the grid-stride loop runs a second, partial trip."""
    g = _gen(1200 + C)
    x = torch.randn((N, C) + dims, generator=g) * 2.0
    t = torch.randint(0, 2, (N, C) + dims, generator=g).float()
    _check_bce(f"S={dims[0] * dims[1] * dims[2]}", x, t)


def test_bce_dice_clamped_denominator():
    """Channel 0: x = -20, target 0, so sum p^2 + sum t^2 ~ 3e-15 < 1e-6 (clamped, B = 0) and only the tiny BCE gradient
    is left; channel 1: logits ~N(0, 40) with a random binary target (the fp32-composition rule applies to it)."""
    g = _gen(1210)
    x = torch.randn((2, 2, 4, 10, 10), generator=g) * 40.0
    t = torch.randint(0, 2, (2, 2, 4, 10, 10), generator=g).float()
    x[:, 0], t[:, 0] = -20.0, 0.0
    assert float((torch.sigmoid(x[:, 0].double()) ** 2).sum()) < 1e-6
    _check_bce("clamped", x, t, saturated_channels=(1,))


# ----------------------------------------------------------------------------- 3. quadrant max-pool
def _same(name, got, ref):
    """Bit-for-bit the reference's values, NaN where and only where the reference has NaN."""
    got = got.detach().double().cpu()
    ref = ref.detach()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.equal(got.isnan(), ref.isnan()), \
        f"{name}: NaN at {int(got.isnan().sum())} elements, the reference at {int(ref.isnan().sum())}"
    bad = int((got.nan_to_num(nan=0.0) != ref.nan_to_num(nan=0.0)).sum())
    print(f"{name}: {bad} of {ref.numel()} elements differ / 0")
    assert bad == 0, f"{name}: {bad} of {ref.numel()} elements differ"


def _check_pool(name, x):
    """x (B, C, S, H, W), H and W even: _QuadMaxPool against MaxPool2d((H/2, W/2), ceil_mode=True) per (sample, depth)
    slice in fp64, output and input gradient, exactly."""
    B, C, S, H, W = x.shape
    xg = x.to(_dev()).requires_grad_(True)
    y = sm._QuadMaxPool.apply(xg)
    _fused(y, sm._QuadMaxPool)
    xr = x.double().requires_grad_(True)
    fr = xr.permute(0, 2, 1, 3, 4).reshape(B * S, C, H, W)
    ref = torch.nn.MaxPool2d(kernel_size=(H // 2, W // 2), stride=(H // 2, W // 2), padding=0, ceil_mode=True)(fr)
    _same(f"maxpool {name} output", y, ref)
    g = _mk(*ref.shape, seed=1301)
    (gx,) = torch.autograd.grad(y, xg, g.to(xg.device))
    (rx,) = torch.autograd.grad(ref, xr, g.double())
    _same(f"maxpool {name} gradient", gx, rx)
    return ref, rx


def _ties(*shape, seed):
    return torch.randint(0, 3, shape, generator=_gen(seed)).float()


@pytest.mark.parametrize("C,hw", [(48, (12, 10)), (64, (12, 10)), (128, (12, 10)), (64, (2, 2)), (64, (4, 66))],
                         ids=["C48", "C64", "C128", "C64-2x2", "C64-4x66"])
def test_quad_maxpool_ties(C, hw):
    """Values in {0, 1, 2}: ~10 equal maxima per 6 x 5 window, spread over the row groups of a block (4 at C = 64, 5 with
    16 idle threads at C = 48, 2 at C = 128); the gradient goes to the row-major first one.  2 x 2: one element per
    window, three of four row groups empty.  4 x 66: more columns than rows, two row groups empty."""
    _check_pool(f"ties C={C} {hw[0]}x{hw[1]}", _ties(2, C, 3, *hw, seed=1310 + C + hw[1]))


@pytest.mark.parametrize("value", [0.0, -3.5], ids=["zeros", "negative"])
def test_quad_maxpool_constant_plane(value):
    """All-equal planes (as after a ReLU): the whole gradient lands on each window's first element."""
    x = torch.full((2, 64, 3, 12, 10), value)
    _, rx = _check_pool(f"constant {value}", x)
    first = torch.zeros(12, 10, dtype=torch.bool)
    for h in (0, 6):
        for w in (0, 5):
            first[h, w] = True
    assert bool((rx[..., ~first] == 0).all()) and bool((rx[..., first] != 0).all())   # (the reference itself)


@pytest.mark.parametrize("rows", [(1,), (2,), (3,), (4,), (1, 2), (0, 3)], ids=lambda r: "rows" + "_".join(map(str, r)))
def test_quad_maxpool_nan(rows):
    """C = 64, 12 x 10: quadrant-local row r is scanned by row group r % 4.  A NaN in any group must come out as the
    pooled value of its window and channel and take that window's gradient, as in MaxPool2d; with two NaNs in a window
    ATen's scan keeps the last.  All other windows stay exact."""
    x = _mk(2, 64, 3, 12, 10, seed=1320)
    for k, r in enumerate(rows):
        x[1, 17, 2, 6 + r, 5 + 2 - k] = float("nan")       # quadrant 3 of slice (1, 2), channel 17
    ref, rx = _check_pool(f"nan rows {rows}", x)
    win = ref.reshape(2, 3, 64, 2, 2)
    assert bool(win[1, 2, 17, 1, 1].isnan()) and int(ref.isnan().sum()) == 1
    r_last = max(rows)
    assert float(rx[1, 17, 2, 6 + r_last, 5 + 2 - rows.index(r_last)]) != 0.0          # (the reference itself)


def test_quad_maxpool_more_than_256_channels():
    """C = 320: a second trip of the channel loop in which only 64 of the 256 lanes hold a channel."""
    _check_pool("ties C=320", _ties(2, 320, 3, 12, 10, seed=1330))
    _check_pool("random C=320", _mk(1, 320, 2, 12, 10, seed=1331))


# ----------------------------------------------------------------------------- 4. cosine distance
def _check_cosdist(name, a, b, zero_voxel=None):
    dev = _dev()
    N = a.shape[0]
    ag = a.to(dev).requires_grad_(True)
    loss = sm.cosine_distance_loss(ag, b.to(dev))
    _fused(loss, sm._CosDist)
    ar = a.double().requires_grad_(True)
    t1 = F.normalize(ar, p=2, dim=1).reshape(N, 64, -1)         # the un-fused branch of cosine_distance_loss
    t2 = F.normalize(b.double(), p=2, dim=1).reshape(N, 64, -1)
    ref = (1 - torch.cosine_similarity(t1, t2, dim=2)).mean()
    _close(f"cosdist {name} value", abs(loss.item() - ref.item()), 1e-6 * max(1.0, abs(ref.item())))
    (g,) = torch.autograd.grad(loss, ag, torch.tensor(2.5, device=dev))
    (gr,) = torch.autograd.grad(ref, ar, torch.tensor(2.5, dtype=torch.float64))
    g = g.double().cpu()
    keep = torch.ones(a.shape[0:1] + a.shape[2:], dtype=torch.bool)
    if zero_voxel is not None:
        # the reference gradient there is g / 1e-12 and dominates any scale: the one voxel that is not compared
        keep[zero_voxel] = False
        assert int((~keep).sum()) == 1
    keep = keep[:, None].expand_as(gr)
    _close(f"cosdist {name} gradient", float((g - gr)[keep].abs().max()), 1e-4 * float(gr[keep].abs().max()))


@pytest.mark.parametrize("N,dims", [(1, (3, 150, 150)), (3, (2, 9, 11))], ids=["N1-S67500", "N3-S198"])
def test_cosine_distance_batch_and_grid_stride(N, dims):
    """N = 1: 67 500 voxels > 16384 blocks x 4 waves, the backward's grid-stride loop; the statistics pass splits the
    sample over 1023 blocks of 66 voxels.  N = 3: 341 blocks per sample wanted, 198 voxels give 4 of 64 with a tail of 6."""
    a, b = _mk(N, 64, *dims, seed=1400 + N), _mk(N, 64, *dims, seed=1410 + N) * 0.5 + 0.1
    _check_cosdist(f"N={N}", a, b)


def test_cosine_distance_zero_voxel():
    """One all-zero voxel in the student tensor: its norm is clamped at 1e-12 and it adds nothing to the statistics."""
    a, b = _mk(2, 64, 3, 10, 12, seed=1420), _mk(2, 64, 3, 10, 12, seed=1421) * 0.5 + 0.1
    a[1, :, 2, 3, 4] = 0.0
    _check_cosdist("zero voxel", a, b, zero_voxel=(1, 2, 3, 4))
