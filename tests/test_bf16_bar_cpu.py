"""tests/bf16_bar.py proved on a CPU emulation of the mixed-precision convolution: operands rounded to bf16, the conv in
torch fp32 with bias and LeakyReLU 0.1, the result rounded with .to(torch.bfloat16), the reference the same conv in fp64.
The correct result has no violation of the per-element bar; three subtly wrong results each have at least one, although
the norm the bf16 kernel tests used before (max |got - ref| / max |ref| < 1e-2) accepts them:

  * a store that truncates (the low 16 bits of the fp32 pattern masked off) instead of rounding to nearest;
  * one bf16 ulp added (+1 in the bit pattern) on 1 % of the elements;
  * one product dropped -- input channel Cin - 1, tap (2, 2, 2) -- along one output row (depth D - 2, row H - 2, every
    column and output channel): what a wrong mask of a half-filled channel chunk or of a ragged brick does.

The reductions bar (stats_bar) gets the same check: the fp32 values summed exactly pass, a sum that misses one voxel
fails."""
import pytest
import torch
import torch.nn.functional as F

from bf16_bar import assert_bf16_bar, assert_stats_bar, bf16_bar, stats_bar

BF = torch.bfloat16
SHAPES = [  # (N, Cin, Cout, D, H, W): 3x3x3 taps, pad 1
    (1, 48, 96, 5, 11, 13),
    (2, 64, 64, 3, 9, 10),
    (1, 320, 320, 4, 5, 5),
]
_cache = {}


def relmax(a, b):
    """The norm of the earlier bf16 tests."""
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30))


def emulation(shape):
    """pre: the fp32 accumulators (conv + bias) of the emulated kernel; drop: the contribution of channel Cin - 1, tap
    (2, 2, 2) to them; ref: act(conv + bias) in fp64 on the same rounded operands.  Computed once per shape."""
    if shape not in _cache:
        N, Cin, Cout, D, H, W = shape
        g = torch.Generator().manual_seed(sum(shape))
        x = torch.randn((N, Cin, D, H, W), generator=g).to(BF)
        w = (torch.randn((Cout, Cin, 3, 3, 3), generator=g) / (Cin * 27) ** 0.5).to(BF)
        b = torch.randn(Cout, generator=g)
        pre = F.conv3d(x.float(), w.float(), b, 1, 1)
        one = torch.zeros(Cout, 1, 3, 3, 3)
        one[:, 0, 2, 2, 2] = w.float()[:, Cin - 1, 2, 2, 2]
        drop = F.conv3d(x.float()[:, Cin - 1:], one, None, 1, 1)
        ref = F.leaky_relu(F.conv3d(x.double(), w.double(), b.double(), 1, 1), 0.1)
        _cache[shape] = (pre, drop, ref)
    return _cache[shape]


def act32(pre):
    return F.leaky_relu(pre, 0.1)


def truncating_store(v32):
    return (v32.contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF)   # exact: the low bits are zero


def one_ulp_on_one_percent(y, seed):
    bits = y.contiguous().view(torch.int16).clone().flatten()
    idx = torch.randperm(bits.numel(), generator=torch.Generator().manual_seed(seed))[:max(1, bits.numel() // 100)]
    bits[idx] += 1
    return bits.view(BF).reshape(y.shape)


@pytest.mark.parametrize("shape", SHAPES)
def test_correct_result_passes_the_per_element_bar(shape):
    pre, _, ref = emulation(shape)
    worst, _ = assert_bf16_bar(f"emulation {shape}", act32(pre).to(BF), ref)
    assert worst < 1.0 and relmax(act32(pre).to(BF), ref) < 1e-2


@pytest.mark.parametrize("shape", SHAPES)
def test_truncating_store_fails_the_new_bar_and_passed_the_old_one(shape):
    pre, _, ref = emulation(shape)
    y = truncating_store(act32(pre))
    violations, worst = bf16_bar(y, ref)
    print(f"truncating store {shape}: {violations} violations, worst {worst:.2f}/1, old norm {relmax(y, ref):.2e}")
    assert violations >= 1 and worst > 1.0
    assert relmax(y, ref) < 1e-2            # the gap, recorded: the old bar accepted this store
    with pytest.raises(AssertionError):
        assert_bf16_bar("truncating store", y, ref)


@pytest.mark.parametrize("shape", SHAPES)
def test_one_ulp_on_one_percent_fails_the_new_bar_and_passed_the_old_one(shape):
    pre, _, ref = emulation(shape)
    y = one_ulp_on_one_percent(act32(pre).to(BF), seed=shape[1])
    violations, worst = bf16_bar(y, ref)
    print(f"one ulp on 1 % {shape}: {violations} violations, worst {worst:.2f}/1, old norm {relmax(y, ref):.2e}")
    assert violations >= 1 and worst > 1.0
    assert relmax(y, ref) < 1e-2


@pytest.mark.parametrize("shape", SHAPES)
def test_dropped_product_fails_the_new_bar(shape):
    pre, drop, ref = emulation(shape)
    D, H = shape[3:5]
    wrong = pre.clone()             # (D - 2, H - 2): the last row whose tap (2, 2, 2) still reads inside the volume
    wrong[:, :, D - 2, H - 2, :] -= drop[:, :, D - 2, H - 2, :]
    y = act32(wrong).to(BF)
    violations, worst = bf16_bar(y, ref)
    print(f"dropped product {shape}: {violations} violations, worst {worst:.2f}/1, old norm {relmax(y, ref):.2e}")
    assert violations >= 1 and worst > 1.0
    if shape[1] == 320:                     # one of 8640 products: below 1e-2 of the largest output
        assert relmax(y, ref) < 1e-2


def test_nan_and_shape_are_not_overlooked():
    ref = torch.linspace(-2, 2, 64, dtype=torch.float64).reshape(1, 4, 16)
    got = ref.to(BF)
    assert bf16_bar(got, ref) == (0, bf16_bar(got, ref)[1]) and bf16_bar(got, ref)[1] <= 1.0
    bad = got.clone()
    bad[0, 1, 3] = float("nan")
    violations, worst = bf16_bar(bad, ref)
    assert violations == 1 and worst != worst
    assert bf16_bar(torch.zeros(3, dtype=BF), torch.zeros(3, dtype=torch.float64)) == (0, 0.0)   # an all-zero reference
    assert bf16_bar(torch.full((3,), 1e-3, dtype=BF), torch.zeros(3, dtype=torch.float64))[0] == 3
    with pytest.raises(AssertionError):
        bf16_bar(got[:, :2], ref)


@pytest.mark.parametrize("shape", SHAPES)
def test_stats_bar_passes_exact_sums_and_fails_a_missing_voxel(shape):
    pre, _, ref = emulation(shape)
    v = act32(pre).double()                 # the fp32 values a kernel would sum, summed exactly
    s1, s2 = v.sum((2, 3, 4)), (v * v).sum((2, 3, 4))
    assert_stats_bar(f"fp32 conv, fp64 sum {shape}", s1, ref)
    assert_stats_bar(f"fp32 conv, fp64 sum of squares {shape}", s2, ref * ref)
    # the middle voxel of the volume left out of every channel sum
    flat = v.flatten(2)
    miss = flat[:, :, flat.shape[2] // 2]
    violations, worst = stats_bar(s1 - miss, ref)
    print(f"missing voxel {shape}: sum {violations} violations, worst {worst:.1f}/1")
    assert violations >= 1 and worst > 1.0
    violations, worst = stats_bar(s2 - miss * miss, ref * ref)
    assert violations >= 1 and worst > 1.0
    with pytest.raises(AssertionError):
        assert_stats_bar("missing voxel", s1 - miss, ref)

