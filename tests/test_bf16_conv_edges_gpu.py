"""The bf16 matrix-core convolution kernels at the shapes where they can go wrong, element by element.

Every case calls the kernel-level entry points (ops.conv_forward, ops.conv_dgrad; hip_backend.gather_gemm for the
fp32-output flag, which no ops call requests) with bf16 channels-last operands, so a result has passed exactly ONE
rounding.  The reference is torch.nn.functional in fp64 on the host on the same bf16-rounded x, w.to(bf16) and dz.  y
and dx are held to bf16_bar.py's per-element bar |got - ref| <= 2^-8 |ref| + acc max|ref|, the conv-epilogue statistics
to its reduction bar |got - sum| <= 5e-6 sum |summand| per (sample, channel).  The kernel that ran is asserted from the
library's route query (route_probe.py) and printed; sample n is scaled and shifted by SAMPLE_AFFINE[n], so a wrong sample
index cannot cancel.

Cases and the geometry each one targets (N = 2 unless stated; "ragged": the lattice is no multiple of the brick, so the
brick's masked row_out entries matter; padding = brick-padded lattice / lattice, a brick is taken up to 1.3x):

  halo bricks (halo_conv_bf16.hip), forward + input gradient, bias + LeakyReLU 0.1, stats_mode 2
    32->32, 64->64   7x15x31        brick 4x8x16 ragged in depth, rows and columns (8x16x32 = 1.26x); two channel tiles
    64->64           7x15x8         brick 8x8x8 (W 8 < 16), ragged in depth and rows (8x16x8 = 1.22x)
    32->32 1x3x3     6x31x30        brick 2x16x16 ragged in rows and columns (the deeper bricks pad D 6 -> 8 and decline)
    48->96           7x16x31        half-filled second 32-channel chunk, Npad 96, ragged brick; the input gradient
                                    (96 -> 48: 27 x 96 products, 56 blocks) is split into 6 tap-range parts: generic
    32+32->32        4x15x30        virtual concat (chunk 1 from x2) on a ragged brick; the gradient of each half
    32->128 1x3x3    6x48x48, N 3   persistent blocks: 81 bricks of 2x16x16, 64 blocks wanted -> 2 bricks per block;
                                    27 bricks per sample is odd, so the block of bricks 26 and 27 crosses from sample
                                    0 to 1 -- the register statistics are flushed and restarted inside a block --
                                    while the boundary 53 | 54 falls between two blocks
  generic gather (gather_gemm_bf16.hip); none of these lattices takes a brick, so the halo switch stays untouched
    64->64           3x7x9          flattened 128-voxel tiles, 189 voxels: the last tile holds 61 rows
    32+64->64, 96->64  4x10x12      32-channel K step (concat split / Cin % 64); forward in 6 tap-range parts (split-K)
    64->16, 64->160  3x9x11         padded output channels: Npad 32 with 16 live, five 32-wide tiles
    32->64 s222      9x10x11        stride phases of the input gradient on unequal lattices (5|4 x 5|5 x 6|5), one grid
    64->128 s122     4x17x15        the same with unit depth stride (9|8 x 8|7)
    32->32 5x5x5     6x7x8          125 taps (split-K: 5 depth-tap parts and the bf16 combine)
    32->32           7x15x31        y requested as fp32 (REHR_GG_Y_F32): generic kernel (halo switched off) and the halo
                                    kernel's own fp32 epilogue, held to the fp32 bar 1e-4 of max
  transposed convolutions, bias, no activation, forward + input gradient
    128->64 k=s=222  3x5x7          tconv_ks: 210 input voxels, the second 128-voxel tile holds 82
    64->32 k=s=122   4x9x10         tconv_ks: 720 voxels, the sixth tile holds 80
    192->64 k=s=222  3x5x7          Cin > 128: tconv_ks declines, the phase grid of the generic kernel
    64->32, 64+32->64 (3,4,4)/(1,2,2)  3x9x11   odd planes, four 3x2x2-tap phases (12 taps: no brick) in one generic grid

Measured on the MI355X, worst ratio to the bar over the y / dx of a group (bar 1), asserted acc 1e-4 | acc 1e-5:
    halo bricks          0.919 .. 0.956 | 0.982 .. 0.990
    generic gather       0.895 .. 0.951 | 0.972 .. 0.986
    transposed           0.926 .. 0.944 | 0.970 .. 0.990
    fp32 output          4e-7 of max in both kernels (0.004 of its bar): the accumulation error itself, unrounded
  and the tightened cases of test_bf16_kernels_gpu.py 0.902 .. 0.955 | 0.974 .. 0.991.  The y / dx figures of the cases
  above equal those of a torch fp32 convolution rounded with .to(bfloat16) on the host to three digits.
The asserted acc stays 1e-4.  It was to drop to 1e-5 if every case sat at or below 0.5 with that term, and no case
can: the half ulp of the store alone brings some element of a tensor to a ratio near 1 whatever acc is (the host
emulation of a correct kernel in test_bf16_bar_cpu.py reads 0.92 at 1e-4 and 0.98 at 1e-5).  The figure at 1e-5 therefore
says nothing about the accumulation, and 1e-4, the project's bar for fp32-stored outputs of the same accumulators, stands.
Statistics, worst ratio to 5e-6 sum |summand|: halo bricks 0.096, generic 0.090, fp32 output 0.047 (test_bf16_kernels_gpu.py:
0.123); the host reference of the same formula (torch fp32 conv on the same operands, summed in fp64) reads 0.207 at worst
(5x5x5 sum of squares).  No kernel comes near the bar, so the factor 5e-6 is asserted as it stands; nothing was re-derived.

Each case was also run once against a library with one arithmetic slip in the path it targets, and failed as intended:
padding voxels of a ragged brick counted in the statistics (all five ragged-brick cases, sum off by > 2e4 bars), the
statistics not restarted at a sample boundary inside a persistent block (the persistent case only), the last tap
skipped in the half-filled chunk (the 48 -> 96 case only) and a truncating store in tconv_ks (both tconv_ks cases, 1.87).

What keeps the old norm (max error over max value below 1e-2), and why: the halo-against-gather cross-check of
test_bf16_kernels_gpu.py compares two bf16 results with each other (two roundings, either of which may fall the other
way), and the outputs of tests/test_mixed_steps_gpu.py and of the InstanceNorm / SE layers of
tests/test_stage2_lattice_gpu.py have passed two roundings and a normalisation; the one-rounding bound does not hold
for them."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

import route_probe
from bf16_bar import assert_bf16_bar, assert_conv_stats
from rehrseg_amd import hip_backend, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
SAMPLE_AFFINE = [(1.0, 0.0), (3.0, 2.0), (0.5, -1.0)]   # as in test_stream_kernels_gpu.py
FP32_BAR = 1e-4                                         # fp32-stored outputs: of the largest value (test_kernels_gpu.py)


def act(shape, seed):
    """bf16 NDHWC activation on the device, sample n = a_n * randn + b_n (rounded once, on the host)."""
    t = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    for n, (a, b) in enumerate(SAMPLE_AFFINE[:shape[0]]):
        t[n] = a * t[n] + b
    return t.to(BF).to(DEV).contiguous(memory_format=torch.channels_last_3d)


def weights(shape, fan_in, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) / fan_in ** 0.5).to(DEV), torch.randn(shape[0], generator=g)


def f64(t):
    return t.detach().double().cpu()


@contextlib.contextmanager
def halo_switch(on):
    hip_backend.USE_HALO_BF16 = on
    try:
        yield
    finally:
        hip_backend.USE_HALO_BF16 = True


def routed(fn):
    """fn() and the kernels of its bf16 gather-GEMM launches, as the library names them."""
    with route_probe.launches() as seen:
        out = fn()
    return out, seen.kernels("gather_gemm_bf16")


S1, P1, P133 = (1, 1, 1), (1, 1, 1), (0, 1, 1)
K3, K133 = (3, 3, 3), (1, 3, 3)
# (name, N, (c1, c2), Cout, (D, H, W), kernel, stride, pad, forward kernel, input-gradient kernels (one per source))
CONV_CASES = [
    ("halo 4x8x16 ragged 32", 2, (32, 0), 32, (7, 15, 31), K3, S1, P1, "halo 4x8x16", ["halo 4x8x16"]),
    ("halo 4x8x16 ragged 64", 2, (64, 0), 64, (7, 15, 31), K3, S1, P1, "halo 4x8x16", ["halo 4x8x16"]),
    ("halo 8x8x8 ragged", 2, (64, 0), 64, (7, 15, 8), K3, S1, P1, "halo 8x8x8", ["halo 8x8x8"]),
    ("halo 2x16x16 ragged", 2, (32, 0), 32, (6, 31, 30), K133, S1, P133, "halo 2x16x16", ["halo 2x16x16"]),
    # the input gradient: ops._tap_split takes it (56 generic blocks <= 160, 27 x 96 >= 2048 products): 6 parts, generic
    ("halo half chunk, Npad 96", 2, (48, 0), 96, (7, 16, 31), K3, S1, P1, "halo 4x8x16", ["generic"]),
    ("halo two sources ragged", 2, (32, 32), 32, (4, 15, 30), K3, S1, P1, "halo 4x8x16", ["halo 4x8x16"] * 2),
    ("halo persistent over samples", 3, (32, 0), 128, (6, 48, 48), K133, S1, P133, "halo 2x16x16", ["halo 2x16x16"]),
    ("generic flat tiles, 61-row tail", 2, (64, 0), 64, (3, 7, 9), K3, S1, P1, "generic", ["generic"]),
    ("generic K 32 from the concat split", 2, (32, 64), 64, (4, 10, 12), K3, S1, P1, "generic", ["generic"] * 2),
    ("generic K 32, Cin 96", 2, (96, 0), 64, (4, 10, 12), K3, S1, P1, "generic", ["generic"]),
    ("generic Cout 16", 2, (64, 0), 16, (3, 9, 11), K3, S1, P1, "generic", ["generic"]),
    ("generic Cout 160", 2, (64, 0), 160, (3, 9, 11), K3, S1, P1, "generic", ["generic"]),
    ("generic stride 222, odd extents", 2, (32, 0), 64, (9, 10, 11), K3, (2, 2, 2), P1, "generic", ["generic"]),
    ("generic stride 122, odd extents", 2, (64, 0), 128, (4, 17, 15), K3, (1, 2, 2), P1, "generic", ["generic"]),
    ("generic 5x5x5 taps", 2, (32, 0), 32, (6, 7, 8), (5, 5, 5), S1, (2, 2, 2), "generic", ["generic"]),
]


def _conv_operands(case):
    name, N, (c1, c2), Cout, dims, K, stride, pad = case[:8]
    seed = 100 * (1 + [c[0] for c in CONV_CASES].index(name))
    x1 = act((N, c1) + dims, seed)
    x2 = act((N, c2) + dims, seed + 1) if c2 else None
    Cin = c1 + c2
    w, b = weights((Cout, Cin) + K, Cin * K[0] * K[1] * K[2], seed + 2)
    return x1, x2, w, b.to(DEV)


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_forward_and_input_gradient_edges(case):
    name, N, (c1, c2), Cout, dims, K, stride, pad, fwd_kernel, dgrad_kernels = case
    x1, x2, w, b = _conv_operands(case)
    cfg = ops.ConvCfg(stride, pad)
    (y, stats), fwd = routed(lambda: ops.conv_forward(x1, x2, w, b, cfg, ops.ACT_LRELU, 0.1, 2))
    wq = f64(w.to(BF))
    xr = f64(x1 if x2 is None else torch.cat([x1, x2], 1)).requires_grad_()
    pre = F.conv3d(xr, wq, None, stride, pad)
    ref = F.leaky_relu(pre.detach() + f64(b).view(1, -1, 1, 1, 1), 0.1)
    dz = act(tuple(ref.shape), 7 + sum(dims))
    (d1, d2), dgr = routed(lambda: ops.conv_dgrad(dz, w, dims, c1, c2, cfg))
    print(f"\n{name}: forward [{', '.join(fwd)}], input gradient [{', '.join(dgr)}]")
    assert fwd == [fwd_kernel] and dgr == dgrad_kernels, (fwd, dgr)
    assert y.dtype == BF and d1.dtype == BF and tuple(y.shape) == tuple(ref.shape)
    pre.backward(f64(dz))
    assert_bf16_bar(f"{name} y", y, ref)
    assert_conv_stats(f"{name} stats", stats, ref)
    assert_bf16_bar(f"{name} dx1", d1, xr.grad[:, :c1])
    if c2:
        assert_bf16_bar(f"{name} dx2", d2, xr.grad[:, c1:])


def test_persistent_case_walks_two_bricks_per_block():
    """halo_brick_plan's arithmetic restated for the 'halo persistent over samples' case: a retuned planner fails here,
    loudly, and does not silently lose the walk across a sample boundary."""
    case = next(c for c in CONV_CASES if c[0] == "halo persistent over samples")
    _, N, _, Cout, (D, H, W), _, _, _, kernel, _ = case
    assert kernel == "halo 2x16x16"
    BD, BH, BW, BN, want_blocks = 2, 16, 16, 32, 256           # halo_conv_bf16.hip: spec(2, 16, 16, 9), BN
    tiles_per_img = -(-D // BD) * -(-H // BH) * -(-W // BW)
    ntiles = N * tiles_per_img
    want = min(max(want_blocks // (ops.pad_rows(Cout) // BN), 1), ntiles)
    tiles_per_block = -(-ntiles // want)
    assert (tiles_per_img, ntiles, want, tiles_per_block) == (27, 81, 64, 2)
    # a block owns bricks [2k, 2k + 2): the sample boundaries 27 and 54 -- 27 is odd -- fall inside block 13 (26 | 27)
    assert tiles_per_img % tiles_per_block == 1 and N == 3


@pytest.mark.parametrize("halo", [False, True], ids=["generic", "halo"])
def test_fp32_output_flag_on_a_ragged_lattice(halo):
    """REHR_GG_Y_F32: bf16 operands, y stored as fp32 -- the same accumulators without the rounding, so the fp32 bar."""
    N, Cin, Cout, dims = 2, 32, 32, (7, 15, 31)
    x = act((N, Cin) + dims, 900)
    w, b = weights((Cout, Cin) + K3, Cin * 27, 902)
    b = b.to(DEV)
    wp, Npad = ops._pack(w, 0, BF)
    y = hip_backend.new_act(N, Cout, *dims, like=x, dtype=torch.float32)
    stats = torch.zeros((N, Cout, 2), dtype=torch.float64, device=DEV)

    def run():
        hip_backend.gather_gemm(x, None, Cin, dims, Cin, dims, S1, (-1, -1, -1), [ops.full_taps(3)] * 3, 3, 3, wp, Npad,
                                y, dims, Cout, (1, 1, 1), (0, 0, 0), b, ops.ACT_LRELU, 0.1, stats, 2, ops.choose_tile(dims))

    with halo_switch(halo):
        _, kernels = routed(run)
    print(f"\nfp32 output: [{', '.join(kernels)}]")
    assert kernels == ["halo 4x8x16" if halo else "generic"]
    ref = F.leaky_relu(F.conv3d(f64(x), f64(w.to(BF)), f64(b), 1, 1), 0.1)
    err = float((f64(y) - ref).abs().max() / ref.abs().max())
    print(f"fp32 output y {err / FP32_BAR:.3f}/1 (bar {FP32_BAR:g} of max)")
    assert err <= FP32_BAR
    assert_conv_stats("fp32 output stats", stats, ref)


# (name, (c1, c2), Cout, input (D, H, W), kernel, stride, pad, forward kernel)
TCONV_CASES = [
    ("tconv_ks 222, 82-row tail", (128, 0), 64, (3, 5, 7), (2, 2, 2), (2, 2, 2), (0, 0, 0), "tconv_ks"),
    ("tconv_ks 122, 80-row tail", (64, 0), 32, (4, 9, 10), (1, 2, 2), (1, 2, 2), (0, 0, 0), "tconv_ks"),
    ("tconv 222 Cin 192: phase grid", (192, 0), 64, (3, 5, 7), (2, 2, 2), (2, 2, 2), (0, 0, 0), "generic"),
    ("tconv 344/122 odd planes", (64, 0), 32, (3, 9, 11), (3, 4, 4), (1, 2, 2), (1, 1, 1), "generic"),
    ("tconv 344/122 two sources", (64, 32), 64, (3, 9, 11), (3, 4, 4), (1, 2, 2), (1, 1, 1), "generic"),
]


@pytest.mark.parametrize("case", TCONV_CASES, ids=[c[0] for c in TCONV_CASES])
def test_conv_transpose_edges(case):
    name, (c1, c2), Cout, dims, K, stride, pad, fwd_kernel = case
    N, Cin = 2, c1 + c2
    seed = 5000 + 100 * [c[0] for c in TCONV_CASES].index(name)
    x1 = act((N, c1) + dims, seed)
    x2 = act((N, c2) + dims, seed + 1) if c2 else None
    # a ConvTranspose3d output sums Cin x (taps per phase) products
    w, _ = weights((Cin, Cout) + K, Cin * K[0] * K[1] * K[2] / (stride[0] * stride[1] * stride[2]), seed + 2)
    b = torch.randn(Cout, generator=torch.Generator().manual_seed(seed + 3)).to(DEV)
    cfg = ops.ConvCfg(stride, pad, transposed=True)
    (y, _), fwd = routed(lambda: ops.conv_forward(x1, x2, w, b, cfg, ops.ACT_NONE, 0.0, 0))
    wq = f64(w.to(BF))
    xr = f64(x1 if x2 is None else torch.cat([x1, x2], 1)).requires_grad_()
    pre = F.conv_transpose3d(xr, wq, None, stride, pad)
    ref = pre.detach() + f64(b).view(1, -1, 1, 1, 1)
    dz = act(tuple(ref.shape), seed + 4)
    (d1, d2), dgr = routed(lambda: ops.conv_dgrad(dz, w, dims, c1, c2, cfg))
    print(f"\n{name}: forward [{', '.join(fwd)}], input gradient [{', '.join(dgr)}]")
    assert fwd == [fwd_kernel] and dgr == ["generic"] * (2 if c2 else 1), (fwd, dgr)
    assert y.dtype == BF and tuple(y.shape) == tuple(ref.shape)
    pre.backward(f64(dz))
    assert_bf16_bar(f"{name} y", y, ref)
    assert_bf16_bar(f"{name} dx1", d1, xr.grad[:, :c1])
    if c2:
        assert_bf16_bar(f"{name} dx2", d2, xr.grad[:, c1:])
