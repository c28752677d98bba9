"""The thin-channel convolution kernels (csrc/direct_conv.hip, csrc/thin_cin_conv.hip) against torch.nn.functional /
torch.nn.grad in fp64 on the CPU, on the same fp32 operands, one row per launch regime.  The rows and the regime each
is there for are in tests/thin_kernel_cases.py; tests/test_thin_kernel_regimes_cpu.py confirms the regime column from the
library's route and size queries without a device.  Routes are forced through rehrseg_amd.hip_backend where
ops.conv_* would choose another kernel (hb.small_cin_fwd, hb.small_cin_wgrad at Cout 32 / 64, hb.im2col,
hb.small_cout_*); the matrix-core rows and the Cout 16 gradients go through ops.conv_forward / ops.conv_wgrad, whose
routing is then part of what is tested.

Which row reaches which kernel (the table's regime column has the block geometry):
  small_cin_fwd_kernel                       VFWD: wave groups 1 / 2 / 4, partial tiles, the persistent walk under both
                                             block caps (512 / N with statistics, 4096 / N without), > 48 KB of LDS
  small_cin_wgrad_kernel<8> / <40>           VWG: blocks over two samples, an idle wave, masked lanes, 69 voxels per block
  im2col_kernel                              IM2COL (bit-equal to a gather), IM2COL_GEMM (with the 1x1x1 weight gradient)
  thin_cin_fwd_kernel<2|4, float|bf16>       MFWD: runs of tiles with a short last block, KW 1 / 2 / 5 / 7 / 8, strides
  thin_cin_wgrad_kernel<2|4, 1|2|10, f32|bf16>  MWG: runs of tiles, every admitted tap-tile count at tap shapes never run
  small_cout_fwd_kernel<2|4>, small_cout_fwd_cg_kernel<2|4, 4|8|16>, small_cout_dgrad_kernel<2|4> (scalar and 16-byte dY
  loads), small_cout_wgrad_kernel<2|4>, small_cout_wgrad_cg_kernel<2|4, 4|8|16>, small_cout_wgrad_halo_kernel<2|4>,
  small_cout2_wgrad_rows_kernel<5>           OUT
Not reached by any test-sized shape: the 8192-block cap of the plain thin-output forward and input gradient (> 16 M
voxels) and the 16384-block cap of the channel-group forward (> 2 M voxels at Cin 64).  The thin5 kernels have their own
fp64 tests.

Operands: x, dy ~ N(0, 1), sample n of x is a_n * x + b_n with (a, b) = (1, 0), (3, 2), (0.5, -1), ... so that a wrong
sample index cannot cancel; w ~ N(0, 1) / sqrt(Cin * T); bias ~ N(0, 1).

Bars (from the arithmetic, as in test_stream_kernels_gpu.py; every test prints "name measured/bar" before it asserts):
every output, input gradient, weight gradient, bias gradient and statistic is an fp32 sum, and
|got - ref| <= 5e-6 * sum |summand| per output element, where sum |summand| is the same fp64 operation on the absolute
values of the operands (+ |bias|); for the statistics the sum over the voxels of that bound (and of its square).  Printed
as the largest ratio (bar 1).  Where the bound is 0 (no summand: padding only) the kernel must return exactly 0.
ReLU / LeakyReLU are applied inside the entry points.  Both are 1-Lipschitz, |act(a) - act(b)| <= |a - b|, so the bar of
the pre-activation holds for the activated output as it stands and no output near the kink has to be excluded.
bf16 stores and bf16 dY: bit-equal to the fp32 kernel on the same values (the store rounds the same fp32 result; the
gradient kernel converts dY exactly).  Weight gradients are called twice and must be bit-equal: slabs are summed in a
fixed order.

Largest measured ratio per family on an MI355X (bar 1):
  vector forward           y 0.081 (2->64 5x7x7)             sum 0.0018   sum of squares 0.0011
  vector weight gradient   dw 0.030 (1->16 3x3x3, 3 samples)  db 0.0084
  im2col + GEMM            dw 0.013 (1->32 5x7x7)            db 0.0026    (the im2col itself is bit-equal)
  matrix-core forward      y 0.057 (1->64 3x3x3, runs)       sum 0.0048   sum of squares 0.0052
  matrix-core gradient     dw 0.012 (1->64 6x5x5)            db 0.0009
  thin-output forward      y 0.036 (80->2 1x3x3)
  thin-output dgrad        dx 0.077 (16->2 5x5x5, 2205 bricks)
  thin-output gradient     dw 0.016 (16->2 5x5x5)            db 0.0043
Wall time of the file on an MI355X: 8.5 s for its 162 tests (the three passes of the 2205-brick row take 1.6 s each, nearly
all of it the fp64 reference on the CPU).

Found by this file: small_cout_wgrad_cg_kernel combined its lanes with LDS float atomics, which land in arrival order --
two launches on the same operands differed in the last bit once a row had more voxels than one wave covers (W >= 13 at
Cin 32).  It now combines in a fixed order (xor butterfly inside a wave, then the four waves in turn).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from rehrseg_amd import hip_backend as hb
from rehrseg_amd import ops
from thin_kernel_cases import IM2COL, IM2COL_GEMM, MFWD, MWG, OUT, VFWD, VWG, FAMILIES, ids

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ACTS = [(ops.ACT_NONE, 0.0), (ops.ACT_RELU, 0.0), (ops.ACT_LRELU, 0.01)]
SAMPLE_AFFINE = [(1.0, 0.0), (3.0, 2.0), (0.5, -1.0), (2.0, 1.0)]


# ----------------------------------------------------------------------------- operands and references
def _randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last_3d)


def _act_dev(t):
    """An activation (N, C, D, H, W) on the device, NDHWC."""
    return _cl(t.to(DEV))


@functools.lru_cache(maxsize=None)
def _operands(fam, i):
    """CPU fp32 operands of row i of a family: x, w, bias, dy (default layout; nothing here is ever written to)."""
    r = FAMILIES[fam][i]
    seed = 7000 + 1000 * sorted(FAMILIES).index(fam) + 8 * i
    T = r["K"][0] * r["K"][1] * r["K"][2]
    x = _randn((r["N"], r["Cin"]) + r["inp"], seed)
    for n in range(r["N"]):
        a, b = SAMPLE_AFFINE[n % 4]
        x[n] = a * x[n] + b
    w = _randn((r["Cout"], r["Cin"]) + r["K"], seed + 1) / (r["Cin"] * T) ** 0.5
    return x, w, _randn((r["Cout"],), seed + 2), _randn((r["N"], r["Cout"]) + r["out"], seed + 3)


@functools.lru_cache(maxsize=None)
def _fwd_ref(fam, i, with_bias=True):
    """fp64 pre-activation and the per-element sum of |summand|."""
    r = FAMILIES[fam][i]
    x, w, b, _ = (t.double() for t in _operands(fam, i))
    b = b if with_bias else None
    return (F.conv3d(x, w, b, r["stride"], r["pad"]),
            F.conv3d(x.abs(), w.abs(), None if b is None else b.abs(), r["stride"], r["pad"]))


def _wgrad_ref(r, x, dy):
    """fp64 (dw, sum |summand| of dw, db, sum |summand| of db) for fp32 operands x, dy."""
    x, dy = x.double(), dy.double()
    shape = (r["Cout"], r["Cin"]) + r["K"]
    return (torch.nn.grad.conv3d_weight(x, shape, dy, r["stride"], r["pad"]),
            torch.nn.grad.conv3d_weight(x.abs(), shape, dy.abs(), r["stride"], r["pad"]),
            dy.sum((0, 2, 3, 4)), dy.abs().sum((0, 2, 3, 4)))


@functools.lru_cache(maxsize=None)
def _wgrad_ref_of(fam, i):
    x, _, _, dy = _operands(fam, i)
    return _wgrad_ref(FAMILIES[fam][i], x, dy)


def _ratio(got, ref, scale):
    """Largest ratio of |got - ref| to 5e-6 * scale (bar 1); scale = the fp64 sum of |summand| per output."""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape == scale.shape, (got.shape, ref.shape, scale.shape)
    assert bool(torch.isfinite(got).all())
    return float(((got - ref).abs() / (5e-6 * scale + 1e-300)).max()), 1.0


def _check(tag, figs):
    """figs: name -> (measured, bar); prints every figure, then asserts all of them."""
    print(f"[thin {tag}] " + " ".join(f"{k} {v:.2e}/{b:.1e}" for k, (v, b) in figs.items()))
    for k, (v, b) in figs.items():
        assert v <= b, (tag, k, v, b)


def _act(z, act, slope):
    return F.relu(z) if act == ops.ACT_RELU else (F.leaky_relu(z, slope) if act == ops.ACT_LRELU else z)


def _stats_figs(stats, mode, z, A, act, slope):
    """Statistics epilogue: (N, Cout, 2) doubles = sum and sum of squares of the activated fp32 outputs over the voxels
    (mode 1: the sum alone, the second slot stays 0)."""
    if mode == 0:
        assert stats is None
        return {}
    st = stats.detach().cpu()
    r = _act(z, act, slope)
    figs = {"sum": _ratio(st[..., 0], r.sum((2, 3, 4)), A.sum((2, 3, 4)))}
    if mode == 2:
        figs["sumsq"] = _ratio(st[..., 1], (r * r).sum((2, 3, 4)), (A * A).sum((2, 3, 4)))
    else:
        assert bool((st[..., 1] == 0).all())
    return figs


# ----------------------------------------------------------------------------- thin input, vector forward
_VF = [(i, m) for i, r in enumerate(VFWD) for m in r.get("stats_modes", (0, 1, 2))]


@pytest.mark.parametrize("i,mode", _VF, ids=[f"{ids(VFWD)[i]}-stats{m}" for i, m in _VF])
def test_vector_forward(i, mode):
    r = VFWD[i]
    x, w, b, _ = _operands("VFWD", i)
    xd, wd = _act_dev(x), w.to(DEV)
    figs = {}
    for with_bias in (True, False) if r.get("bias_free_too") else (True,):
        z, A = _fwd_ref("VFWD", i, with_bias)
        y = hb.new_act(r["N"], r["Cout"], *r["out"], like=xd)
        stats = torch.zeros((r["N"], r["Cout"], 2), dtype=torch.float64, device=DEV) if mode else None
        hb.small_cin_fwd(xd, wd, b.to(DEV) if with_bias else None, y, r["stride"], r["pad"], ops.ACT_NONE, 0.0, stats, mode)
        sfx = "" if with_bias else " (no bias)"
        figs["y" + sfx] = _ratio(y, z, A)
        figs.update({k + sfx: v for k, v in _stats_figs(stats, mode, z, A, ops.ACT_NONE, 0.0).items()})
    _check(f"vfwd {r['name']} stats {mode}", figs)


# ----------------------------------------------------------------------------- thin input, vector weight gradient
@pytest.mark.parametrize("i", range(len(VWG)), ids=ids(VWG))
def test_vector_weight_gradient(i):
    r = VWG[i]
    x, w, _, dy = _operands("VWG", i)
    xd, wd, dyd = _act_dev(x), w.to(DEV), _act_dev(dy)
    cfg = ops.ConvCfg(r["stride"], r["pad"], False)
    assert not hb.small_cin_wgrad_on_mfma(xd, wd, dyd, r["stride"], r["pad"])

    def run(want_bias):
        if r["via"] == "ops":
            return ops.conv_wgrad(dyd, xd, None, wd, cfg, want_bias)
        return hb.small_cin_wgrad(xd, wd, dyd, r["stride"], r["pad"], want_bias)
    dw, db = run(True)
    dw2, db2 = run(True)
    dw3, db3 = run(False)
    assert torch.equal(dw, dw2) and torch.equal(db, db2) and torch.equal(dw, dw3) and db3 is None
    rw, sw, rb, sb = _wgrad_ref_of("VWG", i)
    _check(f"vwg {r['name']}", {"dw": _ratio(dw, rw, sw), "db": _ratio(db, rb, sb)})


# ----------------------------------------------------------------------------- im2col
def _gather(r, x, kpad):
    """out[n, ci * T + tap, o] = x[n, ci, o * stride - pad + tap], 0 in the padding and in columns Cin * T .. Kpad - 1."""
    (KD, KH, KW), (sd, sh, sw), (pd, ph, pw), (Do, Ho, Wo) = r["K"], r["stride"], r["pad"], r["out"]
    xp = F.pad(x, (pw, pw, ph, ph, pd, pd))
    col = torch.zeros((r["N"], kpad, Do, Ho, Wo), dtype=torch.float32)
    k = 0
    for ci in range(r["Cin"]):
        for kd in range(KD):
            for kh in range(KH):
                for kw in range(KW):
                    col[:, k] = xp[:, ci, kd:kd + (Do - 1) * sd + 1:sd, kh:kh + (Ho - 1) * sh + 1:sh,
                                   kw:kw + (Wo - 1) * sw + 1:sw]
                    k += 1
    return col


@pytest.mark.parametrize("i", range(len(IM2COL)), ids=ids(IM2COL))
def test_im2col_is_a_gather(i):
    r = IM2COL[i]
    x, w, _, _ = _operands("IM2COL", i)
    kpad = r["regime"][0]
    col = hb.im2col(_act_dev(x), w.to(DEV), r["out"], r["stride"], r["pad"], kpad)
    assert tuple(col.shape) == (r["N"], kpad) + r["out"]
    ref = _gather(r, x, kpad)
    got = col.cpu().contiguous()
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))     # bit-equal: padding is +0.0
    assert bool((ref[:, r["Cin"] * r["K"][0] * r["K"][1] * r["K"][2]:] == 0).all())


@pytest.mark.parametrize("i", range(len(IM2COL_GEMM)), ids=ids(IM2COL_GEMM))
def test_im2col_gemm_weight_gradient(i):
    r = IM2COL_GEMM[i]
    x, w, _, dy = _operands("IM2COL_GEMM", i)
    xd, wd, dyd = _act_dev(x), w.to(DEV), _act_dev(dy)
    assert not hb.small_cin_wgrad_on_mfma(xd, wd, dyd, r["stride"], r["pad"])
    cfg = ops.ConvCfg(r["stride"], r["pad"], False)
    dw, db = ops.conv_wgrad(dyd, xd, None, wd, cfg, True)
    dw2, db2 = ops.conv_wgrad(dyd, xd, None, wd, cfg, True)
    assert torch.equal(dw, dw2) and torch.equal(db, db2) and dw.shape == w.shape
    rw, sw, rb, sb = _wgrad_ref_of("IM2COL_GEMM", i)
    _check(f"im2col+gemm {r['name']}", {"dw": _ratio(dw, rw, sw), "db": _ratio(db, rb, sb)})


# ----------------------------------------------------------------------------- thin input, matrix-core forward
_MF = [(i, m, a) for i, r in enumerate(MFWD) for m in r.get("stats_modes", (2,))
       for a in ((0, 1, 2) if r.get("acts") and m == 2 else (1,))]


@pytest.mark.parametrize("i,mode,a", _MF, ids=[f"{ids(MFWD)[i]}-stats{m}-{('none', 'relu', 'lrelu')[a]}" for i, m, a in _MF])
def test_matrix_core_forward(i, mode, a):
    r = MFWD[i]
    act, slope = ACTS[a]
    x, w, b, _ = _operands("MFWD", i)
    xd, wd, bd = _act_dev(x), w.to(DEV), b.to(DEV)
    assert hb.small_cin_bf16_out_ok(tuple(x.shape), tuple(w.shape), r["stride"], r["pad"])
    cfg = ops.ConvCfg(r["stride"], r["pad"], False)
    y32, st32 = ops.conv_forward(xd, None, wd, bd, cfg, act, slope, mode)
    with ops.mixed_precision():
        y16, st16 = ops.conv_forward(xd, None, wd, bd, cfg, act, slope, mode)
    assert y32.dtype == torch.float32 and y16.dtype == torch.bfloat16
    assert torch.equal(y16, y32.to(torch.bfloat16))
    assert (st16 is None and st32 is None) or torch.equal(st16, st32)
    z, A = _fwd_ref("MFWD", i)
    figs = {"y": _ratio(y32, _act(z, act, slope), A)}
    figs.update(_stats_figs(st32, mode, z, A, act, slope))
    _check(f"mfwd {r['name']} stats {mode} act {a}", figs)


# ----------------------------------------------------------------------------- thin input, matrix-core weight gradient
@pytest.mark.parametrize("i", range(len(MWG)), ids=ids(MWG))
def test_matrix_core_weight_gradient(i):
    r = MWG[i]
    x, w, _, dy = _operands("MWG", i)
    dy16 = dy.to(torch.bfloat16)                 # the operand of both calls and of the reference: bf16-representable
    xd, wd, d16, d32 = _act_dev(x), w.to(DEV), _act_dev(dy16), _act_dev(dy16.float())
    assert hb.small_cin_wgrad_on_mfma(xd, wd, d32, r["stride"], r["pad"])
    cfg = ops.ConvCfg(r["stride"], r["pad"], False)
    dw, db = ops.conv_wgrad(d32, xd, None, wd, cfg, True)
    dw2, db2 = ops.conv_wgrad(d32, xd, None, wd, cfg, True)
    dw3, db3 = ops.conv_wgrad(d32, xd, None, wd, cfg, False)
    dwb, dbb = ops.conv_wgrad(d16, xd, None, wd, cfg, True)
    dwb3, dbb3 = ops.conv_wgrad(d16, xd, None, wd, cfg, False)
    assert torch.equal(dw, dw2) and torch.equal(db, db2) and torch.equal(dw, dw3) and db3 is None
    assert torch.equal(dwb, dw) and torch.equal(dbb, db) and torch.equal(dwb3, dw) and dbb3 is None
    rw, sw, rb, sb = _wgrad_ref(r, x, dy16.float())
    _check(f"mwg {r['name']}", {"dw": _ratio(dw, rw, sw), "db": _ratio(db, rb, sb)})


# ----------------------------------------------------------------------------- thin output
@pytest.mark.parametrize("i", range(len(OUT)), ids=ids(OUT))
def test_thin_output_forward(i):
    r = OUT[i]
    x, w, b, _ = _operands("OUT", i)
    xd, wd = _act_dev(x), w.to(DEV)
    figs = {}
    for with_bias in (True, False) if r.get("bias_free_too") else (True,):
        z, A = _fwd_ref("OUT", i, with_bias)
        for a in (0, 1, 2) if r.get("acts") else (0,):
            act, slope = ACTS[a]
            y = hb.new_act(r["N"], r["Cout"], *r["out"], like=xd)
            hb.small_cout_fwd(xd, wd, b.to(DEV) if with_bias else None, y, r["pad"], act, slope)
            figs["y" + ("" if with_bias else " (no bias)") + ("", " relu", " lrelu")[a]] = _ratio(y, _act(z, act, slope), A)
    _check(f"out fwd {r['name']}", figs)


@pytest.mark.parametrize("i", range(len(OUT)), ids=ids(OUT))
def test_thin_output_input_gradient(i):
    r = OUT[i]
    x, w, _, dy = _operands("OUT", i)
    dx = hb.small_cout_dgrad(_act_dev(dy), w.to(DEV), tuple(x.shape), r["pad"])
    ref = torch.nn.grad.conv3d_input(tuple(x.shape), w.double(), dy.double(), 1, r["pad"])
    scale = torch.nn.grad.conv3d_input(tuple(x.shape), w.double().abs(), dy.double().abs(), 1, r["pad"])
    _check(f"out dgrad {r['name']}", {"dx": _ratio(dx, ref, scale)})


@pytest.mark.parametrize("i", range(len(OUT)), ids=ids(OUT))
def test_thin_output_weight_gradient(i):
    r = OUT[i]
    x, w, _, dy = _operands("OUT", i)
    xd, wd, dyd = _act_dev(x), w.to(DEV), _act_dev(dy)
    dw, db = hb.small_cout_wgrad(xd, wd, dyd, r["pad"], True)
    dw2, db2 = hb.small_cout_wgrad(xd, wd, dyd, r["pad"], True)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    if r.get("bias_free_too"):
        dw3, db3 = hb.small_cout_wgrad(xd, wd, dyd, r["pad"], False)
        assert torch.equal(dw, dw3) and db3 is None
    rw, sw, rb, sb = _wgrad_ref_of("OUT", i)
    _check(f"out wgrad {r['name']}", {"dw": _ratio(dw, rw, sw), "db": _ratio(db, rb, sb)})
