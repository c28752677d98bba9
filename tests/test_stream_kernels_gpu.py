"""The streaming per-channel kernels (csrc/stream_ew.hip) and the reduction kernels of csrc/elementwise.hip, called
through the rehrseg_amd.hip_backend wrappers, against plain torch in fp64 on the CPU (torch.nn.functional + autograd;
for bf16 on the same bf16-rounded operands).  The fused-block tests reach these kernels with one block per sample and a
channel-group count that divides 256 only; the shapes here are chosen against the launch geometry instead.

Launch geometry of stream_ew.hip (restated in _stream_geometry, asserted per case): a thread owns CPT channels (4 fp32 /
8 bf16), cgn = C / CPT threads cover a row, rpp = 256 // cgn rows are in flight per pass (256 - rpp * cgn threads idle),
a block owns max(ceil(S / (2048 // N)), 32 * rpp) rows rounded up to whole unrolled passes of 4 * rpp, the last block of
a sample carries the tail.  N = 2 unless noted; sample n is a_n * x + b_n with (a, b) = (1, 0), (3, 2), (0.5, -1), so a
wrong sample index cannot cancel.

  fp32   C     D x H x W  (S)       regime
         32    1 x 3 x 683 (2049)   rpp 32, 1024 rows / block: 3 blocks, the last holds one row
         64    2 x 16 x 16 (512)    rpp 16: exactly one full block, no tail
         96    3 x 11 x 13 (429)    cgn 24, rpp 10, 16 idle threads: 2 blocks, tail 109 (unrolled passes + remainder)
         320   4 x 10 x 25 (1000)   cgn 80, rpp 3, 16 idle threads: 11 blocks, tail 40
         512   1 x 7 x 9 (63), 1 x 1 x 1 (1); N = 1 and 3   rpp 2: fewer rows than a block / than row lanes
         4     1 x 5 x 7 (35)       cgn 1, rpp 256: most lanes idle
         1024  1 x 5 x 8 (40), N = 1   cgn 256, rpp 1 (the largest C the entry points take): 2 blocks, tail 8
  bf16   32    1 x 3 x 683 (2049)   rpp 64, 2048 rows / block: 2 blocks, the last holds one row
         48    2 x 26 x 26 (1352)   cgn 6, rpp 42, 4 idle threads: 2 blocks, the last holds 8 rows
         320   4 x 10 x 25 (1000)   cgn 40, rpp 6, 16 idle threads: 6 blocks, tail 40
         64    1 x 1 x 1 (1), N = 3 one row

Reduction kernels of elementwise.hip (column_reduce: 4 channels per thread in both dtypes, a block owns
max(ceil(rows / (2048 // N)), 8 * rpp) rows; _reduce_geometry): per C one single-block shape and one with several
blocks and a tail, see RED_CASES.  The SE gate kernels take any C >= 1: C = 66 and 130 are accepted (no row of the
tables had to change) and give se_gate_bwd_k_kernel unequal slices and an odd pair tail.

Bars (from the arithmetic, not from the kernels; every test prints "name measured/bar" before it asserts):
  * fp32 element-wise outputs (y, dx, dres, mean_rstd, gate means): max |got - ref| <= 1e-5 * max |ref| -- 2-8 fp32
    operations (2^-24 each) on O(1) operands, the bar of the fp32 thin-conv tests.
  * bf16-stored outputs, element by element: |got - ref| <= 2^-8 |ref| + 1e-5 max |ref|.  The arithmetic is fp32, the
    store rounds to nearest: at most half a bf16 ulp, which is 2^-8 relative at a power of two (truncation loses up to
    2^-7); the absolute term covers the fp32 arithmetic including the cancellation in x * sc + sh.  Printed as the
    largest ratio to that per-element bar (bar 1).
  * Reductions (dgamma, dbeta, dgate, conv-bias sums, channel sums, slab / cosine statistics, dw / db / k of the gate):
    |got - ref| <= 5e-6 * sum |summand| per output, the sum over the fp64 reference's summands (the factor and the
    conditioning scale of test_instnorm_backward_carries_the_conv_bias_gradient): partial sums are fp32 over at most
    one unrolled pass / one block row walk and fp64 from there on.  Printed as the largest ratio (bar 1).  Quantities
    kept in fp64 to the end (dgate, slab and cosine statistics) come out far below it.
  * The SE gate itself is sigmoid of a C-term fp32 dot product: |got - ref| <= 1e-5 max |ref| + 0.25 * 5e-6 *
    (sum_k |W[c,k] mean[k]| + |b[c]|) (sigmoid' <= 1/4 on the reduction bar of its argument).  The gate operands keep
    |W mean + b| < ~2.5, where rounding gate to fp32 moves g (1 - g) by < 1e-6 relative (|1 - 2g| / (1 - g) * 2^-24).
  * One row per sample (S = 1): the variance is 0, rstd = eps^-1/2 = 316, the reference is the constant act(beta) and a
    zero gradient, and (x - mean) * rstd is the rounding residue of two terms of size |x * rstd| -- in any fp32
    evaluation.  "max |ref|" is no scale for that: at S = 1 the InstanceNorm comparisons use the size of the cancelling
    terms in its place (max |x rstd gamma| forward, max |rstd gamma dz| for dx, sum |dz x rstd| for dgamma, sum
    |rstd gamma dz| for the conv-bias sums), with the same factors.  Every other case uses the bars above as they are.
  * Activation kink: instnorm_act_bwd recomputes the pre-activation z, so rounding decides the branch within ~1e-6 of 0;
    dy is zeroed where the reference has |z| <= 1e-5 max |z| (asserted to be at most 0.1 % of a case; beta is kept
    near 0.5 so that the S = 1 cases, where z = beta, stay off the kink).  Kernels that take the saved output y get a
    few exact zeros in it: y > 0 takes the positive branch, y == 0 the negative one, as torch's (leaky_)relu backward.

Called twice: every wrapper that draws a zero-initialised fp64 accumulator from hip_backend.zeros_f64, or zeroes a
scratch itself, is called twice in a row; fp32 / bf16 outputs must be bit-equal.  (The cross-block double atomics may
change order between two launches where a sample has three or more blocks; that moves the fp64 sum by ~1e-16 relative
and a float rounded from it with probability ~1e-8 per value.)  The fp64 dgate accumulators themselves must agree to
1e-12 of their conditioning scale, and the second call is the one compared with the reference.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from rehrseg_amd import hip_backend as hb
from rehrseg_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF = torch.float32, torch.bfloat16
EPS = 1e-5
ACTS = [(ops.ACT_NONE, 0.0), (ops.ACT_RELU, 0.0), (ops.ACT_LRELU, 0.01)]
ACT_IDS = ["none", "relu", "lrelu"]
SAMPLE_AFFINE = [(1.0, 0.0), (3.0, 2.0), (0.5, -1.0)]

# (dtype, N, C, (D, H, W), blocks per sample, rows of the last block, idle threads)
STREAM_CASES = [
    (F32, 2, 32, (1, 3, 683), 3, 1, 0),
    (F32, 2, 64, (2, 16, 16), 1, 512, 0),
    (F32, 2, 96, (3, 11, 13), 2, 109, 16),
    (F32, 2, 320, (4, 10, 25), 11, 40, 16),
    (F32, 1, 512, (1, 7, 9), 1, 63, 0),
    (F32, 3, 512, (1, 7, 9), 1, 63, 0),
    (F32, 1, 512, (1, 1, 1), 1, 1, 0),
    (F32, 3, 512, (1, 1, 1), 1, 1, 0),
    (F32, 2, 4, (1, 5, 7), 1, 35, 0),
    (F32, 1, 1024, (1, 5, 8), 2, 8, 0),
    (BF, 2, 32, (1, 3, 683), 2, 1, 0),
    (BF, 2, 48, (2, 26, 26), 2, 8, 4),
    (BF, 2, 320, (4, 10, 25), 6, 40, 16),
    (BF, 3, 64, (1, 1, 1), 1, 1, 0),
]
F32_CASES = [c for c in STREAM_CASES if c[0] == F32]
BF_CASES = [c for c in STREAM_CASES if c[0] == BF]


def _cid(c):
    return f"{'bf16' if c[0] == BF else 'fp32'}-N{c[1]}-C{c[2]}-{'x'.join(map(str, c[3]))}"


def _stream_geometry(S, C, N, cpt):
    """rows_per_block_for / make_span of stream_ew.hip -> (blocks per sample, rows of the last block, idle threads)."""
    cgn = C // cpt
    rpp = 256 // cgn
    rpb = max(-(-S // max(2048 // N, 1)), 32 * rpp)
    rpb = -(-rpb // (4 * rpp)) * (4 * rpp)
    blocks = -(-S // rpb)
    return blocks, S - (blocks - 1) * rpb, 256 - rpp * cgn


def _reduce_geometry(rows, C, N):
    """rows_per_block_for / column_reduce of elementwise.hip -> (blocks over `rows`, rows of the last block)."""
    rpp = 256 // (C // 4)
    rpb = max(-(-rows // max(2048 // N, 1)), 8 * rpp)
    blocks = -(-rows // rpb)
    return blocks, rows - (blocks - 1) * rpb


@pytest.mark.parametrize("case", STREAM_CASES, ids=_cid)
def test_case_lands_in_its_regime(case):
    dt, N, C, dims, blocks, tail, idle = case
    S = dims[0] * dims[1] * dims[2]
    assert _stream_geometry(S, C, N, 8 if dt == BF else 4) == (blocks, tail, idle)


# ----------------------------------------------------------------------------- operands and figures
def _randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def _cl(t, dt):
    return t.to(dt).contiguous(memory_format=torch.channels_last_3d)


@functools.lru_cache(maxsize=None)
def _operands(case):
    """CPU operands of a case in its dtype, NDHWC: x (sample n = a_n x + b_n), r (a second activation), dy, and the
    fp32 per-channel vectors gamma, beta and per-(n, c) gate / k."""
    dt, N, C, dims = case[:4]
    seed = 1000 + STREAM_CASES.index(case) * 16
    x = _randn((N, C) + dims, seed)
    for n, (a, b) in enumerate(SAMPLE_AFFINE[:N]):
        x[n] = a * x[n] + b
    return {
        "x": _cl(x, dt), "r": _cl(_randn((N, C) + dims, seed + 1), dt), "dy": _cl(_randn((N, C) + dims, seed + 2), dt),
        "gamma": torch.rand(C, generator=torch.Generator().manual_seed(seed + 3)) + 0.5,
        "beta": _randn((C,), seed + 4) * 0.1 + 0.5,
        "gate": torch.rand(N, C, generator=torch.Generator().manual_seed(seed + 5)) * 0.9 + 0.05,
        "k": _randn((N, C), seed + 6),
    }


def _dev(t):
    return t.to(DEV)


def _cpu64(t):
    return t.detach().cpu().double()


def _ref(t):
    """fp64 copy in torch's default layout: the reference never sees the kernels' memory format."""
    return t.detach().double().contiguous()


def _act(z, act, slope):
    if act == ops.ACT_RELU:
        return F.relu(z)
    if act == ops.ACT_LRELU:
        return F.leaky_relu(z, slope)
    return z


def _dact(v, act, slope):
    """act'(.) as the kernels and torch's backward take it from a pre-activation or a saved output v: 1 where v > 0."""
    if act == ops.ACT_NONE:
        return torch.ones_like(v, dtype=torch.float64)
    return (v > 0).double() + (v <= 0).double() * slope


def _with_zeros(t, step, dt):
    """t (NDHWC, any dtype) with every step-th element (in NCDHW order) set to exactly 0, NDHWC in dtype dt."""
    t = t.float().contiguous()
    t.view(-1)[::step] = 0
    return _cl(t, dt)


def _elem(got, ref, dt, scale=None):
    """Element-wise figure and bar: fp32 max |got - ref| against 1e-5 * scale; bf16 the largest ratio of |got - ref| to
    2^-8 |ref| + 1e-5 * scale (bar 1).  scale = max |ref| unless the caller gives the conditioning scale."""
    assert got.dtype == dt, (got.dtype, dt)
    got, ref = _cpu64(got), ref.detach()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = float(ref.abs().max()) if scale is None else scale
    d = (got - ref).abs()
    if dt == BF:
        return float((d / (2.0 ** -8 * ref.abs() + 1e-5 * scale + 1e-300)).max()), 1.0
    return float(d.max()), 1e-5 * scale


def _red(got, ref, scale):
    """Largest ratio of |got - ref| to 5e-6 * scale, scale = the fp64 sum of |summand| per output (bar 1)."""
    got, ref = _cpu64(got), ref.detach()
    assert got.shape == ref.shape == scale.shape, (got.shape, ref.shape, scale.shape)
    return float(((got - ref).abs() / (5e-6 * scale + 1e-300)).max()), 1.0


def _check(tag, figs):
    """figs: name -> (measured, bar); prints every figure, then asserts all of them."""
    print(f"[stream {tag}] " + " ".join(f"{k} {v:.2e}/{b:.1e}" for k, (v, b) in figs.items()))
    for k, (v, b) in figs.items():
        assert v <= b, (tag, k, v, b)


def _same(a, b):
    assert len(a) == len(b)
    for s, t in zip(a, b):
        assert (s is None and t is None) or torch.equal(s, t)


# ----------------------------------------------------------------------------- 1, 2: InstanceNorm + activation
def _inorm(x, gamma, beta):
    """InstanceNorm3d(affine) in the operands' precision; one row per sample is spelled out (F.instance_norm refuses
    it): biased variance 0."""
    if x.shape[2] * x.shape[3] * x.shape[4] > 1:
        return F.instance_norm(x, weight=gamma, bias=beta, eps=EPS)
    m = x.mean((2, 3, 4), keepdim=True)
    v = ((x - m) ** 2).mean((2, 3, 4), keepdim=True)
    return (x - m) / torch.sqrt(v + EPS) * gamma.view(1, -1, 1, 1, 1) + beta.view(1, -1, 1, 1, 1)


def _moments(x):
    """fp64 (mean, rstd) per (n, c) and the {sum, sum of squares} buffer the conv epilogues would have formed."""
    s1, s2 = x.sum((2, 3, 4)), (x * x).sum((2, 3, 4))
    m = x.mean((2, 3, 4))
    v = ((x - m[:, :, None, None, None]) ** 2).mean((2, 3, 4))
    return m, 1.0 / torch.sqrt(v + EPS), torch.stack([s1, s2], -1)


@pytest.mark.parametrize("act,slope", ACTS, ids=ACT_IDS)
@pytest.mark.parametrize("case", STREAM_CASES, ids=_cid)
def test_instnorm_act_fwd(case, act, slope):
    dt, N, C, dims = case[:4]
    S = dims[0] * dims[1] * dims[2]
    o = _operands(case)
    x = _ref(o["x"])
    gamma, beta = o["gamma"].double(), o["beta"].double()
    mean, rstd, stats = _moments(x)
    ref = _act(_inorm(x, gamma, beta), act, slope)
    y, mr = hb.instnorm_act_fwd(_dev(o["x"]), _dev(stats), _dev(o["gamma"]), _dev(o["beta"]), EPS, act, slope)
    cond = float((x * (rstd * gamma)[:, :, None, None, None]).abs().max()) if S == 1 else None
    _check(f"instnorm_act_fwd {_cid(case)} {ACT_IDS[act]}", {
        "y": _elem(y, ref, dt, cond),
        "mean": _elem(mr[..., 0], mean, F32),
        "rstd": _elem(mr[..., 1], rstd, F32),
    })


@pytest.mark.parametrize("act,slope", ACTS, ids=ACT_IDS)
@pytest.mark.parametrize("case", STREAM_CASES, ids=_cid)
def test_instnorm_act_bwd(case, act, slope):
    dt, N, C, dims = case[:4]
    S = dims[0] * dims[1] * dims[2]
    o = _operands(case)
    x = _ref(o["x"]).requires_grad_()
    gamma, beta = o["gamma"].double().requires_grad_(), o["beta"].double().requires_grad_()
    mean, rstd, _ = _moments(x.detach())
    z = _inorm(x, gamma, beta)
    zd = z.detach()
    k0 = (rstd * gamma.detach())[:, :, None, None, None]
    zscale = float(zd.abs().max()) if S > 1 else max(float(zd.abs().max()), float((x.detach() * k0).abs().max()))
    keep = zd.abs() > 1e-5 * zscale
    assert int((~keep).sum()) <= 1e-3 * keep.numel(), (int((~keep).sum()), keep.numel())
    dy = _cl(o["dy"].float() * keep.float(), dt)
    _act(z, act, slope).backward(_ref(dy))
    dz = _ref(dy) * _dact(zd, act, slope)
    xhat = (x.detach() - mean[:, :, None, None, None]) * rstd[:, :, None, None, None]
    s_dbeta = dz.abs().sum((0, 2, 3, 4))
    s_dgamma = (dz * xhat).abs().sum((0, 2, 3, 4))
    s_dcb = x.grad.abs().sum((0, 2, 3, 4))
    cond = None
    if S == 1:   # the scale of the terms that cancel (module docstring)
        cond = float((dz * k0).abs().max())
        s_dgamma = s_dgamma + (dz * x.detach() * rstd[:, :, None, None, None]).abs().sum((0, 2, 3, 4))
        s_dcb = s_dcb + (dz * k0).abs().sum((0, 2, 3, 4))
    mr = torch.stack([mean, rstd], -1).float()
    args = (_dev(dy), _dev(o["x"]), _dev(mr), _dev(o["gamma"]), _dev(o["beta"]), act, slope)
    hb.instnorm_act_bwd(*args)
    got = hb.instnorm_act_bwd(*args)
    _same(got, hb.instnorm_act_bwd(*args))
    figs = {"dx": _elem(got[0], x.grad, dt, cond), "dgamma": _red(got[1], gamma.grad, s_dgamma),
            "dbeta": _red(got[2], beta.grad, s_dbeta)}
    if dt == BF:
        gotb = hb.instnorm_act_bwd(*args, want_conv_bias=True)
        _same(gotb, hb.instnorm_act_bwd(*args, want_conv_bias=True))
        _same(gotb[:3], got)
        figs["dconv_bias"] = _red(gotb[3], x.grad.sum((0, 2, 3, 4)), s_dcb)
    _check(f"instnorm_act_bwd {_cid(case)} {ACT_IDS[act]} masked {int((~keep).sum())}", figs)


# ----------------------------------------------------------------------------- 3: SE scale + residual + activation
@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("act,slope", ACTS, ids=ACT_IDS)
@pytest.mark.parametrize("case", STREAM_CASES, ids=_cid)
def test_scale_res_act_fwd_bwd(case, act, slope, with_res):
    dt, N, C, dims = case[:4]
    o = _operands(case)
    # exact zeros of the pre-activation -> exact zeros of the saved output y
    xo, ro = _with_zeros(o["x"], 97, dt), _with_zeros(o["r"], 97, dt)
    x = xo.double().requires_grad_()
    res = ro.double().requires_grad_() if with_res else None
    gate = o["gate"].double().requires_grad_()
    z = x * gate[:, :, None, None, None]
    if with_res:
        z = z + res
    y = _act(z, act, slope)
    assert int((y.detach() == 0).sum()) > 0
    dy = o["dy"].double()
    y.backward(dy)
    tag = f"{_cid(case)} {ACT_IDS[act]} {'res' if with_res else 'nores'}"
    yk = hb.scale_res_act_fwd(_dev(xo), _dev(o["gate"]), _dev(ro) if with_res else None, act, slope)
    _check(f"scale_res_act_fwd {tag}", {"y": _elem(yk, y.detach(), dt)})

    ys = _cl(y.detach().float(), dt)                      # the saved output, in the operands' dtype
    dzr = dy * _dact(ys.double(), act, slope)
    args = (_dev(o["dy"]), _dev(ys), _dev(xo), _dev(o["gate"]), with_res, act, slope)
    first = hb.scale_res_act_bwd(*args)
    dx, dres, dgate = hb.scale_res_act_bwd(*args)
    _same(first[:2], (dx, dres))
    s_dgate = (dzr * x.detach()).abs().sum((2, 3, 4))
    assert float(((_cpu64(first[2]) - _cpu64(dgate)).abs() / (s_dgate + 1e-300)).max()) <= 1e-12
    figs = {"dx": _elem(dx, x.grad, dt), "dgate": _red(dgate, gate.grad, s_dgate)}
    if with_res:
        figs["dres"] = _elem(dres, res.grad, dt)
    else:
        assert dres is None
    _check(f"scale_res_act_bwd {tag}", figs)


# ----------------------------------------------------------------------------- 4: add_channel_const, act, channel_sum
@pytest.mark.parametrize("case", STREAM_CASES, ids=_cid)
def test_add_channel_const(case):
    dt = case[0]
    o = _operands(case)
    ref = o["x"].double() + o["k"].double()[:, :, None, None, None]
    x = _dev(o["x"]).clone(memory_format=torch.preserve_format)
    hb.add_channel_const(x, _dev(o["k"]))
    _check(f"add_channel_const {_cid(case)}", {"x": _elem(x, ref, dt)})


@pytest.mark.parametrize("act,slope", ACTS, ids=ACT_IDS)
@pytest.mark.parametrize("case", F32_CASES, ids=_cid)
def test_act_fwd(case, act, slope):
    o = _operands(case)
    y = hb.act_fwd(_dev(o["x"]), act, slope)
    _check(f"act_fwd {_cid(case)} {ACT_IDS[act]}", {"y": _elem(y, _act(o["x"].double(), act, slope), F32)})


def _saved_output(case, act, slope):
    """(z leaf in fp64, y = act(z) rounded to the case's dtype) with exact zeros in z."""
    dt = case[0]
    z = _with_zeros(_operands(case)["x"], 89, dt).double().requires_grad_()
    y = _act(z, act, slope)
    return z, y, _cl(y.detach().float(), dt)


@pytest.mark.parametrize("act,slope", ACTS, ids=ACT_IDS)
@pytest.mark.parametrize("case", STREAM_CASES, ids=_cid)
def test_act_bwd(case, act, slope):
    dt = case[0]
    dyo = _operands(case)["dy"]
    z, y, ys = _saved_output(case, act, slope)
    assert int((ys == 0).sum()) > 0
    y.backward(dyo.double())
    dx = hb.act_bwd(_dev(dyo), _dev(ys), act, slope)
    _check(f"act_bwd {_cid(case)} {ACT_IDS[act]}", {"dx": _elem(dx, z.grad, dt)})


@pytest.mark.parametrize("case", STREAM_CASES, ids=_cid)
def test_channel_sum(case):
    x = _operands(case)["x"]
    xd = x.double()
    hb.channel_sum(_dev(x))
    got = hb.channel_sum(_dev(x))
    _same((got,), (hb.channel_sum(_dev(x)),))
    _check(f"channel_sum {_cid(case)}", {"sum": _red(got, xd.sum((0, 2, 3, 4)), xd.abs().sum((0, 2, 3, 4)))})


# ----------------------------------------------------------------------------- 5, 6: reductions of elementwise.hip
# (C, (D, H, W), regime): per C one shape that one block covers and one with several blocks and a tail, for both
# launch rules: channel_sum_actgrad walks N * S rows as one sample, the split-K combine S rows per sample (N = 2)
RED_N = 2
RED_CASES = [
    # C, dims, (blocks, tail) of channel_sum_actgrad, (blocks, tail) per sample of sum_slabs with statistics
    (32, (1, 5, 7), (1, 70), (1, 35)),
    (32, (3, 11, 13), (4, 90), (2, 173)),
    (96, (1, 5, 7), (1, 70), (1, 35)),
    (96, (3, 11, 13), (11, 58), (6, 29)),
    (320, (1, 2, 5), (1, 20), (1, 10)),
    (320, (1, 5, 7), (3, 22), (2, 11)),
]


def _rid(c):
    return f"C{c[0]}-{'x'.join(map(str, c[1]))}"


@pytest.mark.parametrize("rc", RED_CASES, ids=_rid)
def test_reduction_case_lands_in_its_regime(rc):
    C, dims, actgrad, slabs = rc
    S = dims[0] * dims[1] * dims[2]
    assert _reduce_geometry(RED_N * S, C, 1) == actgrad
    assert _reduce_geometry(S, C, RED_N) == slabs
    assert (actgrad[0] == 1) == (slabs[0] == 1)


@pytest.mark.parametrize("act,slope", ACTS, ids=ACT_IDS)
@pytest.mark.parametrize("dt", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rc", RED_CASES, ids=_rid)
def test_channel_sum_actgrad(rc, dt, act, slope):
    C, dims = rc[:2]
    seed = 3000 + RED_CASES.index(rc) * 8
    zo = _randn((RED_N, C) + dims, seed)
    zo[1] = 3 * zo[1] + 2
    z = _with_zeros(zo, 53, dt).double().requires_grad_()
    y = _act(z, act, slope)
    ys = _cl(y.detach().float(), dt)
    assert int((ys == 0).sum()) > 0
    dy = _cl(_randn((RED_N, C) + dims, seed + 1), dt)
    y.backward(dy.double())
    hb.channel_sum_actgrad(_dev(dy), _dev(ys), act, slope)
    got = hb.channel_sum_actgrad(_dev(dy), _dev(ys), act, slope)
    _same((got,), (hb.channel_sum_actgrad(_dev(dy), _dev(ys), act, slope),))
    _check(f"channel_sum_actgrad {_rid(rc)} {'bf16' if dt == BF else 'fp32'} {ACT_IDS[act]}",
           {"sum": _red(got, z.grad.sum((0, 2, 3, 4)), z.grad.abs().sum((0, 2, 3, 4)))})


@pytest.mark.parametrize("out_dt", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("with_stats", [False, True], ids=["nostats", "stats"])
@pytest.mark.parametrize("rc", RED_CASES, ids=_rid)
def test_sum_slabs_bias_act(rc, with_stats, out_dt):
    """The split-K combine for 1, 3 and 6 slabs, with and without bias.  y against fp64.  The statistics are by contract
    the sums and sums of squares of the fp32 combined values, before any bf16 store: they are compared with the fp64
    sums of the fp32 output of the same kernel on the same operands (itself compared with fp64 element by element), and
    a bf16 output must be exactly that fp32 output rounded to nearest.  (Against the fp64 combine they would inherit the
    fp32 rounding of a combined value, which ReLU can leave as the only summand of a channel; and rounding 10 or more
    values to bf16 moves their sum by ~2^-9 / sqrt(n) relative, far above the reduction bar.)"""
    C, dims = rc[:2]
    N = RED_N
    seed = 4000 + RED_CASES.index(rc) * 8
    allslabs = _randn((6 * N, C) + dims, seed)
    allslabs[1::2] = 3 * allslabs[1::2] + 2                      # sample 1 of every slab
    bias = _randn((C,), seed + 1)
    for i, (nslab, with_bias) in enumerate([(s, b) for s in (1, 3, 6) for b in (False, True)]):
        act, slope = ACTS[i % 3]
        slabs = _dev(_cl(allslabs[:nslab * N], F32))
        v = allslabs[:nslab * N].double().view(nslab, N, C, *dims).sum(0)
        if with_bias:
            v = v + bias.double().view(1, -1, 1, 1, 1)
        ref = _act(v, act, slope)

        def run(dt):
            stats = torch.zeros((N, C, 2), dtype=torch.float64, device=DEV) if with_stats else None
            y = hb.sum_slabs_bias_act(slabs, nslab, _dev(bias) if with_bias else None, act, slope, stats=stats,
                                      out_dtype=dt)
            assert tuple(y.shape) == (N, C) + dims
            return y, stats

        y, stats = run(out_dt)
        figs = {"y": _elem(y, ref, out_dt)}
        if with_stats:
            y32 = y
            if out_dt == BF:
                y32 = run(F32)[0]
                figs["y32"] = _elem(y32, ref, F32)
                assert torch.equal(y, y32.to(BF))
            v32 = _cpu64(y32)
            figs["sum"] = _red(stats[..., 0], v32.sum((2, 3, 4)), v32.abs().sum((2, 3, 4)))
            figs["sumsq"] = _red(stats[..., 1], (v32 * v32).sum((2, 3, 4)), (v32 * v32).sum((2, 3, 4)))
        _check(f"sum_slabs {_rid(rc)} -> {'bf16' if out_dt == BF else 'fp32'} slabs {nslab} bias {int(with_bias)} "
               f"{ACT_IDS[act]}", figs)


# ----------------------------------------------------------------------------- 7: the SE gate MLP
def _gate_operands(N, C):
    seed = 5000 + C * 4 + N
    S = 150
    mean = _randn((N, C), seed)
    w = _randn((C, C), seed + 1) * (0.5 / C ** 0.5)
    b = _randn((C,), seed + 2) * 0.1
    stats = torch.zeros((N, C, 2), dtype=torch.float64)
    stats[..., 0] = mean.double() * S
    stats[..., 1] = _randn((N, C), seed + 3).double().abs() * S     # (the sums of squares are not read)
    return S, stats, w, b


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("C", [64, 66, 130, 512])
def test_se_gate_fwd(C, N):
    S, stats, w, b = _gate_operands(N, C)
    mean = stats[..., 0] / S
    pre = mean @ w.double().t() + b.double()
    assert float(pre.abs().max()) < 3.0
    ref = torch.sigmoid(pre)
    gate, mk = hb.se_gate_fwd(_dev(stats), _dev(w), _dev(b), N, C, S)
    cond = (mean[:, None, :] * w.double()[None]).abs().sum(2) + b.double().abs()
    d = (_cpu64(gate) - ref).abs()
    bar = 1e-5 * float(ref.max()) + 0.25 * 5e-6 * cond
    _check(f"se_gate_fwd C{C} N{N}", {"gate": (float((d / bar).max()), 1.0), "mean": _elem(mk, mean, F32)})


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("C", [64, 66, 130, 512])
def test_se_gate_bwd(C, N):
    """dw, db and the per-(n, k) constant that add_channel_const spreads over the sample (the gradient of the pooled
    sum: mean = sum / S), from autograd of sigmoid(W mean + b); the kernel is handed the fp32-rounded reference gate
    and mean."""
    S, stats, w, b = _gate_operands(N, C)
    s0 = stats[..., 0].clone().requires_grad_()
    wr, br = w.double().requires_grad_(), b.double().requires_grad_()
    gate = torch.sigmoid((s0 / S) @ wr.t() + br)
    dgate = _randn((N, C), 5900 + C + N).double()
    (gate * dgate).sum().backward()
    gd, mean = gate.detach(), s0.detach() / S
    ds = dgate * gd * (1 - gd)
    first = hb.se_gate_bwd(_dev(dgate), _dev(gd.float()), _dev(mean.float()), _dev(w), S)
    dw, db, k = hb.se_gate_bwd(_dev(dgate), _dev(gd.float()), _dev(mean.float()), _dev(w), S)
    _same(first, (dw, db, k))
    _check(f"se_gate_bwd C{C} N{N}", {
        "dw": _red(dw, wr.grad, (ds[:, :, None] * mean[:, None, :]).abs().sum(0)),
        "db": _red(db, br.grad, ds.abs().sum(0)),
        "k": _red(k, s0.grad, (ds[:, :, None] * w.double()[None]).abs().sum(1) / S),
    })


# ----------------------------------------------------------------------------- 8: channel-normalised cosine distance
@pytest.mark.parametrize("dims", [(1, 1, 7), (3, 11, 13)], ids=["S7", "S429"])
def test_cosdist_stats_and_bwd(dims):
    """S = 7: one block per sample; S = 429, N = 3: 7 blocks of 64 voxels per sample, the last holds 45."""
    N, C = 3, 64
    a = _cl(_randn((N, C) + dims, 92), F32)
    b = _cl(_randn((N, C) + dims, 93) * 0.5 + 0.1, F32)
    ar = a.double().requires_grad_()
    t1 = F.normalize(ar, p=2, dim=1).reshape(N, C, -1)
    t2 = F.normalize(b.double(), p=2, dim=1).reshape(N, C, -1)
    loss = (1 - torch.cosine_similarity(t1, t2, dim=2)).mean()
    loss.backward()
    t1 = t1.detach()
    ref = torch.stack([(t1 * t2).sum(2), (t1 * t1).sum(2), (t2 * t2).sum(2)], -1)
    scale = torch.stack([(t1 * t2).abs().sum(2), (t1 * t1).sum(2), (t2 * t2).sum(2)], -1)
    hb.cosdist_stats(_dev(a), _dev(b))
    stats = hb.cosdist_stats(_dev(a), _dev(b))
    dx = hb.cosdist_bwd(_dev(a), _dev(b), _dev(ref), -1.0 / (N * C))
    _check(f"cosdist S{dims[0] * dims[1] * dims[2]}", {"stats": _red(stats, ref, scale), "dx": _elem(dx, ar.grad, F32)})
