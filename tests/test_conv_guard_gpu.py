"""Guard bands and poisoned buffers around every output, slab, packed panel and scratch of the matrix-core convolution
family (tests/guarded_alloc.py; the helper itself is proven on host tensors in tests/test_guarded_alloc_cpu.py).

Every case is one layer at a shape the neighbouring tables already use (imported from test_kernels_gpu,
test_bf16_conv_edges_gpu and thin_kernel_cases; shapes that exist only inside a test function there are restated next to
the name of that test) and runs twice: plain -- what the suite does today -- and inside the guarded context, where the
inputs sit between NaN guards and every torch.empty / empty_like / zeros of the ops entry points (outputs, split-K slabs,
packed panels, Winograd weight scratch, weight-gradient workspaces, dw / db, the fp64 accumulators) is a NaN-filled
payload between two 64 KiB NaN guards.  The two cheapest cases of a group run a third time with the payloads 16 bytes
off their 256-byte alignment.  Asserted per case:

  * every guard still holds the fill word (a store outside a tensor is a changed byte, not a fault);
  * no output, gradient or statistic holds a NaN (an element left unwritten, or garbage x 0 read from scratch);
  * both runs launched the same kernels (route_probe / the profiling families / wino_wgrad_launches), and the kernels
    named in the table's column where the table has one;
  * y (the convolution's own output), dx and dw are bit-equal between the runs -- the kernels sum in a fixed order -- and
    so is db where the fp32 weight-gradient kernel forms it; db from channel_sum (bf16, transposed), the statistics and
    what is normalised with them pass double atomics and are held to the bars instead;
  * the guarded run meets the neighbouring suites' bars against torch in fp64 on the host: fp32 1e-4 of the reference's
    largest value, bf16 bf16_bar.assert_bf16_bar on bf16-rounded operands (weight gradients 1e-4 of max), statistics
    bf16_bar.assert_conv_stats, thin kernels 5e-6 x sum |summand| (thin5: also its own suite's 1e-5 of max).

Activations are LeakyReLU or none: a ReLU written with fmaxf would turn a NaN into 0.  The thin-channel kernels are not
profiled launches, so for them "the same kernels" is not asserted (their routes are checked in
test_thin_kernel_regimes_cpu.py).  The last test fails if a route name of hip_backend._ROUTE_NAMES / _DIRECT_NAMES or a
weight-gradient family was reached by no case of this file; it reads what the cases above it recorded, so it belongs to
a run of the whole file.

Which row reached which kernel on an MI355X (forward | input gradient per source | weight-gradient family; the test
prints this line for every case):
  WINO ragged 30x31, half last chunk 48->64, depth 1       big8 | big8 | wino_wgrad
  WINO wide tile 60x30, 32 channels 16x16                  w32p | w32p | wino_wgrad
  WINO flattened 13x11 odd extents                         flat8 | flat8 | wgrad
  WINO Npad 96, 8-row lattice                              small | small | wino_wgrad
  FLAT8 odd extents, half chunk (32 tiles per block)       flat8 | generic | wgrad
  FLAT8 one depth tap, 3 channel tiles (64 tiles)          flat8 | generic | wino_wgrad
  w32p shapes 32->32 64x48 and 48->96 60x30, both blocks   w32p;   48->32 33x50: generic (the library's pick)
  virtual concat + InstanceNorm                            big8 | w32p, big8 | wino_wgrad x 2
  flat8 statistics and concat (tiles 1 / 2, SE / IN)       flat8 | generic, generic
  WINO22 ragged 30x32, 16x16                               region22 | region22 | wino22_wgrad
  WINO22 flat 13x11, one depth tap                         flat22 | generic | wgrad
  WINO22 virtual concat + SE                               region22 | region22, generic | wino22_wgrad, wgrad
  HALO rows                                                the table's column (halo bn64 / halo bn32 / generic), wgrad or
                                                           wino_wgrad
  CONVS strided, 5x5x5 (split-K slabs), 1x1x1              generic | generic | wgrad
  TCONVS 128->64 344/122 9x10, 320->320 122                generic | generic | wgrad
  TCONVS 64->32 k = s = 222                                tconv_ks | generic | wgrad
  TCONVS 64->32 344/122 16x16                              halo bn32 | region22 | wgrad
  TCONVS 128->64 344/122 8x24                              halo bn64 | generic | wino22_wgrad
  split-K 4^3 + InstanceNorm, strided 8^3 -> 4^3, 32 taps  generic slabs + combine | generic | wgrad
  split-K 16^3 depth-tap split                             big8 (3 parts) + combine | big8 (3 parts) | wino_wgrad
  WINO_WGRAD rows                                          wino_wgrad; the 80-channel tail and USE_WINOGRAD_WGRAD off: wgrad
  bf16 CONV_CASES / TCONV_CASES                            the tables' columns; the two weight gradients: wgrad_bf16
  weight forms (big8)                                      one pass: 1 one-pass call; pack then transform: none; kept
                                                           forms: 2 rebuilds (panel + scratch), reused by the second call
Wall time of the file on an MI355X: 8.3 s for its 109 tests (the slowest is the first case, WINO ragged 30x31, at 1.3 s;
no other takes more than 0.7 s).

Findings: none in the library -- no guard changed and no poisoned run returned a NaN at any of these rows, skewed
payloads included.  (One correction to a first draft of this file, not to the library: with accumulate=True the weight
gradient also ADDS into dbias, as the header says, so that call now hands it a dbias that holds real values.)
"""
import contextlib
import functools
import zlib
from dataclasses import dataclass

import pytest
import torch
import torch.nn.functional as F

import route_probe
import test_bf16_conv_edges_gpu as te
import test_bf16_kernels_gpu as tb
import test_kernels_gpu as tk
import test_thin_kernels_gpu as tt
import thin_kernel_cases as tc
from bf16_bar import assert_bf16_bar, assert_conv_stats, assert_stats_bar
from guarded_alloc import Guarded
from rehrseg_amd import hip_backend as hb
from rehrseg_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32
TOL = tk.TOL                                  # fp32: of the reference's largest value
WG_FAMILIES = ("wino_wgrad", "wino22_wgrad", "wgrad", "wgrad_bf16")
REACHED = {"fp32": set(), "bf16": set(), "wgrad": set()}      # filled by the cases, read by the last test
K3, S1, P1 = (3, 3, 3), (1, 1, 1), (1, 1, 1)


@pytest.fixture
def guard():
    """guard(skew) -> the guarded context of tests/guarded_alloc.py."""
    def make(skew=0):
        return Guarded(skew=skew)
    return make


@contextlib.contextmanager
def flags(**kw):
    """hip_backend switches for the duration of one run."""
    saved = {k: getattr(hb, k) for k in kw}
    for k, v in kw.items():
        setattr(hb, k, v)
    try:
        yield
    finally:
        for k, v in saved.items():
            setattr(hb, k, v)


def cl(t):
    return t.contiguous(memory_format=torch.channels_last_3d)


def plain_put(t):
    return t.to(DEV)


def f64(t):
    return t.detach().double().cpu()


def bits(t):
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8)


def fp32_bar(name, got, ref, tol=TOL):
    got, ref = f64(got), f64(ref)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = float((got - ref).abs().max()) / (float(ref.abs().max()) + 1e-30)
    print(f"{name} {err / tol:.3f}/1 (bar {tol:g} of max)")
    assert err <= tol, (name, err, tol)


def record(seen):
    """The kernels of the gather-GEMM launches of a probe and the weight-gradient families, noted for the coverage test."""
    for fam, tag in seen:
        if fam in WG_FAMILIES:
            REACHED["wgrad"].add(fam)
    for fam in ("gather_gemm", "wino_conv", "wino22_conv"):
        for k in seen.kernels(fam):
            REACHED["fp32"].update(k.split("+"))
    for k in seen.kernels("gather_gemm_bf16"):
        REACHED["bf16"].update(k.split("+"))
    return {"kernels": seen.kernels(), "wgrad": [fam for fam, _ in seen if fam in WG_FAMILIES]}


def compare_runs(name, plain, guarded, bit_keys):
    """No NaN anywhere, the same launches, and the bit-equal outputs bit-equal."""
    for run in (plain, guarded):
        for k, v in run.items():
            if torch.is_tensor(v):
                assert not bool(torch.isnan(v).any()), f"{name}: NaN in {k}"
                if v.dtype == torch.float64:
                    assert bool((v.abs() < 1e300).all()), f"{name}: the fill word read as fp64 in {k}"
    assert plain["launches"] == guarded["launches"], (name, plain["launches"], guarded["launches"])
    for k in bit_keys:
        if plain.get(k) is None:
            assert guarded.get(k) is None, (name, k)
            continue
        assert plain[k].dtype == guarded[k].dtype and plain[k].shape == guarded[k].shape, (name, k)
        assert torch.equal(bits(plain[k]), bits(guarded[k])), f"{name}: {k} differs between the plain and the guarded run"


# ============================================================================= matrix-core layers (fp32 and bf16)
@dataclass(frozen=True)
class Layer:
    name: str
    group: str
    c: tuple                       # (c1, c2): channels of x1 / x2 (virtual concat)
    Cout: int
    K: tuple
    stride: tuple
    pad: tuple
    dims: tuple                    # (N, D, H, W) of the input
    transposed: bool = False
    tail: str = "lrelu"            # lrelu | none | stats (LeakyReLU + stats_mode 2) | in (InstanceNorm) | se
    dtype: torch.dtype = F32
    parts: tuple = ("fwd", "dgrad", "wgrad")
    flags: tuple = ()              # ((hip_backend switch, value), ...)
    expect: tuple = None           # (forward kernels, input-gradient kernels) where the table names them
    skew: bool = False             # one of the two cheapest of its group: a third run with skew=16
    wino_wgrad: int = None         # wino_wgrad_launches the weight gradient must count, where the table's test says so

    @property
    def spec(self):                # what the operands and the reference depend on (cases that differ in switches share them)
        return (self.c, self.Cout, self.K, self.stride, self.pad, self.dims, self.transposed, self.tail, self.dtype)


def _by(table, col, dims, also=()):
    """The one row of `table` whose column `col` is `dims` (and whose columns `also` = ((index, value), ...) match)."""
    rows = [r for r in table if r[col] == dims and all(r[i] == v for i, v in also)]
    assert len(rows) == 1, (dims, rows)
    return rows[0]


LAYERS = []


def _add(*a, **kw):
    LAYERS.append(Layer(*a, **kw))


# ---- fp32 Winograd forward + input gradient: rows of WINO (Cin, Cout, K, pad, dims)
for _dims, _why, _sk in (((1, 3, 30, 31), "ragged 30x31", False), ((2, 3, 32, 16), "half last chunk 48->64", False),
                         ((1, 1, 16, 16), "depth 1", True), ((1, 2, 60, 30), "wide tile 60x30", False),
                         ((40, 3, 13, 11), "flattened 13x11 odd extents", False), ((1, 2, 8, 16), "Npad 96, 8-row lattice", True),
                         ((1, 4, 16, 16), "32 channels", False)):
    _r = _by(tk.WINO, 4, _dims)
    _add(f"WINO {_why}", "wino", (_r[0], 0), _r[1], _r[2], S1, _r[3], _r[4], skew=_sk)
# rows of FLAT8 (tiles, Cin, Cout, K, pad, dims)
for _dims, _why in (((40, 3, 13, 11), "odd extents, half chunk"), ((30, 2, 20, 28), "one depth tap, 3 channel tiles")):
    _r = _by(tk.FLAT8, 5, _dims)
    _add(f"FLAT8 {_why}", "wino", (_r[1], 0), _r[2], _r[3], S1, _r[4], _r[5], flags=(("WINO_FLAT8_TILES", _r[0]),))
# the shapes of test_winograd_w32_pipelined_kernel (dims, Cin, Cout), both block shapes, statistics epilogue as there
for _dims, _ci, _co in tk.test_winograd_w32_pipelined_kernel.pytestmark[0].args[1]:
    for _blocks in (1, 2):
        _add(f"w32p {_ci}->{_co} {_dims} blocks {_blocks}", "wino", (_ci, 0), _co, K3, S1, P1, _dims, tail="stats",
             parts=("fwd",), flags=(("W32P_BLOCKS", _blocks),))
# test_winograd_virtual_concat_instnorm: x1 (2,32,3,16,16), x2 (2,64,3,16,16), w (64,96,3,3,3)
_add("virtual concat + InstanceNorm", "wino", (32, 64), 64, K3, S1, P1, (2, 3, 16, 16), tail="in")
# test_winograd_flat8_statistics_and_concat: x (32,64,4,12,12), x2 (32,32,4,12,12), w (128,96,3,3,3), SE and InstanceNorm
for _tiles in (1, 2):
    for _tail in ("se", "in"):
        _add(f"flat8 statistics and concat, tiles {_tiles}, {_tail}", "wino", (64, 32), 128, K3, S1, P1, (32, 4, 12, 12),
             tail=_tail, flags=(("WINO_FLAT8_TILES", _tiles),), parts=("fwd", "dgrad"))

# ---- F(2x2,2x2): rows of WINO22 / WINO22_FLAT (Cin, Cout, K, stride, pad, dims), transposed
for _tab, _dims, _why, _sk in ((tk.WINO22, (2, 2, 30, 32), "ragged 30x32", False), (tk.WINO22, (1, 3, 16, 16), "16x16", True),
                               (tk.WINO22_FLAT, (56, 4, 13, 11), "flat 13x11, one depth tap", False)):
    _r = _by(_tab, 5, _dims)
    _add(f"WINO22 {_why}", "wino22", (_r[0], 0), _r[1], _r[2], _r[3], _r[4], _r[5], transposed=True, skew=_sk,
         wino_wgrad=1 if _tab is tk.WINO22 else None)
# test_winograd22_virtual_concat_se: x1 (1,64,2,16,16), x2 (1,32,2,16,16), w (96,64,3,4,4), stride (1,2,2), pad 1
_add("WINO22 virtual concat + SE", "wino22", (64, 32), 64, (3, 4, 4), (1, 2, 2), P1, (1, 2, 16, 16), transposed=True,
     tail="se", skew=True)

# ---- fp32 direct kernels: every row of HALO (Cin, Cout, K, pad, dims, kernel) with the Winograd kernels off
for _i, _r in enumerate(tk.HALO):
    _k = _r[5] if isinstance(_r[5], tuple) else (_r[5], _r[5])
    _add(f"HALO {_r[0]}->{_r[1]} {_r[2]} {_r[4]}", "direct", (_r[0], 0), _r[1], _r[2], S1, _r[3], _r[4],
         flags=(("USE_WINOGRAD", False),), expect=([_k[0]], [_k[1]]), skew=_i in (3, 4))
# rows of CONVS (Cin, Cout, K, stride, pad, dims): the strided, 5x5x5 and 1x1x1 ones
for _r in tk.CONVS:
    if _r[3] != S1 or _r[2] in ((5, 5, 5), (1, 1, 1)):
        _add(f"CONVS {_r[0]}->{_r[1]} {_r[2]} stride {_r[3]} {_r[5]}", "direct", (_r[0], 0), _r[1], _r[2], _r[3], _r[4], _r[5])
# every row of TCONVS (Cin, Cout, K, stride, pad, dims)
for _r in tk.TCONVS:
    _add(f"TCONVS {_r[0]}->{_r[1]} {_r[2]} stride {_r[3]} {_r[5]}", "direct", (_r[0], 0), _r[1], _r[2], _r[3], _r[4], _r[5],
         transposed=True, tail="none")

# ---- split-K: slabs, combine and statistics
# test_split_k_low_resolution_stage_with_instnorm: x (2,128,4,4,4), w (192,128,3,3,3)
_add("split-K 4^3 stage + InstanceNorm", "splitk", (128, 0), 192, K3, S1, P1, (2, 4, 4, 4), tail="in", skew=True)
# test_winograd_depth_tap_split_half_filled_grid: x (2,128,16,16,16), w (128,128,3,3,3)
_add("split-K 16^3 depth-tap split", "splitk", (128, 0), 128, K3, S1, P1, (2, 16, 16, 16), tail="in")
# test_split_k_strided_low_resolution_stage, its 8^3 -> 4^3 stage: x (2,320,8,8,8), w (320,320,3,3,3), stride 2
_add("split-K strided 8^3 -> 4^3", "splitk", (320, 0), 320, K3, (2, 2, 2), P1, (2, 8, 8, 8), tail="in", skew=True)
# test_split_k_many_depth_taps: x (1,64,32,24,20), w (64,64,32,3,3), pad (0,1,1)
_add("split-K 32 depth taps on 24x20", "splitk", (64, 0), 64, (32, 3, 3), S1, (0, 1, 1), (1, 32, 24, 20))

# ---- fp32 weight gradients: rows of WINO_WGRAD (Cin, Cout, K, pad, dims)
for _dims, _why, _n in (((1, 2, 14, 31), "ragged 14x31, three channel tiles", 1), ((2, 3, 16, 16), "80-channel tail", 0),
                        ((2, 4, 16, 32), "16 outputs padded to 32", 1), ((63, 1, 12, 10), "63-slice narrow planes", 1)):
    _r = _by(tk.WINO_WGRAD, 4, _dims, ((0, 80),) if _n == 0 else ())
    _add(f"WINO_WGRAD {_why}", "wgrad", (_r[0], 0), _r[1], _r[2], S1, _r[3], _r[4], tail="none", parts=("wgrad",), wino_wgrad=_n)
for _dims, _ci, _sk in (((1, 4, 16, 32), 64, True), ((2, 3, 16, 16), 32, True)):
    _r = _by(tk.WINO_WGRAD, 4, _dims, ((0, _ci),))
    for _on in (True, False):
        _add(f"WINO_WGRAD {_r[0]}->{_r[1]} {_dims} Winograd {'on' if _on else 'off'}", "wgrad", (_r[0], 0), _r[1], _r[2], S1,
             _r[3], _r[4], tail="none", parts=("wgrad",), flags=(("USE_WINOGRAD_WGRAD", _on),), wino_wgrad=int(_on),
             skew=_sk and not _on)
_r = tk.WINO22[0]
_add("WINO22 weight gradient (transposed)", "wgrad", (_r[0], 0), _r[1], _r[2], _r[3], _r[4], _r[5], transposed=True,
     tail="none", parts=("wgrad",), wino_wgrad=1)

# ---- bf16: every row of CONV_CASES (statistics epilogue as in its suite) and of TCONV_CASES
_BF_WGRAD = ("halo 4x8x16 ragged 64", "generic K 32, Cin 96")      # their weight gradient too (ops.mixed_precision())
_BF_SKEW = ("generic Cout 16", "generic flat tiles, 61-row tail")
for _r in te.CONV_CASES:
    _name, _N, _c, _co, _d, _K, _s, _p, _fk, _dk = _r
    _add(f"bf16 {_name}", "bf16", _c, _co, _K, _s, _p, (_N,) + _d, tail="stats", dtype=BF, expect=([_fk], list(_dk)),
         parts=("fwd", "dgrad") + (("wgrad",) if _name in _BF_WGRAD else ()), skew=_name in _BF_SKEW)
for _r in te.TCONV_CASES:
    _name, _c, _co, _d, _K, _s, _p, _fk = _r
    _add(f"bf16 {_name}", "bf16", _c, _co, _K, _s, _p, (2,) + _d, transposed=True, tail="none", dtype=BF,
         expect=([_fk], ["generic"] * (2 if _c[1] else 1)), parts=("fwd", "dgrad"))

assert len({c.name for c in LAYERS}) == len(LAYERS)


@functools.lru_cache(maxsize=3)
def layer_operands(spec):
    """Host operands of a layer: x1, x2, dz NDHWC (bf16 cases: rounded once, here); sample n is scaled and shifted by
    SAMPLE_AFFINE[n % 3] so that a wrong sample index cannot cancel; w ~ N(0,1) / sqrt(fan in), bias and the tail's
    parameters ~ N(0,1)."""
    (c1, c2), Cout, K, stride, pad, (N, D, H, W), transposed, tail, dtype = spec
    g = torch.Generator().manual_seed(zlib.crc32(repr(spec).encode()))
    Cin, T = c1 + c2, K[0] * K[1] * K[2]

    def act(shape):
        t = torch.randn(shape, generator=g)
        for n in range(shape[0]):
            a, b = te.SAMPLE_AFFINE[n % 3]
            t[n] = a * t[n] + b
        return cl(t.to(dtype))

    o = {"x1": act((N, c1, D, H, W)), "x2": act((N, c2, D, H, W)) if c2 else None}
    fan = Cin * T / (stride[0] * stride[1] * stride[2] if transposed else 1)
    o["w"] = torch.randn(((Cin, Cout) if transposed else (Cout, Cin)) + K, generator=g) / fan ** 0.5
    o["b"] = torch.randn(Cout, generator=g)
    cfg = ops.ConvCfg(stride, pad, transposed)
    o["dz"] = act((N, Cout) + ops._out_dims((D, H, W), o["w"].shape, cfg))
    if tail == "in":
        o["p1"], o["p2"] = torch.randn(Cout, generator=g), torch.randn(Cout, generator=g)
    elif tail == "se":
        o["p1"], o["p2"] = torch.randn(Cout, Cout, 1, 1, 1, generator=g) / Cout ** 0.5, torch.randn(Cout, generator=g)
    return o


_TAIL_ACT = {"lrelu": (ops.ACT_LRELU, 0.1, 0), "none": (ops.ACT_NONE, 0.0, 0), "stats": (ops.ACT_LRELU, 0.1, 2),
             "in": (ops.ACT_NONE, 0.0, 2), "se": (ops.ACT_NONE, 0.0, 1)}
IN_SLOPE, SE_SLOPE = 0.01, 0.2


@functools.lru_cache(maxsize=3)
def layer_reference(spec):
    """torch in fp64 on the host, on the operands as the kernels see them (bf16 cases: bf16-rounded x, dz and weights)."""
    (c1, c2), Cout, K, stride, pad, dims, transposed, tail, dtype = spec
    o = layer_operands(spec)
    xr = f64(o["x1"] if c2 == 0 else torch.cat([o["x1"], o["x2"]], 1)).requires_grad_()
    wr = f64(o["w"].to(dtype)).requires_grad_()
    conv = F.conv_transpose3d if transposed else F.conv3d
    pre = conv(xr, wr, None, stride, pad)
    pre.backward(f64(o["dz"]))
    z = pre.detach() + f64(o["b"]).view(1, -1, 1, 1, 1)
    act, slope, _ = _TAIL_ACT[tail]
    ref = {"y0": F.leaky_relu(z, slope) if act == ops.ACT_LRELU else z, "dx": xr.grad, "dw": wr.grad,
           "db": f64(o["dz"]).sum((0, 2, 3, 4))}
    if tail == "in":
        ref["y"] = F.leaky_relu(F.instance_norm(z, weight=f64(o["p1"]), bias=f64(o["p2"]), eps=1e-5), IN_SLOPE)
    elif tail == "se":
        ref["y"] = F.leaky_relu(tk._se(z, f64(o["p1"]), f64(o["p2"])), SE_SLOPE)
    return ref


def run_layer(c, put):
    o = layer_operands(c.spec)
    d = {k: (put(v) if v is not None else None) for k, v in o.items()}
    cfg = ops.ConvCfg(c.stride, c.pad, c.transposed)
    act, slope, mode = _TAIL_ACT[c.tail]
    N, D, H, W = c.dims
    out, launches = {}, {}
    mixed = ops.mixed_precision() if c.dtype == BF else contextlib.nullcontext()
    with flags(**dict(c.flags)), mixed:
        if "fwd" in c.parts:
            with route_probe.launches() as seen:
                y0, stats = ops.conv_forward(d["x1"], d["x2"], d["w"], d["b"], cfg, act, slope, mode)
            launches["fwd"] = record(seen)
            out["y0"], out["stats"] = y0, stats
            Cc, S = y0.shape[1], y0.shape[2] * y0.shape[3] * y0.shape[4]
            if c.tail == "in":
                out["y"], out["mr"] = hb.instnorm_act_fwd(y0, stats, d["p1"], d["p2"], 1e-5, ops.ACT_LRELU, IN_SLOPE)
            elif c.tail == "se":
                out["gate"], out["mean"] = hb.se_gate_fwd(stats, d["p1"].reshape(Cc, Cc), d["p2"], N, Cc, S)
                out["y"] = hb.scale_res_act_fwd(y0, out["gate"], None, ops.ACT_LRELU, SE_SLOPE)
        if "dgrad" in c.parts:
            with route_probe.launches() as seen:
                out["dx1"], out["dx2"] = ops.conv_dgrad(d["dz"], d["w"], (D, H, W), c.c[0], c.c[1], cfg)
            launches["dgrad"] = record(seen)
        if "wgrad" in c.parts:
            before = hb.wino_wgrad_launches
            with route_probe.launches() as seen:
                out["dw"], out["db"] = ops.conv_wgrad(d["dz"], d["x1"], d["x2"], d["w"], cfg, True)
            launches["wgrad"] = dict(record(seen), wino=hb.wino_wgrad_launches - before)
    out["launches"] = launches
    return out


def check_layer(c, got):
    """The guarded run against fp64, at the bars of the suite the row comes from."""
    ref = layer_reference(c.spec)
    bf = c.dtype == BF
    c1 = c.c[0]
    if "fwd" in c.parts:
        if bf:
            assert got["y0"].dtype == BF
            assert_bf16_bar(f"{c.name} y", got["y0"], ref["y0"])
        else:
            fp32_bar(f"{c.name} y", got["y0"], ref["y0"])
        if c.tail in ("stats", "in"):
            assert_conv_stats(f"{c.name} stats", got["stats"], ref["y0"])
        elif c.tail == "se":
            assert_stats_bar(f"{c.name} stats sum", got["stats"][..., 0], ref["y0"])
        if "y" in ref:
            fp32_bar(f"{c.name} y behind the {c.tail} tail", got["y"], ref["y"])
    if "dgrad" in c.parts:
        for k, r in (("dx1", ref["dx"][:, :c1]), ("dx2", ref["dx"][:, c1:])):
            if k == "dx2" and not c.c[1]:
                assert got[k] is None
            elif bf:
                assert_bf16_bar(f"{c.name} {k}", got[k], r)
            else:
                fp32_bar(f"{c.name} {k}", got[k], r)
    if "wgrad" in c.parts:
        assert got["dw"].dtype == F32
        fp32_bar(f"{c.name} dw", got["dw"], ref["dw"])
        fp32_bar(f"{c.name} db", got["db"], ref["db"])


@pytest.mark.parametrize("c", LAYERS, ids=[c.name.replace(" ", "_") for c in LAYERS])
def test_layer(c, guard):
    plain = run_layer(c, plain_put)
    torch.cuda.synchronize()
    runs = [plain]
    for skew in (0, 16) if c.skew else (0,):
        with guard(skew) as ga:
            got = run_layer(c, ga.guarded)
            n = ga.check()
        runs.append(got)
        print(f"\n{c.name} skew {skew}: {n} guarded allocations, " +
              ", ".join(f"{p} {v['kernels'] or v['wgrad']}" for p, v in got["launches"].items()))
        # db: bit-equal where the fp32 weight-gradient kernel forms it (channel_sum combines by double atomics)
        fused_db = c.dtype == F32 and not c.transposed
        compare_runs(c.name, plain, got, ["y0", "dx1", "dx2", "dw"] + (["db"] if fused_db else []))
        check_layer(c, got)
    launches = plain["launches"]
    if c.expect is not None:
        assert launches["fwd"]["kernels"] == c.expect[0] and launches["dgrad"]["kernels"] == c.expect[1], (c.name, launches)
    if "wgrad" in c.parts:
        fams = launches["wgrad"]["wgrad"]
        assert fams and all(f in WG_FAMILIES for f in fams), (c.name, launches)
        assert launches["wgrad"]["wino"] == sum(f in ("wino_wgrad", "wino22_wgrad") for f in fams), (c.name, launches)
        if c.wino_wgrad is not None:
            assert launches["wgrad"]["wino"] == c.wino_wgrad, (c.name, launches)
        if c.dtype == BF:
            assert set(fams) == {"wgrad_bf16"}, (c.name, launches)


# ============================================================================= accumulate=True into a dst that holds values
def test_weight_gradient_accumulates_into_real_values(guard):
    """hb.wgrad with accumulate=True: dst += dw and dbias += column sums (include/rehrseg_hip.h), both holding real values
    beforehand, on the 64->64 row of WINO_WGRAD, Winograd and direct kernel."""
    r = _by(tk.WINO_WGRAD, 4, (1, 4, 16, 32), ((0, 64),))
    c = Layer("accumulate", "wgrad", (r[0], 0), r[1], r[2], S1, r[3], r[4], tail="none", parts=("wgrad",))
    o, ref = layer_operands(c.spec), layer_reference(c.spec)
    g = torch.Generator().manual_seed(5)
    dst0, db0 = torch.randn(o["w"].shape, generator=g), torch.randn(c.Cout, generator=g)
    Cout, Cin, T, (N, D, H, W) = c.Cout, c.c[0], 27, c.dims

    def run(put, wino):
        x, dz, dst, db = put(o["x1"]), put(o["dz"]), put(dst0), put(db0)
        with flags(USE_WINOGRAD_WGRAD=wino), route_probe.launches() as seen:
            hb.wgrad(dz, Cout, x, Cin, N, (D, H, W), (D, H, W), S1, (-1, -1, -1), [ops.full_taps(3)] * 3, 3, 3, dst, 0,
                     (Cin * T, T, 1), True, db)
        return {"dw": dst, "db": db, "launches": record(seen)}

    for wino in (True, False):
        plain = run(plain_put, wino)
        with guard() as ga:
            got = run(ga.guarded, wino)
            ga.check()
        assert plain["launches"]["wgrad"] == ["wino_wgrad" if wino else "wgrad"]
        compare_runs(f"accumulate wino {wino}", plain, got, ["dw", "db"])
        fp32_bar("accumulate dw", got["dw"], f64(dst0) + ref["dw"])
        fp32_bar("accumulate db", got["db"], f64(db0) + ref["db"])


# ============================================================================= weight forms
FORMS = [  # name, hip_backend switches, kept (a frozen parameter under no_grad: the forms are kept and used twice)
    ("one pass from the parameter", dict(USE_ONEPASS_FORMS=True), False),
    ("pack, then transform", dict(USE_ONEPASS_FORMS=False), False),
    ("kept forms", dict(WEIGHT_FORM_CACHE=True), True),
    ("kept forms switched off", dict(WEIGHT_FORM_CACHE=False), True),
]


@pytest.mark.parametrize("name,sw,frozen", FORMS, ids=[f[0].replace(" ", "_") for f in FORMS])
def test_weight_forms_are_allocated_and_filled_inside_the_context(name, sw, frozen, guard):
    """The pack panel and the Winograd weight-transform scratch of one layer (the big-tile row of WINO, and the two-source
    layer of test_winograd_virtual_concat_instnorm, whose halves are read in place), each way the backend makes them."""
    for c in (next(c for c in LAYERS if c.name == "WINO ragged 30x31"),
              next(c for c in LAYERS if c.name == "virtual concat + InstanceNorm")):
        o, ref = layer_operands(c.spec), layer_reference(c.spec)

        def run(put):
            x1, x2, b = put(o["x1"]), (put(o["x2"]) if o["x2"] is not None else None), put(o["b"])
            w = put(o["w"])
            before = (hb.wino_launches, hb.onepass_form_calls, hb.form_rebuilds)
            with flags(**sw), route_probe.launches() as seen:
                if frozen:
                    w = torch.nn.Parameter(w, requires_grad=False)
                    with torch.no_grad():
                        ys = [ops.fused_conv3d(x1, w, b, 1, 1, x2=x2) for _ in range(2)]
                else:
                    w = w.requires_grad_()
                    ys = [ops.fused_conv3d(x1, w, b, 1, 1, x2=x2)]
            return {"y0": ys[0], "y1": ys[-1], "launches": record(seen),
                    "counts": (hb.wino_launches - before[0], hb.onepass_form_calls - before[1], hb.form_rebuilds - before[2])}

        plain = run(plain_put)
        for skew in (0,) if frozen else (0, 16):
            with guard(skew) as ga:
                got = run(ga.guarded)
                n = ga.check()
            print(f"\nforms [{name}] {c.name} skew {skew}: {n} guarded allocations, kernels {got['launches']['kernels']}, "
                  f"(Winograd launches, one-pass calls, kept-form rebuilds) {got['counts']}")
            compare_runs(f"forms {name}", plain, got, ["y0", "y1"])
        assert plain["counts"] == got["counts"] and got["counts"][0] > 0, (plain["counts"], got["counts"])
        if name == "one pass from the parameter":
            assert got["counts"][1] > 0, got["counts"]
        elif name != "kept forms switched off":      # (without kept forms a frozen parameter takes the one-pass route too)
            assert got["counts"][1] == 0, got["counts"]
        assert (got["counts"][2] > 0) == (name == "kept forms"), got["counts"]
        assert torch.equal(bits(got["y0"]), bits(got["y1"]))
        z = ref["y0"] if c.tail != "lrelu" else None
        if z is None:      # the reference of the lrelu tail is activated: this layer call has no activation
            z = F.conv3d(f64(o["x1"]), f64(o["w"]), f64(o["b"]), 1, 1)
        fp32_bar(f"forms {name} y", got["y0"], z)


# ============================================================================= thin-channel kernels
def _thin_row(fam, name):
    i = next(i for i, r in enumerate(tc.FAMILIES[fam]) if r["name"] == name)
    return i, tc.FAMILIES[fam][i]


def _thin_vfwd(i, r, put):
    x, w, b, _ = tt._operands("VFWD", i)
    xd = put(cl(x))
    y = hb.new_act(r["N"], r["Cout"], *r["out"], like=xd)
    stats = torch.zeros((r["N"], r["Cout"], 2), dtype=torch.float64, device=DEV)
    hb.small_cin_fwd(xd, put(w), put(b), y, r["stride"], r["pad"], ops.ACT_LRELU, 0.01, stats, 2)
    return {"y": y, "stats": stats}


def _thin_fwd_figs(fam, i, out):
    z, A = tt._fwd_ref(fam, i)
    figs = {"y": tt._ratio(out["y"], tt._act(z, ops.ACT_LRELU, 0.01), A)}
    figs.update(tt._stats_figs(out["stats"], 2, z, A, ops.ACT_LRELU, 0.01))
    return figs


def _thin_wgrad(fam, via):
    def run(i, r, put):
        x, w, _, dy = tt._operands(fam, i)
        xd, wd, dyd = put(cl(x)), put(w), put(cl(dy))
        if via == "hb":
            dw, db = hb.small_cin_wgrad(xd, wd, dyd, r["stride"], r["pad"], True)
        else:
            dw, db = ops.conv_wgrad(dyd, xd, None, wd, ops.ConvCfg(r["stride"], r["pad"], False), True)
        return {"dw": dw, "db": db}
    return run


def _thin_wgrad_figs(fam):
    def figs(i, out):
        rw, sw, rb, sb = tt._wgrad_ref_of(fam, i)
        return {"dw": tt._ratio(out["dw"], rw, sw), "db": tt._ratio(out["db"], rb, sb)}
    return figs


def _thin_im2col(i, r, put):
    x, w, _, _ = tt._operands("IM2COL", i)
    return {"col": hb.im2col(put(cl(x)), put(w), r["out"], r["stride"], r["pad"], r["regime"][0])}


def _thin_im2col_figs(i, out):
    r = tc.IM2COL[i]
    ref = tt._gather(r, tt._operands("IM2COL", i)[0], r["regime"][0])
    assert torch.equal(out["col"].cpu().contiguous().view(torch.int32), ref.view(torch.int32))     # a gather: bit-equal
    return {}


def _thin_mfwd(i, r, put):
    x, w, b, _ = tt._operands("MFWD", i)
    xd, wd, bd = put(cl(x)), put(w), put(b)
    cfg = ops.ConvCfg(r["stride"], r["pad"], False)
    y, stats = ops.conv_forward(xd, None, wd, bd, cfg, ops.ACT_LRELU, 0.01, 2)
    with ops.mixed_precision():
        y16, stats16 = ops.conv_forward(xd, None, wd, bd, cfg, ops.ACT_LRELU, 0.01, 2)
    assert y.dtype == F32 and y16.dtype == BF
    return {"y": y, "stats": stats, "y16": y16, "stats16": stats16}


def _thin_mwg(i, r, put):
    x, w, _, dy = tt._operands("MWG", i)
    dy16 = dy.to(BF)
    xd, wd = put(cl(x)), put(w)
    cfg = ops.ConvCfg(r["stride"], r["pad"], False)
    dw, db = ops.conv_wgrad(put(cl(dy16.float())), xd, None, wd, cfg, True)
    dwb, dbb = ops.conv_wgrad(put(cl(dy16)), xd, None, wd, cfg, True)
    return {"dw": dw, "db": db, "dwb": dwb, "dbb": dbb}


def _thin_mwg_figs(i, out):
    r = tc.MWG[i]
    x, _, _, dy = tt._operands("MWG", i)
    rw, sw, rb, sb = tt._wgrad_ref(r, x, dy.to(BF).float())
    assert torch.equal(out["dwb"], out["dw"]) and torch.equal(out["dbb"], out["db"])     # bf16 dY converts exactly
    return {"dw": tt._ratio(out["dw"], rw, sw), "db": tt._ratio(out["db"], rb, sb)}


def _thin_out(i, r, put):
    x, w, b, dy = tt._operands("OUT", i)
    xd, wd, dyd = put(cl(x)), put(w), put(cl(dy))
    y = hb.new_act(r["N"], r["Cout"], *r["out"], like=xd)
    hb.small_cout_fwd(xd, wd, put(b), y, r["pad"], ops.ACT_LRELU, 0.01)
    dx = hb.small_cout_dgrad(dyd, wd, tuple(x.shape), r["pad"])
    dw, db = hb.small_cout_wgrad(xd, wd, dyd, r["pad"], True)
    return {"y": y, "dx": dx, "dw": dw, "db": db}


def _thin_out_figs(i, out):
    r = tc.OUT[i]
    x, w, _, dy = tt._operands("OUT", i)
    z, A = tt._fwd_ref("OUT", i)
    rw, sw, rb, sb = tt._wgrad_ref_of("OUT", i)
    ref = torch.nn.grad.conv3d_input(tuple(x.shape), w.double(), dy.double(), 1, r["pad"])
    scale = torch.nn.grad.conv3d_input(tuple(x.shape), w.double().abs(), dy.double().abs(), 1, r["pad"])
    return {"y": tt._ratio(out["y"], tt._act(z, ops.ACT_LRELU, 0.01), A), "dx": tt._ratio(out["dx"], ref, scale),
            "dw": tt._ratio(out["dw"], rw, sw), "db": tt._ratio(out["db"], rb, sb)}


# family, the row with a partial last tile or an idle wave, run, figures, bit-equal outputs, third run with skew
THIN = [
    ("VFWD", "1->16 3x3x3", _thin_vfwd, lambda i, o: _thin_fwd_figs("VFWD", i, o), ["y"], True),           # last tile 79 of 256
    ("VWG", "2->16 1x3x3 idle wave", _thin_wgrad("VWG", "ops"), _thin_wgrad_figs("VWG"), ["dw", "db"], True),
    ("VWG", "1->32 3x3x9", _thin_wgrad("VWG", "hb"), _thin_wgrad_figs("VWG"), ["dw", "db"], False),        # masked lanes
    ("IM2COL", "3 1x3x3", _thin_im2col, _thin_im2col_figs, ["col"], False),                               # Kpad 28 > 27 columns
    ("IM2COL_GEMM", "1->32 3x3x8", _thin_wgrad("IM2COL_GEMM", "ops"), _thin_wgrad_figs("IM2COL_GEMM"), ["dw", "db"], False),
    ("MFWD", "1->64 3x3x3 runs", _thin_mfwd, lambda i, o: _thin_fwd_figs("MFWD", i, o), ["y", "y16"], False),   # last block: 1 tile
    ("MWG", "2->64 3x3x3 runs", _thin_mwg, _thin_mwg_figs, ["dw", "db", "dwb", "dbb"], False),             # last block: 1 tile
    ("OUT", "48->4 1x1x1 strips of two rows", _thin_out, _thin_out_figs, ["y", "dx", "dw", "db"], False),  # last strip: 1 row
    ("OUT", "32->3 3x3x3", _thin_out, _thin_out_figs, ["y", "dx", "dw", "db"], False),                     # partial bricks
]


@pytest.mark.parametrize("fam,name,run,figs,bit_keys,skew", THIN, ids=[f"{t[0]}-{t[1].replace(' ', '_')}" for t in THIN])
def test_thin_kernels(fam, name, run, figs, bit_keys, skew, guard):
    i, r = _thin_row(fam, name)
    plain = dict(run(i, r, plain_put), launches=None)
    for sk in (0, 16) if skew else (0,):
        with guard(sk) as ga:
            got = dict(run(i, r, ga.guarded), launches=None)
            n = ga.check()
        print(f"\nthin {fam} {name} skew {sk}: {n} guarded allocations")
        compare_runs(f"thin {fam} {name}", plain, got, bit_keys)
        tt._check(f"guarded {fam} {name}", figs(i, got))


def test_thin5(guard):
    """sr_head.2 on the fp32 matrix cores: forward, input gradient and weight gradient at the first shape of
    test_thin5_conv_fp32_vs_fp64 (W 32), at the thin kernels' bar and at that suite's 1e-5 of the largest value."""
    N, D, H, W = tb.test_thin5_conv_fp32_vs_fp64.pytestmark[0].args[1][0]
    assert hb.thin5_supported((N, 16, D, H, W), (2, 16, 5, 5, 5), (2, 2, 2), F32)
    g = torch.Generator().manual_seed(N + D + H + W + 1)
    x, dy = cl(torch.randn(N, 16, D, H, W, generator=g)), cl(torch.randn(N, 2, D, H, W, generator=g))
    w, b = torch.randn(2, 16, 5, 5, 5, generator=g) * 0.05, torch.randn(2, generator=g)

    def run(put):
        xd, wd, dyd = put(x), put(w), put(dy)
        dw, db = hb.thin5_wgrad(xd, wd, dyd, True)
        return {"y": hb.thin5_fwd(xd, wd, put(b)), "dx": hb.thin5_dgrad(dyd, wd, F32), "dw": dw, "db": db, "launches": None}

    plain = run(plain_put)
    with guard() as ga:
        got = run(ga.guarded)
        ga.check()
    compare_runs("thin5", plain, got, ["y", "dx", "dw", "db"])
    xd, wd, dyd, bd = x.double(), w.double(), dy.double(), b.double()
    pairs = {"y": (F.conv3d(xd, wd, bd, padding=2), F.conv3d(xd.abs(), wd.abs(), bd.abs(), padding=2)),
             "dx": (torch.nn.grad.conv3d_input(xd.shape, wd, dyd, padding=2),
                    torch.nn.grad.conv3d_input(xd.shape, wd.abs(), dyd.abs(), padding=2)),
             "dw": (torch.nn.grad.conv3d_weight(xd, w.shape, dyd, padding=2),
                    torch.nn.grad.conv3d_weight(xd.abs(), w.shape, dyd.abs(), padding=2)),
             "db": (dyd.sum((0, 2, 3, 4)), dyd.abs().sum((0, 2, 3, 4)))}
    tt._check("guarded thin5", {k: tt._ratio(got[k], ref, scale) for k, (ref, scale) in pairs.items()})
    for k, (ref, _) in pairs.items():
        fp32_bar(f"thin5 {k}", got[k], ref, 1e-5)


# ============================================================================= coverage (runs last)
_WANTED = ([("fp32", n) for n in list(hb._ROUTE_NAMES.values()) + list(hb._DIRECT_NAMES[False].values())] +
           [("bf16", n) for n in hb._DIRECT_NAMES[True].values()] + [("wgrad", n) for n in WG_FAMILIES])


@pytest.mark.parametrize("kind,name", _WANTED, ids=[f"{k}-{n.replace(' ', '_')}" for k, n in _WANTED])
def test_every_route_was_reached_by_a_case(kind, name):
    assert name in REACHED[kind], f"no case of this file reached the {kind} kernel '{name}' (reached: {sorted(REACHED[kind])})"
