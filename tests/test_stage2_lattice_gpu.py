"""Every conv of oracle.segmodel_oracle.ANISO_PLAN on the lattices of the reference's stage-2 geometry (B = 2,
patch 16 x 320 x 384: utils/seg_utils.py:229,246 with the depth rounded to what the strides of :364 divide) against
torch.nn.functional in fp64 on the CPU, fp32 and under ops.mixed_precision().

  stage  lattice (D,H,W)  C    K      entry stride  choose_tile            _tap_split parts
  0      16 x 320 x 384   32   1x3x3  1,1,1         (4,4,8)                none
  1      16 x 160 x 192   64   1x3x3  1,2,2         (4,4,8)                none
  2      16 x  80 x  96   128  3x3x3  1,2,2         (4,4,8)                none
  3       8 x  40 x  48   256  3x3x3  2,2,2         (4,4,8)                none
  4       4 x  20 x  24   320  3x3x3  2,2,2         (4,4,8)                3
  5       4 x  10 x  12   320  3x3x3  1,2,2         (0,0,0) flattened runs 6

Part A (test_layer_*): one case per distinct layer -- encoder entry and second convs, the decoder's kernel = stride
transposed convs, two-source convs and second convs, the 1x1x1 logits conv.  Stages 3-5 run at their exact lattice;
stages 0-2 keep the full width and two 16-row region rows and are cut in H and D as far as the routing stays what it
is at the full lattice: the Python-side picks (ops.choose_tile, the part count of ops._tap_split, ops.pad_rows) and a
restatement of the library's acceptance rules (_wino_fwd and _wino_wgrad below, read from wino_region_plan, plan_flat8
and wino_wgrad's plan; _halo_bf16 and _tconv_ks ask the library's route query) are asserted equal for the
two lattices, and test_reduced_lattice_takes_the_kernels_of_the_full_lattice runs the fp32 layer at the full lattice on
the device and compares the Winograd launch counters.
Tolerances are the neighbouring suites': fp32 1e-4 of the reference's max (test_kernels_gpu.py); bf16 without
InstanceNorm 1e-2 of max for bf16-stored tensors, 1e-4 for fp32-stored ones (test_bf16_kernels_gpu.py); bf16 with
InstanceNorm the interior-rounding emulation and bars of
test_mixed_steps_gpu.py::test_single_layer_bf16_gradients_against_fp64_on_the_same_rounded_operands.
In the fp32 gradient checks the output gradient is zero on the elements whose reference pre-activation lies within the
forward tolerance of the (Leaky)ReLU kink (_off_the_kink: which branch they take is decided by rounding).
Left out of the comparison: the gradient of a conv bias in front of InstanceNorm (identically zero, what the kernels
return is rounding noise: excluded like in the suites above) and the gradient of the 1-channel image (never formed).

Part B (test_full_lattice_*): the unit-stride 3x3(x3) layers of stages 0-3 and the decoder's tconv_ks layers at the
REAL lattice with N = 2, default kernel against the competing one, compared on the device (tile quantisation and edge
masks at the true extents; not a precision reference).

Part C (test_sr_head_*): sr_head.0 (ops.upsample_conv3d_depth, 32 -> 16, depth 16 -> 64) and sr_head.2 (16 -> 2,
5x5x5) on 384-column slabs.
"""
import itertools

import pytest
import torch
import torch.nn.functional as F

from oracle.bf16_emul import Bf16Emu
from direct_plan_cases import c3, make, tphases
from oracle.segmodel_oracle import ANISO_PLAN
from rehrseg_amd import hip_backend, ops
from rehrseg_amd import lib as L

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = "cuda:0"
BF = torch.bfloat16
FULL = (16, 320, 384)
BATCH = 2


def _mk(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float32)


def _relmax(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).abs().max()) / (float(ref.abs().max()) + 1e-30)


def _l2rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).norm() / (ref.norm() + 1e-300))


def _check(tag, errs, bars):
    """errs / bars: name -> value; prints every figure, then asserts all of them."""
    print(f"[stage2 {tag}] " + " ".join(f"{k} {v:.2e}/{bars[k]:.1e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= bars[k], (tag, k, v, bars[k])


def _off_the_kink(z, dy):
    """dy with zeros where the reference's pre-activation z lies within TOL * max |z| of the activation's kink.  The
    forward bar itself allows the device's z that much error, so on those elements (a few hundred of the millions of a
    stage-0 case) rounding decides which branch of (Leaky)ReLU the backward pass takes, and one flipped branch moves an
    fp32 input gradient by 1e-2 of its max -- in a plain fp32 CPU evaluation just as on the device (the same
    conditioning test_winograd22_flat_conv_transpose drops its activation for).  The forward values are continuous
    across the kink and stay compared everywhere."""
    keep = z.detach().abs() > TOL * float(z.detach().abs().max())
    return dy * keep.to(dy.dtype), int((~keep).sum())


def _dev_relmax(a, b):
    """max |a - b| / max |b| formed on the device (no copy of a 0.5 GB tensor to the host)."""
    return float((a.float() - b.float()).abs().max() / (b.float().abs().max() + 1e-30))


# ----------------------------------------------------------------------------- the layers
def _out_lat(lat, K, s, transposed=False):
    if transposed:
        return tuple(i * k for i, k in zip(lat, K))
    return tuple(ops.conv_out_dim(i, k, st, k // 2) for i, k, st in zip(lat, K, s))


def _plan_layers():
    """(name, kind, (c1, c2), Cout, K, stride, input lattice at 16 x 320 x 384) for every distinct conv of ANISO_PLAN."""
    C, Ks, Ss = ANISO_PLAN["features_per_stage"], ANISO_PLAN["kernel_sizes"], ANISO_PLAN["strides"]
    out, lat, lats, cin = [], FULL, [], 1
    for st in range(6):
        K, s = tuple(Ks[st]), tuple(Ss[st])
        out.append((f"enc{st}.0", "conv", (cin, 0), C[st], K, s, lat))
        lat = _out_lat(lat, K, s)
        out.append((f"enc{st}.1", "conv", (C[st], 0), C[st], K, (1, 1, 1), lat))
        lats.append(lat)
        cin = C[st]
    for lv in range(5):
        below, skip, s = C[5 - lv], C[4 - lv], tuple(Ss[5 - lv])
        out.append((f"dec{lv}.up", "tconv", (below, 0), skip, s, s, lats[5 - lv]))
        K = tuple(Ks[4 - lv])
        out.append((f"dec{lv}.0", "conv", (skip, skip), skip, K, (1, 1, 1), lats[4 - lv]))
        out.append((f"dec{lv}.1", "conv", (skip, 0), skip, K, (1, 1, 1), lats[4 - lv]))
    out.append(("seg", "head", (C[0], 0), 2, (1, 1, 1), (1, 1, 1), FULL))
    return {l[0]: l for l in out}


PLAN_LAYERS = _plan_layers()

# name -> (N, input lattice of the test, Winograd launches fwd + dgrad in fp32, Winograd weight-gradient launches in
# fp32, route).  An input lattice of None = the exact lattice of the plan.  Routes: fp32 / bf16.
R0, R1, R2 = (4, 32, 384), (4, 32, 192), (4, 32, 96)     # stages 0-2: full width, two 16-row regions, one 4-deep brick
CASES = {
    # thin-input kernels (thin_cin_conv.hip: fp32 arithmetic, bf16 store under mixed precision); no Winograd
    "enc0.0": (2, R0, 0, 0, "thin_cin_fwd / thin_cin_wgrad, both precisions"),
    # 32 channels: Npad 32 -> wino_conv_w32p (16 x 16 regions, 2 x 24 of them) / bf16 halo brick 4x8x16 (T = 9);
    # weight gradient wino_wgrad 1 x 1 groups / bf16 LDS brick
    "enc0.1": (2, R0, 2, 1, "w32p Winograd fwd + dgrad, wino_wgrad / halo brick 4x8x16, brick wgrad"),
    # strided entry: generic gather forward; input gradient = 4 phases, dest Npad 32: no F(2x2,2x2)
    "enc1.0": (2, R0, 0, 0, "gather fwd, 4-phase gather dgrad, slab wgrad / the bf16 forms of the same"),
    "enc1.1": (2, R1, 2, 1, "big8 Winograd (2 x 12 regions), wino_wgrad 64 x 64 / halo brick, brick wgrad"),
    # input gradient: the (odd, odd) phase has 3x2x2 taps on a 4 x 16 x 96 lattice, Npad 64 -> wino22_conv (1 launch)
    "enc2.0": (2, R1, 1, 0, "gather fwd, phases with the 2x2-tap one on F(2x2,2x2), slab wgrad / bf16 gather"),
    "enc2.1": (2, R2, 2, 1, "big8 Winograd (2 x 6 regions), wino_wgrad / halo brick 4x8x16 (T = 27), brick wgrad"),
    # 2,2,2 stride: 8 phases, the two (.,odd,odd) ones (1 and 2 depth taps, 2x2 plane taps, 8 x 40 x 48) on wino22_conv
    "enc3.0": (2, None, 2, 0, "gather fwd, 2 of 8 dgrad phases on F(2x2,2x2), slab wgrad / bf16 gather"),
    # 40 x 48 = 2.5 x 3 regions of 16 x 16 (1.2x padding): big8 with a half-empty last region row; the flattened-tile
    # kernel declines (12 staged rows x 50 slots do not fit its 8 pieces per thread)
    "enc3.1": (2, None, 2, 1, "big8 Winograd ragged rows, wino_wgrad / halo brick 4x8x16 (1.0x), brick wgrad"),
    # 4 x 20 x 24: 150 blocks -> 3 depth-tap parts; strided parts have no Winograd form
    "enc4.0": (2, None, 0, 0, "3-part split gather fwd, 8-phase dgrad (2x2-tap phases pad 2.13x: gather), slab wgrad"),
    # Lh % 16 != 0 (no 3-part Winograd split), 8x16 regions pad 1.6x, flat8: 75 units < 128 -> 3-part split gather on
    # (4,4,8) tiles, forward and input gradient; weight gradient: 4 x 16 regions pad exactly 1.333 -> wino_wgrad
    "enc4.1": (2, None, 0, 1, "3-part split gather fwd + dgrad, wino_wgrad (1.333x) / bf16 split gather, slab wgrad"),
    "enc5.0": (2, None, 0, 0, "6-part split gather fwd on (0,0,0) runs, 4-phase dgrad, slab wgrad"),
    # 10 x 12: 30 flat tiles per slice but 20 units < 128 -> 6 parts (3 depth taps x 2 row-tap ranges) on flattened runs;
    # weight gradient: W 12 < 16 -> narrow-plane mode has 21 stages < 128 -> slab kernel
    "enc5.1": (2, None, 0, 0, "6-part split gather fwd + dgrad on (0,0,0) runs, slab wgrad, both precisions"),
    # transposed convs, kernel = stride: tconv_ks takes Cin <= 64 (fp32) / <= 128 (bf16), else one block per (tile, phase)
    "dec0.up": (2, None, 0, 0, "4-phase gather, strided-gather dgrad, slab wgrad"),
    "dec0.0": (2, None, 0, 2, "two-source 3-part split gather, dgrad 3 parts per source, 2 x wino_wgrad / bf16 gather"),
    "dec0.1": (2, None, 0, 1, "as enc4.1"),
    "dec1.up": (2, None, 0, 0, "8-phase gather, strided-gather dgrad, slab wgrad"),
    # N = 1: the fp64 reference of 512 -> 256 on 2 x 15360 voxels alone takes > 4 s; 240 blocks > 160 keeps _tap_split
    # at none, the region rules do not look at N
    "dec1.0": (1, None, 3, 2, "two-source big8 Winograd, one dgrad launch per source, 2 x wino_wgrad / halo brick"),
    "dec1.1": (2, None, 2, 1, "as enc3.1"),
    "dec2.up": (2, None, 0, 0, "8-phase gather (Cin 256), strided-gather dgrad, slab wgrad"),
    "dec2.0": (2, R2, 3, 2, "two-source big8 Winograd, 2 x wino_wgrad / halo brick (c1 128), brick wgrad"),
    "dec2.1": (2, R2, 2, 1, "as enc2.1"),
    "dec3.up": (2, R2, 0, 0, "fp32: 4-phase gather (Cin 128 > 64) / bf16: tconv_ks"),
    "dec3.0": (2, R1, 3, 2, "two-source big8 Winograd, 2 x wino_wgrad / halo brick, brick wgrad"),
    "dec3.1": (2, R1, 2, 1, "as enc1.1"),
    "dec4.up": (2, R1, 0, 0, "tconv_ks, both precisions"),
    "dec4.0": (2, R0, 3, 2, "two-source w32p Winograd, 2 x wino_wgrad / halo brick, brick wgrad"),
    "dec4.1": (2, R0, 2, 1, "as enc0.1"),
    # 1x1x1, 2 output channels: the fp32 thin-output kernels of direct_conv.hip (no bf16 route)
    "seg": (2, R0, 0, 0, "small_cout fwd / dgrad / wgrad (fp32 only)"),
}
NAMES = list(CASES)
INORM = [n for n in NAMES if PLAN_LAYERS[n][1] == "conv"]


# ----------------------------------------------------------------------------- routing, as pure arithmetic
def _up(a, b):
    return -(-a // b) * b


def _wino_fwd(lat, Npad, N, kd):
    """fp32, unit-stride 3x3 plane taps, kd <= 3 depth taps: the Winograd kernel the library picks (wino_route: wino_flat8_plan's
    plan_flat8, then wino_region_plan), or None."""
    Ld, Lh, Lw = lat
    if Npad % 64 == 0 and Lh >= 6 and 6 <= Lw <= 64 and not (Lh % 16 == 0 and Lw % 16 == 0):
        nth, ntw = -(-Lh // 2), -(-Lw // 2)
        ntiles = N * Ld * nth * ntw
        rows = 2 * (62 // ntw + 1) + 2 * (62 // (nth * ntw) + 1) + 4
        if (nth * ntw * 40 <= Lh * Lw * 13 and ntiles >= 64 and -(-ntiles // 64) * (Npad // 64) >= 128 and
                62 // (nth * ntw) + 2 <= 8 and rows * 2 * (ntw + 1) * 8 <= 8 * 512):
            return "flat8"
    if Lh < 8 or Lw < 8:
        return None
    if Lh >= 16 and Lw >= 16 and _up(Lh, 16) * _up(Lw, 16) * 10 <= Lh * Lw * 13:
        return "big8" if Npad % 64 == 0 else "w32p"
    return "8x16" if _up(Lh, 8) * _up(Lw, 16) * 100 <= Lh * Lw * 134 else None


def _halo_bf16(lat, kd):
    """bf16, unit-stride 3x3 plane taps: the brick the library settles on (rehr_gather_gemm_direct_route), or None."""
    kind, variant = hip_backend.direct_route(make([c3(BATCH, 32, 32, tuple(lat), kd=kd)]), 1, True)[0]
    return {1: (4, 8, 16), 2: (8, 8, 8), 3: (2, 16, 16)}[variant] if kind == L.GG_DIRECT_HALO else None


def _wino_wgrad(lat, N, Ca, Cg):
    """fp32, unit-stride 3x3 plane taps: wino_wgrad's plan -- 4 x 16 regions from W >= 16, 8 slices side by side below."""
    Ld, Lh, Lw = lat
    if min(Ca, Cg) < 16 or Ca % 4 or Cg % 4 or Lh < 4 or Lw < 6:
        return None
    if Lw >= 16:
        return "regions" if _up(Lh, 4) * _up(Lw, 16) * 100 <= Lh * Lw * 134 and N * Ld * -(-Lh // 4) * -(-Lw // 16) >= 4 else None
    groups, nbh, nbw = -(-N * Ld // 8), -(-Lh // 4), -(-8 * (Lw + 2) // 16)
    ok = groups * nbh * 4 * nbw * 16 * 100 <= N * Ld * Lh * Lw * 140 and groups * nbh * nbw >= 128
    return "side by side" if ok else None


def _tconv_ks(Cin, Npad, bf16):
    """Does tconv_ks take the four phases of a (1, 2, 2) transposed convolution Cin -> Npad (the same query)?"""
    return hip_backend.direct_route(make(tphases(Cin, Npad, (4, 8, 8), (1, 2, 2))), 4, bf16)[0][0] == L.GG_DIRECT_TCONV_KS


def _parts(p):
    return 0 if p is None else len(p)


def _route(name, N, lat, bf16):
    """Everything shape-driven about one layer on input lattice `lat`: the Python-side picks and the library-side rules."""
    _, kind, (c1, c2), Cout, K, s, _ = PLAN_LAYERS[name]
    Cin = c1 + c2
    r = {}
    if kind == "tconv":
        r["tile"] = ops.choose_tile(tuple(lat))                                      # every phase walks the input lattice
        r["pad_rows"] = ops.pad_rows(Cout)
        r["tconv_ks"] = _tconv_ks(Cin, ops.pad_rows(Cout), bf16)
        return r
    out = _out_lat(lat, K, s)
    r["tile"] = ops.choose_tile(out)
    r["pad_rows"] = (ops.pad_rows(Cout), ops.pad_rows(c1), ops.pad_rows(c2) if c2 else 0)
    if Cin <= 2 or kind == "head":
        return r                                                                      # direct kernels: no lattice tiles
    r["fwd_parts"] = _parts(ops._tap_split(out, N, ops.pad_rows(Cout), [ops.full_taps(k) for k in K], Cin, bf16))
    unit = s == (1, 1, 1)
    if unit:
        taps = [ops.phase_taps(k, 1, k // 2, 0) for k in K]
        r["dgrad_parts"] = tuple(_parts(ops._tap_split(tuple(lat), N, ops.pad_rows(c), taps, Cout, bf16)) for c in (c1, c2) if c)
        r["dgrad_tile"] = ops.choose_tile(tuple(lat))
        split = r["fwd_parts"] > 0
        if bf16:
            r["halo"] = None if split else _halo_bf16(out, K[0])
        else:
            r["wino"] = None if split else _wino_fwd(out, ops.pad_rows(Cout), N, K[0])
            r["wino_dgrad"] = tuple(None if p else _wino_fwd(tuple(lat), ops.pad_rows(c), N, K[0])
                                    for p, c in zip(r["dgrad_parts"], (c1, c2)))
            r["wino_wgrad"] = tuple(_wino_wgrad(out, N, Cout, c) for c in (c1, c2) if c)
    else:
        r["phase_tiles"] = tuple(ops.choose_tile(tuple((lat[a] - ph[a] + s[a] - 1) // s[a] for a in range(3)))
                                 for ph in itertools.product(*(range(v) for v in s)))
    return r


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_route_of_the_tested_lattice_is_the_route_of_the_full_lattice(name, bf16):
    """Pure arithmetic: ops.choose_tile, the part counts of ops._tap_split, ops.pad_rows and the library's acceptance
    rules give the same answers on the lattice the layer is tested on (N of the case) and on the plan's lattice with N = 2."""
    N, lat, _, _, _ = CASES[name]
    full = PLAN_LAYERS[name][6]
    assert _route(name, N, lat or full, bf16) == _route(name, BATCH, full, bf16)


def test_python_side_picks_at_the_full_lattice():
    """The table of the module docstring."""
    want = [((16, 320, 384), 32, (4, 4, 8), 0), ((16, 160, 192), 64, (4, 4, 8), 0), ((16, 80, 96), 128, (4, 4, 8), 0),
            ((8, 40, 48), 256, (4, 4, 8), 0), ((4, 20, 24), 320, (4, 4, 8), 3), ((4, 10, 12), 320, (0, 0, 0), 6)]
    for st, (lat, Cc, tile, parts) in enumerate(want):
        name = f"enc{st}.1"
        assert PLAN_LAYERS[name][6] == lat and PLAN_LAYERS[name][3] == Cc
        for bf16 in (False, True):
            r = _route(name, BATCH, lat, bf16)
            assert r["tile"] == tile and r["fwd_parts"] == parts and r["dgrad_parts"] == (parts,), (name, bf16, r)
    assert _route("dec0.0", BATCH, (4, 20, 24), False)["dgrad_parts"] == (3, 3)
    # the rules either side of W >= 16 and of the grid thresholds
    assert _wino_wgrad((4, 20, 24), 2, 320, 320) == "regions" and _wino_wgrad((4, 10, 12), 2, 320, 320) is None
    assert _wino_fwd((4, 20, 24), 320, 2, 3) is None and _wino_fwd((4, 10, 12), 320, 2, 3) is None
    assert _wino_fwd((8, 40, 48), 256, 2, 3) == "big8" and _wino_fwd((16, 320, 384), 32, 2, 1) == "w32p"
    assert _halo_bf16((4, 20, 24), 3) is None and _halo_bf16((8, 40, 48), 3) == (4, 8, 16)


# ----------------------------------------------------------------------------- part A
def _operands(name, N, lat, seed0):
    _, kind, (c1, c2), Cout, K, s, _ = PLAN_LAYERS[name]
    Cin = c1 + c2
    T = K[0] * K[1] * K[2]
    x1 = _mk(N, c1, *lat, seed=seed0)
    x2 = _mk(N, c2, *lat, seed=seed0 + 1) if c2 else None
    if kind == "tconv":
        w = _mk(Cin, Cout, *K, seed=seed0 + 2) / Cin ** 0.5
    else:
        w = _mk(Cout, Cin, *K, seed=seed0 + 2) / (Cin * T) ** 0.5
    b = _mk(Cout, seed=seed0 + 3) * (0.1 if kind != "head" else 1.0)
    ga = torch.rand(Cout, generator=torch.Generator().manual_seed(seed0 + 4)) + 0.5 if kind == "conv" else None
    be = _mk(Cout, seed=seed0 + 5) * 0.1 if kind == "conv" else None
    return x1, x2, w, b, ga, be


def _hip_layer(name):
    _, kind, _, _, K, s, _ = PLAN_LAYERS[name]
    pad = tuple(k // 2 for k in K)
    if kind == "tconv":
        return lambda x1, x2, w, b, ga, be: ops.fused_conv3d(x1, w, b, s, 0, transposed=True)
    if kind == "head":
        return lambda x1, x2, w, b, ga, be: ops.fused_conv3d(x1, w, b, 1, 0)
    return lambda x1, x2, w, b, ga, be: ops.fused_conv3d(x1, w, b, s, pad, x2=x2, inorm=(ga, be), act=ops.ACT_LRELU, slope=0.01)


def _ref_layer(name, emu=None):
    """torch.nn.functional in whatever dtype the operands have; emu: the device's interior rounding points (see
    oracle/bf16_emul.py and oracle.segmodel_oracle._cna)."""
    _, kind, (c1, c2), _, K, s, _ = PLAN_LAYERS[name]
    pad = tuple(k // 2 for k in K)
    wq = (lambda w: w) if (emu is None or c1 + c2 <= 2) else emu.weight

    def ref(x1, x2, w, b, ga, be):
        if kind == "tconv":
            return F.conv_transpose3d(x1, wq(w), b, s)
        if kind == "head":
            return F.conv3d(x1, w, b)
        y = F.conv3d(x1 if x2 is None else torch.cat([x1, x2], 1), wq(w), b, s, pad)
        if emu is None:
            ref.z = F.instance_norm(y, weight=ga, bias=be, eps=1e-5)
            return F.leaky_relu(ref.z, 0.01)
        y = emu.grad(y)                                           # dz: summed in fp32, stored once as bf16
        mean, var = y.mean((2, 3, 4), keepdim=True), y.var((2, 3, 4), unbiased=False, keepdim=True)
        return F.leaky_relu((emu.fwd(y) - mean) * torch.rsqrt(var + 1e-5) * ga.view(1, -1, 1, 1, 1) + be.view(1, -1, 1, 1, 1), 0.01)
    return ref


OPS = ("x1", "x2", "w", "b", "ga", "be")


def _wants_grad(name):
    """Differentiable operands that are compared: not the 1-channel image, not a conv bias in front of InstanceNorm."""
    _, kind, (c1, c2), _, _, _, _ = PLAN_LAYERS[name]
    return {"x1": c1 > 2, "x2": c2 > 0, "w": True, "b": kind != "conv", "ga": kind == "conv", "be": kind == "conv"}


@pytest.mark.parametrize("name", NAMES)
def test_layer_fp32_against_fp64(name):
    from rehrseg_amd import hip_backend as hb
    N, lat, n_wino, n_wgrad, _ = CASES[name]
    lat = lat or PLAN_LAYERS[name][6]
    vals = _operands(name, N, lat, 1000 + 10 * NAMES.index(name))
    want = _wants_grad(name)
    leaves = [None if v is None else v.to(DEV).requires_grad_(want[k]) for k, v in zip(OPS, vals)]
    rl = [None if v is None else v.double().requires_grad_(want[k]) for k, v in zip(OPS, vals)]
    w0, g0 = hb.wino_launches, hb.wino_wgrad_launches
    y = _hip_layer(name)(*leaves)
    ref = _ref_layer(name)
    yr = ref(*rl)
    dy = _mk(*yr.shape, seed=99)
    if PLAN_LAYERS[name][1] == "conv":
        dy, dropped = _off_the_kink(ref.z, dy)
        print(f"[stage2 {name} fp32] {dropped} of {dy.numel()} output gradients zeroed at the LeakyReLU kink")
    gl = [t for k, t in zip(OPS, leaves) if t is not None and want[k]]
    gg = torch.autograd.grad(y, gl, dy.to(DEV))
    counters = (hb.wino_launches - w0, hb.wino_wgrad_launches - g0)
    rg = torch.autograd.grad(yr, [t for k, t in zip(OPS, rl) if t is not None and want[k]], dy.double())
    errs = {"y": _relmax(y, yr)}
    for k, a, e in zip([k for k, t in zip(OPS, leaves) if t is not None and want[k]], gg, rg):
        errs["d" + k] = _relmax(a, e)
    print(f"[stage2 {name} fp32] Winograd launches fwd+dgrad / wgrad {counters}")
    _check(f"{name} fp32", errs, {k: TOL for k in errs})
    assert counters == (n_wino, n_wgrad), (name, counters)


@pytest.mark.parametrize("name", [n for n in NAMES if n != "seg"])
def test_layer_bf16_against_fp64_on_the_same_rounded_operands(name):
    _, kind, (c1, c2), _, _, _, _ = PLAN_LAYERS[name]
    N, lat, _, _, _ = CASES[name]
    lat = lat or PLAN_LAYERS[name][6]
    vals = list(_operands(name, N, lat, 3000 + 10 * NAMES.index(name)))
    q = lambda t: t.to(BF).float()
    if c1 > 2:                                                   # (the 1-channel image stays fp32 on the device)
        vals[0] = q(vals[0])
        vals[1] = q(vals[1]) if vals[1] is not None else None
    want = _wants_grad(name)
    leaves = [None if v is None else v.to(DEV).requires_grad_(want[k]) for k, v in zip(OPS, vals)]
    rl = [None if v is None else v.double().requires_grad_(want[k]) for k, v in zip(OPS, vals)]
    with ops.mixed_precision():
        y = _hip_layer(name)(*leaves)
    assert y.dtype == BF
    yr = _ref_layer(name, Bf16Emu())(*rl)
    dy = q(_mk(*yr.shape, seed=98))
    keys = [k for k, t in zip(OPS, leaves) if t is not None and want[k]]
    gg = torch.autograd.grad(y, [t for k, t in zip(OPS, leaves) if t is not None and want[k]], dy.to(DEV).to(BF))
    rg = torch.autograd.grad(yr, [t for k, t in zip(OPS, rl) if t is not None and want[k]], dy.double())
    errs = {"y": _relmax(y.float(), yr)}
    if kind == "conv":   # the bars of test_single_layer_bf16_gradients_against_fp64_on_the_same_rounded_operands
        bars = {"y": 2.0 ** -7, "dx1": 1.5e-2, "dx2": 1.5e-2, "dw": 5e-3, "dga": 5e-3, "dbe": 5e-3}
        for k, a, e in zip(keys, gg, rg):
            errs["d" + k] = _l2rel(a, e)
    else:                # test_bf16_kernels_gpu.py: bf16-stored 1e-2 of max, fp32-stored weight / bias gradients 1e-4
        bars = {"y": 1e-2, "dx1": 1e-2, "dw": 1e-4, "db": 1e-4}
        for k, a, e in zip(keys, gg, rg):
            errs["d" + k] = _relmax(a, e)
    _check(f"{name} bf16", errs, bars)


@pytest.mark.parametrize("name", [n for n in NAMES if CASES[n][1] is not None and n != "seg"])
def test_reduced_lattice_takes_the_kernels_of_the_full_lattice(name):
    """fp32 forward + backward of the layer at 2 x C x (its lattice at 16 x 320 x 384) on the device: the Winograd
    launch counters are those of the reduced case (no reference at this size: part B compares kernels there)."""
    from rehrseg_amd import hip_backend as hb
    _, _, (c1, c2), _, _, _, full = PLAN_LAYERS[name]
    _, _, n_wino, n_wgrad, _ = CASES[name]
    vals = _operands(name, 1, (1, 1, 1), 5000)
    want = _wants_grad(name)
    gen = torch.Generator(device=DEV).manual_seed(5)
    xs = [torch.randn(BATCH, c, *full, device=DEV, generator=gen) if c else None for c in (c1, c2)]
    leaves = [x.requires_grad_(want[k]) if x is not None else None for k, x in zip(OPS, xs)] + \
             [None if v is None else v.to(DEV).requires_grad_(want[k]) for k, v in list(zip(OPS, vals))[2:]]
    w0, g0 = hb.wino_launches, hb.wino_wgrad_launches
    y = _hip_layer(name)(*leaves)
    gl = [t for k, t in zip(OPS, leaves) if t is not None and want[k]]
    gg = torch.autograd.grad(y, gl, torch.randn(y.shape, device=DEV, generator=gen))
    assert all(bool(torch.isfinite(g).all()) for g in gg)
    assert (hb.wino_launches - w0, hb.wino_wgrad_launches - g0) == (n_wino, n_wgrad)


@pytest.mark.parametrize("name,parts,tile", [("enc4.1", 3, (4, 4, 8)), ("dec0.0", 3, (4, 4, 8)), ("enc5.1", 6, (0, 0, 0))])
def test_low_resolution_stages_take_the_split(name, parts, tile):
    """Stage 4 takes the 3-part split, stage 5 the 6-part split on the (0,0,0) flattened-run tile: both precisions,
    forward and input gradient (what test_layer_* run is exactly this lattice with N = 2)."""
    _, _, (c1, c2), Cout, K, _, lat = PLAN_LAYERS[name]
    assert CASES[name][0] == BATCH and CASES[name][1] is None
    assert ops.choose_tile(lat) == tile
    for bf16 in (False, True):
        fwd = ops._tap_split(lat, BATCH, ops.pad_rows(Cout), [ops.full_taps(k) for k in K], c1 + c2, bf16)
        assert fwd is not None and len(fwd) == parts
        taps = [ops.phase_taps(k, 1, k // 2, 0) for k in K]
        for c in (c1, c2):
            if c:
                bwd = ops._tap_split(lat, BATCH, ops.pad_rows(c), taps, Cout, bf16)
                assert bwd is not None and len(bwd) == parts


# ----------------------------------------------------------------------------- part B
def _cl(t):
    return t.contiguous(memory_format=torch.channels_last_3d)


def _full_operands(name, dtype, seed):
    _, _, (c1, c2), Cout, K, s, lat = PLAN_LAYERS[name]
    gen = torch.Generator(device=DEV).manual_seed(seed)
    x = _cl(torch.randn(BATCH, c1, *lat, device=DEV, generator=gen).to(dtype))
    return x, gen


@pytest.mark.parametrize("name", ["enc0.1", "enc1.1", "enc2.1", "enc3.1"])
def test_full_lattice_winograd_against_direct_kernels_fp32(name):
    """2 x C x (real lattice): Winograd forward / input gradient / weight gradient against the direct kernels behind
    USE_WINOGRAD / USE_WINOGRAD_WGRAD = False, on the device.  Bars: 2e-5 of max for activations
    (test_winograd_big_tile_kernel_against_direct_kernel_and_fp64), 1e-5 for weight and bias gradients
    (test_winograd_wgrad_64x64_block_against_direct_kernel_and_fp64)."""
    from rehrseg_amd import hip_backend as hb
    _, _, (Cc, _), _, K, _, lat = PLAN_LAYERS[name]
    pad = tuple(k // 2 for k in K)
    x, gen = _full_operands(name, torch.float32, 61)
    dz = _cl(torch.randn(BATCH, Cc, *lat, device=DEV, generator=gen))
    w = (_mk(Cc, Cc, *K, seed=62) / (Cc * K[0] * 9) ** 0.5).to(DEV)
    b = _mk(Cc, seed=63).to(DEV)
    cfg = ops.ConvCfg((1, 1, 1), pad, False)
    saved = hb.USE_WINOGRAD, hb.USE_WINOGRAD_WGRAD
    out = {}
    try:
        for flag in (False, True):
            hb.USE_WINOGRAD = hb.USE_WINOGRAD_WGRAD = flag
            w0, g0 = hb.wino_launches, hb.wino_wgrad_launches
            y, st = ops.conv_forward(x, None, w, b, cfg, ops.ACT_LRELU, 0.01, 2)
            dx = ops.conv_dgrad(dz, w, lat, Cc, 0, cfg)[0]
            dw, db = ops.conv_wgrad(dz, x, None, w, cfg, True)
            assert (hb.wino_launches - w0, hb.wino_wgrad_launches - g0) == ((2, 1) if flag else (0, 0))
            out[flag] = (y, st, dx, dw, db)
    finally:
        hb.USE_WINOGRAD, hb.USE_WINOGRAD_WGRAD = saved
    errs = {k: _dev_relmax(out[True][i], out[False][i]) for k, i in (("y", 0), ("dx", 2), ("dw", 3), ("db", 4))}
    _check(f"{name} full lattice fp32 Winograd vs direct", errs, {"y": 2e-5, "dx": 2e-5, "dw": 1e-5, "db": 1e-5})
    torch.testing.assert_close(out[True][1], out[False][1], rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("name", ["enc0.1", "enc1.1", "enc2.1", "enc3.1"])
def test_full_lattice_halo_brick_against_gather_kernel_bf16(name):
    """The bf16 legs of the same layers: LDS halo brick against the gather kernel (USE_HALO_BF16), brick against slab
    weight gradient (USE_WINOGRAD_WGRAD = False -> REHR_DBG_WGRAD_DIRECT).  Bars of
    test_halo_brick_kernel_matches_gather_kernel_and_torch / test_brick_weight_gradient_bf16_matches_slab_kernel_and_torch.
    The tags of the profiled launches tell the conv kernels apart: forward and input gradient run the 4x8x16 halo brick by
    default and the generic kernel with REHR_DBG_GG_NO_HALO."""
    import route_probe
    from rehrseg_amd import hip_backend as hb
    _, _, (Cc, _), _, K, _, lat = PLAN_LAYERS[name]
    assert _halo_bf16(lat, K[0]) == (4, 8, 16)
    pad = tuple(k // 2 for k in K)
    x, gen = _full_operands(name, BF, 64)
    dz = _cl(torch.randn(BATCH, Cc, *lat, device=DEV, generator=gen).to(BF))
    w = (_mk(Cc, Cc, *K, seed=65) / (Cc * K[0] * 9) ** 0.5).to(DEV)
    b = _mk(Cc, seed=66).to(DEV)
    cfg = ops.ConvCfg((1, 1, 1), pad, False)
    saved = hb.USE_HALO_BF16, hb.USE_WINOGRAD_WGRAD
    out = {}
    try:
        for flag in (False, True):
            hb.USE_HALO_BF16 = hb.USE_WINOGRAD_WGRAD = flag
            with route_probe.launches() as seen:
                y, st = ops.conv_forward(x, None, w, b, cfg, ops.ACT_LRELU, 0.1, 2)
                dx = ops.conv_dgrad(dz, w, lat, Cc, 0, cfg)[0]
            assert seen.kernels("gather_gemm_bf16") == ["halo 4x8x16" if flag else "generic"] * 2, (flag, seen)
            dw, _ = ops.conv_wgrad(dz, x, None, w, cfg, False)
            out[flag] = (y, st, dx, dw)
    finally:
        hb.USE_HALO_BF16, hb.USE_WINOGRAD_WGRAD = saved
    assert out[True][0].dtype == BF and out[True][2].dtype == BF and out[True][3].dtype == torch.float32
    errs = {"y": _dev_relmax(out[True][0], out[False][0]), "stats": _dev_relmax(out[True][1], out[False][1]),
            "dx": _dev_relmax(out[True][2], out[False][2]), "dw": _dev_relmax(out[True][3], out[False][3])}
    _check(f"{name} full lattice bf16 brick vs gather", errs, {"y": 1e-2, "stats": 1e-5, "dx": 1e-2, "dw": 1e-5})


@pytest.mark.parametrize("name,mixed", [("dec4.up", False), ("dec4.up", True), ("dec3.up", True)])
def test_full_lattice_tconv_ks_against_generic_grid(name, mixed, monkeypatch):
    """The decoder's kernel = stride transposed convs that tconv_ks.hip takes (64 -> 32 in both precisions, 128 -> 64 in
    bf16) at 2 x C x (real lattice) against the one-block-per-(tile, phase) grid: 1e-5 of max in fp32, 2^-7 in bf16
    (test_transposed_conv_kernel_equals_stride_fused_kernel).  The tags of the profiled launches tell the two apart."""
    import route_probe
    from rehrseg_amd import hip_backend as hb
    _, _, (Cin, _), Cout, K, s, lat = PLAN_LAYERS[name]
    assert _tconv_ks(Cin, ops.pad_rows(Cout), mixed)
    x, _ = _full_operands(name, BF if mixed else torch.float32, 67)
    w = (_mk(Cin, Cout, *K, seed=68) / Cin ** 0.5).to(DEV)
    b = _mk(Cout, seed=69).to(DEV)
    cfg = ops.ConvCfg(s, (0, 0, 0), True)
    out = {}
    for flag in (True, False):
        monkeypatch.setattr(hb, "USE_TCONV_KS", flag)
        with route_probe.launches() as seen:
            out[flag] = ops.conv_forward(x, None, w, b, cfg, ops.ACT_NONE, 0.0, 0)[0]
        assert seen.kernels() == ["tconv_ks" if flag else "generic"], (flag, seen)
    assert tuple(out[True].shape[2:]) == _out_lat(lat, K, s, True)
    _check(f"{name} full lattice tconv_ks vs generic {'bf16' if mixed else 'fp32'}",
           {"y": _dev_relmax(out[True], out[False])}, {"y": 2.0 ** -7 if mixed else 1e-5})


# ----------------------------------------------------------------------------- part C
def test_sr_head0_upsample_conv_on_a_full_width_slab():
    """sr_head.0 (32 -> 16, 3x3x3, upscale 4, depth 16 -> 64) on 1 x 32 x 16 x 32 x 384: the (1,3,3) part runs as a
    48-channel conv (Npad 64: big8 Winograd on 2 x 24 regions, as on the 320-row plane) on the low-resolution slices.
    Against interpolate -> conv -> ReLU in fp64 at the bar of test_upsample_conv3d_depth."""
    from rehrseg_amd import hip_backend as hb
    lat = (16, 32, 384)
    assert _wino_fwd(lat, ops.pad_rows(48), 1, 1) == _wino_fwd(FULL, ops.pad_rows(48), BATCH, 1) == "big8"
    x = _mk(1, 32, *lat, seed=33)
    w = _mk(16, 32, 3, 3, 3, seed=34) / (32 * 27) ** 0.5
    b = _mk(16, seed=35)
    gin = [t.to(DEV).requires_grad_() for t in (x, w, b)]
    rin = [t.double().requires_grad_() for t in (x, w, b)]
    w0 = hb.wino_launches
    y = ops.upsample_conv3d_depth(*gin, 4, act=ops.ACT_RELU)
    z = F.conv3d(F.interpolate(rin[0], scale_factor=(4, 1, 1), mode="trilinear", align_corners=True), rin[1], rin[2], 1, 1)
    yr = F.relu(z)
    assert tuple(y.shape) == (1, 16, 64, 32, 384)
    dy, dropped = _off_the_kink(z, _mk(*yr.shape, seed=99))
    print(f"[stage2 sr_head.0] {dropped} of {dy.numel()} output gradients zeroed at the ReLU kink")
    gg = torch.autograd.grad(y, gin, dy.to(DEV))
    rg = torch.autograd.grad(yr, rin, dy.double())
    assert hb.wino_launches - w0 == 2
    errs = {"y": _relmax(y, yr), "dx": _relmax(gg[0], rg[0]), "dw": _relmax(gg[1], rg[1]), "db": _relmax(gg[2], rg[2])}
    _check("sr_head.0", errs, {k: TOL for k in errs})


@pytest.mark.parametrize("mixed", [False, True])
def test_sr_head2_thin_output_conv_on_a_full_width_slab(mixed):
    """sr_head.2 (16 -> 2, 5x5x5) on 1 x 16 x 64 x 10 x 384.  thin5_supported declines 384 columns in both precisions
    (thin_conv_f32 takes W <= 128, thin_conv_bf16 W <= 160), so what runs -- and what is tested here -- is the fallback:
    the fp32 thin-output kernels of direct_conv.hip, under mixed precision behind a cast of the bf16 features.  fp32: 1e-4
    of max (test_thin_output_and_half_chunk_convs); mixed: the fp32-stored logits and weight / bias gradients 1e-4, the
    input gradient (cast back to bf16) 1e-2, against fp64 on the same rounded features."""
    from rehrseg_amd import hip_backend as hb
    shape = (1, 16, 64, 10, 384)
    assert not hb.thin5_supported(shape, (2, 16, 5, 5, 5), (2, 2, 2), torch.float32)
    assert not hb.thin5_supported(shape, (2, 16, 5, 5, 5), (2, 2, 2), torch.bfloat16)
    x = _mk(*shape, seed=40)
    w = _mk(2, 16, 5, 5, 5, seed=41) / (16 * 125) ** 0.5
    b = _mk(2, seed=42)
    if mixed:
        x = x.to(BF).float()
    rin = [t.double().requires_grad_() for t in (x, w, b)]
    gin = [t.to(DEV).requires_grad_() for t in (x, w, b)]
    if mixed:
        with ops.mixed_precision():
            y = ops.fused_conv3d(gin[0].to(BF), gin[1], gin[2], 1, 2)
    else:
        y = ops.fused_conv3d(*gin, 1, 2)
    assert y.dtype == torch.float32
    yr = F.conv3d(*rin, 1, 2)
    dy = _mk(*yr.shape, seed=99)
    gg = torch.autograd.grad(y, gin, dy.to(DEV))
    rg = torch.autograd.grad(yr, rin, dy.double())
    errs = {"y": _relmax(y, yr), "dx": _relmax(gg[0], rg[0]), "dw": _relmax(gg[1], rg[1]), "db": _relmax(gg[2], rg[2])}
    _check("sr_head.2 " + ("mixed" if mixed else "fp32"), errs, {"y": TOL, "dx": 1e-2 if mixed else TOL, "dw": TOL, "db": TOL})
