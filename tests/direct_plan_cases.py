"""Descriptor table of the direct gather-GEMM kernels (tests/test_direct_plan_cpu.py, tools/gen_golden_direct_plan.py):
what rehr_gather_gemm_direct_route and the four launch entry points do with rehr_gather_gemm_desc calls, fp32 and bf16.

The descriptors come from the builder of tests/wino_plan_cases.py: dummy aligned pointers that nothing on the host
dereferences, no Winograd scratch.  tests/golden/direct_plan.json holds the return codes of the library BEFORE the route
query existed; the route of a row is therefore written here by hand, next to the predicate that decides it (halo_shared.h:
halo_brick_plan, direct_route; halo_conv.hip: halo_f32_plan; halo_conv_bf16.hip: halo_bf16_plan; tconv_ks.hip:
tconv_ks_match).

Routes: "generic", "tconv_ks", "none" (no direct kernel reaches the operands: REHR_ENOSUP), the fp32 halo variants
"halo bn64" / "halo bn32" (2 x 8 x 8 bricks, 64- / 32-channel tile) and the bf16 bricks "halo 4x8x16" / "halo 8x8x8" /
"halo 2x16x16".  Padding figures are brick-padded lattice / lattice; a brick is taken up to 1.3x."""
import ctypes as C

from rehrseg_amd import lib as L
from wino_plan_cases import BIAS, EHIP, EINVAL, ENOSUP, OK, STATS, X2, Y, c3, desc, taps  # noqa: F401

G, H = L.GG_DIRECT_GENERIC, L.GG_DIRECT_HALO
ROUTES = {"none": (L.GG_DIRECT_NONE, 0), "generic": (G, 0), "tconv_ks": (L.GG_DIRECT_TCONV_KS, 0),
          "halo bn64": (H, 1), "halo bn32": (H, 2), "halo 4x8x16": (H, 1), "halo 8x8x8": (H, 2), "halo 2x16x16": (H, 3)}
F32_ROUTES = ("none", "generic", "tconv_ks", "halo bn64", "halo bn32")
BF16_ROUTES = ("none", "generic", "tconv_ks", "halo 4x8x16", "halo 8x8x8", "halo 2x16x16")
FLAGS = {"0": 0, "NO_HALO": L.DBG_GG_NO_HALO, "NO_TCONV_KS": L.DBG_GG_NO_TCONV_KS}


def k133(**kw):
    """1 x 3 x 3 taps (kd = 1)."""
    return dict(kd=1, **kw)


# (name, desc() arguments, fp32 route, bf16 route, the predicates that decide them)
ROWS = [
    # ---- every variant, and the 1.3x rule per brick
    ("4x16x24 64->64", c3(1, 64, 64, (4, 16, 24)), "halo bn64", "generic",
     "fp32 exact; bf16 4x8x16 pads W 24 -> 32 = 1.333 > 1.3, 8x8x8 pads D 4 -> 8 = 2.0"),
    ("2x8x16 32->32 N2", c3(2, 32, 32, (2, 8, 16)), "halo bn32", "generic",
     "fp32 exact, Npad 32; bf16 4x8x16 pads D 2 -> 4 = 2.0, 8x8x8 lattice below the brick (Ld 2 < 4)"),
    ("8x16x32 64->64", c3(1, 64, 64, (8, 16, 32)), "halo bn64", "halo 4x8x16", "exact in both"),
    ("6x16x32 64->64", c3(1, 64, 64, (6, 16, 32)), "halo bn64", "generic",
     "fp32 exact; bf16 4x8x16 and 8x8x8 both pad D 6 -> 8 = 1.333 > 1.3"),
    ("8x8x8 32->32", c3(1, 32, 32, (8, 8, 8)), "halo bn32", "halo 8x8x8", "bf16 4x8x16: lattice below the brick (Lw 8 < 16)"),
    ("8x24x24 64->64", c3(1, 64, 64, (8, 24, 24)), "halo bn64", "halo 8x8x8", "bf16 4x8x16 pads W 24 -> 32 = 1.333 > 1.3"),
    ("8x8x24 64->16", c3(1, 64, 16, (8, 8, 24)), "halo bn32", "halo 8x8x8", "Npad 32; bf16 4x8x16 1.333 > 1.3"),
    ("15x44x43 64->64", c3(1, 64, 64, (15, 44, 43)), "halo bn64", "halo 4x8x16", "16 x 48 x 48 / 28380 = 1.2989, both"),
    ("13x43x37 64->64", c3(1, 64, 64, (13, 43, 37)), "halo bn64", "generic",
     "fp32 14 x 48 x 40 / 20683 = 1.2996; bf16 4x8x16 1.78 > 1.3, 8x8x8 1.485 > 1.3"),
    ("7x15x15 64->64", c3(1, 64, 64, (7, 15, 15)), "generic", "generic",
     "8 x 16 x 16 / 1575 = 1.3003 > 1.3 for fp32 2x8x8 and bf16 8x8x8; 4x8x16: lattice below the brick"),
    ("7x15x30 64->64", c3(1, 64, 64, (7, 15, 30)), "generic", "generic", "8 x 16 x 32 / 3150 = 1.3003 > 1.3 for every brick"),
    ("5x17x23 64->64", c3(1, 64, 64, (5, 17, 23)), "generic", "generic", "fp32 6 x 24 x 24 / 1955 = 1.77 > 1.3; bf16 3.1, 2.4"),
    ("7x15x23 64->64", c3(1, 64, 64, (7, 15, 23)), "halo bn64", "halo 8x8x8",
     "8 x 16 x 24 / 2415 = 1.27 for fp32 2x8x8 and bf16 8x8x8; bf16 4x8x16 pads 8 x 16 x 32 = 1.70 > 1.3"),
    ("4x15x23 32->32", c3(1, 32, 32, (4, 15, 23)), "halo bn32", "generic",
     "fp32 4 x 16 x 24 / 1380 = 1.11; bf16 4x8x16 1.48 > 1.3, 8x8x8 2.2"),
    # ---- 1 x 3 x 3 taps: the third bf16 brick
    ("133 2x16x16 32->32", c3(1, 32, 32, (2, 16, 16), **k133()), "halo bn32", "halo 2x16x16",
     "T = 9; bf16 4x8x16 pads D 2 -> 4 = 2.0, 8x8x8 Ld 2 < 4"),
    ("133 2x32x48 64->64", c3(1, 64, 64, (2, 32, 48), **k133()), "halo bn64", "halo 2x16x16", "as above"),
    ("133 6x16x16 64->64", c3(1, 64, 64, (6, 16, 16), **k133()), "halo bn64", "halo 2x16x16", "bf16 4x8x16 and 8x8x8 pad D to 8 = 1.333 > 1.3"),
    ("133 4x16x16 32->32", c3(1, 32, 32, (4, 16, 16), **k133()), "halo bn32", "halo 4x8x16", "exact"),
    ("133 1x16x16 32->32", c3(1, 32, 32, (1, 16, 16), **k133()), "generic", "generic",
     "fp32 lattice below the brick (Ld 1 < 2); bf16 2x16x16 takes Ld 1 >= (2 + 1) / 2 but pads 2.0 > 1.3"),
    ("333 2x16x16 32->32", c3(1, 32, 32, (2, 16, 16)), "halo bn32", "generic", "2x16x16 is for T = 9 only; 4x8x16 2.0, 8x8x8 Ld < 4"),
    # ---- the stage-2 lattices of ANISO_PLAN (N = 2), as tests/test_stage2_lattice_gpu.py::_halo_bf16 predicts
    ("enc0.1 16x320x384 32", c3(2, 32, 32, (16, 320, 384), **k133()), "halo bn32", "halo 4x8x16", "exact"),
    ("enc1.1 16x160x192 64", c3(2, 64, 64, (16, 160, 192), **k133()), "halo bn64", "halo 4x8x16", "exact"),
    ("enc2.1 16x80x96 128", c3(2, 128, 128, (16, 80, 96)), "generic", "halo 4x8x16", "fp32 Npad > 64; bf16 exact"),
    ("enc3.1 8x40x48 256", c3(2, 256, 256, (8, 40, 48)), "generic", "halo 4x8x16", "fp32 Npad > 64; bf16 exact"),
    ("enc4.1 4x20x24 320", c3(2, 320, 320, (4, 20, 24)), "generic", "generic",
     "fp32 Npad > 64; bf16 4x8x16 4 x 24 x 32 / 1920 = 1.6 > 1.3, 8x8x8 2.4 (declined)"),
    ("enc5.1 4x10x12 320", c3(2, 320, 320, (4, 10, 12)), "generic", "generic", "fp32 Npad > 64; bf16 lattice below the brick (Lw 12 < 16), 8x8x8 4.3"),
    # ---- entry conditions
    ("stride 2 along h", c3(1, 64, 64, (8, 16, 32), sh=2, Hi=32), "generic", "generic", "stride != 1 (both)"),
    ("Npad 128", c3(1, 64, 128, (8, 16, 32)), "generic", "halo 4x8x16", "fp32 Npad > 64"),
    ("1x1x3 taps", c3(1, 64, 64, (8, 16, 32), kd=1, th=taps(1), bh=0, KH=1), "generic", "generic", "fp32 T < 9; bf16 T not in {9, 27}"),
    ("5x5x3 taps", c3(1, 64, 64, (8, 16, 32), kd=5, th=taps(5), bh=-2, KH=5), "generic", "generic", "fp32 T > 64; bf16 T not in {9, 27}"),
    ("5x5x5 taps", c3(1, 64, 64, (8, 16, 32), kd=5, th=taps(5), bh=-2, KH=5, tw=taps(5), bw=-2, KW=5), "generic", "generic",
     "fp32 T > 64 (and its halo 6 x 12 x 12 = 864 rows: hvox > 416); bf16 T not in {9, 27}"),
    ("4x4x4 taps", c3(1, 64, 64, (8, 16, 32), kd=4, th=taps(4), bh=-2, KH=4, tw=taps(4), bw=-2, KW=4), "generic", "generic",
     "fp32 T = 64 but the halo 5 x 11 x 11 = 605 rows: hvox > 416; bf16 T not in {9, 27}"),
    ("2x3x3 taps", c3(1, 64, 64, (8, 16, 32), kd=2), "halo bn64", "generic", "fp32 T = 18, halo 300 rows; bf16 T not in {9, 27}"),
    ("1x1x9 taps", c3(1, 64, 64, (8, 16, 32), kd=1, th=taps(1), bh=0, KH=1, tw=taps(9), bw=-4, KW=9), "halo bn64", "generic",
     "fp32 T = 9, halo 2 x 8 x 16 = 256 rows; bf16 an axis with more than 3 taps at T = 9"),
    ("1x3x9 taps", c3(1, 64, 64, (8, 16, 32), kd=1, tw=taps(9), bw=-4, KW=9), "halo bn64", "generic",
     "fp32 T = 27, halo 2 x 10 x 16 = 320 rows; bf16 an axis with more than 3 taps at T = 27"),
    ("133 dilated rows", c3(1, 64, 64, (8, 16, 32), kd=1, th=taps(3, off0=-2, offs=2), bh=0), "halo bn64", "generic",
     "fp32 halo 2 x 12 x 10 = 240 rows; bf16 halo > brick + 2 (HH = BH + 4) for all three bricks"),
    ("Cout 60", c3(1, 64, 60, (8, 16, 32)), "halo bn64", "generic", "bf16 Cout % 8"),
    ("ldy 68", c3(1, 64, 64, (8, 16, 32), ldy=68), "halo bn64", "generic", "bf16 ldy % 8"),
    ("y misaligned by 8", c3(1, 64, 64, (8, 16, 32), y=Y + 8), "halo bn64", "generic", "bf16 y & 15"),
    ("virtual concat", c3(1, 64, 64, (8, 16, 32), c1=32, ldx1=32, x2=X2, ldx2=32), "halo bn64", "halo 4x8x16", "c1 on a chunk boundary"),
    ("statistics and activation", c3(2, 32, 32, (8, 16, 32), stats=STATS, stats_mode=2, act=2, bias=BIAS), "halo bn32", "halo 4x8x16", "epilogue only"),
    # ---- 32-bit ranges
    ("source sample 2^32 B in fp32", c3(1, 64, 64, (64, 512, 512)), "none", "halo 4x8x16", "fp32 gg_src_fits (2^32 B; the generic plan declines too); bf16 2^31 B"),
    ("source sample 2^32 B in bf16", c3(1, 64, 64, (128, 512, 512)), "none", "none", "gg_src_fits in both (generic plan too)"),
    ("source rows of 128 channels, 2^32 B in bf16", c3(1, 128, 64, (64, 512, 512)), "none", "none", "gg_src_fits: 2^24 voxels x 128 x 2 B"),
    ("wp over the limit in fp32", c3(1, 622592, 64, (8, 8, 8)), "none", "halo 8x8x8", "fp32 wp_bytes 27 x 64 x 622592 x 4 >= 2^32 - 64; bf16 half of it"),
    ("wp under the limit in fp32", c3(1, 621376, 64, (8, 8, 8)), "halo bn64", "halo 8x8x8", "fp32 wp_bytes = 2^32 - 16384 < 2^32 - 64"),
    ("wp over the limit in bf16", c3(1, 1245184, 64, (8, 8, 8)), "none", "none", "wp_bytes >= 2^32 - 64 in both"),
    ("wp under the limit in bf16", c3(1, 1242752, 64, (8, 8, 8)), "none", "halo 8x8x8", "bf16 wp_bytes = 2^32 - 16384; fp32 twice that"),
    ("y 2^32 B in bf16", c3(1, 64, 64, (8, 16, 32), ldy=524288), "halo bn64", "generic", "bf16 y bytes 4096 x 524288 x 2 >= 2^32 - 64 (buffer stores); fp32 stores through pointers"),
    ("y under 2^32 - 64 B in bf16", c3(1, 64, 64, (8, 16, 32), ldy=524280), "halo bn64", "halo 4x8x16", "bf16 y bytes 2^32 - 65536"),
    # ---- invalid
    ("Cin 24", c3(1, 24, 64, (8, 16, 32)), "EINVAL", "EINVAL", "gg_validate Cin % 16"),
    ("null y", c3(1, 64, 64, (8, 16, 32), y=None), "EINVAL", "EINVAL", "gg_validate"),
]

def tphases(Cin, Cout, plane, s, N=2, parts=None, vary=None, **kw):
    """The stride phases of a kernel == stride transposed convolution Cin -> Cout on input lattice `plane` (what
    ops.conv_transpose3d hands to the multi entry points): one tap each, output stride s, phase p at output offset p.
    parts: only the first so many phases; vary = (index, fields) changes one part; kw changes all."""
    out = []
    Ld, Lh, Lw = plane
    for pd in range(s[0]):
        for ph in range(s[1]):
            for pw in range(s[2]):
                a = c3(N, Cin, Cout, plane, kd=1, bd=0, bh=0, bw=0, td=taps(1, k0=pd), th=taps(1, k0=ph), tw=taps(1, k0=pw),
                       KH=s[1], KW=s[2], osd=s[0], osh=s[1], osw=s[2], obd=pd, obh=ph, obw=pw,
                       Dy=Ld * s[0], Hy=Lh * s[1], Wy=Lw * s[2])
                out.append(dict(a, **kw))
    out = out[:parts]
    if vary:
        out[vary[0]] = dict(out[vary[0]], **vary[1])
    return out


T4, T8 = ["tconv_ks"] * 4, ["tconv_ks"] * 8
G4, G8 = ["generic"] * 4, ["generic"] * 8
HALO = c3(1, 64, 64, (8, 16, 32))           # a halo shape in both precisions
STRIDED = c3(1, 64, 64, (8, 16, 32), sh=2, Hi=32)   # the same layer's operands, a generic shape

# (name, parts, fp32 routes or "EINVAL", bf16 routes or "EINVAL", the predicates that decide them)
MULTI = [
    ("tconv 64->32 s222", tphases(64, 32, (4, 8, 8), (2, 2, 2)), T8, T8, "tconv_ks_match"),
    ("tconv 32->32 s122", tphases(32, 32, (4, 8, 8), (1, 2, 2)), T4, T4, "tconv_ks_match"),
    ("tconv 64->128 s122", tphases(64, 128, (4, 16, 16), (1, 2, 2)), T4, T4, "tconv_ks_match, Npad 128"),
    ("tconv 96->32 s122", tphases(96, 32, (4, 8, 8), (1, 2, 2)), G4, T4, "fp32 Cin > 64: the generic grid; bf16 takes Cin <= 128"),
    ("tconv 128->64 s222", tphases(128, 64, (4, 8, 8), (2, 2, 2)), G8, T8, "fp32 Cin > 64: the generic grid"),
    ("tconv Cin 160", tphases(160, 64, (4, 8, 8), (1, 2, 2)), G4, G4, "Cin > 128"),
    ("tconv Cin 48", tphases(48, 64, (4, 8, 8), (1, 2, 2)), G4, G4, "Cin % 32"),
    ("tconv Cout 160", tphases(64, 160, (4, 8, 8), (1, 2, 2)), G4, G4, "Npad > 128"),
    ("tconv with x2", tphases(64, 32, (4, 8, 8), (1, 2, 2), x2=X2, ldx2=64), G4, G4, "x2 != nullptr"),
    ("tconv with activation", tphases(64, 32, (4, 8, 8), (1, 2, 2), act=1), G4, G4, "act != NONE"),
    ("tconv with statistics", tphases(64, 32, (4, 8, 8), (1, 2, 2), stats=STATS, stats_mode=1), G4, G4, "stats_mode != 0"),
    ("tconv fp32 output", tphases(64, 32, (4, 8, 8), (1, 2, 2), flags=L.GG_Y_F32), G4, G4, "flags & REHR_GG_Y_F32"),
    ("tconv 3 of 4 phases", tphases(64, 32, (4, 8, 8), (1, 2, 2), parts=3), G4[:3], G4[:3], "osd x osh x osw != count"),
    ("tconv into a larger y", tphases(64, 32, (4, 8, 8), (1, 2, 2), Hy=17), G4, G4, "Hy != Hi x osh"),
    ("tconv 3-wide kernel", tphases(64, 32, (4, 8, 8), (1, 2, 2), KW=3), G4, G4, "KW != osw"),
    ("tconv part 1 into another y", tphases(64, 32, (4, 8, 8), (1, 2, 2), vary=(1, dict(y=Y + 0x100000))), G4, G4,
     "d.y != d0.y (bf16: parts that differ in y are split-K parts, the generic grid)"),
    ("tconv part 2 with another bias", tphases(64, 32, (4, 8, 8), (1, 2, 2), vary=(2, dict(bias=BIAS))), G4, G4, "d.bias != d0.bias"),
    ("tconv part 1 with another ldy", tphases(64, 32, (4, 8, 8), (1, 2, 2), vary=(1, dict(ldy=64))), G4, G4, "d.ldy != d0.ldy"),
    ("tconv part 3 with two taps", tphases(64, 32, (4, 8, 8), (1, 2, 2), vary=(3, dict(tw=taps(2, k0=0, ks=1)))), G4, G4, "tw.count != 1"),
    ("tconv part 0 with a tap offset", tphases(64, 32, (4, 8, 8), (1, 2, 2), vary=(0, dict(th=taps(1, off0=1)))), G4, G4, "th.off0 != 0"),
    ("tconv part 1 with a base offset", tphases(64, 32, (4, 8, 8), (1, 2, 2), vary=(1, dict(bw=1))), G4, G4, "d.bw != 0"),
    ("tconv part 2 on a shorter lattice", tphases(64, 32, (4, 8, 8), (1, 2, 2), vary=(2, dict(Lh=7))), G4, G4, "d.Lh != d0.Hi"),
    ("tconv part 1 with the other tap", tphases(64, 32, (4, 8, 8), (1, 2, 2), vary=(1, dict(tw=taps(1, k0=0)))), G4, G4, "d.obw != d.tw.k0"),
    ("tconv part 3 repeats phase 2", tphases(64, 32, (4, 8, 8), (1, 2, 2), vary=(3, dict(tw=taps(1, k0=0), obw=0))), G4, G4, "seen: a phase twice"),
    ("tconv part 1 with an activation", tphases(64, 32, (4, 8, 8), (1, 2, 2), vary=(1, dict(act=1))), G4, G4, "d.act != NONE"),
    ("tconv odd ldy", tphases(64, 32, (4, 8, 8), (1, 2, 2), ldy=33), T4, G4, "bf16 ldy % 2"),
    # ---- parts that are no tconv phases: one decision per part
    ("two halo parts into one y", [HALO, HALO], ["halo bn64"] * 2, ["halo 4x8x16"] * 2, "per part"),
    ("two halo parts into two y", [HALO, dict(HALO, y=Y + 0x100000)], ["halo bn64"] * 2, G4[:2],
     "bf16: split-K parts with different y stay in the generic grid"),
    ("three split-K parts", [dict(HALO, y=Y + 0x100000 * i) for i in range(3)], ["halo bn64"] * 3, G4[:3], "as above"),
    ("halo part, strided part", [HALO, STRIDED], ["halo bn64", "generic"], ["halo 4x8x16", "generic"], "per part; the strided part: stride != 1"),
    ("strided part, halo part", [STRIDED, HALO], ["generic", "halo bn64"], ["generic", "halo 4x8x16"], "per part"),
    # ---- invalid calls
    ("halo part, invalid part", [HALO, dict(HALO, Ld=0)], "EINVAL", "EINVAL", "gg_validate Ld < 1 on part 1"),
    ("halo part, halo part, invalid part", [HALO, HALO, dict(HALO, Cout=0)], "EINVAL", "EINVAL", "gg_validate Cout < 1 on part 2"),
    ("strided part, invalid part", [STRIDED, dict(STRIDED, Ld=0)], "EINVAL", "EINVAL", "gg_validate Ld < 1 on part 1"),
    ("halo part, part with another Npad", [HALO, dict(HALO, Npad=96)], "EINVAL", "EINVAL", "parts of one layer: Npad"),
    ("halo part, part with another wp", [HALO, dict(HALO, wp=0x70000)], "EINVAL", "EINVAL", "parts of one layer: wp"),
    ("strided part, part with another Cin", [STRIDED, dict(STRIDED, Cin=32, c1=32)], ["generic"] * 2, "EINVAL",
     "bf16 only: Cin (the generic launch takes its chunk width from part 0)"),
    ("tconv with an invalid phase", tphases(64, 32, (4, 8, 8), (1, 2, 2), vary=(3, dict(N=0))), "EINVAL", "EINVAL", "gg_validate N < 1"),
]

# bf16 multi-part rows whose recorded code differs from today's for ONE reason: the recorded library launched part 0 (a
# halo shape: REHR_EHIP where there is no device) before it validated the later part; now every part is validated before
# anything launches, and the call is REHR_EINVAL like its fp32 twin always was.
LAUNCHED_BEFORE_VALIDATION = {"halo part, invalid part", "halo part, halo part, invalid part", "halo part, part with another Npad",
                              "halo part, part with another wp"}


def bind(path=None):
    """The four recorded entry points of the library at `path` (any ABI version), or of the in-tree one."""
    lib = C.CDLL(path) if path else L.load()
    P = C.POINTER(L.GatherGemmDesc)
    for n in ("rehr_gather_gemm_f32", "rehr_gather_gemm_bf16"):
        getattr(lib, n).restype, getattr(lib, n).argtypes = C.c_int, [P, C.c_void_p]
    for n in ("rehr_gather_gemm_multi_f32", "rehr_gather_gemm_multi_bf16"):
        getattr(lib, n).restype, getattr(lib, n).argtypes = C.c_int, [P, C.c_int32, C.c_void_p]
    return lib


def make(parts, flags=0):
    arr = (L.GatherGemmDesc * len(parts))(*(desc(**a) for a in parts))
    for d in arr:
        d.debug_flags = flags
    return arr


def row_codes(lib, args):
    """{flag setting: [f32, multi_f32, bf16, multi_bf16]} return codes of one descriptor."""
    out = {}
    for f, bits in FLAGS.items():
        a = make([args], bits)
        out[f] = [int(lib.rehr_gather_gemm_f32(a, None)), int(lib.rehr_gather_gemm_multi_f32(a, 1, None)),
                  int(lib.rehr_gather_gemm_bf16(a, None)), int(lib.rehr_gather_gemm_multi_bf16(a, 1, None))]
    return out


def multi_codes(lib, parts):
    """{flag setting: [multi_f32, multi_bf16]} return codes of one multi-part call."""
    out = {}
    for f, bits in FLAGS.items():
        a = make(parts, bits)
        out[f] = [int(lib.rehr_gather_gemm_multi_f32(a, len(parts), None)), int(lib.rehr_gather_gemm_multi_bf16(a, len(parts), None))]
    return out
