"""Case table of the thin-channel convolution kernels (csrc/direct_conv.hip, csrc/thin_cin_conv.hip) for
tests/test_thin_kernels_gpu.py, with the launch regime every row is there for.  tests/test_thin_kernel_regimes_cpu.py
checks the regime column without a device: against the library's own route and size queries where it has one, and
against the restatements of the launch geometry below where it has none (the forward kernels).

A row is row(name, Cin, Cout, K, N, inp, stride, pad, regime); `inp` = (D, H, W) of the input, pad defaults to
(K - 1) // 2.  The regime tuple of a family is what its *_geometry function returns for the row.

Rows whose extents differ from the first draft of the table, because the regime test showed that the draft missed:
  * matrix-core weight gradient 2->32 3x7x7 stride (1,2,2): 4 x (4,40,140) has 40 tiles under a cap of 64 blocks (one
    tile per block); 4 x (5,40,270) has 75 tiles: two per block, the last block holds one.
  * thin output 48->4 1x1x1: 2 x (4,50,21) has 400 rows in 200 full strips of two; 3 x (3,45,21) has 405 rows: 203
    strips, the last holds one row.
  * thin output 64->4 3x3x3 and 48->2 3x3x3: their halo (4 x 10 x 10 voxels x Cin floats) does not fit the 64 KB of the
    halo-brick weight gradient; they run the channel-group <4,16> and the plain <2> kernel.  32->2 3x3x3 was added for
    small_cout_wgrad_halo_kernel<2>.
  * thin output 64->2 1x3x3: 144 pairs and a 53 KB halo, so its weight gradient is the halo brick <2>, not the
    channel-group kernel (its forward is); 64->2 1x1x1 was added for small_cout_wgrad_cg_kernel<2,16>.
"""
from thin_plan_cases import desc  # noqa: F401  (re-exported for the tests)


def row(name, Cin, Cout, K, N, inp, stride=(1, 1, 1), pad=None, regime=None, **extra):
    pad = tuple((k - 1) // 2 for k in K) if pad is None else pad
    out = tuple((inp[a] + 2 * pad[a] - K[a]) // stride[a] + 1 for a in range(3))
    return dict(name=name, Cin=Cin, Cout=Cout, K=K, N=N, inp=inp, stride=stride, pad=pad, out=out, regime=regime, **extra)


def desc_args(r, **over):
    return dict(Cin=r["Cin"], Cout=r["Cout"], N=r["N"], inp=r["inp"], K=r["K"], stride=r["stride"], pad=r["pad"], **over)


def _cdiv(a, b):
    return -(-a // b)


def _T(r):
    return r["K"][0] * r["K"][1] * r["K"][2]


def _ovox(r):
    return r["out"][0] * r["out"][1] * r["out"][2]


# ----------------------------------------------------------------------------- restated launch geometry
def vfwd_geometry(r, stats):
    """rehr_conv_small_cin_fwd_f32, vector route -> (wave groups, voxels per tile, tiles, voxels of the last tile,
    grid.x, blocks that walk a second tile, dynamic LDS above 48 KB)."""
    groups = r["Cout"] // 16
    vpb = 64 * (4 // groups)
    tiles = _cdiv(_ovox(r), vpb)
    cap = max((512 if stats else 4096) // r["N"], 1)
    bx = min(tiles, cap)
    return groups, vpb, tiles, _ovox(r) - (tiles - 1) * vpb, bx, tiles - bx, r["Cin"] * _T(r) * r["Cout"] * 4 > 48 * 1024


def vwg_geometry(r):
    """small_cin_wgrad_plan + the dispatch of rehr_conv_small_cin_wgrad_f32 -> (kernel, taps per wave, waves that own a
    tap, blocks, voxels per block, voxels of the last block, blocks that straddle two samples)."""
    total = r["N"] * _ovox(r)
    vpb = max(_cdiv(total, 1024), 64)
    blocks = _cdiv(total, vpb)
    tpw = _cdiv(_T(r), 4)
    straddle = sum(1 for b in range(blocks) if (b * vpb) // _ovox(r) != (min(total, (b + 1) * vpb) - 1) // _ovox(r))
    return "<8>" if tpw <= 8 else "<40>", tpw, min(4, _cdiv(_T(r), tpw)), blocks, vpb, total - (blocks - 1) * vpb, straddle


def vwg_workspace_bytes(r):
    g = vwg_geometry(r)
    return g[3] * (r["Cin"] * _T(r) + 1) * 64 * 4


def mfwd_geometry(r):
    """thin_cin_fwd_plan -> (voxel columns of a tile, tiles per sample, grid.x, tiles per block, tiles of the last block)."""
    cols = 64 if r["Cout"] == 32 else 32
    tiles = r["out"][0] * _cdiv(r["out"][1], 4) * _cdiv(r["out"][2], cols)
    bx = min(tiles, max(1024 // r["N"], 1))
    tpb = _cdiv(tiles, bx)
    bx = _cdiv(tiles, tpb)
    return cols, tiles, bx, tpb, tiles - (bx - 1) * tpb


def mwg_geometry(r):
    """thin_cin_wgrad_plan -> (tap tiles of 16 columns, tiles per sample, grid.x, tiles per block, tiles of the last
    block)."""
    ntn = _cdiv(_T(r) + 1, 16)
    tiles = r["out"][0] * _cdiv(r["out"][1], 4) * _cdiv(r["out"][2], 64)
    bx = min(tiles, max(512 // (r["N"] * r["Cin"]), 1))
    tpb = _cdiv(tiles, bx)
    bx = _cdiv(tiles, tpb)
    return ntn, tiles, bx, tpb, tiles - (bx - 1) * tpb


def mwg_workspace_bytes(r):
    g = mwg_geometry(r)
    return g[2] * r["N"] * r["Cin"] * r["Cout"] * 16 * g[0] * 4


HB_D, HB_H, HB_W = 2, 8, 8   # the output brick of the halo weight gradient


def out_geometry(r):
    """The dispatch of rehr_conv_small_cout_{fwd,wgrad}_f32 (sc_cg, sc_halo, the <5>-rows condition, sc_strips) ->
    (forward kernel, weight-gradient kernel, strips, rows per strip | bricks per block, rows | bricks of the last)."""
    Cin, Cout, (KD, KH, KW), N = r["Cin"], r["Cout"], r["K"], r["N"]
    CO = 2 if Cout <= 2 else 4
    cg = Cin in (16, 32, 64)
    fwd = f"cg<{CO},{Cin // 4}>" if cg else f"plain<{CO}>"
    npairs = _T(r) * (Cin // 4)
    hv = (HB_D + KD - 1) * (HB_H + KH - 1) * (HB_W + KW - 1)
    if 128 < npairs <= 512 and (hv * Cin + HB_D * HB_H * HB_W * 4) * 4 <= 64 * 1024:
        rows_floats = (HB_D + KD - 1) * (HB_H + KH - 1) * ((HB_W + 4) * Cin + 16) + HB_D * HB_H * HB_W * 2
        rows5 = (CO == 2 and (KD, KH, KW) == (5, 5, 5) and Cin == 16 and rows_floats * 4 <= 64 * 1024 and
                 (HB_D + KD - 1) * (HB_H + KH - 1) * (HB_W + 4) * (Cin // 4) <= 14 * 256)
        bricks = N * _cdiv(r["out"][0], HB_D) * _cdiv(r["out"][1], HB_H) * _cdiv(r["out"][2], HB_W)
        per = _cdiv(bricks, min(bricks, 2048))
        blocks = _cdiv(bricks, per)
        return fwd, "rows<5>" if rows5 else f"halo<{CO}>", blocks, per, bricks - (blocks - 1) * per
    nrows = N * r["out"][0] * r["out"][1]
    strips = max(min(_cdiv(4096, KD * KH * (1 if cg else Cin // 4)), nrows), 1)
    rpb = _cdiv(nrows, strips)
    strips = _cdiv(nrows, rpb)
    return fwd, fwd, strips, rpb, nrows - (strips - 1) * rpb


def out_workspace_bytes(r):
    return (out_geometry(r)[2] * r["Cout"] * r["Cin"] * _T(r) + 4096) * 4


def pairs16(r):
    """small_cout_dgrad_kernel<2> reads dY two voxels per 16-byte load."""
    return r["Cout"] == 2 and r["out"][2] % 2 == 0 and (r["pad"][2] - (r["K"][2] - 1)) % 2 == 0


S122 = (1, 2, 2)

# ----------------------------------------------------------------------------- vector forward (small_cin_fwd_kernel)
# regime: (vfwd_geometry without statistics, vfwd_geometry with statistics)
VFWD = [
    row("1->16 3x3x3", 1, 16, (3, 3, 3), 2, (5, 17, 19), bias_free_too=True,        # one wave group, 6 full tiles + 79
        regime=((1, 256, 7, 79, 7, 0, False), (1, 256, 7, 79, 7, 0, False))),
    row("2->16 1x7x7 s122", 2, 16, (1, 7, 7), 1, (3, 21, 30), S122,
        regime=((1, 256, 2, 239, 2, 0, False), (1, 256, 2, 239, 2, 0, False))),
    row("1->32 3x3x9", 1, 32, (3, 3, 9), 2, (4, 10, 40), pad=(1, 1, 4),            # KW 9, two wave groups
        regime=((2, 128, 13, 64, 13, 0, False), (2, 128, 13, 64, 13, 0, False))),
    row("1->64 3x3x3 sw3", 1, 64, (3, 3, 3), 3, (4, 30, 300), (1, 1, 3),            # with statistics 18 blocks walk 2 tiles
        regime=((4, 64, 188, 32, 188, 0, False), (4, 64, 188, 32, 170, 18, False))),
    row("1->16 1x3x3 large", 1, 16, (1, 3, 3), 2, (9, 256, 260),                    # 2340 tiles > 4096 / 2 (512 / 2 with statistics)
        regime=((1, 256, 2340, 256, 2048, 292, False), (1, 256, 2340, 256, 256, 2084, False)),
        stats_modes=(0, 2)),
    row("2->64 5x7x7", 2, 64, (5, 7, 7), 1, (3, 6, 20),                             # 125 440 B of weights in LDS
        regime=((4, 64, 6, 40, 6, 0, True), (4, 64, 6, 40, 6, 0, True))),
]

# ----------------------------------------------------------------------------- vector weight gradient
# via: "ops" = ops.conv_wgrad routes there (Cout 16), "hb" = hb.small_cin_wgrad (Cout 32 / 64 would take im2col + GEMM)
VWG = [
    row("1->16 3x3x3 straddle", 1, 16, (3, 3, 3), 3, (2, 5, 5), via="ops",          # 150 voxels: blocks of 64, samples of 50
        regime=("<8>", 7, 4, 3, 64, 22, 2)),
    row("2->16 1x3x3 idle wave", 2, 16, (1, 3, 3), 1, (1, 6, 7), via="ops",         # T 9, tpw 3: wave 3 has no tap
        regime=("<8>", 3, 3, 1, 64, 42, 0)),
    row("2->16 1x7x7 s122", 2, 16, (1, 7, 7), 1, (3, 21, 30), S122, via="ops",
        regime=("<40>", 13, 4, 8, 64, 47, 0)),
    row("1->16 3x7x7", 1, 16, (3, 7, 7), 1, (3, 9, 12), via="ops",
        regime=("<40>", 37, 4, 6, 64, 4, 0)),
    row("1->32 3x3x9", 1, 32, (3, 3, 9), 2, (4, 10, 40), pad=(1, 1, 4), via="hb",   # lanes 32..63 masked
        regime=("<40>", 21, 4, 50, 64, 64, 0)),
    row("1->64 3x3x3 sw3", 1, 64, (3, 3, 3), 2, (4, 10, 40), (1, 1, 3), via="hb",
        regime=("<8>", 7, 4, 18, 64, 32, 1)),
    row("1->16 3x3x3 70000 voxels", 1, 16, (3, 3, 3), 2, (4, 70, 125), via="ops",    # ceil(total / 1024) voxels a block
        regime=("<8>", 7, 4, 1015, 69, 34, 1)),
]

# ----------------------------------------------------------------------------- im2col
# regime: (Kpad, float4 items, grid-stride loop taken: items > 4096 * 256)
IM2COL = [
    row("2 5x7x7", 2, 32, (5, 7, 7), 1, (3, 40, 70), regime=(512, 1075200, True)),
    row("1 3x3x3 s222", 1, 32, (3, 3, 3), 2, (5, 9, 21), (2, 2, 2), regime=(32, 2640, False)),
    row("3 1x3x3", 3, 32, (1, 3, 3), 2, (3, 9, 21), regime=(28, 7938, False)),
]
# im2col + the matrix-core 1x1x1 weight gradient, as ops.conv_wgrad routes these (no thin-input kernel takes them)
IM2COL_GEMM = [
    row("1->32 5x7x7", 1, 32, (5, 7, 7), 2, (3, 9, 37)),
    row("1->32 3x3x8", 1, 32, (3, 3, 8), 2, (3, 9, 37), pad=(1, 1, 4)),
    row("1->32 3x3x3 sw2", 1, 32, (3, 3, 3), 2, (3, 9, 37), (1, 1, 2)),
]

# ----------------------------------------------------------------------------- matrix-core forward (thin_cin_fwd_kernel)
_TAP = dict(N=2, inp=(3, 9, 37))
MFWD = [
    row("1->64 3x3x3 runs", 1, 64, (3, 3, 3), 16, (3, 18, 150), regime=(32, 75, 38, 2, 1), stats_modes=(2,)),
    row("1->32 3x3x3 runs", 1, 32, (3, 3, 3), 16, (5, 18, 150), regime=(64, 75, 38, 2, 1), stats_modes=(2,)),
    row("2->32 1x1x1", 2, 32, (1, 1, 1), **_TAP, regime=(64, 9, 9, 1, 1)),
    row("1->64 1x3x2", 1, 64, (1, 3, 2), **_TAP, regime=(32, 18, 18, 1, 1)),
    row("2->64 3x3x5", 2, 64, (3, 3, 5), **_TAP, regime=(32, 18, 18, 1, 1), stats_modes=(0, 1, 2)),
    row("1->32 1x3x8", 1, 32, (1, 3, 8), **_TAP, pad=(0, 1, 4), regime=(64, 9, 9, 1, 1)),
    row("2->32 1x7x7", 2, 32, (1, 7, 7), **_TAP, regime=(64, 9, 9, 1, 1)),
    row("1->32 3x3x3 sh2", 1, 32, (3, 3, 3), **_TAP, stride=(1, 2, 1), regime=(64, 6, 6, 1, 1), stats_modes=(0, 1, 2),
        acts=True),
    row("2->64 3x3x3 sw2", 2, 64, (3, 3, 3), **_TAP, stride=(1, 1, 2), regime=(32, 9, 9, 1, 1)),
    row("1->64 3x3x3 s222", 1, 64, (3, 3, 3), **_TAP, stride=(2, 2, 2), regime=(32, 4, 4, 1, 1)),
]

# ----------------------------------------------------------------------------- matrix-core weight gradient
_TW = dict(N=1, inp=(4, 9, 70))
MWG = [
    row("2->64 3x3x3 runs", 2, 64, (3, 3, 3), 8, (7, 18, 70), regime=(2, 70, 24, 3, 1)),
    row("2->32 3x7x7 s122 runs", 2, 32, (3, 7, 7), 4, (5, 40, 270), S122, regime=(10, 75, 38, 2, 1)),
    row("1->32 1x1x1", 1, 32, (1, 1, 1), **_TW, regime=(1, 24, 24, 1, 1)),
    row("2->64 2x2x2", 2, 64, (2, 2, 2), **_TW, regime=(1, 12, 12, 1, 1)),
    row("1->64 1x3x5", 1, 64, (1, 3, 5), **_TW, regime=(1, 24, 24, 1, 1)),
    row("2->32 1x5x5", 2, 32, (1, 5, 5), **_TW, regime=(2, 24, 24, 1, 1)),
    row("1->32 1x3x9", 1, 32, (1, 3, 9), **_TW, regime=(2, 24, 24, 1, 1)),        # KW 9: the forward is the vector kernel
    row("1->64 6x5x5", 1, 64, (6, 5, 5), **_TW, regime=(10, 18, 18, 1, 1)),
]

# ----------------------------------------------------------------------------- thin output (small_cout_*)
_S = dict(N=1, inp=(3, 9, 21))
OUT = (
    [row(f"32->2 1x1x1 W{W}", 32, 2, (1, 1, 1), 2, (2, 3, W), regime=("cg<2,8>", "cg<2,8>", 12, 1, 1))
     for W in (5, 8, 13, 16)] +
    [row("16->1 3x3x3", 16, 1, (3, 3, 3), **_S, regime=("cg<2,4>", "cg<2,4>", 27, 1, 1)),
     row("16->2 3x3x3", 16, 2, (3, 3, 3), **_S, regime=("cg<2,4>", "cg<2,4>", 27, 1, 1), acts=True),
     row("16->3 3x3x3", 16, 3, (3, 3, 3), **_S, regime=("cg<4,4>", "cg<4,4>", 27, 1, 1), bias_free_too=True),
     row("16->4 3x3x3", 16, 4, (3, 3, 3), **_S, regime=("cg<4,4>", "cg<4,4>", 27, 1, 1)),
     row("32->4 1x1x1", 32, 4, (1, 1, 1), 2, (3, 9, 21), regime=("cg<4,8>", "cg<4,8>", 54, 1, 1)),
     row("16->4 1x1x1", 16, 4, (1, 1, 1), 2, (3, 9, 21), regime=("cg<4,4>", "cg<4,4>", 54, 1, 1)),
     row("64->2 1x3x3", 64, 2, (1, 3, 3), 2, (3, 9, 21), regime=("cg<2,16>", "halo<2>", 24, 1, 1)),
     row("64->2 1x1x1", 64, 2, (1, 1, 1), 2, (3, 9, 21), regime=("cg<2,16>", "cg<2,16>", 54, 1, 1)),
     row("48->4 1x1x1 strips of two rows", 48, 4, (1, 1, 1), 3, (3, 45, 21), regime=("plain<4>", "plain<4>", 203, 2, 1)),
     row("80->2 1x3x3", 80, 2, (1, 3, 3), 2, (3, 9, 21), regime=("plain<2>", "plain<2>", 54, 1, 1)),
     row("32->3 3x3x3", 32, 3, (3, 3, 3), **_S, regime=("cg<4,8>", "halo<4>", 12, 1, 1)),     # bricks 2 x 2 x 3, all partial
     row("64->4 3x3x3", 64, 4, (3, 3, 3), **_S, regime=("cg<4,16>", "cg<4,16>", 27, 1, 1)),
     row("48->2 3x3x3", 48, 2, (3, 3, 3), **_S, regime=("plain<2>", "plain<2>", 27, 1, 1)),
     row("32->2 3x3x3", 32, 2, (3, 3, 3), **_S, regime=("cg<2,8>", "halo<2>", 12, 1, 1)),
     row("16->4 5x5x5", 16, 4, (5, 5, 5), **_S, regime=("cg<4,4>", "halo<4>", 12, 1, 1)),
     row("16->2 5x5x5", 16, 2, (5, 5, 5), **_S, regime=("cg<2,4>", "rows<5>", 12, 1, 1)),
     row("16->2 5x5x5 2205 bricks", 16, 2, (5, 5, 5), 1, (10, 168, 168), regime=("cg<2,4>", "rows<5>", 1103, 2, 1)),
     row("32->2 5x5x5", 32, 2, (5, 5, 5), **_S, regime=("cg<2,8>", "cg<2,8>", 27, 1, 1)),      # 1000 pairs: past the brick
     row("16->2 3x3x3 pad 0", 16, 2, (3, 3, 3), 2, (3, 9, 21), pad=(0, 0, 0), regime=("cg<2,4>", "cg<2,4>", 14, 1, 1)),
     row("16->2 3x3x3 pad 2", 16, 2, (3, 3, 3), 2, (3, 9, 21), pad=(2, 2, 2), regime=("cg<2,4>", "cg<2,4>", 110, 1, 1))] +
    # the 16-byte dY loads of the input gradient (even Wo, even pw - (KW - 1)) next to the scalar path (W 11)
    [row(f"16->2 1x3x{KW} pw{pw} W{W}", 16, 2, (1, 3, KW), 2, (2, 5, W), pad=(0, 1, pw),
         regime=("cg<2,4>", "cg<2,4>", 20, 1, 1), pairs16=W != 11)
     for KW, pw in ((5, 2), (1, 0), (3, 0), (3, 2)) for W in (10, 22, 11)]
)

FAMILIES = dict(VFWD=VFWD, VWG=VWG, IM2COL=IM2COL, IM2COL_GEMM=IM2COL_GEMM, MFWD=MFWD, MWG=MWG, OUT=OUT)


def ids(rows):
    return [r["name"].replace(" ", "_") for r in rows]
