"""Descriptor table of the fp32 Winograd forward / input-gradient family (tests/test_wino_plan_cpu.py,
tools/gen_golden_wino_plan.py): what rehr_gather_gemm_wino_bytes, rehr_gather_gemm_wino_route and the two fp32 launch
entry points do with a rehr_gather_gemm_desc.

Every row is one descriptor with dummy aligned pointers that nothing on the host dereferences.  tests/golden/wino_plan.json
holds what the library returned BEFORE the route query existed; the route of a row is therefore written here by hand,
next to the predicate of that library (wino_flat8_conv.hip / wino_conv.hip / wino22_conv.hip as of the recording) that
decided it.  Routes: the REHR_GG_ROUTE_* names without the prefix."""
import ctypes as C

from rehrseg_amd import lib as L

X1, X2, WP, Y, WS, STATS, BIAS = 0x10000, 0x20000, 0x30000, 0x40000, 0x100000, 0x50000, 0x60000
EINVAL, ENOSUP, EHIP, OK = -1, -2, -3, 0
ROUTES = {"none": 0, "flat8": 1, "w32p": 2, "big8": 3, "small": 4, "flat22": 5, "region22": 6}
# debug_flags settings every row is queried under
FLAGS = {"0": 0, "NO_FLAT8": L.DBG_GG_NO_FLAT8, "FLAT8_HALF": L.DBG_GG_FLAT8_HALF, "FLAT8_FULL": L.DBG_GG_FLAT8_FULL,
         "W32P_TWO_PER_CU": L.DBG_GG_W32P_TWO_PER_CU, "W32P_ONE_PER_CU": L.DBG_GG_W32P_ONE_PER_CU}
LAUNCH_FLAGS = ("0", "NO_FLAT8")     # the settings the launch codes are recorded under


def taps(count, off0=0, offs=1, k0=0, ks=1):
    return L.AxisTaps(count=count, off0=off0, offs=offs, k0=k0, ks=ks)


def desc(kind="c3", N=1, Cin=64, Cout=64, plane=(4, 16, 16), kd=3, Npad=None, **over):
    """kind "c3": unit-stride "same" convolution, kd x 3 x 3 taps (forward or input gradient of a 3x3x3 / 1x3x3 layer).
    kind "t2": one output phase of a stride-2 transposed convolution with a (kd, 4, 4) kernel -- 2 x 2 plane taps on the
               input lattice, output stride 2.
    kind "s4": the input gradient of that layer -- 4 x 4 plane taps at source stride 2.
    `plane` is the lattice (Ld, Lh, Lw); Npad defaults to Cout rounded up to 32; `over` sets raw fields last."""
    Ld, Lh, Lw = plane
    d = L.GatherGemmDesc()
    d.x1, d.wp, d.y = X1, WP, Y
    d.c1 = d.Cin = d.ldx1 = Cin
    d.Cout = d.ldy = Cout
    d.Npad = Npad if Npad is not None else (Cout + 31) // 32 * 32
    d.N = N
    d.Ld, d.Lh, d.Lw = plane
    d.sd = d.sh = d.sw = d.osd = d.osh = d.osw = 1
    d.Di, d.Dy, d.bd, d.td = Ld, Ld, -(kd // 2), taps(kd)
    if kind == "c3":
        d.Hi, d.Wi, d.Hy, d.Wy = Lh, Lw, Lh, Lw
        d.bh = d.bw = -1
        d.th = d.tw = taps(3)
        d.KH = d.KW = 3
    elif kind == "t2":
        d.Hi, d.Wi, d.Hy, d.Wy = Lh, Lw, 2 * Lh, 2 * Lw
        d.osh = d.osw = 2
        d.th = d.tw = taps(2, off0=0, offs=-1, k0=1, ks=2)     # output parity 0: source offsets 0, -1
        d.KH = d.KW = 4
    elif kind == "s4":
        d.Hi, d.Wi, d.Hy, d.Wy = 2 * Lh, 2 * Lw, Lh, Lw
        d.sh = d.sw = 2
        d.bh = d.bw = -1
        d.th = d.tw = taps(4)
        d.KH = d.KW = 4
    else:
        raise ValueError(kind)
    for k, v in over.items():
        setattr(d, k, v)
    return d


def c3(N, Cin, Cout, plane, **kw):
    return dict(kind="c3", N=N, Cin=Cin, Cout=Cout, plane=plane, **kw)


def t2(N, Cin, Cout, plane, **kw):
    return dict(kind="t2", N=N, Cin=Cin, Cout=Cout, plane=plane, **kw)


def s4(N, Cin, Cout, plane, **kw):
    return dict(kind="s4", N=N, Cin=Cin, Cout=Cout, plane=plane, **kw)


# (name, desc() arguments, route under debug_flags 0, the recorded library's predicate that decides it)
ROWS = [
    # ---- flattened-tile F(2x2,3x3): units = ceil(N Ld tps / 64) x Npad / 64 must reach 128
    ("flat8 12x12 256->256 N32", c3(32, 256, 256, (4, 12, 12)), "flat8", "plan_flat8: 288 units; f8_pick 1.5 x 1.08 < 2 rounds: 32 tiles"),
    ("flat8 12x12 256->256 N16", c3(16, 256, 256, (4, 12, 12)), "flat8", "plan_flat8: 144 units; f8_pick 1.0 x 1.08 > 1 round: 64 tiles"),
    ("flat8 24x24 128->128", c3(4, 128, 128, (8, 24, 24)), "flat8", "plan_flat8: 144 units; f8_pick: 64 tiles"),
    ("flat8 24x24 512->512 N8", c3(8, 512, 512, (4, 24, 24)), "flat8", "plan_flat8: 576 units; f8_pick 2.5 x 1.08 < 3 asks for 32 tiles, whose plan does not hold: 64"),
    ("flat8 12x12 fill 128 units", c3(113, 64, 64, (2, 12, 12)), "flat8", "plan_flat8: 8136 tiles = 128 units, the threshold"),
    ("flat8 12x12 fill 127 units", c3(25, 64, 64, (9, 12, 12)), "none", "plan_flat8 fill threshold (8100 tiles = 127 units); small tile pads 1.78x"),
    ("flat8 7x9 odd plane", c3(64, 128, 128, (8, 7, 9)), "flat8", "plan_flat8: 8 x 10 padded / 63 = 1.27"),
    ("flat8 7x7 pads 1.306", c3(64, 128, 128, (8, 7, 7)), "none", "plan_flat8 padding 640 > 637; wino_workspace_bytes Lh < 8"),
    ("flat8 6x6, eight slices per block", c3(64, 256, 256, (8, 6, 6)), "flat8", "plan_flat8: (64 - 2) / 9 + 2 = 8 = F8_MAXSLOT (the largest reachable: Lh, Lw >= 6)"),
    ("flat8 5x24", c3(64, 128, 128, (8, 5, 24)), "none", "plan_flat8 Lh < 6; wino_workspace_bytes Lh < 8"),
    ("flat8 24x66 -> small tile", c3(8, 128, 128, (8, 24, 66)), "small", "plan_flat8 Lw > 64; big_ok 32 x 80 / 1584 = 1.62; small 24 x 80 / 1584 = 1.21"),
    ("plane 12x66", c3(8, 128, 128, (8, 12, 66)), "none", "plan_flat8 Lw > 64; small tile 16 x 80 / 792 = 1.62 > 1.34"),
    ("flat8 one depth tap", c3(32, 256, 256, (4, 12, 12), kd=1), "flat8", "plan_flat8"),
    ("flat8 four depth taps 12x12", c3(32, 256, 256, (4, 12, 12), kd=4), "none", "plan_flat8 td.count > 3; small tile pads 1.78x"),
    ("flat8 virtual concat", c3(32, 256, 256, (4, 12, 12), c1=128, x2=X2, ldx2=128, ldx1=128), "flat8", "plan_flat8"),
    ("flat8 batch over one buffer -> small tile", c3(114, 256, 256, (64, 24, 24)), "small", "plan_flat8 gg_src_fits (whole batch, 4.3e9 B); small tile 24 x 32 / 576 = 1.333, one buffer per sample"),
    ("flat8 Npad 32 at 24x24 -> small tile", c3(8, 128, 32, (8, 24, 24)), "small", "plan_flat8 Npad % 64; w32_ok 1.78; small 1.333"),
    # ---- F(2x2,3x3) region kernels
    ("w32p 32->32 16x16", c3(2, 32, 32, (8, 16, 16)), "w32p", "w32_ok; w32_groups 2: G = 1"),
    ("w32p 64->96 16x16", c3(2, 64, 96, (8, 16, 16)), "w32p", "w32_ok (Npad 96); w32_groups 2: G = 1"),
    ("w32p 64->32 32x32", c3(2, 64, 32, (8, 32, 32)), "w32p", "w32_ok; w32_groups 4, Cin x taps = 192 > 96: G = 2"),
    ("w32p 32->32 32x32", c3(2, 32, 32, (8, 32, 32)), "w32p", "w32_ok; w32_groups 4 but Cin x taps = 96: two per CU, G = 1"),
    ("w32p 64->32 48x32", c3(2, 64, 32, (8, 48, 32)), "w32p", "w32_ok; 32-row regions pad 64 / 48 = 1.33 > 1.3: groups 2, G = 1"),
    ("big8 64->64 16x16", c3(2, 64, 64, (8, 16, 16)), "big8", "big_ok"),
    ("big8 128->128 32x32", c3(1, 128, 128, (16, 32, 32)), "big8", "big_ok"),
    ("big8 29x29", c3(1, 64, 64, (8, 29, 29)), "big8", "big_ok 1024 / 841 = 1.22 (flat8: too few tiles to fill)"),
    ("big8 four depth taps", c3(2, 64, 64, (8, 16, 16), kd=4), "big8", "big_ok (depth taps are K items)"),
    ("big8 256 depth taps", c3(1, 32, 64, (1, 16, 16), kd=256, Di=256, bd=-128), "big8", "big_ok; td.count = 256 is the limit"),
    ("257 depth taps", c3(1, 32, 64, (1, 16, 16), kd=257, Di=257, bd=-128), "none", "wino_workspace_bytes td.count > 256"),
    ("small 8x16 Npad 32", c3(2, 32, 32, (8, 8, 16)), "small", "w32_ok Lh < 16; small tile 1.0"),
    ("small 28x28 Npad 32", c3(2, 32, 32, (8, 28, 28)), "small", "w32_ok 1024 / 784 = 1.306 > 1.3; small 32 x 32 / 784 = 1.306 <= 1.34"),
    ("small 8x12 Npad 32", c3(2, 32, 32, (8, 8, 12)), "small", "small tile 16 / 12 = 1.333"),
    ("small 23x24 Npad 32", c3(2, 32, 32, (8, 23, 24)), "none", "wino_workspace_bytes 24 x 32 / 552 = 1.39 > 1.34"),
    ("plane 7x16", c3(2, 32, 32, (8, 7, 16)), "none", "wino_workspace_bytes Lh < 8"),
    ("scratch 2^32", c3(1, 2048, 2048, (1, 16, 16), kd=16, Di=16, bd=-8), "none", "wino_workspace_bytes need >= 2^32 - 64"),
    ("source sample over one buffer", c3(1, 64, 64, (64, 512, 512)), "none", "wino_workspace_bytes gg_src_fits (2^32 B)"),
    ("N 65536", c3(65536, 64, 64, (1, 16, 16), kd=1), "none", "gg_validate N > 65535 (the planners' own N bound is behind it)"),
    ("stride 2 along h", c3(2, 64, 64, (8, 16, 16), sh=2, Hi=32), "none", "sh != 1 (every planner)"),
    ("output stride 2", c3(2, 64, 64, (8, 16, 16), osh=2, Hy=32), "none", "osh != 1"),
    ("output offset 1", c3(2, 64, 64, (8, 16, 16), obw=1, Wy=17), "none", "obw != 0"),
    ("lattice is not the whole output", c3(2, 64, 64, (8, 16, 16), Dy=9), "none", "Ld != Dy"),
    ("taps two apart", c3(2, 64, 64, (8, 16, 16), th=taps(3, off0=-1, offs=2), bh=-1), "none", "three_taps"),
    ("taps mirrored", c3(2, 64, 64, (8, 16, 16), th=taps(3, off0=2, offs=-1, k0=2, ks=-1), bh=-1), "big8", "three_taps: +1, 0, -1"),
    # ---- F(2x2,2x2): units x parts must reach 256 for the flattened tiles; 16 x 16 regions pad <= 1.3x, or <= 1.78x with
    # at least 256 blocks
    ("flat22 2-tap 12x12 512->256", t2(32, 512, 256, (4, 12, 12)), "flat22", "plan22_flat: 288 units"),
    ("flat22 2-tap 24x24", t2(8, 256, 128, (8, 24, 24)), "flat22", "plan22_flat: 288 units"),
    ("flat22 4-tap stride 2 12x12", s4(32, 128, 256, (4, 12, 12)), "flat22", "plan22_flat: four source phases"),
    ("flat22 one depth tap", t2(32, 512, 256, (4, 12, 12), kd=1), "flat22", "plan22_flat"),
    ("region22 12x12 512->128: 144 units", t2(32, 512, 128, (4, 12, 12)), "region22", "plan22_flat fill threshold (144 < 256); plan22 1.78x with 256 blocks"),
    ("12x12 512->128 N16", t2(16, 512, 128, (4, 12, 12)), "none", "plan22_flat fill; plan22 1.78x with 128 blocks"),
    ("region22 2-tap 16x16", t2(2, 128, 64, (4, 16, 16)), "region22", "plan22_flat whole regions; plan22"),
    ("region22 4-tap stride 2 32x32", s4(1, 64, 64, (8, 32, 32)), "region22", "plan22"),
    ("region22 2-tap 28x28", t2(1, 128, 64, (4, 28, 28)), "none", "plan22_flat fill; plan22 1.306x with 16 blocks"),
    ("region22 2-tap 29x29", t2(1, 128, 64, (4, 29, 29)), "region22", "plan22 1.22x"),
    ("flat22 2-tap 17x12", t2(64, 512, 128, (4, 17, 12)), "flat22", "plan22_flat: 432 units (NO_FLAT8: plan22 512 / 204 = 2.5 > 1.78, nothing)"),
    ("2-tap 23x24 pads 1.855", t2(1, 128, 64, (128, 23, 24)), "none", "plan22_flat Ld > 127; plan22 1024 / 552 = 1.855 > 1.78 (512 blocks: a full grid)"),
    ("2-tap 10x10", t2(8, 128, 64, (4, 10, 10)), "none", "plan22_flat fill; plan22 Lh < 12"),
    ("2-tap Npad 32", t2(2, 128, 32, (4, 16, 16)), "none", "Npad % 64 (both F(2x2,2x2) planners)"),
    ("2-tap four depth taps", t2(2, 128, 64, (4, 16, 16), kd=4), "none", "td.count > 3 (both)"),
    ("2-tap against 4-tap", t2(2, 128, 64, (4, 16, 16), tw=taps(4), sw=2, bw=-1, Wi=32, osw=1, Wy=16), "none", "ah.nph != aw.nph"),
    ("4-tap with output stride", s4(1, 64, 64, (8, 32, 32), osh=2, Hy=64), "none", "nph == 2 needs a dense output"),
    ("2-tap taps two apart", t2(2, 128, 64, (4, 16, 16), th=taps(2, offs=2)), "none", "plan_axis offs"),
    ("2-tap depth stride 2", t2(2, 128, 64, (4, 16, 16), sd=2, Di=8), "none", "sd != 1"),
    ("region22 Ld 128 (flat22 declines)", t2(4, 128, 128, (128, 12, 12)), "region22", "plan22_flat Ld > 127; plan22 1.78x with 1024 blocks"),
]

# Rows whose 32-tile plan does not hold: a 256-thread block stages at most 8 x 256 16-byte pieces, and the rows that 32
# tiles of these planes read are more (24 x 24: 12 rows x 26 slots x 8 = 2496).  The recorded library then takes 64 tiles,
# whatever f8_pick or REHR_DBG_GG_FLAT8_HALF asked for, without saying so: kept as it was.
HALF_DOES_NOT_FIT = {"flat8 24x24 128->128", "flat8 24x24 512->512 N8", "flat8 7x9 odd plane",
                     "flat8 6x6, eight slices per block"}

# w32p rows on 32-row regions (w32_groups = 4): REHR_DBG_GG_W32P_ONE_PER_CU can give them the 512-thread block
W32P_FOUR_GROUPS = {"w32p 64->32 32x32", "w32p 32->32 32x32"}

# ---- multi-part calls: (name, list of desc() arguments, which all-or-none entry takes them: "split" / "flat-multi" / None)
def _split(parts, each=16, vary=None, N=2, plane=(1, 16, 16), **kw):
    """Depth-tap ranges of one 64 -> 64 layer on a 1 x 16 x 16 lattice (feature_fuse's input gradient in small)."""
    out = []
    for i in range(parts):
        a = c3(N, 64, 64, plane, kd=each, Di=each * parts, bd=-(each * parts // 2),
               td=taps(each, off0=each * i, k0=each * i), y=Y + 0x100000 * i, **kw)
        if vary and i == vary[0]:
            a.update(vary[1])
        out.append(a)
    return out


def _phases(parts, vary=None, N=16, **kw):
    """Output phases of a (3, 4, 4) stride-(1, 2, 2) transposed convolution on 12 x 12 planes, 512 -> 128.  At N = 16 a
    phase has NO route of its own (72 flattened-tile units < 256; 128 region blocks < 256 at 1.78x padding): only the
    all-or-none entry, which counts units x parts, takes it."""
    out = []
    for i in range(parts):
        ph, pw = i // 2, i % 2
        a = t2(N, 512, 128, (4, 12, 12), obh=ph, obw=pw, th=taps(2, off0=ph, offs=-1, k0=1 - ph, ks=2),
               tw=taps(2, off0=pw, offs=-1, k0=1 - pw, ks=2), **kw)
        if vary and i == vary[0]:
            a.update(vary[1])
        out.append(a)
    return out


# What the third column can be checked against where nothing launches: with REHR_GG_WS_ONLY and every part's scratch sized by
# the FORMULA (not by the query), the call returns EHIP (a weight transform was launched) when a Winograd kernel takes the
# parts, and OK (nothing to prepare) when none does.  The many-tap split parts are never launched one by one (td.count > 3
# in a multi call), and the N = 16 phases have no route of their own, so for them EHIP means the all-or-none entry.
MULTI = [
    ("split 2 parts", _split(2), "split"),
    ("split 3 parts", _split(3), "split"),
    ("split 8 parts", _split(8), "split"),
    ("split 4 parts of one depth tap", _split(4, each=1), "split"),
    ("split, bias on part 1", _split(3, vary=(1, dict(bias=BIAS))), None),
    ("split, statistics on part 2", _split(3, vary=(2, dict(stats=STATS, stats_mode=1))), None),
    ("split, activation on part 0", _split(3, vary=(0, dict(act=1))), None),
    ("split, part 2 with another bh", _split(3, vary=(2, dict(bh=0))), None),
    ("split, part 1 with another ldy", _split(3, vary=(1, dict(ldy=128))), None),
    ("split, part 1 with another KW", _split(3, vary=(1, dict(KW=5))), None),
    ("split, N x parts > 65535", _split(2, N=32768), None),
    ("split on 12x12 planes", _split(3, plane=(1, 12, 12)), None),
    ("flat-multi 4 phases", _phases(4), "flat-multi"),
    ("flat-multi 3 phases, one depth tap", _phases(3, N=22, kd=1), "flat-multi"),
    ("flat-multi 2 phases N30", _phases(2, N=30), "flat-multi"),
    ("flat-multi 2 phases N16: 144 units", _phases(2), None),
    ("flat-multi, phase 3 into another y", _phases(4, vary=(3, dict(y=Y + 0x100000))), None),
    ("flat-multi, phase 1 with another bias", _phases(4, vary=(1, dict(bias=BIAS))), None),
    ("flat-multi, phase 1 with another activation", _phases(4, vary=(1, dict(act=1))), None),
    ("flat-multi, phase 2 with statistics", _phases(4, vary=(2, dict(stats=STATS, stats_mode=2))), None),
    ("flat-multi, phase 2 with one depth tap", _phases(4, vary=(2, dict(td=taps(1), bd=0))), None),
    ("flat-multi, phase 3 with another depth origin", _phases(4, vary=(3, dict(td=taps(3, off0=1), bd=-2))), None),
    ("flat-multi, phase 1 from another x2", _phases(4, c1=256, ldx1=256, x2=X2, ldx2=256, vary=(1, dict(x2=X2 + 0x1000))), None),
    ("flat-multi, phase 2 with another ldy", _phases(4, vary=(2, dict(ldy=256))), None),
    ("flat-multi of 4-tap parts", [s4(16, 128, 128, (4, 12, 12))] * 4, None),
]
# The parts of this row have a route of their own (one depth tap each goes to the big tile one by one when the split entry
# declines), so its WS_ONLY code is EHIP either way: the device test test_winograd_depth_tap_split_half_filled_grid
# counts the launches instead.
MULTI_BLIND = {"split 4 parts of one depth tap"}


def bind(path=None):
    """The three recorded entry points of the library at `path` (any ABI version), or of the in-tree one."""
    lib = C.CDLL(path) if path else L.load()
    P = C.POINTER(L.GatherGemmDesc)
    lib.rehr_gather_gemm_wino_bytes.restype, lib.rehr_gather_gemm_wino_bytes.argtypes = C.c_int64, [P]
    lib.rehr_gather_gemm_f32.restype, lib.rehr_gather_gemm_f32.argtypes = C.c_int, [P, C.c_void_p]
    lib.rehr_gather_gemm_multi_f32.restype, lib.rehr_gather_gemm_multi_f32.argtypes = C.c_int, [P, C.c_int32, C.c_void_p]
    return lib


def _make(args, flags):
    d = desc(**args)
    d.debug_flags = flags
    return d


def bytes_by_flag(lib, args):
    return {f: int(lib.rehr_gather_gemm_wino_bytes(C.byref(_make(args, v)))) for f, v in FLAGS.items()}


def _codes(lib, ds):
    """[plain, REHR_GG_WS_ONLY] return codes of the multi entry (and of the single entry, which must agree, for one part)."""
    out = []
    for fl in (0, L.GG_WS_ONLY):
        arr = (L.GatherGemmDesc * len(ds))(*ds)
        for i in range(len(ds)):
            arr[i].flags = fl
        rc = int(lib.rehr_gather_gemm_multi_f32(arr, len(ds), None))
        if len(ds) == 1:
            assert int(lib.rehr_gather_gemm_f32(C.byref(arr[0]), None)) == rc
        out.append(rc)
    return out


# scratch situations: (name, address, size as a function of the queried size)
SITUATIONS = (("queried", WS, lambda n: n), ("one byte short", WS, lambda n: n - 1), ("null", None, lambda n: n),
              ("misaligned by 4", WS + 4, lambda n: n))


def launch_codes(lib, args):
    """{flag setting: {situation: [plain, WS_ONLY]}}.  A row without a route gets a scratch all the same (4096 bytes)."""
    rec = {}
    for f in LAUNCH_FLAGS:
        need = int(lib.rehr_gather_gemm_wino_bytes(C.byref(_make(args, FLAGS[f])))) or 4096
        rec[f] = {}
        for what, addr, size in SITUATIONS:
            d = _make(args, FLAGS[f])
            d.wino_ws, d.wino_ws_bytes = addr, size(need)
            rec[f][what] = _codes(lib, [d])
    return rec


def formula_bytes(d):
    """Scratch of one descriptor by the formula: 16 transformed taps per depth tap for 3 x 3 taps, 9 per source phase for
    2-tap phases (one phase) and 4-tap stride-2 gathers (four)."""
    xforms = {3: 16, 2: 9, 4: 36}[d.th.count]
    return xforms * d.td.count * d.Npad * ((d.Cin + 31) // 32 * 32) * 4


def multi_codes(lib, parts):
    """{situation: [plain, WS_ONLY]} with every part's scratch sized by the formula; the situation applies to the LAST part."""
    rec = {}
    for what, addr, size in SITUATIONS:
        ds = []
        for i, a in enumerate(parts):
            d = _make(a, 0)
            need = formula_bytes(d)
            last = i == len(parts) - 1
            d.wino_ws = (addr if last else WS) and (addr if last else WS) + 0x10000000 * i
            d.wino_ws_bytes = size(need) if last else need
            ds.append(d)
        rec[what] = _codes(lib, ds)
    return rec
