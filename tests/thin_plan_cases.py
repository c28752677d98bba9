"""Descriptor table of the thin-convolution family (tests/test_thin_plan_cpu.py, tools/gen_golden_thin_plan.py): every
entry point that takes a rehr_direct_conv_desc.

Every row is one descriptor with dummy aligned pointers that nothing on the host dereferences.  The comment of a row
names what the library did with it when tests/golden/thin_plan.json was recorded, and why the row is there."""
import ctypes as C

from rehrseg_amd import lib as L

X, W_, Y, DW, DX, OUT, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x100000
BIG = 1 << 40          # workspace size offered where the query reports no size


def desc(Cin=1, Cout=32, N=1, inp=(4, 10, 40), K=(3, 3, 3), stride=(1, 1, 1), pad=None, out=None, **over):
    """Conv3d(Cin -> Cout, K, stride, pad) on an input of extents `inp`; pad defaults to (K - 1) // 2, the output
    extents to what follows from the input, the channel pitches to the channel counts.  `over` sets raw fields last."""
    pad = tuple((k - 1) // 2 for k in K) if pad is None else pad
    out = tuple((inp[a] + 2 * pad[a] - K[a]) // stride[a] + 1 for a in range(3)) if out is None else out
    d = L.DirectConvDesc()
    d.x, d.w, d.y = X, W_, Y
    d.ldx = d.Cin = Cin
    d.ldy = d.Cout = Cout
    d.N = N
    d.Di, d.Hi, d.Wi = inp
    d.Do, d.Ho, d.Wo = out
    d.KD, d.KH, d.KW = K
    d.sd, d.sh, d.sw = stride
    d.pd, d.ph, d.pw = pad
    for k, v in over.items():
        setattr(d, k, v)
    return d


def thin5(W=64, D=16, H=8, N=1, **kw):   # sr_head.2: Conv3d(16 -> 2, 5x5x5, pad 2)
    return dict(Cin=16, Cout=2, N=N, inp=(D, H, W), K=(5, 5, 5), **kw)


def out(Cout=2, Cin=16, k=3, **kw):      # thin-output layers
    return dict(Cin=Cin, Cout=Cout, inp=(4, 9, 21), K=(k, k, k), **kw)


S122 = (1, 2, 2)

# (name, desc() arguments)
ROWS = [
    # ---- thin input: the matrix-core forward and weight gradient (thin_cin_conv.hip)
    ("in 1->32 3x3x3", dict()),                                                 # matrix cores, all four entry points
    ("in 1->64 3x3x3", dict(Cout=64)),                                          # matrix cores
    ("in 2->32 1x3x3", dict(Cin=2, K=(1, 3, 3))),                               # matrix cores, one tap tile
    ("in 1->64 3x7x7 stride 1,2,2", dict(Cout=64, K=(3, 7, 7), stride=S122)),   # the FLAVR stem: ten tap tiles
    ("in 2->64 3x7x7 stride 1,2,2, N 3", dict(Cin=2, Cout=64, N=3, K=(3, 7, 7), stride=S122, inp=(4, 33, 70))),
    ("in 1->32 3x3x3 with statistics", dict(stats=0x70000, stats_mode=2)),      # matrix cores
    ("in 1->32 large", dict(N=2, inp=(64, 256, 256))),                          # matrix cores: blocks walk runs of tiles
    # ---- thin input: the vector kernels of direct_conv.hip
    ("in 1->16 3x3x3", dict(Cout=16)),                                          # VALU; the bf16 entry points decline
    ("in 2->16 1x7x7 stride 1,2,2", dict(Cin=2, Cout=16, K=(1, 7, 7), stride=S122)),  # VALU
    ("in 1->32 3x3x9", dict(K=(3, 3, 9))),                                      # KW = 9: VALU forward and gradient
    ("in 1->32 3x3x8", dict(K=(3, 3, 8), pad=(1, 1, 4))),                       # KW = 8: matrix-core forward, VALU gradient
    ("in 1->32 stride w 2", dict(stride=(1, 1, 2))),                            # matrix-core forward; gradient VALU (patch past the prefetch)
    ("in 1->32 stride w 3", dict(stride=(1, 1, 3))),                            # sw = 3: VALU
    ("in 1->16 large", dict(Cout=16, N=2, inp=(16, 64, 64))),                   # VALU gradient with 1024 blocks
    # ---- the layer mixed precision used to trip over, and its neighbours
    ("in 2->64 5x7x7", dict(Cin=2, Cout=64, K=(5, 7, 7))),                      # fwd VALU (weights 143 360 B + patch > 150 KB); ybf16 ENOSUP
    ("in 2->64 5x7x7 stride 1,2,2", dict(Cin=2, Cout=64, K=(5, 7, 7), stride=S122)),  # the same
    ("in 2->64 7x7x7", dict(Cin=2, Cout=64, K=(7, 7, 7))),                      # both forward routes and both gradients decline
    ("in 2->32 7x7x7", dict(Cin=2, Cout=32, K=(7, 7, 7))),                      # matrix-core forward; gradient ENOSUP (86 taps per wave)
    ("in 1->32 5x7x7", dict(K=(5, 7, 7))),                                      # matrix-core forward, VALU gradient (16 tap tiles)
    # ---- thin input: malformed
    ("in Cout 48", dict(Cout=48)),                                              # EINVAL; the bf16 entry points ENOSUP
    ("in Cin 3", dict(Cin=3)),                                                  # EINVAL / ENOSUP; the im2col takes it
    ("in y misaligned for fp32", dict(y=Y + 8)),                                # fp32 EINVAL; 8 bytes is aligned for bf16
    ("in y misaligned for bf16", dict(y=Y + 4)),                                # fp32 EINVAL, bf16 ENOSUP
    ("in 1->16 y misaligned", dict(Cout=16, y=Y + 8)),                          # EINVAL
    ("in 1->16 wrong output extent", dict(Cout=16, out=(4, 10, 41))),           # EINVAL, the im2col as well
    ("in 1->16 null x", dict(Cout=16, x=None)),                                 # EINVAL everywhere
    ("in 1->16 statistics without a buffer", dict(Cout=16, stats_mode=1)),      # forward EINVAL
    ("in 1->16 N 65536", dict(Cout=16, N=65536, inp=(1, 2, 2))),                # EINVAL (grid.y)
    ("in ldy 34", dict(ldy=34)),                                                # EINVAL / ENOSUP
    # ---- thin output (small_cout_*): channel groups, halo brick, plain
    ("out 16->1 1x1x1", out(1, 16, 1)),                                         # coalesced (CG 4), CO 2
    ("out 16->2 3x3x3", out(2, 16, 3)),                                         # coalesced; 108 pairs: no halo brick
    ("out 32->3 3x3x3", out(3, 32, 3)),                                         # CG 8, CO 4; 216 pairs: halo brick
    ("out 64->4 3x3x3", out(4, 64, 3)),                                         # CG 16; 432 pairs: halo brick
    ("out 48->2 3x3x3", out(2, 48, 3)),                                         # not a coalesced width; halo brick
    ("out 48->4 1x1x1", out(4, 48, 1)),                                         # plain kernels, CO 4
    ("out 32->2 5x5x5", out(2, 32, 5)),                                         # 1000 pairs: past the halo brick
    ("out 16->2 5x5x5 odd extents", out(2, 16, 5)),                             # halo brick, the <5> rows kernel; W = 21: not thin5
    ("out 16->4 5x5x5", out(4, 16, 5)),                                         # halo brick, CO 4 (not the rows kernel)
    ("out 32->2 1x3x3 large", dict(Cin=32, Cout=2, N=2, inp=(32, 128, 128), K=(1, 3, 3))),  # strips capped by 4096 blocks
    ("out 16->5", out(5, 16, 3)),                                               # EINVAL
    ("out 24->2", out(2, 24, 3)),                                               # EINVAL (Cin % 16)
    ("out 16->2 stride 2", out(2, 16, 3, stride=(1, 1, 2))),                    # EINVAL
    ("out 16->2 3x3x9", out(2, 16, 3) | dict(K=(3, 3, 9))),                     # EINVAL (KW > 7)
    ("out 16->2 ldx 18", out(2, 16, 3, ldx=18)),                                # EINVAL
    ("out 16->2 null w", out(2, 16, 3, w=None)),                                # EINVAL
    ("out 64->2 7x7x7", out(2, 64, 7)),                                         # fwd, dgrad ENOSUP (175 KB of weights); im2col ENOSUP
    ("out 64->4 5x5x5", out(4, 64, 5)),                                         # fwd, dgrad ENOSUP (128 KB)
    # ---- sr_head.2 (thin5): widths
    ("thin5 W 32", thin5(32)),                                                  # both precisions
    ("thin5 W 48", thin5(48)),                                                  # ENOSUP (W % 32); small_cout takes it
    ("thin5 W 64", thin5(64)),
    ("thin5 W 96", thin5(96)),
    ("thin5 W 128", thin5(128)),
    ("thin5 W 160", thin5(160)),                                                # bf16 only
    ("thin5 W 192", thin5(192)),                                                # ENOSUP
    # ---- thin5: channel pitch
    ("thin5 ldx 20", thin5(64, ldx=20)),                                        # fp32 only (% 4, not % 8)
    ("thin5 ldx 24", thin5(64, ldx=24)),                                        # both
    ("thin5 ldx 18", thin5(64, ldx=18)),                                        # neither
    # ---- thin5: the 2^32 byte bound of the buffer resource
    ("thin5 2^31 B bf16, 2^32 B fp32", thin5(128, D=1024, H=512)),              # bf16 only
    ("thin5 just under 2^32 B fp32", thin5(128, D=1023, H=512)),                # both
    ("thin5 2^32 B bf16", thin5(128, D=2048, H=512)),                           # neither
    ("thin5 just under 2^32 B bf16", thin5(128, D=2047, H=512)),                # bf16 only
    # ---- thin5: depth segments (N = 1, H = 8: two strips)
    ("thin5 D 15", thin5(64, D=15)),                                            # 1 segment
    ("thin5 D 32", thin5(64, D=32)),                                            # 2 segments
    ("thin5 D 64", thin5(64, D=64)),                                            # 4 segments
    ("thin5 D 256", thin5(64, D=256)),                                          # 16 segments
    ("thin5 D 64, N 256", thin5(64, D=64, N=256)),                              # 512 blocks without a split
    ("thin5 D 40, H 10, N 3", thin5(96, D=40, H=10, N=3)),                      # partial strip, uneven segments
    # ---- thin5: not this layer, or malformed
    ("thin5 pad 1", thin5(64, pad=(1, 1, 1), out=(16, 8, 64))),                 # ENOSUP
    ("thin5 ldy 1", thin5(64, ldy=1)),                                          # ENOSUP
    ("thin5 with activation", thin5(64, act=L.ACT_RELU)),                       # forward EINVAL
    ("thin5 null y", thin5(64, y=None)),                                        # EINVAL
]

QUERIES = ("rehr_conv5_thin_supported", "rehr_conv5_thin_f32_supported", "rehr_conv5_thin_workspace_bytes",
           "rehr_conv5_thin_f32_workspace_bytes", "rehr_conv_small_cin_wgrad_on_mfma",
           "rehr_conv_small_cin_wgrad_workspace_bytes", "rehr_conv_small_cout_wgrad_workspace_bytes")


def _kpad(d):
    return max(4, (d.Cin * d.KD * d.KH * d.KW + 3) // 4 * 4)


# launch entry point -> (call(lib, d, ptrs, ws, ws_bytes), descriptor pointers it requires, further pointers it requires,
#                        workspace query or None)
# `ptrs` holds the pointer arguments that are not descriptor fields: dw, dx, out
def _fwd(name):
    return lambda lib, d, p, ws, n: getattr(lib, name)(C.byref(d), None)


def _wgrad(name):
    return lambda lib, d, p, ws, n: getattr(lib, name)(C.byref(d), p["dw"], None, ws, n, None)


ENTRIES = {
    "rehr_conv_small_cin_fwd_f32": (_fwd("rehr_conv_small_cin_fwd_f32"), "xwy", (), None),
    "rehr_conv_small_cin_fwd_ybf16": (_fwd("rehr_conv_small_cin_fwd_ybf16"), "xwy", (), None),
    "rehr_conv_small_cin_wgrad_f32": (_wgrad("rehr_conv_small_cin_wgrad_f32"), "xwy", ("dw",),
                                      "rehr_conv_small_cin_wgrad_workspace_bytes"),
    "rehr_conv_small_cin_wgrad_dybf16": (_wgrad("rehr_conv_small_cin_wgrad_dybf16"), "xwy", ("dw",),
                                         "rehr_conv_small_cin_wgrad_workspace_bytes"),
    "rehr_im2col_f32": (lambda lib, d, p, ws, n: lib.rehr_im2col_f32(C.byref(d), p["out"], _kpad(d), None), "x", ("out",),
                        None),
    "rehr_conv_small_cout_fwd_f32": (_fwd("rehr_conv_small_cout_fwd_f32"), "xwy", (), None),
    "rehr_conv_small_cout_dgrad_f32": (lambda lib, d, p, ws, n: lib.rehr_conv_small_cout_dgrad_f32(C.byref(d), p["dx"], None),
                                       "xwy", ("dx",), None),
    "rehr_conv_small_cout_wgrad_f32": (_wgrad("rehr_conv_small_cout_wgrad_f32"), "xwy", ("dw",),
                                       "rehr_conv_small_cout_wgrad_workspace_bytes"),
}
for _sfx, _q in (("bf16", "rehr_conv5_thin_workspace_bytes"), ("f32", "rehr_conv5_thin_f32_workspace_bytes")):
    ENTRIES["rehr_conv5_thin_fwd_" + _sfx] = (
        lambda lib, d, p, ws, n, f="rehr_conv5_thin_fwd_" + _sfx: getattr(lib, f)(C.byref(d), ws, n, None), "xwy", (), _q)
    ENTRIES["rehr_conv5_thin_dgrad_" + _sfx] = (
        lambda lib, d, p, ws, n, f="rehr_conv5_thin_dgrad_" + _sfx: getattr(lib, f)(C.byref(d), p["dx"], 16, ws, n, None),
        "wy", ("dx",), _q)
    ENTRIES["rehr_conv5_thin_wgrad_" + _sfx] = (_wgrad("rehr_conv5_thin_wgrad_" + _sfx), "xy", ("dw",), _q)


def queries(lib, args):
    d = desc(**args)
    return {q: int(getattr(lib, q)(C.byref(d))) for q in QUERIES}


def launch_codes(lib, args):
    """Return code of every launch entry point for the row: as given ("base": with the queried workspace size, where it
    takes one), one byte short, a null workspace, and each required pointer null in turn.  Only meaningful where no
    device can take the launch: an accepted descriptor then comes back REHR_EHIP."""
    rec = {}
    for name, (call, dptrs, optrs, query) in ENTRIES.items():
        d = desc(**args)
        ptrs = {"dw": DW, "dx": DX, "out": OUT}
        need = int(getattr(lib, query)(C.byref(d))) if query else 0
        size = need if need > 0 else BIG
        r = {"base": call(lib, d, ptrs, WS, size)}
        if query:
            if need > 0:
                r["one byte short"] = call(lib, d, ptrs, WS, need - 1)
            r["null workspace"] = call(lib, d, ptrs, None, size)
        for f in dptrs:
            dn = desc(**args)
            setattr(dn, f, None)
            r["null " + f] = call(lib, dn, ptrs, WS, size)
        for f in optrs:
            r["null " + f] = call(lib, d, dict(ptrs, **{f: None}), WS, size)
        rec[name] = {k: int(v) for k, v in r.items()}
    return rec
