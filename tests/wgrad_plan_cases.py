"""Descriptor table of the weight-gradient planners (tests/test_wgrad_plan_cpu.py, tools/gen_golden_wgrad_plan.py).

Every row is one rehr_wgrad_desc with tiny extents and dummy 16-byte-aligned pointers that nothing on the host
dereferences.  The comment of a row names the route the library took for it when tests/golden/wgrad_plan.json was
recorded (fp32 route / bf16 route; "-" = rejected), and why the row is there."""
from rehrseg_amd import lib as L

DIRECT = L.DBG_WGRAD_DIRECT
NO_SKIP = L.DBG_WGRAD_NO_TAP_SKIP


def desc(Ca=32, Cg=32, N=2, lat=(4, 16, 16), K=(3, 3, 3), stride=(1, 1, 1), pad=None, gdims=None, flags=0, **over):
    """Weight gradient of a convolution with kernel K: l = the tensor on the lattice `lat` (Ca channels), g = the gathered
    tensor (Cg channels) of extents `gdims` (default: what the lattice reaches, (lat - 1) * stride + K - 2 * pad); pad
    defaults to (K - 1) // 2.  `over` sets raw descriptor fields last."""
    pad = tuple((k - 1) // 2 for k in K) if pad is None else pad
    gdims = tuple((lat[a] - 1) * stride[a] + K[a] - 2 * pad[a] for a in range(3)) if gdims is None else gdims
    T = K[0] * K[1] * K[2]
    d = L.WgradDesc()
    d.l, d.g, d.dst = 0x1000, 0x2000, 0x3000
    d.ldl = d.Ca = Ca
    d.ldg = d.Cg = Cg
    d.N = N
    d.Ld, d.Lh, d.Lw = lat
    d.Dg, d.Hg, d.Wg = gdims
    d.sd, d.sh, d.sw = stride
    d.bd, d.bh, d.bw = (-p for p in pad)
    d.td, d.th, d.tw = (L.AxisTaps(count=k) for k in K)
    d.KH, d.KW = K[1], K[2]
    d.dst_sa, d.dst_sc, d.dst_st = Cg * T, T, 1
    d.debug_flags = flags
    for k, v in over.items():
        setattr(d, k, v)
    return d


S2 = dict(stride=(2, 2, 2), lat=(2, 8, 8), gdims=(4, 16, 16))                    # 3x3x3, stride 2, pad 1
T22 = dict(N=2, lat=(2, 8, 16), K=(3, 4, 4), stride=(1, 2, 2), pad=(1, 1, 1))  # transposed 3x4x4, stride (1, 2, 2)

# (name, desc() arguments)                                                      # fp32 route / bf16 route: why
ROWS = [
    # ---- Winograd F(2x2,3x3), wide planes: the four group shapes
    ("wino 32x32", dict()),                                                     # Winograd fa 1 fb 1 / brick KD 3
    ("wino 32x64", dict(Cg=64)),                                                # Winograd 1x2 / brick
    ("wino 64x32", dict(Ca=64)),                                                # Winograd 2x1 / brick
    ("wino 64x64", dict(Ca=64, Cg=64)),                                         # Winograd, the eight-wave block / brick
    ("wino 64x64 with dbias", dict(Ca=64, Cg=64, dbias=0x4000)),                # Winograd, same size / - (dbias)
    ("wino 16x32", dict(Ca=16)),                                                # Winograd, 16 padded to 32 / brick
    ("wino 1x3x3", dict(K=(1, 3, 3))),                                          # Winograd, one depth tap / brick KD 1
    ("wino 5 depth taps", dict(N=1, lat=(8, 16, 16), K=(5, 3, 3))),             # Winograd, many depth taps / slab 32
    ("wino 32x32 no tap skip", dict(flags=NO_SKIP)),                            # Winograd, same plan without skipping
    # ---- Winograd, narrow planes (Lw < 16: eight slices side by side)
    ("wino narrow N8", dict(N=8, lat=(8, 12, 12))),                             # Winograd G 8, N % 8 == 0: tap skip / slab
    ("wino narrow N2", dict(N=2, lat=(32, 12, 12))),                            # Winograd G 8, no tap skip / slab 32
    # ---- Winograd refused
    ("wino refused: 5x17 plane pads to 8x32", dict(lat=(4, 5, 17))),            # slab 32 (Lh < 8: no brick) / slab
    ("wino refused: narrow 5x6 plane", dict(N=8, lat=(8, 5, 6))),               # slab 32 (Lw < 8: no brick) / slab
    ("wino refused: narrow, 21 items < 128", dict(lat=(4, 12, 12))),            # slab 32 (brick pads 576 -> 1024) / slab
    ("wino refused: 96x96 pads to 128x128", dict(Ca=96, Cg=96)),                # slab 32 (9 tile pairs: no brick) / brick
    ("wino refused: valid conv, Hg != Lh", dict(pad=(0, 0, 0))),                # brick / brick KD 3 (taps 0, 1, 2)
    ("wino refused: 36x32 pads to 64x32", dict(Ca=36)),                         # brick, masked tiles / - (Ca % 8)
    # ---- F(2x2,2x2): stride-2 four-tap transposed taps, >= 64 channels
    ("wino22 64x64", dict(Ca=64, Cg=64, **T22)),                                # F(2x2,2x2) / slab 64
    ("wino22 128x64", dict(Ca=128, Cg=64, **T22)),                              # F(2x2,2x2) / slab 64
    ("wino22 refused: dbias", dict(Ca=64, Cg=64, dbias=0x4000, **T22)),         # slab 64 / - (dbias)
    ("wino22 refused: 32 channels", dict(**T22)),                               # slab 32 / slab 32
    # ---- fp32 brick with the Winograd path forced off
    ("direct 32x32 3x3x3", dict(flags=DIRECT)),                                 # brick / slab 32 (DIRECT: no bf16 brick)
    ("direct 64x64 3x3x3", dict(Ca=64, Cg=64, flags=DIRECT)),                   # brick, 4 tile pairs / slab 64
    ("direct 32x32 1x3x3", dict(K=(1, 3, 3), flags=DIRECT)),                    # brick, 9 taps / slab 32
    ("direct 64x64 1x3x3", dict(Ca=64, Cg=64, K=(1, 3, 3), flags=DIRECT)),      # brick / slab 64
    # ---- fp32 brick refused
    ("direct 128x128: 16 tile pairs", dict(Ca=128, Cg=128, flags=DIRECT)),      # slab 128 / slab 128
    ("direct 1x16x16 lattice", dict(lat=(1, 16, 16), K=(1, 3, 3), flags=DIRECT)),  # slab 32 (Ld < 2) / slab 32
    ("direct 4x12x12: bricks pad 1.78x", dict(lat=(4, 12, 12), flags=DIRECT)),  # slab 32 / slab 32
    # ---- slab kernels: tile sizes
    ("stride 2, 128x128", dict(Ca=128, Cg=128, **S2)),                          # slab 128 / slab 128
    ("stride 2, 64x128", dict(Ca=64, Cg=128, **S2)),                            # slab 64 (the smaller side's tile) / slab 64
    ("stride 2, 32x32", dict(**S2)),                                            # slab 32 / slab 32
    ("stride 2, 48x32", dict(Ca=48, **S2)),                                     # slab 32, masked / slab 32, masked
    ("stride 2, 20x36", dict(Ca=20, Cg=36, **S2)),                              # slab 32, masked / - (Ca % 8)
    ("1x1x1 taps", dict(Cg=64, lat=(4, 8, 8), K=(1, 1, 1))),                    # slab 32 / slab 32
    # ---- many blocks: the split-count searches have a real choice (large extents, but nothing is allocated)
    ("large wino 32x32", dict(N=4, lat=(16, 64, 64))),                          # Winograd / brick
    ("large wino 64x64", dict(Ca=64, Cg=64, N=4, lat=(16, 64, 64))),            # Winograd / brick
    ("large wino narrow", dict(N=16, lat=(16, 12, 12))),                        # Winograd G 8 / slab 32
    ("large wino22 64x64", dict(Ca=64, Cg=64, **dict(T22, N=4, lat=(8, 32, 32)))),  # F(2x2,2x2) / slab 64
    ("large direct 32x32", dict(N=4, lat=(16, 64, 64), flags=DIRECT)),          # brick / slab 32
    ("large direct 64x64", dict(Ca=64, Cg=64, N=3, lat=(10, 40, 56), flags=DIRECT)),  # brick / slab 64
    ("large direct 128x128", dict(Ca=128, Cg=128, N=3, lat=(10, 40, 56), flags=DIRECT)),  # slab 128 / slab 128
    ("large stride 2, 32x32", dict(N=4, stride=(2, 2, 2), lat=(16, 32, 32), gdims=(32, 64, 64))),  # slab 32 / slab 32
    ("large stride 2, 64x64", dict(Ca=64, Cg=64, N=3, stride=(2, 2, 2), lat=(9, 30, 34), gdims=(18, 60, 68))),  # slab 64
    # ---- REHR_ENOSUP
    ("g of 4 GiB", dict(Ca=64, Cg=64, N=64, lat=(64, 64, 64))),                 # - ENOSUP / brick (2 GiB of bf16)
    ("2^31 lattice voxels", dict(N=2048, lat=(64, 128, 128))),                  # - ENOSUP / - ENOSUP
    ("one split of l reaches 4 GiB", dict(lat=(4, 32, 32), K=(1, 1, 1), ldl=1 << 20)),  # - ENOSUP / slab 32 (2 GiB)
    # ---- REHR_EINVAL
    ("null l", dict(l=None)),                                                   # - / -
    ("Ca = 30", dict(Ca=30)),                                                   # - / -
    ("ldl = 34", dict(ldl=34)),                                                 # - / -
    ("misaligned g", dict(g=0x2004)),                                           # - / -
    ("tap count 0", dict(td=L.AxisTaps(count=0))),                              # - / -
    ("ldl = 36", dict(ldl=36)),                                                 # Winograd / - (ldl % 8)
    ("dbias given", dict(dbias=0x4000)),                                        # Winograd / - (dbias)
]

