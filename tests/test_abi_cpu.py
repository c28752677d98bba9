"""The C-ABI library loads without a GPU and exports exactly what include/rehrseg_hip.h
declares; argument validation rejects malformed descriptors before any launch."""
import ctypes as C

import pytest

from rehrseg_amd import lib as L


def test_library_exports_every_declared_symbol():
    lib = L.load()
    declared = L.declared_symbols()
    assert len(declared) >= 20
    assert set(declared) == set(L.PROTOTYPES), set(declared) ^ set(L.PROTOTYPES)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.rehr_abi_version() == L.ABI_VERSION


def test_struct_sizes_match_header_layout():
    # int32/float/pointer fields only, natural alignment: sizes are a cheap layout check
    assert C.sizeof(L.AxisTaps) == 20
    assert C.sizeof(L.GatherGemmDesc) % 8 == 0 and C.sizeof(L.WgradDesc) % 8 == 0


def test_malformed_descriptors_are_rejected_without_launching():
    lib = L.load()
    d = L.GatherGemmDesc()  # all zero: null pointers
    assert lib.rehr_gather_gemm_f32(C.byref(d), None) == -1
    w = L.WgradDesc()
    assert lib.rehr_wgrad_f32(C.byref(w), None) == -1
    assert lib.rehr_wgrad_workspace_bytes(C.byref(w)) == -1
    assert lib.rehr_pack_weights_f32(None, None, 1, 1, 1, 1, 0, None) == -1
    assert lib.rehr_act_fwd_f32(None, None, 4, 0, 0.0, None) == -1
    dc = L.DirectConvDesc()
    assert lib.rehr_conv_small_cin_fwd_f32(C.byref(dc), None) == -1


def test_product_path_refuses_cpu_tensors():
    import torch
    from rehrseg_amd import ops
    with pytest.raises(L.RehrsegHipError):
        ops.fused_conv3d(torch.randn(1, 32, 2, 4, 4), torch.randn(32, 32, 3, 3, 3), None, 1, 1)


def test_flag_constants_of_the_binding_equal_the_header():
    """Every REHR_GG_* / REHR_DBG_* bit the Python binding uses carries the value the header defines (a renumbered bit
    would silently select another kernel or, for REHR_GG_WS_ONLY / _READY, skip or repeat a weight transform)."""
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rehrseg_hip.h")).read()
    defs = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define\s+REHR_(\w+)\s+(0x[0-9a-fA-F]+|\d+)\s", hdr)}
    checked = 0
    for name in dir(L):
        if name.startswith(("GG_", "DBG_")) and isinstance(getattr(L, name), int):
            assert name in defs, f"lib.{name} has no REHR_{name} in the header"
            assert defs[name] == getattr(L, name), (name, defs[name], getattr(L, name))
            checked += 1
    assert checked >= 12
    assert defs["GG_WS_READY"] != defs["GG_WS_ONLY"] and defs["GG_Y_F32"] == 1


def _gg_base(**over):
    """One well-formed gather-GEMM descriptor (32 -> 32 channels, 2x2x2 lattice onto a 2x2x2 output, one tap per axis,
    dummy 16-byte-aligned pointers that nothing on the host dereferences), with `over` applied on top."""
    d = L.GatherGemmDesc()
    d.x1, d.wp, d.y = 0x1000, 0x2000, 0x3000
    d.c1 = d.Cin = d.Cout = d.Npad = d.ldx1 = d.ldy = 32
    d.N = d.KH = d.KW = 1
    d.Di = d.Hi = d.Wi = d.Ld = d.Lh = d.Lw = d.Dy = d.Hy = d.Wy = 2
    d.sd = d.sh = d.sw = d.osd = d.osh = d.osw = 1
    d.td = d.th = d.tw = L.AxisTaps()
    for k, v in over.items():
        setattr(d, k, v)
    return d


EINVAL, EHIP = -1, -3
# (row, fields broken on the base descriptor, (f32, bf16) return code).  The codes are what the library returned before
# the two validate() copies were merged into gg_shared.h; EHIP = the descriptor was accepted and the launch found no device.
_GG_ROWS = [
    ("null x1", dict(x1=None), (EINVAL, EINVAL)),
    ("null wp", dict(wp=None), (EINVAL, EINVAL)),
    ("null y", dict(y=None), (EINVAL, EINVAL)),
    ("Cin = 8", dict(Cin=8, c1=8), (EINVAL, EINVAL)),
    ("Cin = 24", dict(Cin=24, c1=24), (EINVAL, EINVAL)),
    ("c1 = 0", dict(c1=0), (EINVAL, EINVAL)),
    ("c1 = Cin + 16", dict(c1=48), (EINVAL, EINVAL)),
    ("c1 = 16 of Cin = 64, x2 given", dict(Cin=64, c1=16, x2=0x4000, ldx2=48), (EINVAL, EINVAL)),
    ("c1 = 32 of Cin = 64, null x2", dict(Cin=64, c1=32), (EINVAL, EINVAL)),
    ("ldx1 = 30", dict(ldx1=30), (EINVAL, EINVAL)),
    ("ldx1 = 36: whole 16-byte pieces of fp32, not of bf16", dict(ldx1=36), (EHIP, EINVAL)),
    ("ldx1 = 40: whole 16-byte pieces of both (the rest of the base descriptor is accepted)", dict(ldx1=40), (EHIP, EHIP)),
    ("misaligned wp", dict(wp=0x2004), (EINVAL, EINVAL)),
    ("Npad = 48", dict(Npad=48), (EINVAL, EINVAL)),
    ("Npad < Cout", dict(Cout=40, ldy=40), (EINVAL, EINVAL)),
    ("Ld = 0", dict(Ld=0), (EINVAL, EINVAL)),
    ("tap count 0", dict(td=L.AxisTaps(count=0)), (EINVAL, EINVAL)),
    ("tile 2x2x2", dict(tile_d=2, tile_h=2, tile_w=2), (EINVAL, EINVAL)),
    ("stats_mode = 1, null stats", dict(stats_mode=1), (EINVAL, EINVAL)),
    ("N = 65536", dict(N=65536), (EINVAL, EINVAL)),
    ("obd = -1", dict(obd=-1), (EINVAL, EINVAL)),
    ("last lattice point outside y", dict(osd=2), (EINVAL, EINVAL)),
    ("ldy < Cout", dict(ldy=16), (EINVAL, EINVAL)),
]
# count = 2 on the multi entry points: the second phase differs from the (well-formed) first one
_GG_PAIR_ROWS = [
    ("differing Npad", dict(Npad=64), (EINVAL, EINVAL)),
    ("differing wp", dict(wp=0x5000), (EINVAL, EINVAL)),
    ("differing Cin: fp32 plans each phase on its own, bf16 takes the K step from phase 0", dict(Cin=64, c1=64, ldx1=64),
     (EHIP, EINVAL)),
]


def test_gather_gemm_validation_codes_are_pinned():
    """Return code of the four gather-GEMM entry points for one broken field at a time.  Runs only where there is no
    device: a descriptor that is wrongly accepted then meets "no device", not a launch on dummy pointers."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("dummy pointers: only where an accepted descriptor cannot be launched")
    lib = L.load()
    entries = ((lib.rehr_gather_gemm_f32, lib.rehr_gather_gemm_multi_f32),
               (lib.rehr_gather_gemm_bf16, lib.rehr_gather_gemm_multi_bf16))
    for name, over, want in _GG_ROWS:
        d = _gg_base(**over)
        for (single, multi), w in zip(entries, want):
            assert single(C.byref(d), None) == w, (name, single.__name__)
            assert multi(C.byref(d), 1, None) == w, (name, multi.__name__)
    for name, over, want in _GG_PAIR_ROWS:
        pair = (L.GatherGemmDesc * 2)(_gg_base(), _gg_base(**over))
        for (_, multi), w in zip(entries, want):
            assert multi(pair, 2, None) == w, (name, multi.__name__)
    nine = (L.GatherGemmDesc * 9)(*[_gg_base() for _ in range(9)])
    for _, multi in entries:
        assert multi(nine, 0, None) == EINVAL, ("count = 0", multi.__name__)
        assert multi(nine, 9, None) == EINVAL, ("count = 9", multi.__name__)
