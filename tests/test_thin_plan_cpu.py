"""The host side of the thin-convolution family (everything driven by rehr_direct_conv_desc) is pinned without a device:
the size and route queries, and, where no device can take a launch, the return code of every launch entry point.
tests/golden/thin_plan.json was recorded with the library as it was before the family's host code was merged into
direct_shared.h (tools/gen_golden_thin_plan.py)."""
import ctypes as C
import json
import os

import pytest
import torch

from rehrseg_amd import hip_backend as hb
from rehrseg_amd import lib as L
from thin_plan_cases import ENTRIES, QUERIES, ROWS, desc, launch_codes, queries

EINVAL, ENOSUP, EHIP = -1, -2, -3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "thin_plan.json")
# rehr_conv_small_cout_wgrad_f32 has no unsupported shape: whatever small_cout_ok lets through, one of its kernels takes
NEVER_ENOSUP = {"rehr_conv_small_cout_wgrad_f32"}
# The size query of the thin-input weight gradient speaks for an fp32 dY: with dY at an address that only suits bf16 it
# reports the vector kernel's slabs (179 200 B), while the bf16 launch takes the matrix-core route and needs 49 152 B --
# one byte less than the QUERY is therefore still enough there.  Recorded as the library had it.
SHORT_STILL_ENOUGH = {("in y misaligned for fp32", "rehr_conv_small_cin_wgrad_dybf16")}


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)["rows"]


def _rows(g, prefix):
    return {name: (args, g[name]) for name, args in ROWS if name.startswith(prefix)}


def test_table_reaches_every_route_and_error_code():
    """The recorded values themselves show that the table is not one-sided."""
    g = _golden()
    assert len(ROWS) >= 40 and set(g) == {name for name, _ in ROWS}
    assert len(ENTRIES) == 14
    for e in ENTRIES:
        codes = {r["launch"][e]["base"] for r in g.values()}
        assert codes == {EINVAL, EHIP} | (set() if e in NEVER_ENOSUP else {ENOSUP}), (e, codes)
    for name, r in g.items():
        for e, v in r["launch"].items():
            if v["base"] != EHIP:
                continue
            # an accepted descriptor: every variation is malformed
            for what, code in v.items():
                if what == "base" or (what == "one byte short" and (name, e) in SHORT_STILL_ENOUGH):
                    continue
                assert code == EINVAL, (name, e, what, code)
            if ENTRIES[e][3]:
                assert "one byte short" in v and "null workspace" in v, (name, e)

    # ---- sr_head.2
    t5 = _rows(g, "thin5 ")
    ok = lambda r: (r["queries"]["rehr_conv5_thin_supported"], r["queries"]["rehr_conv5_thin_f32_supported"])  # noqa: E731
    by_w = {a["inp"][2]: ok(r) for n, (a, r) in t5.items() if n.startswith("thin5 W ")}
    assert by_w == {32: (1, 1), 48: (0, 0), 64: (1, 1), 96: (1, 1), 128: (1, 1), 160: (1, 0), 192: (0, 0)}
    assert ok(t5["thin5 W 64"][1]) == (1, 1)    # ldx 16
    assert ok(t5["thin5 ldx 20"][1]) == (0, 1) and ok(t5["thin5 ldx 24"][1]) == (1, 1)
    for name, want in (("thin5 2^31 B bf16, 2^32 B fp32", (1, 0)), ("thin5 just under 2^32 B fp32", (1, 1)),
                       ("thin5 2^32 B bf16", (0, 0)), ("thin5 just under 2^32 B bf16", (1, 0))):
        a, r = t5[name]
        D, H, W = a["inp"]
        assert ok(r) == want and want == (int(D * H * W * 32 < 2 ** 32), int(D * H * W * 64 < 2 ** 32)), name
    # workspace = blocks x (25*16*16 + 16) floats, blocks = N x strips x depth segments: N = 1, H = 8 is two strips
    slab = (25 * 16 * 16 + 16) * 4
    segs = {a["inp"][0]: r["queries"]["rehr_conv5_thin_workspace_bytes"] // (2 * slab)
            for n, (a, r) in t5.items() if n in ("thin5 D 15", "thin5 D 32", "thin5 D 64", "thin5 D 256")}
    assert segs == {15: 1, 32: 2, 64: 4, 256: 16}
    a, r = t5["thin5 D 64, N 256"]
    assert r["queries"]["rehr_conv5_thin_workspace_bytes"] == 256 * 2 * 1 * slab   # no split
    for r in g.values():
        q = r["queries"]
        both = {q["rehr_conv5_thin_f32_workspace_bytes"], q["rehr_conv5_thin_workspace_bytes"]} - {ENOSUP}
        assert len(both) <= 1, q   # the slabs have one layout in both precisions

    # ---- thin input
    tin = _rows(g, "in ")
    fwd = lambda n, e="rehr_conv_small_cin_fwd_f32": tin[n][1]["launch"][e]["base"]  # noqa: E731
    ybf = "rehr_conv_small_cin_fwd_ybf16"
    assert {a.get("Cout", 32) for a, _ in tin.values()} >= {16, 32, 64, 48}
    assert {a.get("K", (3, 3, 3))[2] for a, _ in tin.values()} >= {8, 9}
    assert {a.get("stride", (1, 1, 1))[2] for a, _ in tin.values()} >= {1, 2, 3}
    assert (fwd("in y misaligned for fp32"), fwd("in y misaligned for fp32", ybf)) == (EINVAL, EHIP)
    assert (fwd("in y misaligned for bf16"), fwd("in y misaligned for bf16", ybf)) == (EINVAL, ENOSUP)
    for n in ("in 2->64 5x7x7", "in 2->64 5x7x7 stride 1,2,2"):   # fp32 runs, a bf16 output is not on offer
        assert (fwd(n), fwd(n, ybf), tin[n][1]["queries"]["rehr_conv_small_cin_wgrad_on_mfma"]) == (EHIP, ENOSUP, 0)
    assert (fwd("in 2->64 7x7x7"), fwd("in 2->64 7x7x7", ybf)) == (ENOSUP, ENOSUP)
    assert (fwd("in 2->32 7x7x7"), fwd("in 2->32 7x7x7", ybf)) == (EHIP, EHIP)
    on_mfma = [r["queries"]["rehr_conv_small_cin_wgrad_on_mfma"] for _, r in tin.values()]
    assert 5 <= sum(on_mfma) <= len(on_mfma) - 5

    # ---- thin output
    tout = _rows(g, "out ")
    acc = {n: a for n, (a, r) in tout.items() if r["launch"]["rehr_conv_small_cout_wgrad_f32"]["base"] == EHIP}
    assert {a["Cout"] for a in acc.values()} == {1, 2, 3, 4} and 5 in {a["Cout"] for a, _ in tout.values()}
    assert {a["Cin"] for a in acc.values()} == {16, 32, 48, 64}
    assert {a["K"] for a in acc.values()} >= {(1, 1, 1), (3, 3, 3), (5, 5, 5)}
    assert "out 16->2 5x5x5 odd extents" in acc      # Cout 2, Cin 16, 5x5x5: the <5> rows kernel


def test_queries_equal_the_recorded_ones():
    lib = L.load()
    g = _golden()
    for name, args in ROWS:
        got = queries(lib, args)
        assert got == g[name]["queries"], (name, got, g[name]["queries"])
    assert set(QUERIES) == set(next(iter(g.values()))["queries"])


def test_forward_route_query_is_what_the_bf16_forward_accepted():
    """rehr_conv_small_cin_fwd_on_mfma answers for the shape (and y's alignment, when y is given) what
    rehr_conv_small_cin_fwd_ybf16 did with the row when the table was recorded."""
    lib = L.load()
    g = _golden()
    taken = 0
    for name, args in ROWS:
        d = desc(**args)
        want = g[name]["launch"]["rehr_conv_small_cin_fwd_ybf16"]["base"] not in (EINVAL, ENOSUP)
        assert bool(lib.rehr_conv_small_cin_fwd_on_mfma(C.byref(d))) == want, name
        taken += want
    assert taken >= 10
    assert not lib.rehr_conv_small_cin_fwd_on_mfma(None)


def test_python_asks_the_library():
    """hb.thin5_supported and hb.small_cin_bf16_out_ok hold no shape rule of their own."""
    g = _golden()
    for name, args in ROWS:
        if args.get("ldx", args.get("Cin", 1)) != args.get("Cin", 1) or "ldy" in args or "out" in args:
            continue   # the Python predicates speak for dense tensors with the output extent the conv gives
        d = desc(**args)
        x_shape = (d.N, d.Cin, d.Di, d.Hi, d.Wi)
        w_shape = (d.Cout, d.Cin, d.KD, d.KH, d.KW)
        pad, stride = (d.pd, d.ph, d.pw), (d.sd, d.sh, d.sw)
        q = g[name]["queries"]
        if stride == (1, 1, 1):
            assert hb.thin5_supported(x_shape, w_shape, pad) == bool(q["rehr_conv5_thin_supported"]), name
            assert hb.thin5_supported(x_shape, w_shape, pad, torch.float32) == bool(q["rehr_conv5_thin_f32_supported"]), name
            assert not hb.thin5_supported(x_shape, w_shape, pad, torch.float16), name
        if d.y == 0x30000 and d.x and d.w and not (d.stats_mode and not d.stats):
            want = g[name]["launch"]["rehr_conv_small_cin_fwd_ybf16"]["base"] not in (EINVAL, ENOSUP)
            assert hb.small_cin_bf16_out_ok(x_shape, w_shape, stride, pad) == want, name
    saved = hb.USE_THIN5_F32
    try:
        hb.USE_THIN5_F32 = False
        assert not hb.thin5_supported((1, 16, 16, 8, 64), (2, 16, 5, 5, 5), (2, 2, 2), torch.float32)
        assert hb.thin5_supported((1, 16, 16, 8, 64), (2, 16, 5, 5, 5), (2, 2, 2))
    finally:
        hb.USE_THIN5_F32 = saved


def test_launch_codes_equal_the_recorded_ones():
    """Every entry point, every row, every variation (queried workspace size, one byte less, null workspace, each required
    pointer null).  Runs only where there is no device: an accepted descriptor then meets "no device" (REHR_EHIP), not a
    launch on dummy pointers."""
    if torch.cuda.is_available():
        pytest.skip("dummy pointers: only where an accepted descriptor cannot be launched")
    lib = L.load()
    g = _golden()
    for name, args in ROWS:
        got = launch_codes(lib, args)
        for e in ENTRIES:
            assert got[e] == g[name]["launch"][e], (name, e, got[e], g[name]["launch"][e])
