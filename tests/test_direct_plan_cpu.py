"""The host side of the direct gather-GEMM kernels (halo_conv.hip, halo_conv_bf16.hip, tconv_ks.hip and the generic
kernels) is pinned without a device: rehr_gather_gemm_direct_route against the routes written by hand in
tests/direct_plan_cases.py, and, where no device can take a launch, the return codes of the four launch entry points
against tests/golden/direct_plan.json, recorded with the library as it was before that host code was merged into
halo_shared.h (tools/gen_golden_direct_plan.py).

Where nothing can launch, a call that reaches a kernel comes back REHR_EHIP, one whose operands no direct kernel reaches
REHR_ENOSUP, an invalid one REHR_EINVAL: that is how the recorded codes check the hand-written routes."""
import ctypes as C
import json
import os

import pytest
import torch

from rehrseg_amd import hip_backend
from rehrseg_amd import lib as L
from direct_plan_cases import (BF16_ROUTES, EHIP, EINVAL, ENOSUP, F32_ROUTES, FLAGS, LAUNCHED_BEFORE_VALIDATION, MULTI, ROUTES, ROWS,
                               bind, make, multi_codes, row_codes)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "direct_plan.json")
# the rejection predicates the table must reach: each a phrase of the last column of some row WITHOUT that route
REJECTIONS_F32 = ("stride != 1", "Npad > 64", "T < 9", "T > 64", "lattice below the brick", "1.3003 > 1.3", "hvox > 416",
                  "gg_src_fits", "wp_bytes")
REJECTIONS_BF16 = ("stride != 1", "T not in {9, 27}", "more than 3 taps at T = 9", "more than 3 taps at T = 27", "Cout % 8", "ldy % 8",
                   "y & 15", "halo > brick + 2", "lattice below the brick", "1.333 > 1.3", "1.3003 > 1.3", "gg_src_fits", "wp_bytes",
                   "y bytes", "T = 9 only", "(declined)")
REJECTIONS_TCONV = ("Cin > 64", "Cin > 128", "Cin % 32", "Npad > 128", "x2 != nullptr", "act != NONE", "stats_mode != 0", "REHR_GG_Y_F32",
                    "!= count", "Hy != Hi x osh", "KW != osw", "d.y != d0.y", "d.bias != d0.bias", "d.ldy != d0.ldy", "tw.count != 1",
                    "th.off0 != 0", "d.bw != 0", "d.Lh != d0.Hi", "d.obw != d.tw.k0", "a phase twice", "d.act != NONE", "ldy % 2")


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _query(parts, bf16, flags=0):
    """[(kind, variant)] per part, or "EINVAL"."""
    arr = make(parts, flags)
    out = (C.c_int32 * len(parts))()
    rc = L.load().rehr_gather_gemm_direct_route(arr, len(parts), int(bf16), out)
    assert rc in (0, EINVAL)
    return "EINVAL" if rc else [(r & 255, r >> 8) for r in out]


def _want(routes, flags="0", bf16=False):
    """The hand-written routes under a flag setting: NO_HALO sends the bf16 halo shapes to the generic grid (fp32 does not
    look at it); NO_TCONV_KS sends every phase to the generic grid."""
    if routes == "EINVAL":
        return routes
    routes = [routes] if isinstance(routes, str) else routes
    if flags == "NO_HALO" and bf16:
        routes = ["generic" if r.startswith("halo") else r for r in routes]
    if flags == "NO_TCONV_KS":
        routes = ["generic" if r == "tconv_ks" else r for r in routes]
    return [ROUTES[r] for r in routes]


def _code(routes):
    """Return code of the launch where nothing can launch."""
    if routes == "EINVAL":
        return EINVAL
    return ENOSUP if ROUTES["none"] in routes else EHIP


def test_table_is_not_one_sided():
    g = _golden()
    assert len(ROWS) >= 40 and set(g["rows"]) == {r[0] for r in ROWS} and set(g["multi"]) == {m[0] for m in MULTI}
    f32 = [r[2] for r in ROWS] + [x for m in MULTI if m[2] != "EINVAL" for x in set(m[2])]
    bf16 = [r[3] for r in ROWS] + [x for m in MULTI if m[3] != "EINVAL" for x in set(m[3])]
    for name in F32_ROUTES:
        assert f32.count(name) >= 3, name
    for name in BF16_ROUTES:
        assert bf16.count(name) >= 3, name
    assert {r for r in f32 + bf16 if r != "EINVAL"} == set(ROUTES)
    why32 = " | ".join(r[4] for r in ROWS if not r[2].startswith("halo"))
    why16 = " | ".join(r[4] for r in ROWS if not r[3].startswith("halo"))
    for word in REJECTIONS_F32:
        assert word in why32, word
    for word in REJECTIONS_BF16:
        assert word in why16, word
    whyt = " | ".join(m[4] for m in MULTI if "tconv_ks" not in m[2] or "tconv_ks" not in m[3])
    for word in REJECTIONS_TCONV:
        assert word in whyt, word
    # fp32 declines the 96- and 128-channel phases that bf16 takes
    assert {m[0] for m in MULTI if m[3] != "EINVAL" and "tconv_ks" in m[3] and "tconv_ks" not in m[2]} == {"tconv 96->32 s122", "tconv 128->64 s222"}
    # just above and just below the 1.3x rule, and the split-K rule, the invalid calls and the parts counts
    assert any("1.2989" in r[4] and r[2].startswith("halo") and r[3].startswith("halo") for r in ROWS)
    assert sum("split-K" in m[4] or "as above" in m[4] for m in MULTI) >= 2
    assert sum(m[2] == "EINVAL" or m[3] == "EINVAL" for m in MULTI) >= 6 and sum(r[2] == "EINVAL" for r in ROWS) >= 2
    assert {len(m[1]) for m in MULTI} >= {2, 3, 4, 8}
    # the stage-2 lattices with the bricks tests/test_stage2_lattice_gpu.py::_halo_bf16 predicts
    stage2 = {r[0].split()[1]: r[3] for r in ROWS if r[0].startswith("enc")}
    assert stage2 == {"16x320x384": "halo 4x8x16", "16x160x192": "halo 4x8x16", "16x80x96": "halo 4x8x16", "8x40x48": "halo 4x8x16",
                      "4x20x24": "generic", "4x10x12": "generic"}
    assert LAUNCHED_BEFORE_VALIDATION < {m[0] for m in MULTI}
    codes = {c for r in g["rows"].values() for v in r.values() for c in v}
    assert codes == {EINVAL, ENOSUP, EHIP}


def test_route_query():
    """The hand-written routes under every flag setting; the Python binding; null arguments."""
    for name, args, f32, bf16, _ in ROWS:
        for f, bits in FLAGS.items():
            assert _query([args], False, bits) == _want(f32, f), (name, f)
            assert _query([args], True, bits) == _want(bf16, f, True), (name, f)
    for name, parts, f32, bf16, _ in MULTI:
        for f, bits in FLAGS.items():
            assert _query(parts, False, bits) == _want(f32, f), (name, f)
            assert _query(parts, True, bits) == _want(bf16, f, True), (name, f)
    assert hip_backend.direct_route(make(MULTI[0][1]), 8, True) == [ROUTES["tconv_ks"]] * 8
    with pytest.raises(L.RehrsegHipError):
        hip_backend.direct_route(make([ROWS[-1][1]]), 1, False)
    lib = L.load()
    out = (C.c_int32 * 9)()
    assert lib.rehr_gather_gemm_direct_route(None, 1, 0, out) == EINVAL
    assert lib.rehr_gather_gemm_direct_route(make([ROWS[0][1]]), 1, 0, None) == EINVAL
    assert lib.rehr_gather_gemm_direct_route(make([ROWS[0][1]] * 9), 9, 0, out) == EINVAL
    assert lib.rehr_gather_gemm_direct_route(make([ROWS[0][1]]), 0, 1, out) == EINVAL


def test_recorded_codes_agree_with_the_hand_written_routes():
    """The golden file against the table alone (no library): EHIP where the route reaches a kernel, ENOSUP for "none",
    EINVAL for an invalid call -- except the bf16 rows the recorded library launched into before it validated them."""
    g = _golden()
    for name, _, f32, bf16, _ in ROWS:
        for f in FLAGS:
            assert g["rows"][name][f] == [_code(_want(f32, f))] * 2 + [_code(_want(bf16, f, True))] * 2, (name, f)
    for name, _, f32, bf16, _ in MULTI:
        for f in FLAGS:
            want16 = _code(_want(bf16, f, True))
            if name in LAUNCHED_BEFORE_VALIDATION and f != "NO_HALO":
                assert want16 == EINVAL
                want16 = EHIP
            assert g["multi"][name][f] == [_code(_want(f32, f)), want16], (name, f)


def test_launch_codes_equal_the_recorded_ones():
    """Every row and multi-part row, every flag setting, the four entry points.  Runs only where there is no device: an
    accepted descriptor then meets "no device" (REHR_EHIP), not a launch on dummy pointers."""
    if torch.cuda.is_available():
        pytest.skip("dummy pointers: only where an accepted descriptor cannot be launched")
    lib = bind()
    g = _golden()
    for r in ROWS:
        assert row_codes(lib, r[1]) == g["rows"][r[0]], r[0]
    for m in MULTI:
        got, rec = multi_codes(lib, m[1]), g["multi"][m[0]]
        if m[0] in LAUNCHED_BEFORE_VALIDATION:
            # part 0 is a halo shape and a later part is invalid: the recorded library had launched part 0 (EHIP here)
            # before it looked at the later part; every part is validated first now.  NO_HALO never launched early.
            for f in FLAGS:
                assert rec[f] == [EINVAL, EINVAL if f == "NO_HALO" else EHIP] and got[f] == [EINVAL, EINVAL], (m[0], f)
        else:
            assert got == rec, m[0]
