"""The host side of the fp32 Winograd forward / input-gradient family is pinned without a device: the scratch query under
every debug-flag setting, the route query, and, where no device can take a launch, the return codes of
rehr_gather_gemm_f32 / rehr_gather_gemm_multi_f32.  tests/golden/wino_plan.json was recorded with the library as it was
before the family's host code was merged into wino_shared.h (tools/gen_golden_wino_plan.py); the routes are written by
hand in tests/wino_plan_cases.py.

A scratch that is one byte short (or null, or misaligned) is NOT an error for this family: the launch falls through to the
direct kernels.  On a machine without a device that launch fails like the Winograd one would, so REHR_EHIP in both
situations is the recorded and correct answer (unlike the weight gradient, whose short workspace is REHR_EINVAL); with
REHR_GG_WS_ONLY the two differ -- EHIP from the transform launch against OK for "nothing to prepare"."""
import ctypes as C
import json
import os

import pytest
import torch

from rehrseg_amd import lib as L
from wino_plan_cases import (EHIP, EINVAL, FLAGS, HALF_DOES_NOT_FIT, MULTI, MULTI_BLIND, OK, ROUTES, ROWS, W32P_FOUR_GROUPS, _make,
                             bind, bytes_by_flag, launch_codes, multi_codes)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wino_plan.json")
F23 = (ROUTES["flat8"], ROUTES["w32p"], ROUTES["big8"], ROUTES["small"])
F22 = (ROUTES["flat22"], ROUTES["region22"])
# the rejection predicates the table must reach: each a word of the fourth column of some row WITHOUT a route
REJECTIONS = ("sh != 1", "osh != 1", "obw != 0", "Ld != Dy", "three_taps", "plan_axis offs", "td.count > 3", "td.count > 256",
              "Lh < 6", "Lh < 8", "Lh < 12", "Lw > 64", "padding 640 > 637", "> 1.34", "> 1.78", "fill threshold",
              "need >= 2^32", "gg_src_fits", "N > 65535", "Npad % 64", "ah.nph != aw.nph", "sd != 1")


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _route(lib, args, flags=0):
    r = int(lib.rehr_gather_gemm_wino_route(C.byref(_make(args, flags))))
    assert 0 <= r < 1 << 16
    return r & 255, r >> 8


def test_table_is_not_one_sided():
    g = _golden()
    assert len(ROWS) >= 40 and set(g["rows"]) == {r[0] for r in ROWS} and set(g["multi"]) == {m[0] for m in MULTI}
    routes = [r[2] for r in ROWS]
    for name in ROUTES:
        assert routes.count(name) >= 3, name
    why = " | ".join(r[3] for r in ROWS if r[2] == "none")
    for word in REJECTIONS:
        assert word in why, word
    # F8_MAXSLOT cannot be exceeded behind Lh, Lw >= 6 (nine tiles per slice: (64 - 2) / 9 + 2 = 8 slices): the row
    # that reaches exactly eight stands for it
    assert any("= F8_MAXSLOT" in r[3] and r[2] == "flat8" for r in ROWS)
    taken = [m[2] for m in MULTI]
    assert taken.count("split") >= 3 and taken.count("flat-multi") >= 3 and taken.count(None) >= 12
    assert {len(m[1]) for m in MULTI} >= {2, 3, 4, 8}
    # The hand-written third column against the recorded library: with REHR_GG_WS_ONLY a call whose parts a Winograd
    # kernel takes launched a transform (EHIP where nothing can launch), one that none takes had nothing to prepare (OK);
    # a last part whose scratch is short, null or misaligned makes an all-or-none entry decline.
    for name, _, want in MULTI:
        if name in MULTI_BLIND:
            continue
        rec = g["multi"][name]
        assert rec["queried"][1] == (EHIP if want else OK), (name, rec)
        assert [rec[s][1] for s in ("one byte short", "null", "misaligned by 4")] == [OK] * 3, (name, rec)
    assert MULTI_BLIND < {m[0] for m in MULTI} and len(MULTI_BLIND) == 1
    codes = {c for r in g["rows"].values() for v in r["launch"]["0"].values() for c in v}
    assert codes == {EINVAL, -2, EHIP, OK}


def test_scratch_query_equals_the_recorded_one():
    lib = bind()
    g = _golden()["rows"]
    for name, args, _, _ in ROWS:
        assert bytes_by_flag(lib, args) == g[name]["bytes"], name
    assert lib.rehr_gather_gemm_wino_bytes(None) == 0 and lib.rehr_gather_gemm_wino_route(None) == 0


def test_route_query():
    """The hand-written routes; route 0 exactly when the recorded scratch size is 0; the size is what the route's
    transform needs; the flags do what they say."""
    lib = L.load()
    g = _golden()["rows"]
    for name, args, want, _ in ROWS:
        d = _make(args, 0)
        cpad = (d.Cin + 31) // 32 * 32
        assert _route(lib, args)[0] == ROUTES[want], (name, _route(lib, args))
        for f, bits in FLAGS.items():
            route, variant = _route(lib, args, bits)
            nbytes = g[name]["bytes"][f]
            assert (route == 0) == (nbytes == 0), (name, f)
            if route in F23:
                assert nbytes == d.td.count * 16 * d.Npad * cpad * 4, (name, f)
            elif route in F22:
                nphase = 4 if d.th.count == 4 else 1
                assert nbytes == nphase * d.td.count * 9 * d.Npad * cpad * 4, (name, f)
            if f == "NO_FLAT8":
                assert route not in (ROUTES["flat8"], ROUTES["flat22"]), name
            elif route != _route(lib, args)[0]:
                raise AssertionError((name, f, "only NO_FLAT8 changes a route"))
            if route == ROUTES["flat8"]:
                half = 2 if name in HALF_DOES_NOT_FIT else 1
                assert variant == {"FLAT8_HALF": half, "FLAT8_FULL": 2}.get(f, variant) and variant in (1, 2), (name, f)
            elif route == ROUTES["w32p"]:
                assert variant in (1, 2), (name, f)
                if f == "W32P_TWO_PER_CU":
                    assert variant == 1, name
                if f == "W32P_ONE_PER_CU":      # one 512-thread block needs 32-row regions
                    assert variant == (2 if name in W32P_FOUR_GROUPS else 1), name
            else:
                assert variant == 0, (name, f)
    variants = {(r[2], _route(lib, r[1])[1]) for r in ROWS}
    assert len(HALF_DOES_NOT_FIT) < sum(r[2] == "flat8" for r in ROWS) / 2
    assert variants >= {("flat8", 1), ("flat8", 2), ("w32p", 1), ("w32p", 2)}


def test_launch_codes_equal_the_recorded_ones():
    """Every row and multi-part row, every scratch situation, plain and with REHR_GG_WS_ONLY.  Runs only where there is no
    device: an accepted descriptor then meets "no device" (REHR_EHIP), not a launch on dummy pointers."""
    if torch.cuda.is_available():
        pytest.skip("dummy pointers: only where an accepted descriptor cannot be launched")
    lib = bind()
    g = _golden()
    for name, args, _, _ in ROWS:
        assert launch_codes(lib, args) == g["rows"][name]["launch"], name
    for name, parts, _ in MULTI:
        assert multi_codes(lib, parts) == g["multi"][name], name
    # WS_ONLY tells the routes apart where nothing can launch: the transform launch fails exactly when a kernel of the
    # family takes the descriptor with its scratch, and a short, null or misaligned scratch leaves nothing to prepare
    for name, _, want, _ in ROWS:
        rec = g["rows"][name]["launch"]["0"]
        if rec["queried"][0] == EINVAL:
            continue
        assert rec["queried"][1] == (EHIP if want != "none" else OK), name
        assert [rec[s][1] for s in ("one byte short", "null", "misaligned by 4")] == [OK] * 3, name
