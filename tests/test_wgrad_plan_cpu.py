"""The host side of the weight-gradient family is pinned without a device: which route a descriptor takes and with what
plan shows in the workspace size, and the size the query reports is the size the launch insists on."""
import ctypes as C
import json
import os

import pytest

from rehrseg_amd import lib as L
from wgrad_plan_cases import ROWS, desc

EINVAL, ENOSUP, EHIP = -1, -2, -3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_plan.json")


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)["rows"]


def test_table_reaches_every_route_and_error_code():
    """The recorded values themselves show that the table is not one-sided (a table that only ever met the slab kernel
    would pin nothing about the route decision)."""
    g = _golden()
    assert len(ROWS) >= 30 and set(g) == {name for name, _ in ROWS}
    f32 = [r["f32_bytes"] for r in g.values()]
    bf16 = [r["bf16_bytes"] for r in g.values()]
    for codes in (f32, bf16):
        assert EINVAL in codes and ENOSUP in codes and sum(c > 0 for c in codes) >= 20
    assert 8 <= sum(r["uses_winograd"] for r in g.values()) <= len(g) - 8
    # the example of the four routes on one shape: 32 x 32 channels, N = 2, lattice 4 x 16 x 16, 3 x 3 x 3 taps
    assert (g["wino 32x32"]["f32_bytes"], g["direct 32x32 3x3x3"]["f32_bytes"]) == (196800, 442880)
    assert (g["wino 32x32"]["bf16_bytes"], g["direct 32x32 3x3x3"]["bf16_bytes"]) == (442368, 221184)


def test_wgrad_queries_equal_the_recorded_plans():
    lib = L.load()
    g = _golden()
    for name, args in ROWS:
        d = desc(**args)
        got = {"f32_bytes": int(lib.rehr_wgrad_workspace_bytes(C.byref(d))),
               "uses_winograd": int(lib.rehr_wgrad_uses_winograd(C.byref(d))),
               "bf16_bytes": int(lib.rehr_wgrad_bf16_workspace_bytes(C.byref(d)))}
        assert got == g[name], (name, got, g[name])
        # a size query may come before the destination is allocated
        d.dst = None
        assert int(lib.rehr_wgrad_workspace_bytes(C.byref(d))) == g[name]["f32_bytes"], name
        assert int(lib.rehr_wgrad_uses_winograd(C.byref(d))) == g[name]["uses_winograd"], name
        assert int(lib.rehr_wgrad_bf16_workspace_bytes(C.byref(d))) == g[name]["bf16_bytes"], name


def test_wgrad_launch_insists_on_the_size_the_query_reports():
    """For every accepted row: one byte less than the query is REHR_EINVAL, the queried size is accepted (REHR_EHIP: the
    launch found no device), a null workspace is REHR_EINVAL; a rejected row is rejected by the launch with the same code.
    Runs only where there is no device: an accepted descriptor then meets "no device", not a launch on dummy pointers.
    (A query can succeed where the launch then refuses splits > 65535.  No descriptor gets there today -- the slab plan
    stops at 1024 splits, the fp32 brick plan at 65535, the bf16 brick plan at 256 -- so the table has no such row.)"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("dummy pointers: only where an accepted descriptor cannot be launched")
    lib = L.load()
    entries = ((lib.rehr_wgrad_workspace_bytes, lib.rehr_wgrad_f32), (lib.rehr_wgrad_bf16_workspace_bytes, lib.rehr_wgrad_bf16))
    accepted = 0
    for name, args in ROWS:
        for query, launch in entries:
            d = desc(**args)
            need = int(query(C.byref(d)))
            d.workspace = 0x10000
            if need < 0:
                d.workspace_bytes = 1 << 40
                assert launch(C.byref(d), None) == need, (name, launch.__name__)
                continue
            accepted += 1
            d.workspace_bytes = need - 1
            assert launch(C.byref(d), None) == EINVAL, (name, launch.__name__, "one byte short")
            d.workspace_bytes = need
            assert launch(C.byref(d), None) == EHIP, (name, launch.__name__, "queried size")
            d.workspace = None
            assert launch(C.byref(d), None) == EINVAL, (name, launch.__name__, "null workspace")
            d.workspace, d.dst = 0x10000, None
            assert launch(C.byref(d), None) == EINVAL, (name, launch.__name__, "null dst")
    assert accepted >= 60
