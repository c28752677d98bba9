"""Every row of tests/thin_kernel_cases.py lands in the launch regime its table entry claims -- checked without a device.

The route (matrix cores or vector kernels, halo brick or strips) and the block counts come from the library's own
queries: rehr_conv_small_cin_{fwd,wgrad}_on_mfma, and the workspace sizes, which are a block count times a known slab
(rehr_conv_small_cin_wgrad_workspace_bytes: grid.x * N * Cin * Cout * NTP * 4 on the matrix cores, blocks * (Cin * T + 1)
* 64 * 4 on the vector route; rehr_conv_small_cout_wgrad_workspace_bytes: (strips * Cout * Cin * T + 4096) * 4).  The
forward geometry has no query; thin_kernel_cases restates it and the claimed tuple must be what the restatement gives."""
import ctypes as C

import pytest

from rehrseg_amd import lib as L
import thin_kernel_cases as T
from thin_kernel_cases import IM2COL, IM2COL_GEMM, MFWD, MWG, OUT, VFWD, VWG, desc, desc_args, ids


def _q(name, r, **over):
    d = desc(**desc_args(r, **over))
    return int(getattr(L.load(), name)(C.byref(d)))


def _routes(r):
    return _q("rehr_conv_small_cin_fwd_on_mfma", r), _q("rehr_conv_small_cin_wgrad_on_mfma", r)


@pytest.mark.parametrize("r", VFWD, ids=ids(VFWD))
def test_vector_forward_rows(r):
    assert _routes(r)[0] == 0
    plain, stats = r["regime"]
    assert T.vfwd_geometry(r, False) == plain
    if stats is not None:
        assert T.vfwd_geometry(r, True) == stats
    assert r["Cin"] * T._T(r) * r["Cout"] * 4 <= 150 * 1024      # the vector kernel's own bound


def test_vector_forward_rows_cover_the_regimes():
    g = [r["regime"] for r in VFWD]
    assert {x[0][0] for x in g} == {1, 2, 4}                       # wave groups 1, 2, 4
    assert any(x[1] is not None and x[1][5] > 0 for x in g)        # persistent walk under the 512 / N cap
    assert any(x[0][5] > 0 for x in g)                             # ... and under the 4096 / N cap
    assert any(x[0][6] for x in g)                                 # more than 48 KB of dynamic LDS
    assert all(x[0][3] < x[0][1] for x in g[:3])                   # partial last tiles


@pytest.mark.parametrize("r", VWG, ids=ids(VWG))
def test_vector_weight_gradient_rows(r):
    assert _routes(r)[1] == 0
    assert (r["Cout"] == 16) == (r["via"] == "ops")                # ops.conv_wgrad sends Cout % 32 != 0 there by itself
    assert T.vwg_geometry(r) == r["regime"]
    assert _q("rehr_conv_small_cin_wgrad_workspace_bytes", r) == T.vwg_workspace_bytes(r)


def test_vector_weight_gradient_rows_cover_the_regimes():
    g = [r["regime"] for r in VWG]
    assert {x[0] for x in g} == {"<8>", "<40>"}
    assert any(x[2] < 4 for x in g) and any(x[6] > 0 for x in g) and any(x[4] > 64 and x[5] < x[4] for x in g)
    assert {r["Cout"] for r in VWG} == {16, 32, 64}


@pytest.mark.parametrize("r", IM2COL, ids=ids(IM2COL))
def test_im2col_rows(r):
    kpad, items, strided = r["regime"]
    assert kpad % 4 == 0 and 0 <= kpad - r["Cin"] * T._T(r)
    assert items == r["N"] * T._ovox(r) * (kpad // 4) and strided == (items > 4096 * 256)


@pytest.mark.parametrize("r", IM2COL_GEMM, ids=ids(IM2COL_GEMM))
def test_im2col_gemm_rows(r):
    assert r["Cout"] % 32 == 0 and _routes(r)[1] == 0              # ops.conv_wgrad: columns + the 1x1x1 weight gradient


@pytest.mark.parametrize("r", MFWD, ids=ids(MFWD))
def test_matrix_core_forward_rows(r):
    assert _routes(r)[0] == 1
    assert T.mfwd_geometry(r) == r["regime"]


@pytest.mark.parametrize("r", MWG, ids=ids(MWG))
def test_matrix_core_weight_gradient_rows(r):
    assert _routes(r)[1] == 1
    assert T.mwg_geometry(r) == r["regime"]
    assert _q("rehr_conv_small_cin_wgrad_workspace_bytes", r) == T.mwg_workspace_bytes(r)


def test_matrix_core_rows_cover_the_regimes():
    assert {(r["Cout"], r["regime"][0]) for r in MWG} >= {(32, 1), (32, 2), (32, 10), (64, 1), (64, 2), (64, 10)}
    for rows in (MFWD, MWG):
        assert sum(1 for r in rows if r["regime"][3] > 1 and r["regime"][4] < r["regime"][3]) >= 2
    assert {r["K"][2] for r in MFWD} >= {1, 2, 5, 8} and {r["stride"][1:] for r in MFWD} >= {(2, 1), (1, 2), (2, 2)}
    assert _routes([r for r in MWG if r["K"] == (1, 3, 9)][0]) == (0, 1)


@pytest.mark.parametrize("r", OUT, ids=ids(OUT))
def test_thin_output_rows(r):
    assert T.out_geometry(r) == r["regime"]
    assert _q("rehr_conv_small_cout_wgrad_workspace_bytes", r) == T.out_workspace_bytes(r)
    if "pairs16" in r:
        assert T.pairs16(r) == r["pairs16"]
    T_ = T._T(r)
    assert T_ * (2 if r["Cout"] <= 2 else 4) * r["Cin"] * 4 <= 64 * 1024   # forward / input gradient take the row


def test_thin_output_rows_reach_every_kernel():
    fwd = {r["regime"][0] for r in OUT}
    wg = {r["regime"][1] for r in OUT}
    cg = {f"cg<{co},{c}>" for co in (2, 4) for c in (4, 8, 16)}
    assert fwd == cg | {"plain<2>", "plain<4>"}
    assert wg == cg | {"plain<2>", "plain<4>", "halo<2>", "halo<4>", "rows<5>"}
    assert {r["Cout"] for r in OUT} == {1, 2, 3, 4}
    assert any(r["regime"][1] == "rows<5>" and r["regime"][3:] == (2, 1) for r in OUT)      # two bricks per block, last: one
    assert any(r["regime"][1] == "plain<4>" and r["regime"][3:] == (2, 1) for r in OUT)     # two rows per strip, last: one
    assert sum(1 for r in OUT if r.get("pairs16")) == 8
