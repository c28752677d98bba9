"""rehr_gather_gemm_wino_forms_f32 where nothing can launch: the symbol is declared on both sides of the binding,
malformed arguments are REHR_EINVAL, a call whose parts would not all run a Winograd kernel is REHR_ENOSUP (the caller
needs the panel), and a valid call reaches the launch -- REHR_EHIP without a device."""
import ctypes as C

import pytest
import torch

import wino_plan_cases as W
from rehrseg_amd import lib as L

NAME = "rehr_gather_gemm_wino_forms_f32"
WPTR = 0x7000000     # the parameter: a dummy aligned address nothing on the host dereferences


def _arr(parts, scratch=True):
    arr = (L.GatherGemmDesc * len(parts))()
    for i, a in enumerate(parts):
        d = W.desc(**a)
        if scratch:
            d.wino_ws, d.wino_ws_bytes = W.WS + 0x10000000 * i, W.formula_bytes(d)
        arr[i] = d
    return arr


def _call(arr, n, w=WPTR, D0=64, D1=64, T=27, dest_dim=0, dest_lo=0, src_lo=0):
    return int(L.load().rehr_gather_gemm_wino_forms_f32(arr, n, w, D0, D1, T, dest_dim, dest_lo, src_lo, None))


def test_symbol_is_declared_in_header_and_binding():
    assert NAME in L.declared_symbols()
    assert NAME in L.PROTOTYPES
    assert hasattr(L.load(), NAME)


def test_malformed_arguments_are_einval():
    big8 = [W.c3(2, 64, 64, (8, 16, 16))]
    assert _call(None, 1) == W.EINVAL
    assert _call(_arr(big8), 0) == W.EINVAL
    assert _call(_arr(big8), 9) == W.EINVAL
    assert _call(_arr(big8), 1, w=None) == W.EINVAL
    assert _call(_arr(big8), 1, w=WPTR + 2) == W.EINVAL
    assert _call(_arr(big8), 1, dest_dim=2) == W.EINVAL
    assert _call(_arr(big8), 1, dest_lo=-1) == W.EINVAL
    assert _call(_arr(big8), 1, D0=0) == W.EINVAL
    assert _call(_arr(big8), 1, dest_lo=1) == W.EINVAL            # rows [1, 65) of 64
    assert _call(_arr(big8), 1, D1=128, src_lo=65) == W.EINVAL    # channels [65, 129) of 128
    assert _call(_arr(big8), 1, T=9) == W.EINVAL                  # three depth taps in a one-slice kernel
    assert _call(_arr(big8), 1, T=28) == W.EINVAL                 # no whole number of 3 x 3 planes
    bad = _arr(big8)
    bad[0].Cin = 17                                               # what the launch rejects
    assert _call(bad, 1) == W.EINVAL
    bad = _arr(big8)
    bad[0].tw = W.taps(3, k0=1)                                   # taps 1..3 of a 3-wide kernel
    assert _call(bad, 1) == W.EINVAL


@pytest.mark.skipif(torch.cuda.is_available(), reason="with a device the valid calls launch (tests/test_onepass_forms_gpu.py)")
def test_routes_without_a_device():
    # no route: "plane 7x16"
    assert _call(_arr([W.c3(2, 32, 32, (8, 7, 16))]), 1, D0=32, D1=32) == W.ENOSUP
    # a route, but no scratch / too small a scratch
    assert _call(_arr([W.c3(2, 64, 64, (8, 16, 16))], scratch=False), 1) == W.ENOSUP
    short = _arr([W.c3(2, 64, 64, (8, 16, 16))])
    short[0].wino_ws_bytes -= 1
    assert _call(short, 1) == W.ENOSUP
    # valid: every family reaches its launch
    assert _call(_arr([W.c3(2, 64, 64, (8, 16, 16))]), 1) == W.EHIP                                     # big8
    assert _call(_arr([W.c3(2, 32, 32, (8, 8, 16))]), 1, D0=32, D1=32) == W.EHIP                        # small
    assert _call(_arr([W.t2(2, 128, 64, (4, 16, 16))]), 1, D0=128, D1=64, T=48, dest_dim=1) == W.EHIP   # region22
    assert _call(_arr(W._split(3)), 3, T=432) == W.EHIP                                                 # joint split
    assert _call(_arr(W._phases(4)), 4, D0=512, D1=128, T=48, dest_dim=1) == W.EHIP                     # joint phases
    # a sub-range of a wider parameter
    assert _call(_arr([W.c3(2, 64, 64, (8, 16, 16))]), 1, D0=128, D1=256, dest_lo=64, src_lo=192) == W.EHIP
