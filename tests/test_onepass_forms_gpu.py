"""One-pass weight forms (rehr_gather_gemm_wino_forms_f32): the transform-domain weights of the fp32 Winograd kernels
written straight from the parameter must be, byte for byte, what the panel path (rehr_pack_weights_f32, then the
transform launch of REHR_GG_WS_ONLY) writes into the same scratch -- padding included -- for every route, both
orientations, channel sub-ranges, tap selections and multi-part calls.  End to end, ops.fused_conv3d and a FLAVR step
give the same bits with hip_backend.USE_ONEPASS_FORMS on and off."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import wino_plan_cases as W
from oracle.detinit import det_tensor
from rehrseg_amd import hip_backend as be
from rehrseg_amd import lib as L
from rehrseg_amd import ops
from rehrseg_amd.models.FLAVR.FLAVR_arch import UNet_3D_3D

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
SENTINEL = 12345.0     # what neither path writes stays what it was, in both buffers


def _phases22(N, Cin, Cout, plane, kd=3):
    """The four output phases of a (kd, 4, 4) stride-(1, 2, 2) transposed convolution, as ops._phased_gather issues them."""
    out = []
    for ph in range(2):
        for pw in range(2):
            out.append(W.t2(N, Cin, Cout, plane, kd=kd, obh=ph, obw=pw, th=W.taps(2, off0=ph, offs=-1, k0=1 - ph, ks=2),
                            tw=W.taps(2, off0=pw, offs=-1, k0=1 - pw, ks=2)))
    return out


MIRROR = W.taps(3, off0=2, offs=-1, k0=0, ks=1)    # with bh = -1: source offsets +1, 0, -1 take weights 0, 1, 2

# (name, parts (desc() arguments), routes of the parts, weight shape (D0, D1, KD, KH, KW), dest_dim, dest_lo, src_lo)
CASES = [
    ("big8", [W.c3(2, 64, 64, (8, 16, 16))], ["big8"], (64, 64, 3, 3, 3), 0, 0, 0),
    ("w32p", [W.c3(2, 32, 32, (8, 16, 16))], ["w32p"], (32, 32, 3, 3, 3), 0, 0, 0),
    ("small", [W.c3(2, 32, 32, (8, 8, 16))], ["small"], (32, 32, 3, 3, 3), 0, 0, 0),
    ("flat8 kd3", [W.c3(32, 256, 256, (4, 12, 12))], ["flat8"], (256, 256, 3, 3, 3), 0, 0, 0),
    ("flat8 kd1", [W.c3(32, 256, 256, (4, 12, 12), kd=1)], ["flat8"], (256, 256, 1, 3, 3), 0, 0, 0),
    ("region22 2-tap phase", [W.t2(2, 128, 64, (4, 16, 16))], ["region22"], (128, 64, 3, 4, 4), 1, 0, 0),
    ("region22 4-tap stride 2", [W.s4(1, 64, 64, (8, 32, 32))], ["region22"], (64, 64, 3, 4, 4), 0, 0, 0),
    ("flat22", [W.t2(32, 512, 256, (4, 12, 12))], ["flat22"], (512, 256, 3, 4, 4), 1, 0, 0),
    # ---- edges
    ("Cin 48 big8", [W.c3(2, 48, 64, (8, 16, 16))], ["big8"], (64, 48, 3, 3, 3), 0, 0, 0),
    ("Cin 48 small", [W.c3(2, 48, 32, (8, 8, 16))], ["small"], (32, 48, 3, 3, 3), 0, 0, 0),
    ("Cout 96", [W.c3(2, 64, 96, (8, 16, 16))], ["w32p"], (96, 64, 3, 3, 3), 0, 0, 0),
    ("Cout 40 Npad 64", [W.c3(2, 64, 40, (8, 16, 16), Npad=64)], ["big8"], (40, 64, 3, 3, 3), 0, 0, 0),
    ("input gradient, mirrored taps", [W.c3(2, 64, 128, (8, 16, 16), th=MIRROR, tw=MIRROR, td=W.taps(3, off0=2, offs=-1))],
     ["big8"], (64, 128, 3, 3, 3), 1, 0, 0),
    ("concat half 0 of 256", [W.c3(2, 64, 128, (8, 16, 16), th=MIRROR, tw=MIRROR)], ["big8"], (64, 256, 3, 3, 3), 1, 0, 0),
    ("concat half 1 of 256", [W.c3(2, 64, 128, (8, 16, 16), th=MIRROR, tw=MIRROR)], ["big8"], (64, 256, 3, 3, 3), 1, 128, 0),
    ("source sub-range", [W.c3(2, 128, 64, (8, 16, 16))], ["big8"], (64, 256, 3, 3, 3), 0, 0, 128),
    ("transposed, destination sub-range", [W.s4(1, 64, 64, (8, 32, 32))], ["region22"], (128, 64, 3, 4, 4), 0, 64, 0),
    ("three-part depth-tap split", W._split(3), ["big8"] * 3, (64, 64, 48, 3, 3), 0, 0, 0),
    ("four phases, one grid", W._phases(4), ["flat22"] * 4, (512, 128, 3, 4, 4), 1, 0, 0),
    ("four phases, a launch each", _phases22(2, 128, 64, (4, 16, 16)), ["region22"] * 4, (128, 64, 3, 4, 4), 1, 0, 0),
]


def _ptr(t):
    return t.data_ptr()


def _descs(parts, dummy, wp, scratch):
    arr = (L.GatherGemmDesc * len(parts))()
    for i, a in enumerate(parts):
        d = W.desc(**a)
        d.x1 = _ptr(dummy)
        d.x2 = _ptr(dummy) if d.x2 else None
        d.y = _ptr(dummy)
        d.wp = wp
        d.wino_ws, d.wino_ws_bytes = _ptr(scratch[i]), scratch[i].numel() * 4
        arr[i] = d
    return arr


@pytest.mark.parametrize("name,parts,routes,wshape,dest_dim,dest_lo,src_lo", CASES, ids=[c[0] for c in CASES])
def test_forms_from_the_parameter_equal_the_panel_path(name, parts, routes, wshape, dest_dim, dest_lo, src_lo):
    dev = torch.device("cuda:0")
    lib = L.load()
    w = torch.randn(wshape, generator=torch.Generator().manual_seed(len(name))).to(dev)
    d0 = W.desc(**parts[0])
    A, B, T = d0.Cout, d0.Cin, wshape[2] * wshape[3] * wshape[4]
    part = None
    if dest_lo or wshape[dest_dim] != A:
        part = (dest_dim, dest_lo, A)
    if src_lo or wshape[1 - dest_dim] != B:
        assert part is None
        part = (1 - dest_dim, src_lo, B)
    dummy = torch.zeros(64, device=dev)
    sizes = [W.formula_bytes(W.desc(**a)) // 4 for a in parts]
    want = [torch.full((n,), SENTINEL, device=dev) for n in sizes]
    got = [torch.full((n,), SENTINEL, device=dev) for n in sizes]

    # today's path: the panel of the (narrowed) parameter, then the transforms of the call
    panel = be.pack_weights(w, A, d0.Npad, B, T, dest_dim == 1, part=part)
    arr = _descs(parts, dummy, _ptr(panel), want)
    if len(parts) == 1:     # the table's route is the route of the library (multi-part rows: wino_plan_cases.MULTI)
        assert be.wino_route(arr[0])[0] == W.ROUTES[routes[0]]
        assert lib.rehr_gather_gemm_wino_bytes(C.byref(arr[0])) == sizes[0] * 4
    for i in range(len(parts)):
        arr[i].flags = L.GG_WS_ONLY
    L.check(lib.rehr_gather_gemm_multi_f32(arr, len(parts), None), "panel path")

    # one pass: wp is not read (the scratch stands in for it: non-null, aligned)
    arr2 = _descs(parts, dummy, _ptr(got[0]), got)
    L.check(lib.rehr_gather_gemm_wino_forms_f32(arr2, len(parts), _ptr(w), wshape[0], wshape[1], T, dest_dim, dest_lo,
                                                src_lo, None), "one pass")
    torch.cuda.synchronize()
    for i in range(len(parts)):
        assert (want[i] != SENTINEL).any()
        assert torch.equal(got[i], want[i]), (name, i)


def test_parts_without_a_winograd_kernel_are_refused():
    """No route, no scratch: REHR_ENOSUP and nothing written."""
    dev = torch.device("cuda:0")
    lib = L.load()
    w = torch.randn(32, 32, 3, 3, 3).to(dev)
    dummy = torch.zeros(64, device=dev)
    ws = [torch.full((1 << 16,), SENTINEL, device=dev)]
    arr = _descs([W.c3(2, 32, 32, (8, 7, 16))], dummy, _ptr(dummy), ws)       # "plane 7x16": no route
    assert lib.rehr_gather_gemm_wino_forms_f32(arr, 1, _ptr(w), 32, 32, 27, 0, 0, 0, None) == W.ENOSUP
    arr = _descs([W.c3(2, 32, 32, (8, 16, 16))], dummy, _ptr(dummy), ws)
    arr[0].wino_ws_bytes = 64                                                # a route, but the scratch is too small
    assert lib.rehr_gather_gemm_wino_forms_f32(arr, 1, _ptr(w), 32, 32, 27, 0, 0, 0, None) == W.ENOSUP
    torch.cuda.synchronize()
    assert bool((ws[0] == SENTINEL).all())


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last_3d)


def _conv_both_ways(run):
    outs = []
    for on in (True, False):
        be.USE_ONEPASS_FORMS = on
        try:
            n0, w0 = be.onepass_form_calls, be.wino_launches
            outs.append(run())
            outs[-1].append((be.onepass_form_calls - n0, be.wino_launches - w0))
        finally:
            be.USE_ONEPASS_FORMS = True
    return outs


E2E = [
    # (name, N, Cin, Cout, (D, H, W), x2 channels, transposed)
    ("big8", 2, 64, 64, (8, 16, 16), 0, False),
    ("flat22", 32, 512, 256, (4, 12, 12), 0, True),
    ("concat 128 -> 64 +x2", 2, 128, 64, (4, 16, 16), 64, False),
]


@pytest.mark.parametrize("name,N,Cin,Cout,dims,c2,transposed", E2E, ids=[c[0] for c in E2E])
def test_fused_conv3d_same_bits_with_and_without_the_panel(name, N, Cin, Cout, dims, c2, transposed):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(11)
    c1 = Cin - c2
    x1 = _cl(torch.randn(N, c1, *dims, generator=g).to(dev))
    x2 = _cl(torch.randn(N, c2, *dims, generator=g).to(dev)) if c2 else None
    if transposed:
        w0 = torch.randn(Cin, Cout, 3, 4, 4, generator=g).to(dev) * 0.05
        kw = dict(stride=(1, 2, 2), padding=(1, 1, 1), transposed=True)
    else:
        w0 = torch.randn(Cout, Cin, 3, 3, 3, generator=g).to(dev) * 0.05
        kw = dict(stride=1, padding=1)

    def run():
        w = torch.nn.Parameter(w0.clone())
        a = x1.clone().requires_grad_()
        b = x2.clone().requires_grad_() if x2 is not None else None
        y = ops.fused_conv3d(a, w, None, x2=b, **kw)
        dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(3)).to(dev)
        y.backward(_cl(dy) * 1.0)
        torch.cuda.synchronize()
        return [y.detach(), a.grad, w.grad] + ([b.grad] if b is not None else [])

    new, old = _conv_both_ways(run)
    assert new[-1][0] >= 2 and old[-1][0] == 0          # forward and input gradient(s) took the one-pass entry
    assert new[-1][1] == old[-1][1]                     # the Winograd launch counter means what it meant
    for a, b in zip(new[:-1], old[:-1]):
        assert torch.equal(a, b), name


def test_flavr_step_same_gradients_with_and_without_the_panel():
    dev = torch.device("cuda:0")
    g = np.load(os.path.join(GOLD, "flavr_c1_n8.npz"))
    ic, ni, no, unc, hw = (int(v) for v in g["meta"])
    assert not unc
    ref = UNet_3D_3D(ic, "unet_18", ni, no)
    sd = {k: det_tensor(k, tuple(v.shape)) for k, v in ref.state_dict().items()}
    x = torch.from_numpy(g["x"]).to(dev)
    tgt = torch.from_numpy(g["target"]).to(dev)

    def run():
        m = UNet_3D_3D(ic, "unet_18", ni, no)
        m.load_state_dict(sd)
        m = m.to(dev)
        opt = torch.optim.Adam(m.parameters(), lr=1e-4)
        out = m(x.clone())
        out = out[0] if isinstance(out, (tuple, list)) else out
        (out - tgt).abs().mean().backward()
        grads = [p.grad.clone() for p in m.parameters() if p.grad is not None]     # (unused heads take none)
        assert len(grads) > 40
        opt.step()
        torch.cuda.synchronize()
        return [out.detach()] + grads + [p.detach() for p in m.parameters()]

    new, old = _conv_both_ways(run)
    assert new[-1][0] > 10 and old[-1][0] == 0
    assert new[-1][1] == old[-1][1]
    assert len(new) == len(old)
    for i, (a, b) in enumerate(zip(new[:-1], old[:-1])):
        assert torch.equal(a, b), i
