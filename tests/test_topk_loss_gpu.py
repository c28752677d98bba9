"""Top-k cross-entropy + soft Dice on the device (csrc/seg_loss_topk.hip: rehr_seg_topk_{fwd,bwd}_f32; DESIGN section
3.20) against tests/topk_oracle.py in fp64, at the smallest shapes where the kernels can go wrong.

Bars, those of tests/test_seg_loss_gpu.py: value 1e-5 relative, logit gradient 1e-4 of the largest oracle gradient
magnitude.  The device selects on its fp32 map, the oracle on an fp64 one: a map element whose oracle value lies within
1e-5 * max(|t|, 1e-6) of the threshold t may fall on either side, so its voxel is left out of the gradient comparison
(never of the value).  At most max(2, K / 200) elements may be left out; that is asserted on the oracle alone, before
the device is touched.  Every comparison prints "name measured / bar" before it asserts."""
import functools

import pytest
import torch

import topk_oracle as to
from rehrseg_amd import hip_backend as hb
from rehrseg_amd import lib as L
from rehrseg_amd import ops
from rehrseg_amd.train_steps import train_segsr_step
from rehrseg_amd.utils import augment as A
from rehrseg_amd.utils import seg_utils as su
from test_segmodel_cpu import build

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(2, 2, 3, 5, 7),        # S = 105: no multiple of 4; M = 210 < the 256 bins of one radix histogram
          (1, 3, 2, 9, 13),       # N = 1: the map with an uncertainty is still (1, 1, ...)
          (3, 4, 1, 4, 33),       # N = 3: the 9 S map; C = 4
          (2, 2, 6, 10, 12),      # tests/test_seg_loss_gpu.py's
          (2, 2, 16, 40, 48)]     # M = 61 440 / 122 880: several blocks, several radix digits
KS = [10, 1, 37.5, 100]
PLAN = dict(n_stages=3, features_per_stage=[32, 64, 96], kernel_sizes=[[1, 3, 3], [1, 3, 3], [3, 3, 3]],
            strides=[[1, 1, 1], [1, 2, 2], [2, 2, 2]], n_conv_per_stage=[2, 2, 2], n_conv_per_stage_decoder=[2, 2],
            num_classes=2, upscale=4)   # tests/test_train_steps_gpu.py's


def _close(name, err, bar):
    print(f"{name}: {err:.3e} / {bar:.3e}")
    assert err <= bar, f"{name}: error {err:.3e} > bar {bar:.3e}"


def _node(t):
    assert t.grad_fn is not None and type(t.grad_fn).__name__ == "_FusedDCTopKBackward", \
        f"not the fused path: {type(t.grad_fn).__name__}"


@functools.lru_cache(maxsize=None)
def _inputs(i):
    N, Cc, D, H, W = SHAPES[i]
    g = torch.Generator().manual_seed(100 + i)
    logits = torch.randn(SHAPES[i], generator=g) * 2
    target = torch.randint(0, Cc, (N, 1, D, H, W), generator=g).float()
    unc = 1 - torch.randint(0, 256, (N, 1, D, H, W), generator=g).float() / 255.0 * 0.99
    return logits, target, unc


@functools.lru_cache(maxsize=None)
def _oracle(i, k, with_unc):
    """Computed once per case and shared; nothing changes it."""
    logits, target, unc = _inputs(i)
    return to.dc_and_topk(logits, target, unc if with_unc else None, k=k)


def _left_out(o):
    """The oracle's ambiguous map elements, their number checked against the cap, as a mask over the (N, D, H, W) voxels."""
    amb = to.ambiguous(o["m"], o["K"])
    n, cap = int(amb.sum()), max(2, o["K"] / 200)
    print(f"ambiguous map elements: {n} / {cap:g} (K = {o['K']}, t = {o['t']:.6g})")
    assert n <= cap
    return amb if amb.dim() == 4 else amb.any(0)          # m[j, i, ...]: the voxel (i, ...) of the logits


def _flat(t, N):
    return t.reshape(N, -1).contiguous()


# ----------------------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("with_unc", [False, True])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_device_matches_oracle(i, k, with_unc):
    o = _oracle(i, k, with_unc)
    skip = _left_out(o)                                   # before the device is touched
    logits, target, unc = _inputs(i)
    lg = logits.to(DEV).requires_grad_(True)
    val = su._build_loss(topk=k)(lg, target.to(DEV), unc.to(DEV) if with_unc else None)
    _node(val)
    val.backward()
    ref = float(o["value"])
    _close("value", abs(float(val.detach()) - ref), 1e-5 * abs(ref))
    err = (lg.grad.double().cpu() - o["grad"]).abs() * (~skip)[:, None]
    _close("gradient", float(err.max()), 1e-4 * float(o["grad"].abs().max()))


def test_upstream_gradient_of_three():
    o = _oracle(3, 10, True)
    skip = _left_out(o)
    logits, target, unc = _inputs(3)
    lg = logits.to(DEV).requires_grad_(True)
    val = su._build_loss(topk=10)(lg, target.to(DEV), unc.to(DEV))
    (val * 3.0).backward()                                # goes through the device scalar
    err = (lg.grad.double().cpu() / 3.0 - o["grad"]).abs() * (~skip)[:, None]
    _close("gradient / 3", float(err.max()), 1e-4 * float(o["grad"].abs().max()))


def _launch(logits, target, unc, K, workspace=None, w=(1.0, 1.0, 1e-5, False)):
    """The launch layer directly: (stats, workspace, dlogits) for an upstream gradient of 1."""
    N = logits.shape[0]
    t, u = _flat(target, N).to(DEV), (None if unc is None else _flat(unc, N).to(DEV))
    stats, ws = hb.seg_topk_fwd(logits, t, u, K, workspace)
    dl = hb.seg_topk_bwd(logits, t, u, K, stats, ws, *w, torch.ones(1, device=DEV))
    return stats, ws, dl


@pytest.mark.parametrize("with_unc", [False, True])
def test_channel_sliced_logits(with_unc):
    """logits that are channels 1..2 of a six-channel NDHWC tensor: ld = 6."""
    o = _oracle(3, 10, with_unc)
    skip = _left_out(o)
    logits, target, unc = _inputs(3)
    unc = unc if with_unc else None
    N, Cc, D, H, W = SHAPES[3]
    wide = ops.to_cl(torch.full((N, 6, D, H, W), 1e30).to(DEV))       # a neighbour read by mistake would show
    wide[:, 1:3] = logits.to(DEV)
    sliced = wide[:, 1:3]
    assert hb._ndhwc_ld(sliced, "test") == 6 and not sliced.permute(0, 2, 3, 4, 1).is_contiguous()
    stats, _, dl = _launch(sliced, target, unc, o["K"])
    dense = _launch(ops.to_cl(logits.to(DEV)), target, unc, o["K"])
    n = N * Cc * 3
    assert torch.equal(stats[n + 1:n + 3], dense[0][n + 1:n + 3]) and torch.equal(stats[-1:], dense[0][-1:])
    assert torch.allclose(stats, dense[0], rtol=1e-12, atol=0)        # atomic sums: the order of three blocks
    assert dl.shape == sliced.shape and dl.permute(0, 2, 3, 4, 1).is_contiguous()
    err = (dl.double().cpu() - o["grad"]).abs() * (~skip)[:, None]
    _close("sliced gradient", float(err.max()), 1e-4 * float(o["grad"].abs().max()))
    assert bool((wide[:, 0] == 1e30).all()) and bool((wide[:, 3:] == 1e30).all())


# ----------------------------------------------------------------------------- 2. the selection is exact
@pytest.mark.parametrize("with_unc", [False, True])
@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_selection_is_exact_on_the_device_map(i, k, with_unc):
    logits, target, unc = _inputs(i)
    unc = unc if with_unc else None
    N, Cc = SHAPES[i][:2]
    S = logits[0, 0].numel()
    M = (N * N if with_unc else N) * S
    K = int(M * k / 100)
    lg = ops.to_cl(logits.to(DEV))
    t, u = _flat(target, N).to(DEV), (None if unc is None else _flat(unc, N).to(DEV))
    stats, ws = hb.seg_topk_fwd(lg, t, u, K)
    m = hb.seg_topk_map(ws, N, S, with_unc).clone()
    assert m.numel() == M and tuple(m.shape) == ((N, N, S) if with_unc else (N, S))
    # the map is the oracle's, in fp32: the fast log's absolute error near 1 (2^-21.4) and the rounding of the
    # exponentials' sum (another 2^-21 in the log), then the roundings of the subtraction and of the product with the
    # uncertainty (2^-23 of the value each)
    ref_m = _oracle(i, k, with_unc)["m"].reshape(-1)
    _close("map", float((m.double().cpu().reshape(-1) - ref_m).abs().max()), 1e-6 + 2.0 ** -22 * float(ref_m.abs().max()))
    thr = torch.sort(m.reshape(-1)).values[M - K]
    n = N * Cc * 3
    got_t, n_gt, n_eq, above = stats[-1], stats[n + 1], stats[n + 2], stats[n + 3]
    assert torch.equal(got_t.to(torch.float32).view(torch.int32), thr.view(torch.int32)) and \
        float(got_t) == float(thr)                                            # bit for bit
    assert int(n_gt) == int((m > thr).sum()) and int(n_eq) == int((m == thr).sum())
    assert int(n_gt) < K <= int(n_gt) + int(n_eq)
    if k == 100:
        assert int(n_gt) == M - int(n_eq) and float(got_t) == float(m.min())
    want = float(m[m > thr].double().sum())
    _close("sum above the threshold", abs(float(above) - want), 1e-12 * max(want, 1e-30))
    again, _ = hb.seg_topk_fwd(lg, t, u, K)
    assert torch.equal(again[n + 1:n + 3], stats[n + 1:n + 3]) and torch.equal(again[-1:], stats[-1:])


# ----------------------------------------------------------------------------- 3. ties
def test_tie_case_on_the_device():
    logits, target = to.tie_case()
    o = to.dc_and_topk(logits, target, None, k=50, weight_dice=0.0)
    lg = logits.to(DEV).requires_grad_(True)
    val = su._build_loss(weight_dice=0, topk=50)(lg, target.to(DEV))
    _node(val)
    val.backward()
    _close("tie value", abs(float(val.detach()) - 12.5), 1e-6)
    stats, ws, _ = _launch(ops.to_cl(logits.to(DEV)), target, None, 16)
    assert stats[-4:].tolist() == [5.0, 27.0, 200.0, 0.0] and not bool(torch.signbit(stats[-1]))
    m = hb.seg_topk_map(ws, 1, 32, False)
    assert not bool(torch.signbit(m).any())               # zeros enter the map as +0
    tied = (o["m"] == 0).reshape(-1)
    g = lg.grad.double().cpu()[0].reshape(2, -1)
    for c in range(2):
        assert float(g[c][tied].max() - g[c][tied].min()) == 0.0
    _close("tie gradient", float((lg.grad.double().cpu() - o["grad"]).abs().max()), 1e-4 * float(o["grad"].abs().max()))


def test_unsaturated_ties_share_the_gradient():
    """Every voxel the same logits and label: the whole map is one value, n_gt = 0, n_eq = M, and every voxel carries
    weight K / M.  (The tie case above saturates: softmax - onehot is 0 at its tied voxels.)"""
    N, Cc, D, H, W = 2, 3, 2, 5, 7
    logits = torch.tensor([1.0, -0.5, 0.25]).view(1, 3, 1, 1, 1).expand(N, Cc, D, H, W).contiguous()
    target = torch.zeros(N, 1, D, H, W)
    o = to.dc_and_topk(logits, target, None, k=37.5)
    assert o["n_gt"] == 0 and o["n_eq"] == 140 and o["K"] == 52
    lg = logits.to(DEV).requires_grad_(True)
    val = su._build_loss(topk=37.5)(lg, target.to(DEV))
    val.backward()
    _close("all-tied value", abs(float(val.detach()) - float(o["value"])), 1e-5 * abs(float(o["value"])))
    g = lg.grad.double().cpu()
    _close("all-tied gradient", float((g - o["grad"]).abs().max()), 1e-4 * float(o["grad"].abs().max()))
    assert float(g[:, 0].max() - g[:, 0].min()) == 0.0 and float(g[:, 0].abs().min()) > 0


def test_nan_in_the_map_makes_the_loss_nan():
    logits, target, _ = _inputs(0)
    bad = logits.clone()
    bad[1, 0, 2, 3, 4] = float("nan")
    val = su._build_loss(topk=10)(bad.to(DEV), target.to(DEV))
    assert bool(torch.isnan(val))


# ----------------------------------------------------------------------------- 4. workspace
GUARD, PATTERN = 4096, 0xA5


class Tight:
    """A workspace of exactly query(*args) bytes with the guard behind it (tests/test_pipeline_workspace_gpu.py's)."""

    def __init__(self, query, *args):
        n = int(query(*args))
        assert n > 0, n
        self.buf = torch.full((n + GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
        self.ws = self.buf[:n]
        assert self.ws.data_ptr() % 16 == 0 and self.ws.numel() == n

    def check(self):
        torch.cuda.synchronize()
        guard = self.buf[self.ws.numel():]
        assert guard.numel() == GUARD and bool((guard == PATTERN).all()), "the kernels wrote past the queried size"


def _same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    assert torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


@pytest.mark.parametrize("with_unc", [False, True])
@pytest.mark.parametrize("shape", [(2, 2, 3, 5, 7), (2, 2, 4, 10, 12)])      # S = 105: the map is padded; S = 480: not
def test_workspace_of_exactly_the_queried_size(shape, with_unc):
    N, Cc, D, H, W = shape
    S = D * H * W
    g = torch.Generator().manual_seed(21)
    logits = ops.to_cl((torch.randn(shape, generator=g) * 2).to(DEV))
    target = torch.randint(0, Cc, (N, 1, D, H, W), generator=g).float()
    unc = (1 - torch.rand((N, 1, D, H, W), generator=g) * 0.99) if with_unc else None
    K = int((N * N if with_unc else N) * S * 0.1)
    roomy = _launch(logits, target, unc, K)
    tight = Tight(L.load().rehr_seg_topk_workspace_bytes, N, Cc, S, int(with_unc))
    assert (N * S * 4) % 16 == (8 if S == 105 else 0)
    got = _launch(logits, target, unc, K, workspace=tight.ws)
    tight.check()
    # at most two blocks add into every statistic: a + b is b + a, so the runs agree to the bit
    _same(got[0], roomy[0])
    _same(got[2], roomy[2])
    _same(hb.seg_topk_map(got[1], N, S, with_unc), hb.seg_topk_map(roomy[1], N, S, with_unc))


def test_launch_layer_refuses_bad_operands():
    logits, target, _ = _inputs(0)
    lg, t = ops.to_cl(logits.to(DEV)), _flat(target, 2).to(DEV)
    with pytest.raises(L.RehrsegHipError):
        hb.seg_topk_fwd(lg, t, None, 0)
    with pytest.raises(L.RehrsegHipError):
        hb.seg_topk_fwd(lg, t, None, 211)
    with pytest.raises(L.RehrsegHipError):
        hb.seg_topk_fwd(logits.to(DEV), t, None, 21)                  # NCDHW memory
    with pytest.raises(L.RehrsegHipError):
        hb.seg_topk_fwd(lg, t[:, :100], None, 21)
    with pytest.raises(L.RehrsegHipError):
        hb.seg_topk_fwd(lg, t, None, 21, workspace=torch.empty(64, dtype=torch.uint8, device=DEV))    # REHR_EINVAL


# ----------------------------------------------------------------------------- 5. softmax properties
def test_softmax_properties():
    g = torch.Generator().manual_seed(5)
    shape = (2, 2, 16, 64, 64)
    logits = (torch.randn(shape, generator=g) * 2).to(DEV).requires_grad_(True)
    target = torch.randint(0, 2, (2, 1, 16, 64, 64), generator=g).float().to(DEV)
    mod = su._build_loss(topk=10)
    val = mod(logits, target)
    _node(val)
    val.backward()
    assert bool(torch.isfinite(val))
    gmax = float(logits.grad.abs().max())
    # every class term is rounded once in fp32: C * 2^-24 of the largest term, with room
    _close("gradient sum over classes", float(logits.grad.sum(1).abs().max()), 1e-6 * gmax)
    assert gmax > 0
    val2 = mod(logits.detach() + 7.5, target)
    _close("uniform logit shift", abs(float(val2) - float(val.detach())), 1e-5)


# ----------------------------------------------------------------------------- 6. the stage-2 step
@pytest.mark.parametrize("deep", [False, True])
def test_train_segsr_step_with_the_topk_loss(deep, monkeypatch):
    from oracle.detinit import det_input
    dev = torch.device(DEV)
    img = det_input("tk.img", (2, 1, 6, 32, 32), "rand") * 2 + 0.5
    lab = det_input("tk.lr", (2, 1, 6, 32, 32), "randint2")
    lab_hr = det_input("tk.hr", (2, 1, 24, 32, 32), "randint2")
    unc = 1 - det_input("tk.u", (2, 1, 6, 32, 32), "rand") * 0.99
    if deep:
        out = A.DownsampleSegForDSTransform2(A.DEEP_SUPERVISION_SCALES, 0, also=("uncertainty",))(
            seg=lab.to(dev), uncertainty=unc.to(dev))
        labs, uncs = out["seg"], out["uncertainty"]
    else:
        labs, uncs = lab.to(dev), unc.to(dev)
    fused = []
    fwd = hb.seg_topk_fwd
    monkeypatch.setattr(hb, "seg_topk_fwd", lambda *a, **kw: (fused.append(a[0].shape), fwd(*a, **kw))[1])

    def step(topk):
        model, sd = build(PLAN, dev, deep_supervision=deep)
        opt = torch.optim.SGD(model.parameters(), lr=1e-2)
        loss = train_segsr_step(model, None, None, opt, img.clone().to(dev), labs, lab_hr.to(dev), uncs,
                                su._build_loss(deep, topk=topk), su._build_loss(False, topk=topk))
        return model, sd, loss

    old, _, _ = step(None)
    assert fused == []
    new, sd, loss = step(10)
    assert bool(torch.isfinite(loss))
    assert len(fused) == (3 if deep else 2)               # a launch pair per weighted LR level, one for the HR logits
    had = [k for k, p in old.named_parameters() if p.grad is not None]
    assert had
    params = dict(new.named_parameters())
    for k in had:
        assert params[k].grad is not None, k
    moved = [k for k in had if not torch.equal(params[k].detach().cpu(), sd[k])]
    assert any("seg_layers" in k for k in moved) and any(k.startswith("encoder.stages.0") for k in moved)
    assert len(moved) >= len(had) // 2
