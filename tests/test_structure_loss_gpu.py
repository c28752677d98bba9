"""Stage-1 structure losses on the MI355X: the kernels of csrc/sr_losses.hip through models.losses and autograd against
the fp64 oracle of tests/structure_loss_cases.py (where the bars are derived) on the smallest shapes at which each thing
can go wrong, through the channels-last strided view, run to run, against rehr_sr_metrics_f32's SSIM, under a non-unit
grad_output, and inside one train_sr_step of a tiny FLAVR network.

  (1, 1, 1, 11, 11)   one valid window position, every pixel a border for Sobel
  (2, 1, 3, 12, 43)   W crosses a 32-tile with both halos, N > 1, D > 1
  (1, 2, 2, 45, 37)   ragged tiles on both axes, C > 1
  (1, 1, 1, 70, 67)   three tiles on both axes
  (1, 1, 2, 1, 5)     ssim = 0: Sobel on a one-row slice
"""
import numpy as np
import pytest
import torch

import sr_metrics_cases as sc
import structure_loss_cases as lc
from rehrseg_amd import hip_backend as hb
from rehrseg_amd.models.FLAVR.FLAVR_arch import UNet_3D_3D
from rehrseg_amd.models.losses import StructureLoss, l1_sobel_loss, l2_sobel_loss
from rehrseg_amd.train_steps import train_sr_step
from rehrseg_amd.utils import seg_utils as su
from rehrseg_amd.utils import sr_utils as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = lc.TERMS["all"]


def _dev(*arrays):
    return tuple(torch.from_numpy(np.array(a)).to(DEV) for a in arrays)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run(loss_fn, p, t, go=None):
    x, y = _dev(p, t)
    x.requires_grad_()
    loss = loss_fn(x, y)
    assert loss.is_cuda and loss.dim() == 0 and loss.dtype == torch.float32
    (loss if go is None else loss * go).backward()
    assert x.grad.is_cuda and x.grad.shape == x.shape
    return float(loss.detach()), x.grad.cpu().numpy()


@pytest.mark.parametrize("term", list(lc.TERMS))
@pytest.mark.parametrize("shape", lc.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", lc.KINDS)
def test_kernels_against_the_oracle(kind, shape, term):
    p, t, rng, ref = lc.reference(kind, shape, term)
    value, grad = _run(StructureLoss(*lc.TERMS[term], data_range=rng), p, t)
    lc.check(f"kernel {kind} {shape} {term}", value, grad, p, t, lc.TERMS[term], rng, ref)


@pytest.mark.parametrize("kind", lc.KINDS)
def test_sobel_on_a_one_row_slice(kind):
    w = (1.0, 0.5, 0.0, 1.3)
    p, t, rng = lc.make_case(kind, lc.ROW_SHAPE)
    value, grad = _run(StructureLoss(*w, data_range=rng), p, t)
    lc.check(f"kernel {kind} {lc.ROW_SHAPE}", value, grad, p, t, w, rng)
    x, y = _dev(p, t)
    with pytest.raises(hb.L.RehrsegHipError, match="ENOSUP"):
        StructureLoss(ssim=1.0)(x, y)


def test_reference_named_functions_and_their_argument_order():
    p, t, rng = lc.make_case("a", (1, 2, 2, 45, 37))
    for fn, w in ((l1_sobel_loss, (1.0, 0.0, 0.0, 1.0)), (l2_sobel_loss, (0.0, 1.0, 0.0, 1.0))):
        value, grad = _run(lambda x, y: fn(y, x), p, t)
        lc.check(f"kernel {fn.__name__}", value, grad, p, t, w, rng)
        v2, g2 = _run(StructureLoss(*w), p, t)
        assert v2 == value and np.array_equal(g2, grad)


def test_channels_last_view_gives_the_bits_of_its_contiguous_copy():
    """The network's output is channels-last (N, 2, D, H, W): hat[:, 0:1] has innermost stride 2 and is not copied; the
    target is a channel of a cropped contiguous NCDHW tensor."""
    shape = (2, 1, 3, 45, 37)
    p, t, rng = lc.make_case("a", shape)
    pd, td = _dev(p, t)
    net = torch.cat((pd, torch.randn_like(pd)), 1).contiguous(memory_format=torch.channels_last_3d).requires_grad_()
    big = torch.zeros((2, 2, 5, 45, 37), device=DEV)
    big[:, 0:1, 1:4] = td
    view, tgt = net[:, 0:1], big[:, 0:1, 1:4]
    assert view.stride()[-1] == 2 and not view.is_contiguous() and not tgt.is_contiguous()
    fn = StructureLoss(*ALL, data_range=rng)
    loss = fn(view, tgt)
    loss.backward()
    x = pd.clone().requires_grad_()
    want = fn(x, td)
    want.backward()
    assert torch.equal(_bits(loss), _bits(want))
    assert torch.equal(_bits(net.grad[:, 0:1]), _bits(x.grad)) and not net.grad[:, 1:].any()
    # the launch layer writes d input into given strides as well
    w = ALL
    _, _, fields = hb.structure_loss_fwd(view.detach(), tgt, w, rng)
    out = torch.full_like(net, 7.0)
    got = hb.structure_loss_bwd(view.detach(), tgt, w, fields, torch.ones(1, device=DEV), out=out[:, 0:1])
    assert got.data_ptr() == out.data_ptr() and torch.equal(_bits(out[:, 0:1]), _bits(x.grad))
    assert bool((out[:, 1:] == 7.0).all())


def test_two_calls_give_identical_bits():
    p, t, rng = lc.make_case("b", (2, 1, 3, 70, 67))
    x, y = _dev(p, t)
    go = torch.full((1,), 0.37, device=DEV)
    loss, stats, fields = hb.structure_loss_fwd(x, y, ALL, rng)
    grad = hb.structure_loss_bwd(x, y, ALL, fields, go)
    for _ in range(3):
        l2, s2, f2 = hb.structure_loss_fwd(x, y, ALL, rng)
        assert torch.equal(_bits(l2), _bits(loss)) and torch.equal(s2.view(torch.int64), stats.view(torch.int64))
        assert torch.equal(_bits(hb.structure_loss_bwd(x, y, ALL, f2, go)), _bits(grad))


@pytest.mark.parametrize("kind", sc.KINDS)
def test_one_minus_the_ssim_term_is_sr_metrics_ssim(kind):
    shape = (2, 1, 3, 45, 37)
    p, t, rng = lc.make_case(kind, shape)
    x, y = _dev(p, t)
    loss, stats, _ = hb.structure_loss_fwd(x, y, (0.0, 0.0, 1.0, 0.0), rng, need_grad=False)
    q = sr.sr_quality(hb.sr_metrics(x[:, 0], y[:, 0], data_range=rng), 3 * 45 * 37, rng)
    want = sc.oracle(p[:, 0], t[:, 0], data_range=rng)
    ssim64 = want[:, 2] / want[:, 3]
    d32 = float(np.abs(sc.ssim_torch_fp32(p[:, 0], t[:, 0], rng) - ssim64).max())
    dist = abs((1.0 - float(loss)) - q["ssim"])
    print(f"{kind}: 1 - loss {1.0 - float(loss):.8f}  sr_quality ssim {q['ssim']:.8f}  distance {dist:.3e}  "
          f"bound {max(4 * d32, sc.SSIM_FLOOR):.3e}")
    assert dist <= max(4 * d32, sc.SSIM_FLOOR)
    assert abs((1.0 - float(loss)) - float(ssim64.mean())) <= max(4 * d32, sc.SSIM_FLOOR)
    # the per-sample sums are sr_metrics' own, bit for bit
    assert torch.equal(stats[:, 2].view(torch.int64), hb.sr_metrics(x[:, 0], y[:, 0], data_range=rng)[:, 2].view(torch.int64))
    # and at every single-channel shape of the cases: one window position, a tile edge with both halos, three tiles
    for s in (s for s in lc.SHAPES if s[1] == 1):
        p, t, rng = lc.make_case(kind, s)
        x, y = _dev(p, t)
        _, stats, _ = hb.structure_loss_fwd(x, y, (0.0, 0.0, 1.0, 0.0), rng, need_grad=False)
        assert torch.equal(stats[:, 2].view(torch.int64),
                           hb.sr_metrics(x[:, 0], y[:, 0], data_range=rng)[:, 2].view(torch.int64)), s


@pytest.mark.parametrize("kind", lc.KINDS)
def test_identical_images_give_exactly_zero(kind):
    _, t, rng = lc.make_case(kind, (1, 2, 2, 45, 37))
    value, grad = _run(StructureLoss(*ALL, data_range=rng), t, t)
    assert value == 0.0 and np.isfinite(grad).all()


def test_grad_output_scales_the_gradient_and_is_read_on_the_device():
    p, t, rng = lc.make_case("a", (2, 1, 3, 12, 43))
    fn = StructureLoss(*ALL)
    _, g1 = _run(fn, p, t)
    _, g3 = _run(fn, p, t, go=-3.0)
    assert np.abs(g3 - np.float32(-3.0) * g1).max() <= 2.0 ** -23 * np.abs(g3).max()
    # no host synchronisation in either direction
    x, y = _dev(p, t)
    x.requires_grad_()
    fn(x, y).backward()
    warm = x.grad.clone()
    x.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        fn(x, y).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(_bits(x.grad), _bits(warm))


def test_a_weight_of_zero_skips_its_term():
    p, t, rng = lc.make_case("b", (2, 1, 3, 12, 43))
    x, y = _dev(p, t)
    _, stats, fields = hb.structure_loss_fwd(x, y, ALL, rng)
    for k in range(4):
        w = tuple(v if i == k else 0.0 for i, v in enumerate(ALL))
        _, s, f = hb.structure_loss_fwd(x, y, w, rng)
        assert torch.equal(s[:, k].view(torch.int64), stats[:, k].view(torch.int64))
        assert not s[:, [i for i in range(4) if i != k]].any()
        assert (f is not None) == (k == 2) and (f is None or torch.equal(_bits(f[..., 5:-5, 5:-5]),
                                                                          _bits(fields[..., 5:-5, 5:-5])))


class _Recorder(torch.nn.Module):
    """Stands where loss_obj stands and remembers what the step handed it and what came back."""

    def __init__(self, inner):
        super().__init__()
        self.inner, self.seen = inner, []

    def forward(self, input, target):
        loss = self.inner(input, target)
        self.seen.append((input.detach().clone(), target.detach().clone(), loss.detach().clone()))
        return loss


def _one_step(unc, loss_obj):
    """One train_sr_step of a freshly seeded tiny network on one seeded batch -> (loss, {parameter name: gradient})."""
    torch.manual_seed(0)
    model = UNet_3D_3D(2, "unet_18", 4, 4, use_uncertainty=unc).to(DEV).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    g = torch.Generator().manual_seed(5)
    lr = torch.rand((2, 2, 4, 32, 32), generator=g).to(DEV)
    hr = torch.rand((2, 2, 16, 32, 32), generator=g)
    hr[:, 1] = (hr[:, 1] > 0.5).float()
    loss = train_sr_step(model, opt, None, lr, hr.to(DEV), loss_obj, su.BCEDiceLoss(1.0, 1.0), 4.0, 4, unc)
    return loss, {name: prm.grad for name, prm in model.named_parameters() if prm.grad is not None}


@pytest.mark.parametrize("unc", [False, True], ids=["plain", "uncertainty"])
def test_one_train_sr_step_with_the_structure_loss(unc):
    """Every parameter the step trains under L1Loss (the network holds a few its forward pass never reads) gets a finite
    gradient under the structure loss, and the loss is the oracle's on the model's own output."""
    w = (1.0, 0.0, 1.0, 1.0)
    _, plain = _one_step(unc, torch.nn.L1Loss())
    rec = _Recorder(StructureLoss(l1=1.0, ssim=1.0, sobel=1.0))
    loss, grads = _one_step(unc, rec)
    assert loss.is_cuda and loss.dim() == 0 and bool(torch.isfinite(loss))
    assert len(plain) >= 60 and set(grads) == set(plain)
    for name, grad in grads.items():
        assert bool(torch.isfinite(grad).all()), name
        assert not torch.equal(grad, plain[name]), name            # and it is another gradient than L1's
    assert len(rec.seen) == (2 if unc else 1)
    for i, (inp, tgt, got) in enumerate(rec.seen):
        assert tuple(inp.shape) == tuple(tgt.shape) == (2, 1, 4, 32, 32)
        p, t = inp.cpu().numpy(), tgt.cpu().numpy()
        v64, _, dv32, _ = lc.yardstick(p, t, w)
        bound = max(4 * dv32, lc.value_floor(p, t, w, 1.0))
        print(f"train_sr_step pair {i}: loss {float(got):.7f}  oracle {v64:.7f}  distance {abs(float(got) - v64):.3e}  "
              f"bound {bound:.3e}")
        assert abs(float(got) - v64) <= bound
