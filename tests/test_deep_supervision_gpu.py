"""Deep supervision on the device: the one-launch label pyramid (csrc/seg_loss_ds.hip: label_pyramid_kernel) bit for bit
against scipy.ndimage.zoom, the one-launch multi-level loss (seg_loss_ds_{fwd,bwd}_kernel<2,3,4>) against the project's
own DC_and_weighted_CE_loss composition on the CPU in fp64 summed with the level weights, the joint stage-2 step with a
deep-supervision network against the CPU oracles, and the data set's label lists.

Bars are those of tests/test_loss_kernels_gpu.py (value 1e-5 * max(1, |ref|), per-level gradient 1e-4 * max |ref gradient
of that level|), tests/test_train_steps_gpu.py (loss 2e-4 relative, parameter updates max(2e-3, 6 x the oracle's own
fp32-vs-fp64 distance)) and tests/test_mixed_steps_gpu.py:127-128 (the two loss inequalities under mixed precision).
Every comparison prints "name measured / bar" before it asserts, and every loss test asserts that the value came out of
the fused autograd node `_FusedDSDCCE`: the Python sum over levels cannot pass.
"""
import itertools
import random

import numpy as np
import pytest
import torch
from scipy import ndimage

from oracle import aux_oracle as ao
from oracle import segmodel_oracle as so
from oracle.bf16_emul import Bf16Emu
from oracle.detinit import det_input, det_tensor
from rehrseg_amd import ops
from rehrseg_amd.models.FLAVR.FLAVR_arch import UNet_3D_3D
from rehrseg_amd.models.seg_model import Distiller
from rehrseg_amd.train_steps import train_segsr_step
from rehrseg_amd.utils import augment as A
from rehrseg_amd.utils import seg_utils as su
from rehrseg_amd.utils.train_set import TrainSetMultipleSegSREfficient
from test_segmodel_cpu import build, canonical

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UP = 3.0   # upstream gradient: goes through the device scalar
PLAN = dict(n_stages=3, features_per_stage=[32, 64, 96], kernel_sizes=[[1, 3, 3], [1, 3, 3], [3, 3, 3]],
            strides=[[1, 1, 1], [1, 2, 2], [2, 2, 2]], n_conv_per_stage=[2, 2, 2], n_conv_per_stage_decoder=[2, 2],
            num_classes=2, upscale=4)   # tests/test_train_steps_gpu.py's


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _close(name, err, bar):
    print(f"{name}: {err:.3e} / {bar:.3e}")
    assert err <= bar, f"{name}: error {err:.3e} > bar {bar:.3e}"


def _fused(t, node):
    assert t.grad_fn is not None and type(t.grad_fn).__name__ == node.__name__ + "Backward", \
        f"not the fused path: {type(t.grad_fn).__name__}"


# ----------------------------------------------------------------------------- 1. label pyramid
def _zoom(vol, ext):
    return ndimage.zoom(vol, [m / n for m, n in zip(ext, vol.shape)], order=0, mode="nearest", grid_mode=True)


def _check_pyramid(shape, scales):
    g = _gen(2000 + shape[-1])
    seg = torch.randint(0, 4, shape, generator=g).float()
    unc = 0.01 + 0.99 * (1 - torch.rand(shape, generator=g))          # (0.01, 1]
    extents = A.pyramid_extents(shape[2:], scales)
    tr = A.DownsampleSegForDSTransform2(scales, 0, input_key="seg", output_key="seg", also=("uncertainty",))
    seg_dev, unc_dev = seg.to(DEV), unc.to(DEV)
    out = tr(seg=seg_dev, uncertainty=unc_dev, data=seg_dev)
    assert out["data"] is seg_dev and len(out["seg"]) == len(out["uncertainty"]) == len(scales)
    for key, src in (("seg", seg), ("uncertainty", unc)):
        for l, (ext, got) in enumerate(zip(extents, out[key])):
            assert tuple(got.shape) == tuple(shape[:2]) + ext and got.dtype == torch.float32, (key, l, got.shape)
            got = got.cpu().numpy()
            for b in range(shape[0]):
                ref = _zoom(src[b, 0].numpy(), ext)
                assert ref.shape == ext
                bad = int((got[b, 0] != ref).sum())
                print(f"pyramid {key} level {l} {ext} sample {b}: {bad} of {ref.size} voxels differ / 0")
                assert bad == 0
    ones = [l for l, s in enumerate(scales) if all(float(v) == 1 for v in s)]
    assert ones
    for l in ones:           # the all-ones level is the input's values
        assert torch.equal(out["seg"][l], seg_dev) and torch.equal(out["uncertainty"][l], unc_dev)
    return extents


def test_pyramid_odd_extents():
    """7 x 22 x 37: no axis divides, 3.5 -> 4 and 5.5 -> 6 round half to even, the coarsest in-plane extents are 1."""
    shape = (2, 1, 7, 22, 37)
    scales = [s for s in A.DEEP_SUPERVISION_SCALES if min(np.round(np.array(shape[2:]) * np.array(s))) >= 1]
    scales = scales + [[0.5, 0.5, 0.5]]
    assert len(scales) == 7                   # all six of the reference's leave a voxel here
    ext = _check_pyramid(shape, scales)
    assert ext[1] == (7, 11, 18) and ext[3] == (4, 3, 5) and ext[5] == (2, 1, 1) and ext[6] == (4, 11, 18)


def test_pyramid_power_of_two():
    ext = _check_pyramid((1, 1, 16, 64, 96), A.DEEP_SUPERVISION_SCALES)
    assert ext == [(16, 64, 96), (16, 32, 48), (16, 16, 24), (8, 8, 12), (4, 4, 6), (4, 2, 3)]


# ----------------------------------------------------------------------------- 2. multi-level loss
LEVELS = [(6, 32, 32), (6, 16, 16), (3, 8, 8), (2, 4, 4), (1, 2, 3)]   # the last: S = 6, under one wave


def _ref_weights(n=5):
    return su._build_loss(True).weight_factors[:n]


def _dcce(do_bg=False, smooth=1e-5, w_ce=1, w_dice=1):
    return su.DC_and_weighted_CE_loss({"batch_dice": False, "smooth": smooth, "do_bg": do_bg, "ddp": False},
                                      {"reduction": "none"}, weight_ce=w_ce, weight_dice=w_dice, ignore_label=None,
                                      dice_class=su.SoftDiceLoss)


def _inputs(C, N, dims, n_labels, seed):
    g = _gen(seed)
    logits = [torch.randn((N, C) + d, generator=g) * 2.0 for d in dims]
    lab_dims = list(dims) + [(1, 1, 2)] * (n_labels - len(dims))
    labels = [torch.randint(0, C, (N, 1) + d, generator=g).float() for d in lab_dims]
    uncs = [1.0 - torch.randint(0, 256, (N, 1) + d, generator=g).float() / 255.0 * 0.99 for d in lab_dims]
    return logits, labels, uncs


def _reference(cfg, weights, logits, labels, uncs):
    """sum_l w_l * DC_and_weighted_CE_loss on the CPU in fp64 (CPU tensors never take a fused path): value and the
    gradient of every level (None where the weight is 0)."""
    inner = _dcce(**cfg)
    xs = [x.double().requires_grad_(True) for x in logits]
    val = 0
    for l, x in enumerate(xs):
        if weights[l] != 0:
            val = val + weights[l] * inner(x, labels[l].double(), None if uncs is None else uncs[l].double())
    assert val.dtype == torch.float64
    (val * UP).backward()
    return float(val.detach()), [None if x.grad is None else x.grad / UP for x in xs]


def _check_ds(name, cfg, weights, logits, labels, uncs):
    rv, rg = _reference(cfg, weights, logits, labels, uncs)
    wrap = su.DeepSupervisionWrapper(_dcce(**cfg), weights)
    xg = [x.to(DEV).requires_grad_(True) for x in logits]
    args = [xg, [t.to(DEV) for t in labels]] + ([] if uncs is None else [[u.to(DEV) for u in uncs]])
    val = wrap(*args)
    _fused(val, su._FusedDSDCCE)
    (val * UP).backward()
    _close(f"ds {name} value", abs(float(val.detach()) - rv), 1e-5 * max(1.0, abs(rv)))
    for l, (x, r) in enumerate(zip(xg, rg)):
        if r is None:
            assert x.grad is None, f"level {l} carries weight 0 and must get no gradient"
            print(f"ds {name} level {l}: no gradient / none")
            continue
        got = x.grad.double().cpu() / UP
        _close(f"ds {name} gradient of level {l}", float((got - r).abs().max()), 1e-4 * float(r.abs().max()))
    return val, xg


@pytest.mark.parametrize("with_unc", [False, True], ids=["nounc", "unc"])
@pytest.mark.parametrize("N", [1, 2, 5])
@pytest.mark.parametrize("C", [2, 3, 4])
def test_ds_loss_classes_and_batch(C, N, with_unc):
    """Five levels from 6144 voxels down to 6, the reference's weights; N = 5 leaves a second chunk of one sample
    (SL_MAXN = 4) that pairs with the uncertainty sum over all five."""
    logits, labels, uncs = _inputs(C, N, LEVELS, 5, 3000 + 16 * C + N)
    _check_ds(f"C{C}-N{N}-{'unc' if with_unc else 'nounc'}", {}, _ref_weights(), logits, labels,
              uncs if with_unc else None)


def test_ds_loss_grid_stride_next_to_six_voxels():
    """S = 3 * 419 * 419 = 526 683 takes 2048 blocks and a second, partial trip; the 6-voxel level behind it owns the
    single last block of the grid."""
    logits, labels, uncs = _inputs(2, 2, [(3, 419, 419), (1, 2, 3)], 2, 3100)
    _check_ds("grid-stride", {}, (0.75, 0.25), logits, labels, uncs)


@pytest.mark.parametrize("do_bg", [False, True], ids=["nobg", "bg"])
def test_ds_loss_weight_dice_zero_with_uncertainty_and_background(do_bg):
    """weight_dice = 0 with an uncertainty list is the reference's stage-2 pairing for the LR output; do_bg both ways
    with both terms on."""
    logits, labels, uncs = _inputs(2, 2, LEVELS, 5, 3200 + do_bg)
    _check_ds(f"wdice0-{do_bg}", dict(w_dice=0, do_bg=do_bg), _ref_weights(), logits, labels, uncs)
    _check_ds(f"both-{do_bg}", dict(w_ce=0.3, w_dice=2.0, smooth=1.0, do_bg=do_bg), _ref_weights(), logits, labels,
              uncs)


def test_ds_loss_skips_a_zero_weight():
    logits, labels, uncs = _inputs(3, 2, LEVELS[:3], 3, 3300)
    _, xg = _check_ds("skip", {}, (1.0, 0.0, 0.25), logits, labels, uncs)
    assert xg[1].grad is None and xg[0].grad is not None and xg[2].grad is not None


def test_ds_launch_gives_a_zero_weight_level_no_blocks():
    """The launch layer itself (the wrapper never hands it a zero weight): a level with weight 0 may hold None, its
    statistics row stays zero, it gets no gradient buffer, and the other levels equal the single-level entry points."""
    from rehrseg_amd import hip_backend as hb
    logits, labels, uncs = _inputs(2, 2, LEVELS[:3], 3, 3350)
    xs = [x.to(DEV).contiguous(memory_format=torch.channels_last_3d) for x in logits]
    ts = [t.to(DEV).reshape(2, -1) for t in labels]
    us = [u.to(DEV).reshape(2, -1) for u in uncs]
    w = (1.0, 0.0, 0.25)
    hole = lambda v: [v[0], None, v[2]]   # noqa: E731
    stats = hb.seg_loss_ds_fwd(hole(xs), hole(ts), hole(us), w)
    assert tuple(stats.shape) == (3, 13) and float(stats[1].abs().max()) == 0.0
    go = torch.full((1,), UP, device=DEV)
    dl = hb.seg_loss_ds_bwd(hole(xs), hole(ts), hole(us), w, stats, 1.0, 1.0, 1e-5, False, go)
    assert dl[1] is None
    for l in (0, 2):
        st = hb.seg_loss_fwd(xs[l], ts[l], us[l])
        _close(f"ds launch level {l} statistics vs the single-level launch", float((stats[l] - st).abs().max()),
               1e-12 * float(st.abs().max()))     # the same <= 2048 fp32 block sums per statistic, all of one sign,
        #                                           added in another order in fp64: <= 2048 * 2^-53 = 2.3e-13 relative
        g1 = hb.seg_loss_bwd(xs[l], ts[l], us[l], st, 1.0, 1.0, 1e-5, False, go * w[l])
        _close(f"ds launch level {l} gradient vs the single-level launch", float((dl[l] - g1).abs().max()),
               1e-4 * float(g1.abs().max()))


def test_ds_loss_six_labels_for_five_logits():
    """The reference's table has six entries, the network five outputs: zip stops at the logits."""
    logits, labels, uncs = _inputs(2, 2, LEVELS, 6, 3400)
    rv, rg = _reference({}, _ref_weights(), logits, labels[:5], uncs[:5])
    wrap = su._build_loss(True)
    xg = [x.to(DEV).requires_grad_(True) for x in logits]
    val = wrap(xg, [t.to(DEV) for t in labels], [u.to(DEV) for u in uncs])
    _fused(val, su._FusedDSDCCE)
    (val * UP).backward()
    _close("ds six-for-five value", abs(float(val.detach()) - rv), 1e-5 * max(1.0, abs(rv)))
    for l, (x, r) in enumerate(zip(xg, rg)):
        _close(f"ds six-for-five gradient of level {l}", float((x.grad.double().cpu() / UP - r).abs().max()),
               1e-4 * float(r.abs().max()))


def test_ds_loss_one_level_equals_the_single_level_node():
    logits, labels, uncs = _inputs(3, 5, LEVELS[:1], 1, 3500)
    val, xg = _check_ds("one level", {}, (1.0,), logits, labels, uncs)
    x1 = logits[0].to(DEV).requires_grad_(True)
    single = _dcce()(x1, labels[0].to(DEV), uncs[0].to(DEV))
    _fused(single, su._FusedDCCE)
    (single * UP).backward()
    ref = float(single.detach())
    _close("ds one level vs _FusedDCCE value", abs(float(val.detach()) - ref), 1e-5 * max(1.0, abs(ref)))
    _close("ds one level vs _FusedDCCE gradient", float((xg[0].grad - x1.grad).abs().max()),
           1e-4 * float(x1.grad.abs().max()))


def test_ds_loss_refusals_on_the_device():
    logits, labels, uncs = _inputs(2, 2, LEVELS[:2], 2, 3600)
    wrap = su._build_loss(True)
    xg = [x.to(DEV) for x in logits]
    with pytest.raises(TypeError, match="list or tuple"):
        wrap(xg, [t.to(DEV) for t in labels], uncs[0].to(DEV))
    with pytest.raises(ValueError, match=r"\(2, 2, 6, 16, 16\).*\(2, 1, 6, 32, 32\)"):
        wrap(xg, [labels[0].to(DEV), labels[0].to(DEV)])


# ----------------------------------------------------------------------------- 3. joint stage-2 step
def _flavr(dev):
    m = UNet_3D_3D(2, "unet_18", 4, 4, use_uncertainty=True)
    sd = {k: det_tensor(k, tuple(v.shape)) for k, v in m.state_dict().items()}
    m.load_state_dict(sd)
    return m.to(dev).eval(), sd


def _distiller(dev):
    dist = Distiller(64, 64, 0.0, 1.0, 1.0)
    dsd = {k: det_tensor(k, tuple(v.shape)) for k, v in dist.state_dict().items()}
    dist.load_state_dict(dsd)
    return dist.to(dev), dsd


def _step_inputs(tag):
    img = det_input(tag + ".img", (2, 1, 6, 32, 32), "rand") * 2 + 0.5
    lab_lr = det_input(tag + ".lr", (2, 1, 6, 32, 32), "randint2")
    lab_hr = det_input(tag + ".hr", (2, 1, 24, 32, 32), "randint2")
    unc = 1 - det_input(tag + ".u", (2, 1, 6, 32, 32), "rand") * 0.99
    return img, lab_lr, lab_hr, unc


def _pyramids(lab_lr, unc):
    """The label / uncertainty lists through the new transform step (on the device), and copies on the host."""
    tr = A.DownsampleSegForDSTransform2(A.DEEP_SUPERVISION_SCALES, 0, also=("uncertainty",))
    out = tr(seg=lab_lr.to(DEV), uncertainty=unc.to(DEV))
    assert len(out["seg"]) == 6 and tuple(out["seg"][1].shape) == (2, 1, 6, 16, 16)
    return out["seg"], out["uncertainty"], [t.cpu() for t in out["seg"]], [t.cpu() for t in out["uncertainty"]]


def _oracle_loss(o, dw, db, tf, img_o, labs, uncs, lab_hr, weights, dt, emu=None):
    cfg = dict(PLAN, deep_supervision=True)
    segs, s_sr, sk = so.seg_model(o, img_o.to(dt), cfg, return_features=True, emu=emu)
    assert len(segs) == 2
    loss = 0
    for l, s in enumerate(segs):
        if weights[l] != 0:
            loss = loss + weights[l] * ao.dc_and_weighted_ce(s, labs[l].to(dt), uncs[l].to(dt), weight_dice=0.0)
    loss = loss + ao.dc_and_weighted_ce(s_sr, lab_hr.to(dt), None)
    return loss + ao.distiller_loss(dw, db, sk[1], tf.to(dt), 0.0, 1.0, 1.0, emu=emu)


def test_joint_step_with_deep_supervision():
    dev = torch.device(DEV)
    teacher, tsd = _flavr(dev)
    student, ssd = build(PLAN, dev, deep_supervision=True)
    dist, dsd = _distiller(dev)
    img, lab_lr, lab_hr, unc = _step_inputs("ds2")
    labs_dev, uncs_dev, labs, uncs = _pyramids(lab_lr, unc)
    loss_lr = su._build_loss(True, weight_dice=0)
    weights = loss_lr.weight_factors
    opt = torch.optim.SGD(itertools.chain(student.parameters(), dist.parameters()), lr=1e-3, momentum=0.99,
                          nesterov=True, weight_decay=3e-5)
    img_dev = img.clone().to(dev)
    loss = train_segsr_step(student, teacher, dist, opt, img_dev, labs_dev, lab_hr.to(dev), uncs_dev, loss_lr,
                            su._build_loss(False, weight_dice=1))
    img_o = img.clone()
    with torch.no_grad():
        tf = ao.teacher_features(tsd, img_o, lab_lr)      # the teacher reads level 0
    assert torch.allclose(img_dev.cpu(), img_o, atol=1e-5)
    shapes = so.segmodel_shapes(PLAN)

    def oracle_step(dt):
        dw = dsd["distill.weight"].to(dt).clone().requires_grad_()
        db = dsd["distill.bias"].to(dt).clone().requires_grad_()
        o2 = {k: v.detach().to(dt).clone().requires_grad_() for k, v in ssd.items() if k in shapes}
        r2 = _oracle_loss(o2, dw, db, tf[1], img_o, labs, uncs, lab_hr, weights, dt)
        olds = {k: v.detach().clone() for k, v in o2.items()}
        oopt = torch.optim.SGD(list(o2.values()) + [dw, db], lr=1e-3, momentum=0.99, nesterov=True, weight_decay=3e-5)
        r2.backward()
        oopt.step()
        return float(r2.detach()), {k: (v.detach() - olds[k]).double() for k, v in o2.items()}

    ref, d32 = oracle_step(torch.float32)
    _, d64 = oracle_step(torch.float64)
    _close("ds joint step loss", abs(loss.item() - ref), 2e-4 * abs(ref))
    new = {canonical(k): v.detach().cpu() for k, v in student.state_dict().items()}
    assert "decoder.seg_layers.0.weight" in d32 and float(d32["decoder.seg_layers.0.weight"].abs().max()) > 0
    worst = ("", 0.0, 0.0)
    for k in d32:
        if k.endswith("conv.bias"):       # zero gradient behind InstanceNorm: the update is weight decay only
            continue
        d_hip = (new[k] - ssd[k]).double()
        e = float((d_hip - d32[k]).norm() / (d32[k].norm() + 1e-30))
        cond = float((d32[k] - d64[k]).norm() / (d64[k].norm() + 1e-30))
        assert e <= max(2e-3, 6 * cond), (k, e, cond)
        if e > worst[1]:
            worst = (k, e, cond)
    print("ds joint step: worst parameter-update l2-rel vs the oracle's SGD step (name, hip-vs-fp32, fp32-vs-fp64):", worst)


def test_joint_step_zero_weight_leaves_the_coarse_head_alone():
    """Weights (1, 0): the coarse output's 1x1x1 head (decoder.seg_layers[0]) gets no gradient, so SGD with weight decay
    neither decays nor moves it; the fine head moves."""
    dev = torch.device(DEV)
    teacher, _ = _flavr(dev)
    student, ssd = build(PLAN, dev, deep_supervision=True)
    dist, _ = _distiller(dev)
    img, lab_lr, lab_hr, unc = _step_inputs("ds2")
    labs_dev, uncs_dev, _, _ = _pyramids(lab_lr, unc)
    loss_lr = su.DeepSupervisionWrapper(su._build_loss(False, weight_dice=0), (1.0, 0.0))
    opt = torch.optim.SGD(itertools.chain(student.parameters(), dist.parameters()), lr=1e-3, momentum=0.99,
                          nesterov=True, weight_decay=3e-5)
    train_segsr_step(student, teacher, dist, opt, img.clone().to(dev), labs_dev, lab_hr.to(dev), uncs_dev, loss_lr,
                     su._build_loss(False, weight_dice=1))
    coarse, fine = student.decoder.seg_layers[0], student.decoder.seg_layers[1]
    assert coarse.weight.grad is None and coarse.bias.grad is None
    for name, p in (("weight", coarse.weight), ("bias", coarse.bias)):
        assert torch.equal(p.detach().cpu(), ssd[f"decoder.seg_layers.0.{name}"])
    assert not torch.equal(fine.weight.detach().cpu(), ssd["decoder.seg_layers.1.weight"])


def test_joint_step_with_deep_supervision_mixed_precision():
    dev = torch.device(DEV)
    teacher, tsd = _flavr(dev)
    student, ssd = build(PLAN, dev, deep_supervision=True)
    dist, dsd = _distiller(dev)
    img, lab_lr, lab_hr, unc = _step_inputs("ds2")
    labs_dev, uncs_dev, labs, uncs = _pyramids(lab_lr, unc)
    loss_lr = su._build_loss(True, weight_dice=0)
    opt = torch.optim.SGD(itertools.chain(student.parameters(), dist.parameters()), lr=0.0)
    with ops.mixed_precision():
        loss = train_segsr_step(student, teacher, dist, opt, img.clone().to(dev), labs_dev, lab_hr.to(dev), uncs_dev,
                                loss_lr, su._build_loss(False, weight_dice=1))
    shapes = so.segmodel_shapes(PLAN)

    def oracle(dt, emu):
        img_o = img.clone().to(dt)
        with torch.no_grad():
            tf = ao.teacher_features({k: v.to(dt) for k, v in tsd.items()}, img_o, lab_lr.to(dt), emu=emu, upto=1)
        o = {k: v.detach().to(dt).clone() for k, v in ssd.items() if k in shapes}
        with torch.no_grad():
            return float(_oracle_loss(o, dsd["distill.weight"].to(dt), dsd["distill.bias"].to(dt), tf[1], img_o, labs,
                                      uncs, lab_hr, loss_lr.weight_factors, dt, emu))

    l32, lE = oracle(torch.float32, None), oracle(torch.float64, Bf16Emu())
    got = loss.item()
    print("ds joint step bf16: loss hip", got, "oracle fp32", l32, "oracle bf16-emulated", lE)
    print(f"ds joint step bf16 vs fp32: {abs(got - l32):.3e} / {max(2e-3 * abs(l32), 2.5 * abs(lE - l32)):.3e}")
    print(f"ds joint step bf16 vs emulated: {abs(got - lE):.3e} / {max(1e-3 * abs(lE), 1.5 * abs(lE - l32)):.3e}")
    assert abs(got - l32) <= max(2e-3 * abs(l32), 2.5 * abs(lE - l32)), (got, l32, lE)
    assert abs(got - lE) <= max(1e-3 * abs(lE), 1.5 * abs(lE - l32)), (got, l32, lE)


# ----------------------------------------------------------------------------- 4. data set
def test_data_set_returns_the_label_pyramid():
    g = _gen(4000)
    shape = (40, 36, 16)                                 # (x, y, z)
    vols = [{"img": (torch.rand(shape, generator=g) * 300).to(DEV),
             "seg": torch.randint(0, 2, shape, generator=g).to(torch.uint8).to(DEV),
             "uncertainty": torch.randint(0, 256, shape, generator=g).to(torch.uint8).to(DEV)} for _ in range(2)]
    args = (None, ["a", "b"], 2.0, 1.0, [32, 32, 4], [32, 32, 4])
    plain = TrainSetMultipleSegSREfficient(*args, random_flip=True, uncertainty=True, device=DEV, volumes=vols)
    deep = TrainSetMultipleSegSREfficient(*args, random_flip=True, uncertainty=True, device=DEV, volumes=vols,
                                          deep_supervision=True)
    random.seed(21)
    a = plain.batch([0, 1, 1])
    after_plain = random.random()
    random.seed(21)
    b = deep.batch([0, 1, 1])
    assert random.random() == after_plain                # the draw stream is unchanged
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])          # img, label
    extents = A.pyramid_extents((4, 32, 32), A.DEEP_SUPERVISION_SCALES)
    for key, full, levels in (("label_lr", a[1], b[1]), ("uncertainty_lr", a[3], b[3])):
        assert isinstance(levels, list) and len(levels) == 6
        assert torch.equal(levels[0], full)
        for l, (ext, got) in enumerate(zip(extents, levels)):
            assert tuple(got.shape) == (3, 1) + ext, (key, l, got.shape)
            for i in range(3):
                ref = _zoom(full[i, 0].cpu().numpy(), ext)
                assert np.array_equal(got[i, 0].cpu().numpy(), ref), (key, l, i)
    random.seed(22)
    item = deep[1]
    assert isinstance(item[1], list) and tuple(item[1][3].shape) == (1,) + extents[3]
    assert isinstance(item[3], list) and tuple(item[3][0].shape) == (1, 4, 32, 32)


def test_training_transform_chain_appends_the_pyramid():
    """train_transform="nnunet" with deep_supervision: the pyramid is the last step of the chain.  Same seeds, same
    draws: data, seg_sr and level 0 of seg / uncertainty are bit-equal to the chain without it, the other levels are
    the scipy zoom of level 0 (of the AUGMENTED maps), and np.random ends in the same state."""
    g = _gen(4100)
    shape = (40, 36, 16)
    vols = [{"img": (torch.rand(shape, generator=g) * 300).to(DEV),
             "seg": torch.randint(0, 2, shape, generator=g).to(torch.uint8).to(DEV),
             "uncertainty": torch.randint(0, 256, shape, generator=g).to(torch.uint8).to(DEV)}]
    args = (None, ["a"], 2.0, 1.0, [32, 32, 4], [32, 32, 4])
    kw = dict(uncertainty=True, device=DEV, volumes=vols, train_transform="nnunet")
    plain = TrainSetMultipleSegSREfficient(*args, **kw)
    deep = TrainSetMultipleSegSREfficient(*args, deep_supervision=True, **kw)
    assert deep._pyramid is None and deep.train_transform.pyramid is not None and plain.train_transform.pyramid is None
    random.seed(5), np.random.seed(6)
    a = plain.batch([0, 0, 0, 0])
    after = np.random.uniform()
    random.seed(5), np.random.seed(6)
    b = deep.batch([0, 0, 0, 0])
    assert np.random.uniform() == after
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    extents = A.pyramid_extents(tuple(a[1].shape[2:]), A.DEEP_SUPERVISION_SCALES)
    for full, levels in ((a[1], b[1]), (a[3], b[3])):
        assert len(levels) == 6 and torch.equal(levels[0], full)
        for ext, got in zip(extents, levels):
            assert tuple(got.shape) == (4, 1) + ext
            for i in range(4):
                assert np.array_equal(got[i, 0].cpu().numpy(), _zoom(full[i, 0].cpu().numpy(), ext))
