"""Stage-2 validation on the MI355X (csrc/seg_eval.hip): evaluate_case against the reference's own outputs
(tests/golden/eval_case.npz), the fused tiled predictor against the unchanged torch predictor, the finalize kernel
against torch and numpy at the reference's case size, the single host sync of a case, and the global Dice of
evaluate_cases.

The kernels round `acc + p * g` once, as torch does on the CPU (tests/test_eval_cpu.py checks that bit for bit).  On
the device, torch's elementwise kernels do not keep to one rule for `fp16 += fp32`: measured here, large contiguous
operands round the fp32 operand to fp16 before the sum, strided views round once.  The device comparison therefore
allows at most 0.2 % of the voxels to differ, by a few fp16 ulps (rtol 5e-3); every other voxel is equal."""
import warnings

import numpy as np
import pytest
import torch

from rehrseg_amd import hip_backend as hb
from rehrseg_amd.utils import seg_utils as su
from test_eval_cpu import CASES, G

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


class DevToy(torch.nn.Module):
    """A position- and orientation-sensitive toy network built from device ops only (no host tensors, no syncs)."""

    def __init__(self, sep=2, scale=1.0):
        super().__init__()
        self.sep, self.scale = sep, scale

    def forward(self, x):
        sh = torch.roll(x, shifts=(1, 2), dims=(3, 4))
        lr = torch.cat([x * 0.5 + sh * 0.25, -x * 0.75 + sh * sh * 0.125 - 0.1], 1) * self.scale
        return lr, torch.repeat_interleave(lr, self.sep, dim=2) * 1.5


def _bits(t):
    return t.contiguous().view(torch.int16)


def _assert_near_bitwise(got, want, frac=2e-3):
    """equal values, except at most `frac` of the voxels a few fp16 ulps apart (a rounding difference in one tile,
    carried through the later tiles' sums and the normalisation)"""
    off = got != want
    n = int(off.sum())
    assert n <= frac * got.numel(), (n, got.numel())
    assert torch.allclose(got.float(), want.float(), rtol=5e-3, atol=1e-4)


@pytest.mark.parametrize("case", CASES)
def test_evaluate_case_matches_reference_fixture(case):
    from toy_models import ToySegNet
    sep = int(G["sep"])
    img, label = G[f"{case}_img"].astype(np.float32), G[f"{case}_label"].astype(np.float32)
    net = ToySegNet(sep=sep).to(DEV)
    pred_lr, pred_hr, lr_label, dice = su.evaluate_case(net, img, label, float(sep), list(G[f"{case}_patch"]),
                                                        get_HR_results=True, device=DEV)
    assert pred_lr.dtype == np.uint8 and np.array_equal(pred_lr, G[f"{case}_pred_lr"])
    assert pred_hr.dtype == np.uint8 and np.array_equal(pred_hr, G[f"{case}_pred_hr"])
    assert not lr_label.is_cuda and np.array_equal(lr_label.numpy(), G[f"{case}_lr_label"])
    assert isinstance(dice, np.float64) and dice == G[f"{case}_dice_lr"]


def _segmodel():
    from test_segmodel_cpu import SMALL, build
    return build(SMALL, DEV)[0].eval()


def _compare(net, data, patch, out_idx, sep, gauss, pad_lo):
    """fused predictor on the un-padded volume vs the unchanged predictor on the padded one."""
    padded, sl_rev = su.pad_nd_image(data, patch, "constant", {"value": 0}, True, None)
    slicers = su._internal_get_sliding_window_slicers(padded.shape[1:], patch_size=patch)
    ps = [patch[0] * sep, patch[1], patch[2]] if out_idx else patch
    with torch.no_grad():
        want = su._internal_predict_sliding_window_return_logits(padded.clone(), slicers, net, True, out_idx, sep, ps,
                                                                 use_gaussian=gauss, deep_supervision=False)
        again = su._internal_predict_sliding_window_return_logits(padded.clone(), slicers, net, True, out_idx, sep,
                                                                  ps, use_gaussian=gauss, deep_supervision=False)
        got = su._fused_predict_sliding_window_return_logits(data.to(DEV), slicers, net, out_idx, sep, ps,
                                                             use_gaussian=gauss, deep_supervision=False,
                                                             pad=[s.start for s in sl_rev[1:]])
    assert [s.start for s in sl_rev[1:]] == list(pad_lo)
    assert got.dtype == torch.half and got.shape == want.shape
    return got, want, again


@pytest.mark.parametrize("out_idx,sep,gauss", [(0, 1, True), (1, 2, False)])
def test_fused_predictor_bit_identical_toy(out_idx, sep, gauss):
    from toy_models import ToySegNet
    g = torch.Generator().manual_seed(11)
    data = torch.randn(1, 5, 37, 29, generator=g)                    # thinner and narrower than the tile: padded
    got, want, _ = _compare(ToySegNet(sep=2).to(DEV), data, [8, 16, 32], out_idx, sep, gauss, (1, 0, 1))
    _assert_near_bitwise(got, want)
    data = torch.randn(1, 20, 70, 61, generator=g)                   # several tiles per axis
    got, want, _ = _compare(ToySegNet(sep=2).to(DEV), data, [8, 24, 20], out_idx, sep, gauss, (0, 0, 0))
    _assert_near_bitwise(got, want)


@pytest.mark.parametrize("out_idx,sep,gauss", [(0, 1, True), (1, 4, False)])
def test_fused_predictor_bit_identical_segmodel(out_idx, sep, gauss):
    """The HIP SegModel (SMALL plan; its HR head is 4x deep, so sep = 4).  The model is first compared with a re-run of
    itself: when the model is bitwise deterministic the fused logits must meet the torch predictor as the module
    docstring says, and otherwise lie within the model's own run-to-run difference."""
    net = _segmodel()
    g = torch.Generator().manual_seed(12)
    data = torch.randn(1, 6, 40, 44, generator=g)
    got, want, again = _compare(net, data, [8, 32, 32], out_idx, sep, gauss, (1, 0, 0))
    if torch.equal(_bits(want), _bits(again)):
        _assert_near_bitwise(got, want)
    else:
        noise = float((want.float() - again.float()).abs().max())
        assert float((got.float() - want.float()).abs().max()) <= noise, noise


def _finalize_case(seed, inf=False):
    """random fp16 accumulators of a 20 x 455 x 633 padded case with exact ties, cropped to 17 x 450 x 630"""
    g = torch.Generator().manual_seed(seed)
    D, H, W = 20, 455, 633
    counts = (torch.rand(D, H, W, generator=g) * 11.5 + 0.5).half()
    logits = (torch.randn(2, D, H, W, generator=g) * 3).half() * counts
    tie = torch.rand(D, H, W, generator=g) < 0.01
    logits[1][tie] = logits[0][tie]
    logits = logits.half()
    if inf:
        logits[0, 3, 7, 9], counts[3, 7, 9] = 60000.0, 2 ** -14     # 60000 / 2^-14 overflows fp16
    gt = (torch.rand(17, 450, 630, generator=g) < 0.3).to(torch.uint8)
    crop = (slice(1, 18), slice(2, 452), slice(1, 631))
    return logits, counts, gt, crop, tie


def test_finalize_matches_torch_at_reference_size():
    logits, counts, gt, crop, tie = _finalize_case(5)
    lg, cn, gtd = logits.to(DEV), counts.to(DEV), gt.to(DEV)
    stats = torch.zeros(4, dtype=torch.int64, device=DEV)
    labels = torch.empty(tuple(gt.shape), dtype=torch.uint8, device=DEV)
    want_norm = lg / cn                                              # torch's fp16 division on the device
    hb.seg_eval_finalize(lg, cn, stats, crop, labels, gtd)
    assert torch.equal(_bits(lg), _bits(want_norm))
    norm = lg.cpu()[(slice(None),) + crop]
    want = torch.softmax(norm.float(), dim=0).numpy().argmax(0).astype(np.uint8)
    got = labels.cpu().numpy()
    assert np.array_equal(got, want)
    assert int(tie[crop].sum()) > 10000 and (got[tie[crop].numpy()] == 0).all()   # exact ties: the lowest class
    st = stats.cpu().numpy()
    assert st[0] == 0
    assert (st[1], st[2], st[3]) == (np.sum(want * gt.numpy()), np.sum(want), np.sum(gt.numpy()))
    # the HR form: no crop, no labels, plain argmax of the fp16 logits
    lg2 = logits.to(DEV)
    hr = torch.empty(tuple(counts.shape), dtype=torch.uint8, device=DEV)
    st2 = torch.zeros(4, dtype=torch.int64, device=DEV)
    hb.seg_eval_finalize(lg2, cn, st2, None, hr)
    assert torch.equal(hr.long(), torch.argmax(lg2, dim=0)) and int(st2.abs().sum()) == 0


def test_finalize_flags_inf_and_evaluate_case_raises():
    logits, counts, gt, crop, _ = _finalize_case(6, inf=True)
    stats = torch.zeros(4, dtype=torch.int64, device=DEV)
    hb.seg_eval_finalize(logits.to(DEV), counts.to(DEV), stats, crop)
    assert int(stats[0].cpu()) == 1
    img, label = G["thin_img"].astype(np.float32), G["thin_label"].astype(np.float32)
    with pytest.raises(RuntimeError, match="inf"):
        su.evaluate_case(DevToy(scale=6e4), img, label, 1, [8, 16, 16], device=DEV)


def _count_syncs(fn):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            out = fn()
        finally:
            torch.cuda.set_sync_debug_mode(0)
    return out, [w for w in rec if "called a synchronizing" in str(w.message)]


@pytest.mark.parametrize("net", ["toy", "segmodel"])
def test_evaluate_case_makes_one_host_sync(net):
    model = DevToy(sep=4) if net == "toy" else _segmodel()
    g = np.random.RandomState(3)
    img = g.randint(0, 256, size=(1, 10, 70, 80)).astype(np.float32)
    lab = (g.rand(1, 10, 70, 80) < 0.4).astype(np.float32)
    run = lambda: su.evaluate_case(model, img, lab, 4, [8, 32, 32], get_HR_results=True, device=DEV)  # noqa: E731
    first = run()                                                      # warm-up: cached Gaussian, packed weights
    torch.cuda.synchronize()
    out, syncs = _count_syncs(run)
    assert len(syncs) == 1, [str(w.message) for w in syncs]
    assert np.array_equal(out[0], first[0]) and np.array_equal(out[1], first[1]) and out[3] == first[3]
    # the tile loop alone makes none
    stats = torch.zeros(4, dtype=torch.int64, device=DEV)
    vol = su.preprocess_image(img)[0][0].to(DEV)
    torch.cuda.synchronize()
    slicers = su._internal_get_sliding_window_slicers((10, 70, 80), patch_size=[8, 32, 32])
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            lg, cn = su._fused_tiles(vol, (0, 0, 0), slicers, model, 0, False, 1, su._device_gaussian((8, 32, 32),
                                                                                                       str(DEV)))
            hb.seg_eval_finalize(lg, cn, stats)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert int(stats[0].cpu()) == 0


def test_evaluate_cases_global_dice_equals_concatenated_maps(capsys):
    from rehrseg_amd.train_steps import evaluate_cases
    net = DevToy(sep=1)
    g = np.random.RandomState(4)
    cases = []
    for k, shape in enumerate(((1, 5, 24, 13), (1, 12, 40, 50), (1, 9, 33, 47))):
        img = g.randint(0, 256, size=shape).astype(np.float32)
        cases.append((f"c{k}", img, (img + g.randint(-40, 40, size=shape) < 90).astype(np.uint8)))
    mean = evaluate_cases(net, cases, [16, 16, 8], device=DEV)
    out = capsys.readouterr().out
    glob = float(next(line for line in out.splitlines() if line.startswith("Global dice")).split(": ")[1])
    maps, dice = [], []
    for _, img, lab in cases:
        r = su.evaluate_case(net, img, lab, 1, [8, 16, 16], device=DEV)
        maps.append(r[0].ravel())
        dice.append(r[3])
    assert glob == su.calculate_dice(np.concatenate(maps), np.concatenate([c[2].ravel() for c in cases]))
    assert mean == sum(dice) / len(dice)
