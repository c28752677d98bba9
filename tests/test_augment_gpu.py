"""The device augmentation chain (csrc/augment.hip, rehrseg_amd/utils/augment.py) against the fixtures of
tools/gen_golden_augment.py, and its place in both training data sets."""
import glob
import os
import random

import numpy as np
import pytest
import torch

from feed_cases import EFF_CASES, KERNEL, MULTI_CASES, volumes_multi, volumes_seg
from rehrseg_amd.utils import augment as A
from rehrseg_amd.utils.seg_utils import get_training_transforms

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SPATIAL = sorted(glob.glob(os.path.join(GOLDEN, "augment_spatial_*.npz")))
ROT = {"x": (-np.pi, np.pi), "y": (0, 0), "z": (0, 0)}


def _load(path):
    with np.load(path) as f:
        return {k: f[k] for k in f.files}


def _np(t):
    return t.detach().cpu().numpy()


def _close(a, b, tol=1e-5):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = np.abs(a - b).max() / max(np.abs(b).max(), 1e-12)
    assert err < tol, err


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32).to(DEV)


@pytest.mark.parametrize("path", SPATIAL, ids=lambda p: os.path.basename(p)[:-4])
def test_warp_against_the_reference(path):
    g = _load(path)
    angle, scale = float(g["angle"]), float(g["scale"])
    draw = {"angle": None if np.isnan(angle) else angle, "scale": None if np.isnan(scale) else scale}
    keys = {k[3:]: _t(g[k]) for k in g if k.startswith("in_")}
    img = {"data", "uncertainty"}
    out = A.warp_keys([draw], keys, img, tuple(int(v) for v in g["out_hw"]))
    _close(_np(out["data"]), g["out_data"])
    for key in ("seg", "seg_sr"):
        np.testing.assert_array_equal(_np(out[key]), g["out_" + key].astype(np.float32), err_msg=key)
    if "uncertainty" in keys:
        _close(_np(out["uncertainty"]), g["out_uncertainty"])


def _intensity(x, **p):
    tr = A.TrainingTransforms(None, ROT["x"], False, False, [])
    return _np(tr.apply([{"intensity": p}], data=_t(x)[None, None])["data"])[0, 0]


def test_each_intensity_transform():
    g = _load(os.path.join(GOLDEN, "augment_intensity.npz"))
    x = g["x"]
    for s in (0.5, 0.83):
        _close(_intensity(x, blur=s), g[f"blur_{s}"])
    _close(_intensity(x, brightness=1.17), g["brightness_1.17"])
    for f in (0.8, 1.2):
        _close(_intensity(x, contrast=f), g[f"contrast_{f}"])
    for z in (0.5, 0.61, 0.93):
        _close(_intensity(x, lowres=z), g[f"lowres_{z}"])
    for gm in (0.75, 1.4):
        _close(_intensity(x, gamma=gm), g[f"gamma_{gm}"])
        _close(_intensity(x, gamma_inv=gm), g[f"gamma_inv_{gm}"])


def test_noise_moments_and_determinism():
    x = np.zeros((4, 64, 64), np.float32)
    a = _intensity(x, noise=(0.05, 1234))
    b = _intensity(x, noise=(0.05, 1234))
    np.testing.assert_array_equal(a, b)
    assert abs(a.mean()) < 2e-3 and abs(a.std() - 0.05) < 2e-3
    assert not np.array_equal(a, _intensity(x, noise=(0.05, 1235)))


def test_whole_chain_under_a_seed():
    g = _load(os.path.join(GOLDEN, "augment_chain.npz"))
    tr = get_training_transforms([3, 24, 32], ROT, None, None, True, use_mask_for_norm=[False],
                                 extra_keys=["seg", "seg_sr"])
    np.random.seed(int(g["seed"]))
    out = tr(data=_t(g["in_data"]), seg=_t(g["in_seg"]), seg_sr=_t(g["in_seg_sr"]))
    assert np.random.uniform() == float(g["next_uniform"])  # the draws consumed equal the reference's
    _close(_np(out["data"]), g["out_data"])
    np.testing.assert_array_equal(_np(out["seg"]), g["out_seg"].astype(np.float32))
    np.testing.assert_array_equal(_np(out["seg_sr"]), g["out_seg_sr"].astype(np.float32))


def _multi(name, nnunet):
    from rehrseg_amd.utils.train_set import TrainSetMultiple
    shapes, ps, sep, blur, flip, seed, draws = MULTI_CASES[name]
    return TrainSetMultiple(None, list(range(len(shapes))), sep, 1.0, None, None, ps, flip, DEV, blur=blur,
                            volumes=volumes_multi(seed, shapes), blur_kernel=KERNEL, nnunet_transform=nnunet)


@pytest.mark.parametrize("batched", [False, True])
def test_stage1_nnunet_transform(batched):
    name = "multi_2d_blur"
    draws = MULTI_CASES[name][-1]
    plain, aug = _multi(name, False), _multi(name, True)
    outs = []
    for ds in (plain, aug):
        random.seed(5)
        np.random.seed(3)
        if batched:
            o = []
            for k in range(0, draws, 2):
                lr, hr = ds.batch([k % 2, (k + 1) % 2])
                o += [(lr[0], hr[0]), (lr[1], hr[1])]
        else:
            o = [ds[k % 2] for k in range(draws)]
        outs.append([(_np(lr), _np(hr)) for lr, hr in o])
    differs = 0
    for (lr0, hr0), (lr1, hr1) in zip(*outs):
        np.testing.assert_array_equal(lr1, lr0)                 # LR image (blurred source) and LR label
        np.testing.assert_array_equal(hr1[1], hr0[1])           # HR label
        differs += not np.array_equal(hr1[0], hr0[0])
    assert differs > 0


def test_stage1_without_blur_derives_lr_from_the_augmented_hr():
    from rehrseg_amd.utils.train_set import TrainSetMultiple
    shapes, ps, sep, blur, flip, seed, draws = MULTI_CASES["multi_3d_noblur"]
    ds = TrainSetMultiple(None, [0], sep, 1.0, None, None, ps, flip, DEV, blur=False,
                          volumes=volumes_multi(seed, shapes), nnunet_transform=True)
    random.seed(1)
    np.random.seed(1)
    lr, hr = ds[0]
    assert lr.shape[0] == 2 and hr.shape[0] == 2
    assert torch.isfinite(lr).all() and torch.isfinite(hr).all()


def _eff(target, unc=True):
    from rehrseg_amd.utils.train_set import TrainSetMultipleSegSREfficient
    shapes, ps, sep, _, flip, norm, seed, draws = EFF_CASES["eff_unc"]
    return TrainSetMultipleSegSREfficient(None, list(range(len(shapes))), float(sep), 1.0, ps, target, flip, unc,
                                          norm=norm, device=DEV, volumes=volumes_seg(seed, shapes),
                                          train_transform="nnunet")


def test_stage2_nnunet_transform():
    target = (6, 8, 3)  # (x, y, z): in-plane (y, x) = (8, 6) out of the (10, 10) patch
    ds = _eff(target)
    random.seed(2)
    np.random.seed(4)
    single = [ds[k % 2] for k in range(8)]
    for img, lab_lr, lab, u in single:
        assert tuple(img.shape[-2:]) == (8, 6) and tuple(lab.shape[-2:]) == (8, 6)
        assert tuple(u.shape) == tuple(img.shape) and tuple(lab_lr.shape) == tuple(img.shape)
        assert img.dtype == torch.float32 and u.dtype == torch.float32
        assert set(np.unique(_np(lab_lr))) <= {0.0, 1.0} and set(np.unique(_np(lab))) <= {0.0, 1.0}
    random.seed(2)
    np.random.seed(4)
    batched = []
    for k in range(0, 8, 2):
        b = ds.batch([0, 1])
        batched += [tuple(o[j] for o in b) for j in range(2)]
    for s, b in zip(single, batched):
        for x, y in zip(s, b):
            np.testing.assert_array_equal(_np(x), _np(y))


def test_stage2_chain_does_not_synchronise():
    ds = _eff((6, 8, 3))
    random.seed(0)
    np.random.seed(0)
    for _ in range(8):  # warm-up: cached prefilter tables, first-touch allocations
        ds.batch([0, 1])
    torch.cuda.synchronize()
    np.random.seed(12)
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(16):  # enough items that every transform fires at least once (see below)
            ds.batch([0, 1])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    np.random.seed(12)
    tr = ds.train_transform
    fired = set()
    for _ in range(16):
        for d in tr.draw(2):
            fired |= set(d["intensity"]) | {k for k, v in d["spatial"].items() if v is not None}
    assert {"blur", "lowres", "contrast", "gamma", "angle", "scale"} <= fired, fired
