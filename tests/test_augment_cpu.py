"""Host side of the device augmentation chain (rehrseg_amd/utils/augment.py): the spatial draw protocol against the
reference's own augment_spatial (tests/golden/augment_spatial_*.npz, tools/gen_golden_augment.py), the host tap
tables (prefilter, Gaussian, zoom) through the CPU emulation of the kernels against the fixtures, and the refusal of
arguments REHRSeg never passes."""
import glob
import os

import numpy as np
import pytest

import augment_emu as E
from rehrseg_amd.utils import augment as A
from rehrseg_amd.utils.seg_utils import get_training_transforms

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SPATIAL = sorted(glob.glob(os.path.join(GOLDEN, "augment_spatial_*.npz")))
ROT = {"x": (-np.pi, np.pi), "y": (0, 0), "z": (0, 0)}


def _load(path):
    with np.load(path) as f:
        return {k: f[k] for k in f.files}


def _close(a, b, tol=1e-5):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    err = np.abs(a - b).max() / max(np.abs(b).max(), 1e-12)
    assert err < tol, err


def test_fixtures_cover_the_cases():
    names = {os.path.basename(p)[len("augment_spatial_"):-4] for p in SPATIAL}
    assert {"rot_scale_up", "rot_scale_down", "rot_only", "crop_only", "scale_down"} <= names
    cases = [_load(p) for p in SPATIAL]
    assert any(c["n_labels"] == 3 for c in cases)
    assert any("out_uncertainty" in c for c in cases) and any("out_uncertainty" not in c for c in cases)


@pytest.mark.parametrize("path", SPATIAL, ids=lambda p: os.path.basename(p)[:-4])
def test_spatial_draw_protocol(path):
    g = _load(path)
    np.random.seed(int(g["seed"]))
    d = A.draw_spatial(ROT["x"])
    for key in ("angle", "scale"):
        want = float(g[key])
        assert (d[key] is None) == np.isnan(want)
        if d[key] is not None:
            assert d[key] == want
    assert np.random.uniform() == float(g["next_uniform"])


@pytest.mark.parametrize("path", SPATIAL, ids=lambda p: os.path.basename(p)[:-4])
def test_spatial_emulation(path):
    g = _load(path)
    angle, scale = float(g["angle"]), float(g["scale"])
    draw = {"angle": None if np.isnan(angle) else angle, "scale": None if np.isnan(scale) else scale}
    hw = tuple(g["in_data"].shape[2:])
    p = A.warp_params(draw, hw)
    out_hw = tuple(int(v) for v in g["out_hw"])
    _close(E.spatial(g["in_data"][0], p, out_hw), g["out_data"][0])
    for key in ("seg", "seg_sr"):
        np.testing.assert_array_equal(E.warp(g["in_" + key][0].astype(np.float32), p, out_hw, True),
                                      g["out_" + key][0])
    if "in_uncertainty" in g:
        _close(E.spatial(g["in_uncertainty"][0], p, out_hw), g["out_uncertainty"][0])


def test_intensity_tap_tables():
    g = _load(os.path.join(GOLDEN, "augment_intensity.npz"))
    x = g["x"]
    for s in (0.5, 0.83):
        _close(E.blur(x, s), g[f"blur_{s}"])
    for z in (0.5, 0.61, 0.93):
        _close(E.lowres(x, z), g[f"lowres_{z}"])


def test_chain_draws_match_the_fixture():
    g = _load(os.path.join(GOLDEN, "augment_chain.npz"))
    np.random.seed(int(g["seed"]))
    tr = get_training_transforms([3, 24, 32], ROT, None, None, True, use_mask_for_norm=[False],
                                 extra_keys=["seg", "seg_sr"])
    d = tr.draw(1)[0]
    assert repr(sorted(d["intensity"].items())) == str(g["params"])
    assert "noise" not in d["intensity"]
    assert np.random.uniform() == float(g["next_uniform"])


@pytest.mark.parametrize("kw", [dict(deep_supervision_scales=[[1, 1, 1]]), dict(mirror_axes=(0, 1)),
                                dict(do_dummy_2d_data_aug=False), dict(order_resampling_data=1),
                                dict(order_resampling_seg=0), dict(border_val_seg=0), dict(use_mask_for_norm=[True]),
                                dict(is_cascaded=True), dict(regions=[1]), dict(ignore_label=2)])
def test_unsupported_arguments_raise(kw):
    args = dict(patch_size=[3, 24, 32], rotation_for_DA=ROT, deep_supervision_scales=None, mirror_axes=None,
                do_dummy_2d_data_aug=True)
    args.update(kw)
    with pytest.raises(NotImplementedError):
        get_training_transforms(**args)


def test_my_spatial_transform_refuses_3d_and_elastic():
    with pytest.raises(NotImplementedError):
        A.MySpatialTransform([8, 8, 8], random_crop=False, border_mode_data="constant", border_cval_seg=-1,
                             order_seg=1, do_elastic_deform=False)
    with pytest.raises(NotImplementedError):
        A.MySpatialTransform([8, 8], random_crop=False, border_mode_data="constant", border_cval_seg=-1, order_seg=1,
                             do_elastic_deform=True, p_el_per_sample=1)
