"""Fixtures of the device augmentation chain (rehrseg_amd/utils/augment.py): tests/golden/augment_*.npz.

Spatial cases run the REFERENCE's own MySpatialTransform / augment_spatial (utils/seg_utils.py:377-630) under a
seeded np.random, with stand-ins registered for its absent imports (SimpleITK, acvl_utils, nnunetv2, batchgenerators:
see tools/gen_golden.py).  The batchgenerators coordinate helpers and interpolate_img it calls are restated below over
scipy.ndimage; the stand-in rotate_coords_2d / scale_coords record the angle and scale the reference drew.

Intensity cases are restatements of batchgenerators 0.25 (noise_transforms, color_transforms,
resample_augmentations) and skimage.transform.resize (ndimage.zoom, grid_mode=True, mode 'nearest', clip) with
explicit parameters; the chain case composes the reference's spatial step with them under a seed at which noise
does not fire (draws from np.random where batchgenerators uses Python's random, as the port does).

    python tools/gen_golden_augment.py      # rewrites tests/golden/augment_*.npz
"""
import os
import sys
import types

import numpy as np
import scipy.ndimage as ndi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gen_golden import OUT, _Finder  # noqa: E402

RECORD = {}


# ----------------------------------------------------------------------------- batchgenerators helpers, restated
def create_zero_centered_coordinate_mesh(shape):
    tmp = tuple([np.arange(i) for i in shape])
    coords = np.array(np.meshgrid(*tmp, indexing="ij")).astype(float)
    for d in range(len(shape)):
        coords[d] -= ((np.array(shape).astype(float) - 1) / 2.)[d]
    return coords


def rotate_coords_2d(coords, angle):
    RECORD["angle"] = angle
    rot = np.array([[np.cos(angle), -np.sin(angle)], [np.sin(angle), np.cos(angle)]])
    return np.dot(coords.reshape(len(coords), -1).transpose(), rot).transpose().reshape(coords.shape)


def scale_coords(coords, scale):
    RECORD["scale"] = scale
    return coords * scale


def interpolate_img(img, coords, order=3, mode="nearest", cval=0.0, is_seg=False):
    if is_seg and order != 0:
        unique_labels = np.unique(img)
        result = np.zeros(coords.shape[1:], img.dtype)
        for c in unique_labels:
            res_new = ndi.map_coordinates((img == c).astype(float), coords, order=order, mode=mode, cval=cval)
            result[res_new >= 0.5] = c
        return result
    return ndi.map_coordinates(img.astype(float), coords, order=order, mode=mode, cval=cval).astype(img.dtype)


def _unused(*a, **k):
    raise RuntimeError("not used on the path of these fixtures")


def import_reference_seg_utils():
    m = types.ModuleType("batchgenerators.augmentations.utils")
    m.__dict__.update(create_zero_centered_coordinate_mesh=create_zero_centered_coordinate_mesh,
                      rotate_coords_2d=rotate_coords_2d, scale_coords=scale_coords, interpolate_img=interpolate_img,
                      elastic_deform_coordinates=_unused, rotate_coords_3d=_unused, resize_segmentation=_unused,
                      resize_multichannel_image=_unused, elastic_deform_coordinates_2=_unused)
    sys.meta_path.insert(0, _Finder())
    sys.modules["batchgenerators.augmentations.utils"] = m
    sys.path.insert(0, "/root/reference")
    import utils.seg_utils as su
    return su


def spatial_transform(su, out_hw, extra_keys, enable_uncertainty):
    """MySpatialTransform exactly as get_training_transforms builds it (utils/seg_utils.py:656-670)."""
    return su.MySpatialTransform(
        out_hw, patch_center_dist_from_border=None, do_elastic_deform=False, alpha=(0, 0), sigma=(0, 0),
        do_rotation=True, angle_x=(-np.pi, np.pi), angle_y=(0, 0), angle_z=(0, 0), p_rot_per_axis=1, do_scale=True,
        scale=(0.7, 1.4), border_mode_data="constant", border_cval_data=0, order_data=3, border_mode_seg="constant",
        border_cval_seg=-1, order_seg=1, random_crop=False, label_key=extra_keys, p_el_per_sample=0,
        p_scale_per_sample=0.2, p_rot_per_sample=0.2, independent_scale_for_each_axis=False,
        enable_uncertainty=enable_uncertainty)


# ----------------------------------------------------------------------------- intensity transforms, restated
def gauss_blur(x, sigma):
    return ndi.gaussian_filter(x, sigma, order=0)


def brightness(x, m):
    return x * m


def contrast(x, factor):
    mn, minm, maxm = x.mean(), x.min(), x.max()
    y = (x - mn) * factor + mn
    y[y < minm] = minm
    y[y > maxm] = maxm
    return y


def sk_resize(x, shape, order):
    """skimage resize(mode='edge', anti_aliasing=False, clip=True) of a float64 image."""
    zoom = [o / i for o, i in zip(shape, x.shape)]
    out = ndi.zoom(x, zoom, order=order, mode="nearest", grid_mode=True)
    return np.clip(out, x.min(), x.max())


def lowres(x, zoom, ignore_axes=(0,)):
    shp = np.array(x.shape)
    tgt = np.round(shp * zoom).astype(int)
    for i in ignore_axes:
        tgt[i] = shp[i]
    down = sk_resize(x.astype(float), tgt, 0)
    return sk_resize(down, shp, 3).astype(x.dtype)


def gamma(x, g, invert, eps=1e-7):
    if invert:
        x = -x
    mn, sd = x.mean(), x.std()
    minm = x.min()
    rnge = x.max() - minm
    x = np.power(((x - minm) / float(rnge + eps)), g) * float(rnge + eps) + minm
    x = x - x.mean()
    x = x / (x.std() + 1e-8) * sd
    x = x + mn
    return -x if invert else x


def _either(lo, hi):
    if np.random.random() < 0.5 and lo < 1:
        return np.random.uniform(lo, 1)
    return np.random.uniform(max(lo, 1), hi)


def intensity_chain(x):
    """get_training_transforms :678-688 on one (z, y, x) single-channel item; returns the output and the parameters."""
    p = {}
    if np.random.uniform() < 0.1:
        raise RuntimeError("noise fired: pick another seed")
    if np.random.uniform() < 0.2 and np.random.uniform() <= 0.5:
        p["blur"] = np.random.uniform(0.5, 1.0)
        x = gauss_blur(x, p["blur"])
    if np.random.uniform() < 0.15:
        np.random.uniform(0.75, 1.25)
        p["brightness"] = np.random.uniform(0.75, 1.25)
        x = brightness(x, p["brightness"])
    if np.random.uniform() < 0.15 and np.random.uniform() < 1:
        p["contrast"] = _either(0.75, 1.25)
        x = contrast(x, p["contrast"])
    if np.random.uniform() < 0.25 and np.random.uniform() < 0.5:
        p["lowres"] = np.random.uniform(0.5, 1)
        x = lowres(x, p["lowres"])
    for key, inv, prob in (("gamma_inv", True, 0.1), ("gamma", False, 0.3)):
        if np.random.uniform() < prob:
            p[key] = _either(0.7, 1.5)
            x = gamma(x, p[key], inv)
    return x, p


# ----------------------------------------------------------------------------- cases
def volumes(rs, depth_lr, depth_hr, hw, n_labels):
    img = rs.standard_normal((1, 1, depth_lr) + hw).astype(np.float32)
    img = ndi.gaussian_filter(img, (0, 0, 0, 2, 2)).astype(np.float32) * 3
    lab_hr = np.zeros((1, 1, depth_hr) + hw, np.uint8)
    yy, xx = np.mgrid[:hw[0], :hw[1]]
    for k in range(1, n_labels):
        r = rs.uniform(5, 12)
        cy, cx = rs.uniform(8, hw[0] - 8), rs.uniform(8, hw[1] - 8)
        lab_hr[..., (yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = k
    lab_hr[..., ::2, :, :] = np.roll(lab_hr[..., ::2, :, :], 2, axis=-1)
    lab_lr = lab_hr[:, :, ::depth_hr // depth_lr]
    unc = (1 - rs.randint(0, 256, (1, 1, depth_lr) + hw) / 255. * 0.99).astype(np.float32)
    return img, lab_lr, lab_hr, unc


def spatial_case(su, name, seed, want, n_labels, unc, hw=(40, 48), out_hw=(24, 32)):
    rs = np.random.RandomState(1000 + seed)
    img, lab_lr, lab_hr, u = volumes(rs, 3, 6, hw, n_labels)
    keys = ["seg", "seg_sr"] + (["uncertainty"] if unc else [])
    tr = spatial_transform(su, list(out_hw), keys, unc)
    d = {"data": img[0][None].reshape(1, 3, *hw).copy(), "seg": lab_lr.reshape(1, 3, *hw).copy(),
         "seg_sr": lab_hr.reshape(1, 6, *hw).copy()}
    if unc:
        d["uncertainty"] = u.reshape(1, 3, *hw).copy()
    RECORD.clear()
    np.random.seed(seed)
    out = tr(**{k: v.copy() for k, v in d.items()})
    nxt = np.random.uniform()
    angle, scale = RECORD.get("angle"), RECORD.get("scale")
    got = (angle is not None, scale is not None, None if scale is None else scale > 1)
    assert all(w is None or w == g for w, g in zip(want, got)), (name, want, got)
    rec = {"seed": seed, "in_data": d["data"], "in_seg": d["seg"], "in_seg_sr": d["seg_sr"],
           "out_data": out["data"], "out_seg": out["seg"], "out_seg_sr": out["seg_sr"],
           "angle": np.float64(np.nan if angle is None else angle),
           "scale": np.float64(np.nan if scale is None else scale), "next_uniform": np.float64(nxt),
           "out_hw": np.array(out_hw), "n_labels": n_labels}
    if unc:
        rec["in_uncertainty"], rec["out_uncertainty"] = d["uncertainty"], out["uncertainty"]
    return rec


def find_seed(su, start, want):
    """first seed from `start` whose spatial draw has (rotation?, scale?, scale > 1?) == want (None: either)."""
    for seed in range(start, start + 5000):
        np.random.seed(seed)
        rot = np.random.uniform() < 0.2
        if rot:
            np.random.uniform(), np.random.uniform()
        sc = np.random.uniform() < 0.2
        up = None
        if sc:
            up = not (np.random.random() < 0.5)
        got = (rot, sc, up)
        if all(w is None or w == g for w, g in zip(want, got)):
            return seed
    raise RuntimeError(want)


def main():
    su = import_reference_seg_utils()
    os.makedirs(OUT, exist_ok=True)
    cases = {"rot_scale_up": ((True, True, True), 3, True), "rot_scale_down": ((True, True, False), 2, False),
             "rot_only": ((True, False, None), 3, False), "crop_only": ((False, False, None), 3, True),
             "scale_down": ((False, True, False), 3, False)}
    for i, (name, (want, n_labels, unc)) in enumerate(cases.items()):
        seed = find_seed(su, 100 * i, want)
        np.savez_compressed(os.path.join(OUT, f"augment_spatial_{name}.npz"),
                            **spatial_case(su, name, seed, want, n_labels, unc))

    rs = np.random.RandomState(7)
    x = ndi.gaussian_filter(rs.standard_normal((3, 24, 32)), (0, 1.5, 1.5)).astype(np.float32) * 2 + 0.3
    rec = {"x": x}
    for s in (0.5, 0.83):
        rec[f"blur_{s}"] = gauss_blur(x.copy(), s)
    rec["brightness_1.17"] = brightness(x.copy(), 1.17)
    for f in (0.8, 1.2):
        rec[f"contrast_{f}"] = contrast(x.copy(), f)
    for z in (0.5, 0.61, 0.93):
        rec[f"lowres_{z}"] = lowres(x.copy(), z)
    for g in (0.75, 1.4):
        rec[f"gamma_{g}"] = gamma(x.copy(), g, False)
        rec[f"gamma_inv_{g}"] = gamma(x.copy(), g, True)
    np.savez_compressed(os.path.join(OUT, "augment_intensity.npz"), **rec)

    # whole chain (spatial + intensity) of one stage-2 style item under a seed at which noise does not fire and at
    # least three intensity transforms do
    rs = np.random.RandomState(11)
    img, lab_lr, lab_hr, _ = volumes(rs, 3, 6, (40, 48), 3)
    for seed in range(20000):
        np.random.seed(seed)
        tr = spatial_transform(su, [24, 32], ["seg", "seg_sr"], False)
        d = {"data": img.reshape(1, 3, 40, 48).copy(), "seg": lab_lr.reshape(1, 3, 40, 48).copy(),
             "seg_sr": lab_hr.reshape(1, 6, 40, 48).copy()}
        RECORD.clear()
        out = tr(**d)
        try:
            y, p = intensity_chain(out["data"][0].copy())
        except RuntimeError:
            continue
        if len(p) >= 3 and "lowres" in p and RECORD:
            break
    np.savez_compressed(os.path.join(OUT, "augment_chain.npz"), seed=seed, in_data=img, in_seg=lab_lr,
                        in_seg_sr=lab_hr, out_data=y[None, None], out_seg=out["seg"][None],
                        out_seg_sr=out["seg_sr"][None], next_uniform=np.float64(np.random.uniform()),
                        params=np.array(repr(sorted(p.items()))),
                        angle=np.float64(RECORD.get("angle", np.nan)), scale=np.float64(RECORD.get("scale", np.nan)))
    print("seed", seed, p, RECORD)


if __name__ == "__main__":
    main()
