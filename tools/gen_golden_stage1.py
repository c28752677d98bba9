"""Fixture for the stage-1 volume preparation (tests/golden/stage1_smore.npz), produced by running the REFERENCE's own
postprocess_smore (utils/sr_utils.py:244-277, the branch without an SR network) in the build container (import recipe:
tools/gen_golden.py) with real scipy on five small merged (x, y, z, 2) volumes: channel 0 smooth random intensities in
[0, ~1000], channel 1 a binary blob.

Stand-ins for what is absent offline, each inside the reference module only:
  parse_image   returns the in-memory array of the "file" it is asked for, the separation it is given, lr_axis 0 and
                the FWHM this repository derives from (separation, 1.0)
  parse_kernel  this repository's Gaussian slice profile (utils/blur_kernel_ops.py), recorded in the fixture; the
                reference asks degrade for 'rf-pulse-slr' (UNPINNED)

Cases (the keys carry the case's name):
  odd      (21, 19, 6, 2) x 4   odd in-plane sizes: partial blocks and blur edges
  wide_x   (70, 9, 3, 2)  x 4   x crosses a 64-wide tile
  wide_y   (9, 70, 2, 2)  x 2   two-sample lines
  tie      (16, 16, 7, 2) x 3   the order-0 tie at output slice 15 (position 4.5)
  single   (5, 4, 1, 2)   x 4   one slice: no recursion, every output equals the input

and `prefilter_x` (9, 70, 6) with scipy.ndimage.spline_filter1d(x, 3, axis, mode='mirror') along each axis, computed in
float64 and rounded to float32 once, for the prefilter kernel on its own.

    python tools/gen_golden_stage1.py     # rewrites tests/golden/stage1_smore.npz
"""
import os
import sys

import numpy as np
import scipy.ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gen_golden import OUT, import_reference  # noqa: E402

CASES = {"odd": ((21, 19, 6), 4), "wide_x": ((70, 9, 3), 4), "wide_y": ((9, 70, 2), 2), "tie": ((16, 16, 7), 3),
         "single": ((5, 4, 1), 4)}
PREFILTER_SHAPE = (9, 70, 6)


def smooth(rng, shape):
    """Random intensities in [0, ~1000], smoothed a little so that neighbouring slices correlate as anatomy does."""
    a = scipy.ndimage.uniform_filter(rng.rand(*shape), size=3, mode="nearest")
    a = (a - a.min()) / (a.max() - a.min())
    return (1000.0 * a).astype(np.float32)


def volume(name, shape):
    rng = np.random.RandomState(sum(map(ord, name)))
    x, y, z = np.meshgrid(*(np.linspace(-1, 1, n) if n > 1 else np.zeros(1) for n in shape), indexing="ij")
    blob = np.exp(-1.5 * ((x - 0.2) ** 2 + (y + 0.1) ** 2 + 0.25 * z ** 2))
    lab = (blob + 0.3 * rng.rand(*shape) > 0.6).astype(np.float32)
    return np.stack([smooth(rng, shape), lab], axis=-1)


def main():
    import rehrseg_amd.utils.blur_kernel_ops as bko
    import rehrseg_amd.utils.parse_image_file as pif
    import_reference()
    import utils.sr_utils as sr

    files, kernels = {}, {}

    def parse_image(path, slice_thickness=None, target_thickness=None):
        a = files[os.path.basename(path)]
        return (a, float(slice_thickness / target_thickness), 0,
                pif.blur_fwhm_voxels(float(slice_thickness), float(target_thickness)), None, None, a.min(), a.max())

    def parse_kernel(fpath, name, fwhm):
        assert fpath is None and name == "rf-pulse-slr"
        return kernels.setdefault(float(fwhm), bko.parse_kernel(None, "gaussian", fwhm))

    sr.parse_image = parse_image
    sr.parse_kernel = parse_kernel

    rec = {}
    for name, (shape, sep) in CASES.items():
        vol = volume(name, shape)
        files[name] = vol
        kernels.clear()
        img_hr, label_hr, fx, fy = sr.postprocess_smore(name, sep, "merge", None)
        (kernel,) = kernels.values()
        Z = int(round(shape[2] * sep))
        assert img_hr.shape == shape[:2] + (Z, 1) and img_hr.dtype == np.float32
        assert label_hr.shape == img_hr.shape and label_hr.dtype == np.uint8
        assert fx.shape == (Z, 1, shape[0], shape[1]) and fy.shape == (Z, 1, shape[1], shape[0])
        assert 0.02 < label_hr.mean() < 0.98 and set(np.unique(label_hr)) == {0, 1}
        rec.update({f"{name}_vol": vol, f"{name}_sep": np.float64(sep), f"{name}_kernel": kernel.numpy().reshape(-1),
                    f"{name}_img_hr": img_hr, f"{name}_label_hr": label_hr, f"{name}_image_x_rgb": fx,
                    f"{name}_image_y_rgb": fy})
    # the tie of the order-0 zoom: position 4.5 at output slice 15 of the 7 -> 21 axis takes slice 5, not the even 4
    t = rec["tie_vol"][..., 1]
    assert (t[..., 4] != t[..., 5]).any() and np.array_equal(rec["tie_label_hr"][..., 15, 0], t[..., 5].astype(np.uint8))

    x = smooth(np.random.RandomState(5), PREFILTER_SHAPE)
    rec["prefilter_x"] = x
    for axis in range(3):
        rec[f"prefilter_axis{axis}"] = scipy.ndimage.spline_filter1d(x, 3, axis=axis, output=np.float64,
                                                                     mode="mirror").astype(np.float32)

    path = os.path.join(OUT, "stage1_smore.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in rec.items() if k.endswith("img_hr")})


if __name__ == "__main__":
    main()
