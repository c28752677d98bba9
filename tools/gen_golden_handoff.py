"""Fixture for the stage-1 -> stage-2 handoff (tests/golden/handoff_flavr.npz), produced by running the REFERENCE's own
inference_flavr and postprocess_flavr (utils/sr_utils.py:137-242, :279-304) in the build container (import recipe:
tools/gen_golden.py) with the deterministic UNet_3D_3D(2, 'unet_18', 4, 4, use_uncertainty=True) of the inference
fixture on one (20, 18, 6, 2) volume: three different extents, channel 0 raw intensities, channel 1 binary.

Stand-ins for what is absent offline or needs a GPU, each inside the reference module only:
  parse_image       returns the in-memory array of the "file" it is asked for, lr_axis 0 (what it yields for every
                    array that is not 2-D), the min / max of that array and a fixed FWHM
  parse_kernel      this repository's Gaussian slice profile (utils/blur_kernel_ops.py), recorded in the fixture
  sitk              keeps written arrays in a dict under their file names
  os.path.exists    looks into that dict
  Tensor.cuda       the identity (apply_to_vol_flavr hard-codes it), as in tools/gen_golden_inference.py
  inv_normalize     the reference's own, wrapped to keep a copy of what it returns (the segmentation channel before
                    inference_flavr thresholds it in place)

ASSUMPTION, UNPINNED: a volume written from a SimpleITK array A is read back by the nibabel stand-in as
A.transpose(2, 1, 0) in float32 (SimpleITK indexes arrays (z, y, x), nibabel (x, y, z)).  Neither library can be run
here; with a direction matrix that is not the identity nibabel's axes may differ.

postprocess_flavr runs twice: as train_all.py drives it (its `_uncertainty` file name never exists: zeros), and with
the written uncertainty map stored under the name it does look for.

    python tools/gen_golden_handoff.py     # rewrites tests/golden/handoff_flavr.npz
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gen_golden import OUT, import_reference, load_det  # noqa: E402

SHAPE = (20, 18, 6, 2)
THICK, TARGET = 4.0, 1.0
REL_BAR = 1e-4          # tests/test_inference_gpu.py's bar on the network output, relative to its largest magnitude
MAX_EXCLUDED = 0.01     # share of label voxels whose pre-threshold value may lie within the bar of 0


def volume():
    rng = np.random.RandomState(11)
    x, y, z = np.meshgrid(*(np.linspace(-1, 1, n) for n in SHAPE[:3]), indexing="ij")
    blob = np.exp(-3.0 * ((x - 0.2) ** 2 + (y + 0.1) ** 2 + 0.5 * z ** 2))
    img = np.round(40.0 + 180.0 * blob + 25.0 * rng.rand(*SHAPE[:3]))          # integer intensities 40 .. 245
    lab = (blob + 0.1 * rng.rand(*SHAPE[:3]) > 0.6).astype(np.float32)
    return np.stack([img.astype(np.float32), lab], axis=-1)


class _Image:
    def __init__(self, array):
        self.array = np.array(array)

    def SetSpacing(self, *_):
        pass

    SetOrigin = SetDirection = SetSpacing

    def GetSpacing(self):
        return (1.0, 1.0, THICK)

    def GetOrigin(self):
        return (0.0, 0.0, 0.0)

    def GetDirection(self):
        return (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


def main():
    import rehrseg_amd.utils.blur_kernel_ops as bko
    import rehrseg_amd.utils.parse_image_file as pif
    fa = import_reference()
    import utils.sr_utils as sr

    files, kept = {}, []
    fwhm = pif.blur_fwhm_voxels(THICK, TARGET)
    kernel = bko.parse_kernel(None, "gaussian", fwhm)

    def parse_image(path, slice_thickness=None, target_thickness=None):
        a = files[path]
        return a, float(slice_thickness / target_thickness), 0, fwhm, None, None, a.min(), a.max()

    def write(img, path):
        files[path] = img.array.transpose(2, 1, 0).astype(np.float32)      # the unpinned read-back, see above

    ref_inv = sr.inv_normalize

    def inv_normalize(*a, **k):
        r = ref_inv(*a, **k)
        kept.append(np.array(r))
        return r

    sr.parse_image = parse_image
    sr.parse_kernel = lambda *a, **k: kernel
    sr.inv_normalize = inv_normalize
    sr.sitk = types.SimpleNamespace(ReadImage=lambda p: _Image(np.zeros(1)), GetImageFromArray=_Image, WriteImage=write)
    sr.os = types.SimpleNamespace(path=types.SimpleNamespace(join=os.path.join, exists=lambda p: p in files))

    model = fa.UNet_3D_3D(2, "unet_18", 4, 4, batchnorm=False, joinType="concat", upmode="transpose",
                          use_uncertainty=True).eval()
    load_det(model)
    vol = volume()
    files["in/case.nii.gz"] = vol
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        sr.inference_flavr(model, "img+seg", "in/case.nii.gz", "ref/case.nii.gz", "out/case.nii.gz", THICK, TARGET,
                           "cpu", False)
        sr.inference_flavr(model, "uncertainty", "in/case.nii.gz", "ref/case.nii.gz", "out/case.nii.gz", THICK, TARGET,
                           "cpu", True)
    finally:
        torch.Tensor.cuda = orig_cuda
    assert len(kept) == 2
    back = lambda a: np.ascontiguousarray(a.transpose(2, 1, 0))  # noqa: E731  undo the read-back: the written arrays
    rec = {"vol": vol, "kernel": kernel.numpy().reshape(-1), "sep": np.float64(THICK / TARGET),
           "img": back(files["out/case_img.nii.gz"]), "seg": back(files["out/case_seg.nii.gz"]).astype(np.uint8),
           "uncertainty": back(files["out/case_uncertainty.nii.gz"]),
           "seg_pre": np.ascontiguousarray(kept[0][:, :, 1, :]),
           "net_absmax": np.float32(np.abs((kept[0] - vol.min()) / (vol.max() - vol.min())).max())}
    assert rec["img"].shape == (4 * (SHAPE[2] - 1), SHAPE[1], SHAPE[0]) and rec["seg_pre"].shape == rec["img"].shape
    assert np.array_equal(rec["seg"], (rec["seg_pre"] > 0).astype(np.uint8))

    image, label, unc = sr.postprocess_flavr("case.nii.gz", int(THICK / TARGET), "out")
    rec.update(post_img=image, post_seg=label.astype(np.uint8), post_unc_absent=unc.astype(np.uint8))
    assert not unc.any() and image.shape == SHAPE[:2] + (4 * (SHAPE[2] - 1),)
    files["out/case.nii.gz"] = files["out/case_uncertainty.nii.gz"]     # the name postprocess_flavr looks for
    image2, label2, unc2 = sr.postprocess_flavr("case.nii.gz", int(THICK / TARGET), "out")
    assert unc2.dtype == np.uint8 and np.array_equal(image2, image) and np.array_equal(label2, label)
    rec["post_unc"] = unc2

    # the label check leaves out voxels whose pre-threshold value is within the image bar of 0: at most 1 % may be
    bar = REL_BAR * float(rec["net_absmax"]) * float(vol.max() - vol.min())
    excluded = float((np.abs(rec["seg_pre"]) <= bar).mean())
    assert excluded <= MAX_EXCLUDED, excluded
    assert 0.02 < rec["seg"].mean() < 0.98 and len(np.unique(unc2)) > 16 and np.ptp(rec["img"]) > 10

    path = os.path.join(OUT, "handoff_flavr.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes; bar", bar, "excluded share", excluded, "label share",
          float(rec["seg"].mean()), "img range", float(rec["img"].min()), float(rec["img"].max()),
          "unc range", float(rec["uncertainty"].min()), float(rec["uncertainty"].max()))


if __name__ == "__main__":
    main()
