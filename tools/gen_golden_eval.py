"""Fixture for stage-2 validation (tests/golden/eval_case.npz), produced by running the REFERENCE's own
evaluate_case and calculate_dice (utils/seg_utils.py:730-784) in the build container (import recipe:
tools/gen_golden.py) with tests/toy_models.ToySegNet as the network.

Stand-ins for what is absent offline or needs a GPU, each for the duration of the call only:
  read_image        returns the array it is given (the cases are in memory; SimpleITK is absent)
  pad_nd_image      the mirror's restatement of acvl_utils' (parity unpinned)
  compute_gaussian  the mirror's restatement of nnunetv2's (parity unpinned)
  torch.device      'cuda' maps to the CPU inside the reference module (its predictor hard-codes the device), the
                    same trick tools/gen_golden_inference.py plays with `.cuda()`

Two cases, both with get_HR_results=True and slice_separation=2: one thinner than the tile in depth and narrower in
width (the padding and its revert slicer matter), one with several tiles along every axis.

    python tools/gen_golden_eval.py     # rewrites tests/golden/eval_case.npz
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gen_golden import OUT, import_reference  # noqa: E402
from toy_models import ToySegNet  # noqa: E402

CASES = (("thin", (1, 5, 24, 13), [8, 16, 16]), ("multi", (1, 12, 40, 50), [6, 16, 20]))
SEP = 2


class _TorchOnCPU(types.ModuleType):
    """`torch` as the reference module sees it, with torch.device('cuda') answering the CPU."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def device(*a, **k):
        if a and str(a[0]).startswith("cuda"):
            return torch.device("cpu")
        return torch.device(*a, **k)


def case_inputs(shape, seed):
    rng = np.random.RandomState(seed)
    raw = rng.randint(0, 256, size=shape).astype(np.uint8)            # integer intensities, as a scanner stores them
    # the toy network's class 1 favours dark voxels near the volume's origin: so does the label
    label = (raw.astype(np.float32) + rng.randint(-40, 40, size=shape) < 60).astype(np.uint8)
    return raw, label


def main():
    import rehrseg_amd.utils.seg_utils as mirror
    import_reference()
    import utils.seg_utils as su

    su.read_image = lambda x: (np.asarray(x, dtype=np.float32), {})
    su.pad_nd_image = mirror.pad_nd_image
    su.compute_gaussian = mirror.compute_gaussian
    su.torch = _TorchOnCPU("torch")

    rec = {"sep": np.int64(SEP)}
    net = ToySegNet(sep=SEP)
    for i, (tag, shape, patch) in enumerate(CASES):
        raw, label = case_inputs(shape, i)
        pred_lr, pred_hr, lr_label, dice = su.evaluate_case(net, raw.astype(np.float32), label.astype(np.float32),
                                                            slice_separation=SEP, patch_size=patch,
                                                            get_HR_results=True)
        rec.update({f"{tag}_img": raw, f"{tag}_label": label, f"{tag}_patch": np.asarray(patch, np.int64),
                    f"{tag}_pred_lr": pred_lr, f"{tag}_pred_hr": pred_hr,
                    f"{tag}_lr_label": lr_label.numpy().astype(np.float32), f"{tag}_dice_lr": np.float64(dice)})
        assert pred_lr.dtype == np.uint8 and pred_hr.dtype == np.uint8 and 0.05 < dice < 0.95, (tag, dice)
    # calculate_dice on its own: uint8 maps (numpy's uint64 sums), and a float32 label map (float32 sums)
    rng = np.random.RandomState(7)
    a = (rng.rand(3, 17, 19) > 0.6).astype(np.uint8)
    b = (rng.rand(3, 17, 19) > 0.5).astype(np.uint8)
    rec.update(dice_a=a, dice_b=b, dice_u8=np.float64(su.calculate_dice(a, b)),
               dice_f32=np.float64(su.calculate_dice(a, b.astype(np.float32))),
               dice_smooth=np.float64(su.calculate_dice(a * 0, b * 0, smooth=1.0)))
    path = os.path.join(OUT, "eval_case.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes",
          {k: float(v) for k, v in rec.items() if k.endswith("dice_lr") or k.startswith("dice_") and v.ndim == 0})


if __name__ == "__main__":
    main()
