"""Fixture for the intensity normalisations (tests/golden/intensity_norm.npz), produced by running the REFERENCE's own
percentile_normalization and zeroone_normalization (utils/seg_utils.py:74-135) in the build container (import recipe:
tools/gen_golden.py): the array branch on a 3-D array and on the 5-D volume taken as one item, the tensor branch on
the (2, 1, 5, 9, 11) volume, percentile_normalization also with (5, 95, strictlyPositive=False) on data with
negative values.  Data: non-negative, about 40 % exact zeros, a heavy right tail.  The numpy version is recorded:
under numpy 2 the reference's percentile results are float64 (its float64 bounds promote), under numpy 1 float32.

    python tools/gen_golden_intensity.py     # rewrites tests/golden/intensity_norm.npz
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gen_golden import OUT, import_reference  # noqa: E402


def volume(shape, seed):
    g = np.random.RandomState(seed)
    x = np.exp(g.randn(*shape) * 1.2 + 4.0)
    x[g.rand(*shape) < 0.4] = 0.0
    return x.astype(np.float32)


def main():
    import_reference()
    import utils.seg_utils as su

    vol5, arr3 = volume((2, 1, 5, 9, 11), 0), volume((7, 10, 13), 1)
    shifted = arr3 - np.float32(60.0)
    rec = {"numpy_version": np.array(np.__version__), "vol5": vol5, "arr3": arr3, "shifted": shifted}
    rec["perc_arr3"] = su.percentile_normalization(arr3.copy())
    rec["perc_vol5_array"] = su.percentile_normalization(vol5.copy())
    rec["perc_vol5_tensor"] = su.percentile_normalization(torch.from_numpy(vol5.copy())).numpy()
    rec["perc_shifted_5_95"] = su.percentile_normalization(shifted.copy(), 5, 95, False)
    rec["perc_shifted_pos"] = su.percentile_normalization(shifted.copy(), 5, 95, True)
    rec["zeroone_arr3"] = su.zeroone_normalization(arr3.copy())
    rec["zeroone_vol5_array"] = su.zeroone_normalization(vol5.copy())
    t = torch.from_numpy(vol5.copy())
    rec["zeroone_vol5_tensor"] = su.zeroone_normalization(t).numpy()
    rec["zeroone_vol5_tensor_after"] = t.numpy()          # the reference writes the caller's tensor
    path = os.path.join(OUT, "intensity_norm.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes", {k: (v.dtype, v.shape) for k, v in rec.items()})


if __name__ == "__main__":
    main()
