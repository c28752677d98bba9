"""fp64 gradients of the oracle's cfg-2 step for its small tensors (biases: at most SMALL elements), the yardstick
source of tests/test_full_size_oracle_gpu.py::test_cfg2_flavr_128cube_against_cpu_reference_path.  The same
deterministic weights, input and target as that test, through oracle/flavr_oracle.py in float64 on the CPU.

The fp32 CPU path's own rounding distance on a cancelling bias gradient (a sum over every voxel) depends on how the
host splits that sum among its threads; with these stored fp64 gradients the test measures it live, for the fp32 run
it compares against, instead of reading a distance recorded on another host.

    python tools/gen_golden_fp64_small_grads.py      # rewrites tests/golden/fp64_small_grads_cfg2.npz (CPU only)
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import flavr_oracle as fo  # noqa: E402
from oracle.detinit import det_input, det_tensor  # noqa: E402

SMALL = 1024
OUT = os.path.join(ROOT, "tests", "golden", "fp64_small_grads_cfg2.npz")


def main():
    from rehrseg_amd.models.FLAVR.FLAVR_arch import UNet_3D_3D
    sd = {k: det_tensor(k, tuple(v.shape)) for k, v in UNet_3D_3D(1, "unet_18", 128, 4).state_dict().items()}
    x = det_input("cfg2.x", (1, 1, 128, 128, 128), "rand")
    tgt = det_input("cfg2.t", (1, 1, 4, 128, 128), "rand")
    t0 = time.time()
    osd = {k: v.detach().clone().to(torch.float64).requires_grad_() for k, v in sd.items()}
    r = fo.unet_3d_3d(osd, x.to(torch.float64).clone(), 1, 128, 4)
    loss = (r - tgt.to(torch.float64)).abs().mean()
    loss.backward()
    rec = {k: v.grad.numpy() for k, v in osd.items() if v.grad is not None and v.numel() <= SMALL}
    rec["__loss__"] = np.array(float(loss.detach()))
    np.savez_compressed(OUT, **rec)
    print(f"{len(rec) - 1} tensors, loss {float(loss.detach()):.12f}, {time.time() - t0:.0f} s on "
          f"{torch.get_num_threads()} threads -> {OUT}")


if __name__ == "__main__":
    main()
