"""Feed plus device augmentation per training batch (GPU box): stage-2 batches of two with and without
train_transform="nnunet" at the BASELINE stage-2 geometry and at the reference's default tile ([14, 320, 384] out of
patch_size_ori = tile + 64 in-plane), and the stage-1 batch with and without nnunet_transform.  The chain's draws are
random, so each number is a mean over many batches under one seed.

    python tools/bench_augment.py"""
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rehrseg_amd.utils.train_set import TrainSetMultiple, TrainSetMultipleSegSREfficient  # noqa: E402


def timed(fn, reps=50):
    random.seed(0)
    np.random.seed(0)
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def main():
    rng = np.random.RandomState(0)
    sep = 4
    for label, ps, target in (("BASELINE stage-2 (192x192x40 feed)", (192, 192, 40), (128, 128, 40)),
                              ("reference tile [14, 320, 384]", (448, 384, 14), (384, 320, 14))):
        shape = (ps[0] + 8, ps[1] + 8, ps[2] * sep + 8)
        vols = [dict(img=rng.rand(*shape).astype(np.float32), seg=(rng.rand(*shape) > 0.5).astype(np.uint8),
                     uncertainty=rng.randint(0, 256, size=shape).astype(np.uint8)) for _ in range(2)]
        res = {}
        for tt in (None, "nnunet"):
            ds = TrainSetMultipleSegSREfficient(None, [0, 1], float(sep), 1.0, ps, target, True, True,
                                                device="cuda:0", volumes=vols, train_transform=tt)
            res[tt] = timed(lambda: ds.batch([0, 1]))
        print(f"stage-2 B=2 {label}: feed {res[None] * 1e3:.3f} ms, feed + augmentation {res['nnunet'] * 1e3:.3f} ms "
              f"(augmentation {(res['nnunet'] - res[None]) * 1e3:.3f} ms)", flush=True)
    shape = (320, 320, 96)
    image = np.stack((rng.rand(*shape).astype(np.float32), (rng.rand(*shape) > 0.5).astype(np.float32)), -1)
    for B, ps in ((16, (96, 96, 1)), (4, (128, 128, 128))):
        res = {}
        for nn in (False, True):
            ds = TrainSetMultiple(None, [0], 4.0, 1.0, None, None, ps, True, "cuda:0", volumes=[image],
                                  blur_kernel=np.array([0.05, 0.2, 0.5, 0.2, 0.05], np.float32), nnunet_transform=nn)
            res[nn] = timed(lambda: ds.batch([0] * B))
        print(f"stage-1 B={B} x {ps}: feed {res[False] * 1e3:.3f} ms, feed + augmentation {res[True] * 1e3:.3f} ms",
              flush=True)


if __name__ == "__main__":
    main()
