"""Seconds per subject of the stage-1 -> stage-2 handoff: utils/sr_utils.stage2_volumes (device code end to end)
against the composed path it replaces -- apply_to_vol_flavr (device network, result copied to the host), the tail of
inference_flavr / postprocess_flavr in numpy and torch on the CPU, and the upload through
TrainSetMultipleSegSREfficient(volumes=<numpy>) -- with no file IO on either side.  Also the achieved bytes / s of the
scatter and prep kernels against the measured 6.29 TB/s copy peak.

    python tools/bench_handoff.py [--shape 320 320 11] [--subjects 3] [--out profiles/handoff_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.detinit import det_tensor  # noqa: E402
from rehrseg_amd import hip_backend as hb  # noqa: E402
from rehrseg_amd.models.FLAVR.FLAVR_arch import UNet_3D_3D  # noqa: E402
from rehrseg_amd.utils import sr_utils as sr  # noqa: E402
from rehrseg_amd.utils.blur_kernel_ops import parse_kernel  # noqa: E402
from rehrseg_amd.utils.parse_image_file import blur_fwhm_voxels, inv_normalize  # noqa: E402
from rehrseg_amd.utils.train_set import TrainSetMultipleSegSREfficient  # noqa: E402

PEAK = 6.29e12
DEV = "cuda:0"


def composed(model, vol, kernel, phases):
    """The parent path for one subject: numpy volume in, data set with the volume in HBM out."""
    t0 = time.perf_counter()
    image = torch.from_numpy(vol.transpose(2, 0, 1, 3)).to(DEV).permute(0, 3, 2, 1)
    rot = sr.apply_to_vol_flavr(model, image, 0)                           # ends in .cpu(): a sync
    t1 = time.perf_counter()
    final = rot.permute(0, 3, 1, 2).numpy().astype(np.float32)
    final = inv_normalize(final, vol.min(), vol.max(), a=0, b=1).transpose(2, 0, 1, 3)
    img = final[0].transpose(2, 1, 0)
    seg = (final[1] > 0).astype("uint8").transpose(2, 1, 0)
    img = (img - np.min(img)) / (np.max(img) - np.min(img)) * 255.0
    it = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))).unsqueeze(1)
    img = F.conv2d(it, kernel, padding="same").squeeze(1).numpy().transpose(1, 2, 0)
    t2 = time.perf_counter()
    ds = TrainSetMultipleSegSREfficient(None, ["s"], 4.0, 1.0, [8, 8, 2], [8, 8, 2], uncertainty=True, device=DEV,
                                        volumes=[{"img": img, "seg": seg, "uncertainty": np.zeros_like(seg)}])
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    for k, v in (("network + copy to host", t1 - t0), ("host tail", t2 - t1), ("data set upload", t3 - t2)):
        phases[k] = phases.get(k, 0.0) + v
    return ds


def device_path(model, vol, kernel, phases):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dvol = torch.from_numpy(vol).to(DEV)
    vols = sr.stage2_volumes(model, [dvol], 4, kernel)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    ds = TrainSetMultipleSegSREfficient(None, ["s"], 4.0, 1.0, [8, 8, 2], [8, 8, 2], uncertainty=True, device=DEV,
                                        volumes=vols)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    for k, v in (("upload + gather / network / scatter + prep", t1 - t0), ("data set (device z-score)", t2 - t1)):
        phases[k] = phases.get(k, 0.0) + v
    return ds


def kernel_rate(fn, nbytes, reps=20):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    s = e0.elapsed_time(e1) * 1e-3 / reps
    return s, nbytes / s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[320, 320, 11], help="stored (x, y, z): stage 2 sees 4 (z - 1)")
    ap.add_argument("--subjects", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    X, Y, Z = a.shape
    model = UNet_3D_3D(2, "unet_18", 4, 4, use_uncertainty=True).eval()
    model.load_state_dict({k: det_tensor(k, tuple(v.shape)) for k, v in model.state_dict().items()})
    model = model.to(DEV)
    kernel = parse_kernel(None, "gaussian", blur_fwhm_voxels(4.0, 1.0))
    rng = np.random.RandomState(0)
    vols = [np.stack([rng.rand(X, Y, Z).astype(np.float32) * 400, (rng.rand(X, Y, Z) > 0.5).astype(np.float32)], -1)
            for _ in range(a.subjects)]
    lines = [f"stage-1 -> stage-2 handoff, stored volume {X}x{Y}x{Z}x2, stage-2 volume {X}x{Y}x{4 * (Z - 1)}, "
             f"separation 4, blur taps {kernel.numel()}, {a.subjects} subjects after one warm-up each"]
    composed(model, vols[0], kernel, {})
    device_path(model, vols[0], kernel, {})
    res = {}
    for name, fn in (("composed (parent) path", composed), ("device path (stage2_volumes)", device_path)):
        phases = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for v in vols:
            fn(model, v, kernel, phases)
        res[name] = (time.perf_counter() - t0) / a.subjects
        lines.append(f"{name}: {res[name]:.4f} s / subject")
        lines += [f"    {k}: {v / a.subjects:.4f} s" for k, v in phases.items()]
    c, d = res["composed (parent) path"], res["device path (stage2_volumes)"]
    lines.append(f"ratio composed / device: {c / d:.2f}x" + ("" if d < c else "  (the device path is NOT faster)"))

    # kernels alone: bytes that must cross HBM once
    Zo, b = 4 * (Z - 1), min(32, Z - 1)
    Xp, Yp = X + (-X) % 16, Y + (-Y) % 16
    net = torch.randn(b, 4, Xp, Yp, 2, device=DEV).permute(0, 4, 1, 2, 3)
    img = torch.empty(Zo, Y, X, device=DEV)
    seg = torch.empty(Zo, Y, X, device=DEV, dtype=torch.uint8)
    in_mm, mm = hb.minmax(net.contiguous()), hb.minmax_new(DEV)
    s, r = kernel_rate(lambda: hb.sr_volume_scatter(net, in_mm, 0, img, seg, mm), b * 4 * X * Y * (8 + 4 + 1))
    lines.append(f"rehr_sr_volume_scatter_f32 ({b} windows): {s * 1e6:.1f} us, {r / 1e12:.2f} TB/s = {r / PEAK:.1%} of peak")
    vol = torch.rand(X, Y, Zo, device=DEV)
    vmm, taps = hb.minmax(vol), kernel.reshape(-1).to(DEV)
    s, r = kernel_rate(lambda: hb.stage2_prep(vol, vmm, taps), vol.numel() * 8)
    lines.append(f"rehr_stage2_prep_f32: {s * 1e6:.1f} us, {r / 1e12:.2f} TB/s = {r / PEAK:.1%} of peak")
    dv = torch.from_numpy(vols[0]).to(DEV)
    nb = min(32, Z - 1)
    s, r = kernel_rate(lambda: hb.sr_window_gather(dv, 0, nb), (nb + 3) * X * Y * 8 + nb * 4 * Xp * Yp * 8)
    lines.append(f"rehr_sr_window_gather_f32 ({nb} windows): {s * 1e6:.1f} us, {r / 1e12:.2f} TB/s = {r / PEAK:.1%} of peak")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
