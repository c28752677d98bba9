"""Seconds per subject of the stage-1 volume preparation: utils/sr_utils.stage1_volumes (device code end to end, the
upload of the stored volume included) against the composed path it replaces -- the z-upsampling on the host (the CPU
statement of the zoom, tests/stage1_emu.py, standing in for scipy; its time is reported separately and NOT counted),
then the upload and today's tap-table route for the two blurs (TrainSetMultiple(volumes=[(x, y, Z, 2) arrays])) -- with
no file IO on either side.  Also the achieved bytes / s of the three kernels against the measured 6.29 TB/s copy peak
(DESIGN section 3): the bytes each must move across HBM once, over device-event time.

The two paths are timed alternately, `--rounds` times over `--subjects` subjects each, after a warm-up of both.

    python tools/bench_stage1.py [--shape 320 320 11] [--subjects 3] [--rounds 5] [--out profiles/stage1_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import stage1_emu  # noqa: E402
from rehrseg_amd import hip_backend as hb  # noqa: E402
from rehrseg_amd.utils import sr_utils as sr  # noqa: E402
from rehrseg_amd.utils.blur_kernel_ops import parse_kernel  # noqa: E402
from rehrseg_amd.utils.parse_image_file import blur_fwhm_voxels  # noqa: E402
from rehrseg_amd.utils.train_set import TrainSetMultiple  # noqa: E402

PEAK = 6.29e12
DEV = "cuda:0"
SEP = 4


def data_set(volumes, kernel):
    return TrainSetMultiple(None, ["s"], float(SEP), 1.0, None, None, (16, 16, 1), True, DEV, volumes=volumes,
                            blur_kernel=kernel)


def host_zoom(vol):
    """The host's share of the composed path: (x, y, z, 2) -> (x, y, Z, 2) as scipy.ndimage.zoom would."""
    t = torch.from_numpy(vol)
    img, lab = stage1_emu.zoom_depth(t, *(torch.from_numpy(a) for a in sr.zoom_taps(vol.shape[2], SEP)))
    return np.stack([img.numpy(), lab.numpy().astype(np.float32)], -1)


def composed(zoomed, kernel):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ds = data_set([zoomed], kernel)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, ds


def device_path(vol, kernel):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ds = data_set(sr.stage1_volumes([vol], SEP, kernel, DEV), kernel)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, ds


def kernel_rate(fn, nbytes, reps=50):
    for _ in range(3):
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
    ap.add_argument("--shape", type=int, nargs=3, default=[320, 320, 11], help="stored (x, y, z)")
    ap.add_argument("--subjects", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stage1 measures on the GPU; there is none here")
    X, Y, n = a.shape
    Z = int(round(n * SEP))
    kernel = parse_kernel(None, "gaussian", blur_fwhm_voxels(float(SEP), 1.0))
    rng = np.random.RandomState(0)
    vols = [np.stack([rng.rand(X, Y, n).astype(np.float32) * 400, (rng.rand(X, Y, n) > 0.5).astype(np.float32)], -1)
            for _ in range(a.subjects)]
    t0 = time.perf_counter()
    zoomed = [host_zoom(v) for v in vols]
    host_s = (time.perf_counter() - t0) / a.subjects
    lines = [f"stage-1 volume preparation, stored volume {X}x{Y}x{n}x2, separation {SEP} -> {X}x{Y}x{Z}, blur taps "
             f"{kernel.numel()}, {a.subjects} subjects x {a.rounds} alternating rounds after one warm-up of each path"]
    _, ds_c = composed(zoomed[0], kernel)
    _, ds_d = device_path(vols[0], kernel)
    # both paths hold the same blurred copies (one fmaf per tap on either side); the zoomed image within its one rounding
    same = all(torch.equal(p[0], q[0]) for p, q in ((ds_c.imgs_filtered_x, ds_d.imgs_filtered_x),
                                                     (ds_c.imgs_filtered_y, ds_d.imgs_filtered_y),
                                                     (ds_c.imgs_hr, ds_d.imgs_hr), (ds_c.labels_hr, ds_d.labels_hr)))
    lines.append(f"the two data sets hold bit-identical tensors: {same}")
    tc, td = [], []
    for _ in range(a.rounds):
        tc.append(sum(composed(z, kernel)[0] for z in zoomed) / a.subjects)
        td.append(sum(device_path(v, kernel)[0] for v in vols) / a.subjects)
    c, d = float(np.median(tc)), float(np.median(td))
    lines.append(f"composed path (upload of the zoomed volume + tap-table blurs): median {c:.5f} s / subject "
                 f"(min {min(tc):.5f}, max {max(tc):.5f})")
    lines.append(f"    not counted: the z-upsampling on the host, {host_s:.4f} s / subject (numpy statement, one thread)")
    lines.append(f"device path (upload of the stored volume + stage1_volumes): median {d:.5f} s / subject "
                 f"(min {min(td):.5f}, max {max(td):.5f})")
    lines.append(f"ratio composed / device: {c / d:.2f}x" + ("" if d < c else "  (the device path is NOT faster)"))

    # kernels alone: bytes that must cross HBM once
    dv = torch.from_numpy(vols[0]).to(DEV)
    tabs = sr.zoom_taps(n, SEP, dv.device)
    s, r = kernel_rate(lambda: hb.zoom_depth(dv, *tabs), X * Y * (n * 8 + Z * 5))
    lines.append(f"rehr_zoom_depth_f32: {s * 1e6:.1f} us, {r / 1e12:.2f} TB/s = {r / PEAK:.1%} of the copy peak")
    img = hb.zoom_depth(dv, *tabs)[0]
    taps = kernel.reshape(-1).to(DEV)
    for axis in (0, 1):
        s, r = kernel_rate(lambda: hb.blur_to_slices(img, taps, axis), img.numel() * 8)
        lines.append(f"rehr_blur_to_slices_f32 axis {axis}: {s * 1e6:.1f} us, {r / 1e12:.2f} TB/s = {r / PEAK:.1%} of the "
                     "copy peak")
    for axis in (0, 2):
        s, r = kernel_rate(lambda: hb.bspline_prefilter(img, axis), img.numel() * 8)
        lines.append(f"rehr_bspline_prefilter_axis_f64acc_f32 axis {axis} of {tuple(img.shape)}: {s * 1e6:.1f} us, "
                     f"{r / 1e12:.2f} TB/s = {r / PEAK:.1%} of the copy peak")
    lines.append("(event time over 50 back-to-back calls, allocation of the outputs included; the volumes fit the 256 MB "
                 "last-level cache, so a rate above the HBM peak is possible)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
