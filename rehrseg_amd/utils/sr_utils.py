"""Whole-volume self-SR inference (mirror of the reference's utils/sr_utils.py, hot-path part only).

apply_to_vol_flavr (ref utils/sr_utils.py:102-135) slides a 4-slice window over the through-plane axis and
calls the network once per window at batch 1.  The windows are independent, so here they are gathered on
the device and pushed through the network in large batches (same kernels as training, far fewer launches,
full CUs at 16-multiple slice sizes); the result tensor is identical in layout and values.

The stage-1 -> stage-2 handoff (inference_flavr :137-242, zeroonenorm / postprocess_flavr :279-304; train_all.py:393-462)
runs on the device as well: `sr_volume_flavr` feeds the windows straight out of the stored (x, y, z, 2) volume and
scatters the network's output into the final volumes, `postprocess_flavr_volume` normalises and blurs them, and
`stage2_volumes` returns what TrainSetMultipleSegSREfficient(volumes=...) consumes without leaving HBM.  The
reference-named wrappers `inference_flavr` / `postprocess_flavr` take arrays and a dict where the reference takes file
names (nibabel and SimpleITK are absent).

The step in front of stage 1 (postprocess_smore :244-277, the default path of train_all.py:321-330) runs on the device
too: `postprocess_smore_volume` zooms the stored volume along its slice axis as scipy.ndimage.zoom does (order 3 for the
image, order 0 for the label) and blurs the result in-plane, and `stage1_volumes` returns what
TrainSetMultiple(volumes=...) keeps without an upload."""
import math

import numpy as np
import torch

from .. import ops


def _window_indices(S):
    """Slice indices of every window exactly as the reference builds them (-1 = zero slice)."""
    wins = []
    for st in range(0, S - 1):
        if st == 0:
            src = list(range(0, min(3, S)))
            idx = [-1] * (4 - len(src)) + src
        elif st == S - 2:
            src = list(range(st - 1, S))
            idx = src + [-1] * (4 - len(src))
        else:
            idx = list(range(st - 1, st + 3))
        wins.append(idx)
    return wins


def apply_to_vol_flavr(model, image, pred_out_idx=None, window_batch=32):
    """image (slices, C, X, Y) -> (4*(slices-1), C_out, Y, X) on the CPU, as the reference returns it."""
    ori_x, ori_y = image.shape[2], image.shape[3]
    pad_x, pad_y = (-ori_x) % 16, (-ori_y) % 16
    if pad_x or pad_y:
        image = torch.nn.functional.pad(image, (0, pad_y, 0, pad_x))
    S = image.shape[0]
    wins = _window_indices(S)
    if not wins:
        raise ValueError("apply_to_vol_flavr needs at least two slices")
    src = torch.cat([image, torch.zeros_like(image[:1])], 0)            # index S (= -1) is the zero slice
    idx = torch.tensor(wins, device=image.device) % (S + 1)             # (n_windows, 4)
    outs = []
    for i in range(0, len(wins), window_batch):
        b = src[idx[i:i + window_batch]]                                # (b, 4, C, X, Y)
        batch_input = b.permute(0, 2, 1, 4, 3).contiguous()             # (b, C, 4, Y, X): a fresh tensor (the model
        with torch.inference_mode():                                    # rewrites channel 0 of its input in place)
            sr = model(batch_input)
            if pred_out_idx is not None and isinstance(sr, tuple):
                sr = sr[pred_out_idx]
        outs.append(sr.detach()[:, :, :, :ori_y, :ori_x])
    res = torch.cat(outs, 0)                                            # (n_windows, C_out, 4, Y, X)
    res = res.permute(0, 2, 1, 3, 4).reshape(-1, res.shape[1], ori_y, ori_x)
    return res.cpu()


# ----------------------------------------------------------------------------- stage-1 -> stage-2 handoff on the device
def _integral_separation(slice_separation):
    sep = int(round(float(slice_separation)))
    if sep < 1 or abs(float(slice_separation) - sep) > 1e-9:
        # with an integral separation find_integer_p (utils/patch_ops.py:27-46) returns 0 at once (scale_tilde == 1):
        # no reflect padding in front of the network and no crop behind it.  Only that case is built.
        raise ValueError(f"slice_separation must be integral, got {slice_separation!r}")
    return sep


def _model_device(model):
    return next(model.parameters()).device


def _as_device_volume(volume, device):
    if isinstance(volume, torch.Tensor):
        return volume.to(device=device, dtype=torch.float32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(volume, dtype=np.float32)).to(device)


def sr_volume_flavr(model, volume, slice_separation, enable_uncertainty=False, window_batch=32):
    """inference_flavr (ref :137-242) without files: `volume` is the merged (x, y, z, 2) array or device tensor (image,
    label); returns device tensors in the layout the reference hands to SimpleITK, (4 (z - 1), y, x):

      img          float32, the network's channel 0 after inv_normalize(., orig_min, orig_max, a=0, b=1)
      seg          uint8, channel 1 after the same inv_normalize, > 0
      uncertainty  float32 (enable_uncertainty), output 1 of the network after the same inv_normalize (:217-231; its two
                   z_axis_to_lr_axis calls and the transpose(1, 2, 0, 3) cancel to the image's layout)
      minmax       int32 [4]: min / max codes of img, then of uncertainty (hip_backend.minmax_decode reads them)

    orig_min / orig_max span both channels of the input, as parse_image's (:73-74).  Gather, network and scatter run per
    batch of `window_batch` windows in the caller's precision mode; nothing here reads device memory from the host."""
    _integral_separation(slice_separation)
    be = ops.get_backend()
    dev = _model_device(model)
    vol = _as_device_volume(volume, dev)
    if vol.dim() != 4 or vol.shape[3] != 2:
        raise ValueError(f"expected an (x, y, z, 2) volume, got {tuple(vol.shape)}")
    X, Y, Z, _ = vol.shape
    if Z < 2:
        raise ValueError("sr_volume_flavr needs at least two slices")
    n_windows, n_out = Z - 1, int(model.n_outputs)
    in_mm = be.minmax(vol)
    mm = be.minmax_new(dev, 2)
    img = torch.empty((n_windows * n_out, Y, X), device=dev, dtype=torch.float32)
    seg = torch.empty((n_windows * n_out, Y, X), device=dev, dtype=torch.uint8)
    unc = torch.empty_like(img) if enable_uncertainty else None
    with torch.inference_mode():
        for w0 in range(0, n_windows, window_batch):
            b = min(window_batch, n_windows - w0)
            sr = model(be.sr_window_gather(vol, w0, b))
            out, sigma = (sr[0], sr[1]) if isinstance(sr, tuple) else (sr, sr)   # pred_out_idx of a plain output: itself
            be.sr_volume_scatter(out.float(), in_mm, w0, img, seg, mm[0:2])
            if enable_uncertainty:
                be.sr_volume_scatter(sigma.float(), in_mm, w0, unc, None, mm[2:4])
    res = {"img": img, "seg": seg, "minmax": mm}
    if enable_uncertainty:
        res["uncertainty"] = unc
    return res


_taps_cache = {}   # (taps bytes, device) -> float32 device vector: a run blurs every subject with one profile


def _device_taps(blur_kernel, device):
    k = np.ascontiguousarray(np.asarray(blur_kernel, dtype=np.float32).reshape(-1))
    key = (k.tobytes(), str(device))
    if key not in _taps_cache:
        _taps_cache[key] = torch.from_numpy(k).to(device)
    return _taps_cache[key]


def postprocess_flavr_volume(img, seg, blur_kernel, uncertainty=None, minmax=None):
    """postprocess_flavr (ref :284-304) on the device.  img / seg / uncertainty are the volumes as sr_volume_flavr
    returns them, (zo, y, x); the reference reads them back through nibabel as (x, y, zo), and that is the shape of all
    three results (contiguous, as the data set wants them):

      image        float32: zeroonenorm, then the blur `blur_kernel` (a parse_kernel result) along x, zero-padded 'same'
      label        uint8 (the reference keeps nibabel's float32 of the same values)
      uncertainty  uint8: zeros without a map (what train_all.py always gets: its `_uncertainty` path never exists), else
                   (zeroonenorm(u) * 255).astype('uint8') -- values up to 65025 wrapped into 8 bits, as written

    `minmax`: the code buffer of sr_volume_flavr (saves the two reductions); None computes them here."""
    be = ops.get_backend()
    xyz = lambda t: t.permute(2, 1, 0).contiguous()  # noqa: E731  SimpleITK array (z, y, x) -> nibabel (x, y, z)
    image = xyz(img)
    mm_img = minmax[0:2] if minmax is not None else be.minmax(image)
    image = be.stage2_prep(image, mm_img, _device_taps(blur_kernel, img.device))
    label = xyz(seg)
    if uncertainty is None:
        unc = torch.zeros_like(label)
    else:
        u = xyz(uncertainty)
        unc = be.stage2_unc_u8(u, minmax[2:4] if minmax is not None else be.minmax(u))
    return image, label, unc


def stage2_volumes(model, volumes, slice_separation, blur_kernel, enable_uncertainty=False, window_batch=32):
    """train_all.py:393-462 for a list of merged (x, y, z, 2) subjects: the {'img', 'seg', 'uncertainty'} dicts of
    TrainSetMultipleSegSREfficient(volumes=...), resident on the model's device.  `window_batch` is sr_volume_flavr's:
    the network's kernels pick their tiling by batch size, so two batchings agree to rounding, not bit for bit."""
    res = []
    for v in volumes:
        r = sr_volume_flavr(model, v, slice_separation, enable_uncertainty, window_batch)
        image, label, unc = postprocess_flavr_volume(r["img"], r["seg"], blur_kernel, r.get("uncertainty"), r["minmax"])
        res.append({"img": image, "seg": label, "uncertainty": unc})
    return res


def _no_files(what):
    if isinstance(what, (str, bytes)) or hasattr(what, "__fspath__"):
        raise ImportError("reading or writing image files needs nibabel and SimpleITK, which are not installed; pass the "
                          "merged (x, y, z, 2) volume as an array and a dict for the results instead")


def inference_flavr(model, sr_mode, in_fpath, ref_fpath, out_fpath, slice_thickness, target_thickness, device,
                    enable_uncertainty):
    """The reference's signature (:137) with an (x, y, z, 2) array for `in_fpath` and a dict for `out_fpath`, which
    receives '_img' / '_seg' ('img+seg') and '_uncertainty' (enable_uncertainty) as device tensors in the written
    (zo, y, x) layout.  `ref_fpath` (spacing, origin, direction of the written files) is unused."""
    for f in (in_fpath, out_fpath):
        _no_files(f)
    if sr_mode not in ("img+seg", "uncertainty"):
        raise ValueError("sr_mode: 'img+seg' or 'uncertainty' (the reference's 'img' / 'seg' modes index a channel "
                         "their one-channel result does not have)")
    model = model.to(device)
    r = sr_volume_flavr(model, in_fpath, float(slice_thickness / target_thickness), bool(enable_uncertainty))
    if sr_mode == "img+seg":
        out_fpath["_img"], out_fpath["_seg"] = r["img"], r["seg"]
    if enable_uncertainty:
        out_fpath["_uncertainty"] = r["uncertainty"]


def postprocess_flavr(subject, slice_seperation=4, sr_path=None):
    """The reference's signature (:284) with the dict inference_flavr filled for `sr_path`; the blur is the Gaussian of
    parse_kernel at the FWHM parse_image derives from (slice_seperation, 1.0).  An '_uncertainty' entry is used when
    present -- the reference looks for a file name that never exists and always returns zeros."""
    _no_files(sr_path)
    if sr_path is None:
        _no_files("")
    _integral_separation(slice_seperation)
    from .blur_kernel_ops import parse_kernel
    from .parse_image_file import blur_fwhm_voxels
    kernel = parse_kernel(None, "gaussian", blur_fwhm_voxels(float(slice_seperation), 1.0))
    return postprocess_flavr_volume(sr_path["_img"], sr_path["_seg"], kernel, sr_path.get("_uncertainty"))


# ----------------------------------------------------------------------------- stage-1 volume preparation on the device
_zoom_cache = {}   # (n, separation, device) -> (idx, w, nn) on the device: one table per line length of a run


def zoom_taps(n, separation, device=None):
    """scipy.ndimage.zoom(a, separation, order) along an axis of n samples (mode='constant', grid_mode=False) as tables,
    computed in Python doubles in ndimage's own order of operations: Z = round(n * separation) output samples, sample j
    at p = j * ((n - 1) / (Z - 1)) (Z == 1: p = 0).

      idx  int32 [Z, 4]    floor(p) - 1 .. floor(p) + 2, indices outside the axis mirrored about the end samples
      w    float64 [Z, 4]  the cubic B-spline weights at p - floor(p) (order 3, applied to the prefiltered line)
      nn   int32 [Z]       floor(p + 0.5) (order 0: half up, not half to even)

    A position that rounding carries beyond n - 1 is outside the axis for ndimage and reads cval = 0: zero weights and
    nn = -1.  With `device`, the tables as device tensors, cached per (n, separation, device)."""
    n = int(n)
    Z = int(round(n * float(separation)))
    if n < 1 or Z < 1:
        raise ValueError(f"zoom_taps: {n} samples at separation {separation!r} leave no output sample")
    if device is not None:
        key = (n, float(separation), str(device))
        if key not in _zoom_cache:
            _zoom_cache[key] = tuple(torch.from_numpy(t).to(device) for t in zoom_taps(n, separation))
        return _zoom_cache[key]
    step = (n - 1) / (Z - 1) if Z > 1 else 1.0
    idx = np.zeros((Z, 4), np.int32)
    w = np.zeros((Z, 4), np.float64)
    nn = np.full((Z,), -1, np.int32)
    period = 2 * n - 2

    def mirror(i):
        if n == 1:
            return 0
        i = abs(i) % period
        return period - i if i >= n else i

    for j in range(Z):
        p = j * step
        if p > n - 1:
            continue
        f = math.floor(p)
        idx[j] = [mirror(f - 1 + q) for q in range(4)]
        y = p - f
        t = 1.0 - y
        w0 = t * t * t / 6.0
        w1 = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0
        w2 = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0
        w[j] = [w0, w1, w2, 1.0 - w0 - w1 - w2]
        nn[j] = math.floor(p + 0.5)
    return idx, w, nn


def postprocess_smore_volume(volume, slice_separation, blur_kernel, device=None):
    """postprocess_smore (ref :244-277, the branch without an SR network) on the device.  `volume` is the merged
    (x, y, z, 2) array or device tensor (image, label), `blur_kernel` a parse_kernel result; returns device tensors under
    the reference's names, with Z = round(z * slice_separation):

      img_hr       (x, y, Z, 1) float32  scipy.ndimage.zoom(image, (1, 1, slice_separation), order=3)
      label_hr     (x, y, Z, 1) uint8    zoom(label, ..., order=0).astype('uint8')
      image_x_rgb  (Z, 1, x, y) float32  img_hr blurred along x (F.conv2d, padding='same')
      image_y_rgb  (Z, 1, y, x) float32  img_hr blurred along y

    The unit axes are views.  Nothing here reads device memory from the host.  `device`: where a host array goes (a
    tensor stays where it is); default cuda."""
    be = ops.get_backend()
    if isinstance(volume, torch.Tensor):
        dev = volume.device if device is None else torch.device(device)
    else:
        dev = torch.device("cuda" if device is None else device)
    vol = _as_device_volume(volume, dev)
    if vol.dim() != 4 or vol.shape[3] != 2:
        raise ValueError(f"expected an (x, y, z, 2) volume, got {tuple(vol.shape)}")
    img, label = be.zoom_depth(vol, *zoom_taps(vol.shape[2], slice_separation, vol.device))
    taps = _device_taps(blur_kernel, vol.device)
    return {"img_hr": img.unsqueeze(3), "label_hr": label.unsqueeze(3),
            "image_x_rgb": be.blur_to_slices(img, taps, 0).unsqueeze(1),
            "image_y_rgb": be.blur_to_slices(img, taps, 1).unsqueeze(1)}


def stage1_volumes(volumes, slice_separation, blur_kernel, device=None):
    """train_all.py:321-330 for a list of merged (x, y, z, 2) subjects: the dicts TrainSetMultiple(volumes=...) keeps as
    they are, resident on the device."""
    return [postprocess_smore_volume(v, slice_separation, blur_kernel, device) for v in volumes]


def postprocess_smore(subject, slice_seperation=4, data_path=None, sr_path=None):
    """The reference's signature (:244) with the merged (x, y, z, 2) array, or a dict subject -> array, for `data_path`;
    the blur is the Gaussian of parse_kernel at the FWHM parse_image derives from (slice_seperation, 1.0), where the
    reference asks degrade for 'rf-pulse-slr' (absent; unpinned).  Returns (img_hr, label_hr, image_x_rgb, image_y_rgb)
    as device tensors."""
    if sr_path is not None:
        raise NotImplementedError("postprocess_smore(sr_path=...) reads the output of the 2-D WDSR network "
                                  "(inference_smore), which is out of scope (SURVEY section 2); pass data_path")
    _no_files(data_path)
    if data_path is None:
        _no_files("")
    volume = data_path[subject] if isinstance(data_path, dict) else data_path
    _no_files(volume)
    from .blur_kernel_ops import parse_kernel
    from .parse_image_file import blur_fwhm_voxels
    kernel = parse_kernel(None, "gaussian", blur_fwhm_voxels(float(slice_seperation), 1.0))
    r = postprocess_smore_volume(volume, float(slice_seperation), kernel)
    return r["img_hr"], r["label_hr"], r["image_x_rgb"], r["image_y_rgb"]


# ----------------------------------------------------------------------------- stage-1 validation
def sr_quality(stats, voxels_per_sample, data_range=1.0):
    """The quality numbers of accumulated (n, 7) sr_metrics stats (one row per validation sample) as Python numbers:
    l1, mse and ssim are means over the samples, psnr the mean of 10 log10(data_range^2 / mse_n) (inf where a sample's
    mse is 0), dice the Dice of the summed exact counts (calculate_dice's smoothing, 1e-5), n the number of samples.
    The one place that reads the stats on the host."""
    from .seg_utils import _dice_from_counts
    s = stats.detach().to("cpu", torch.float64).numpy().reshape(-1, 7)
    if s.shape[0] == 0:
        raise ValueError("sr_quality needs the stats of at least one sample")
    mse = s[:, 1] / float(voxels_per_sample)
    with np.errstate(divide="ignore"):
        psnr = 10.0 * np.log10(float(data_range) ** 2 / mse)
    inter, n_pred, n_tgt = (int(round(float(v))) for v in s[:, 4:7].sum(0))
    return {"l1": float((s[:, 0] / float(voxels_per_sample)).mean()), "mse": float(mse.mean()),
            "psnr": float(psnr.mean()), "ssim": float((s[:, 2] / s[:, 3]).mean()),
            "dice": float(_dice_from_counts(inter, n_pred, n_tgt)), "n": int(s.shape[0])}
