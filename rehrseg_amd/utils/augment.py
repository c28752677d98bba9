"""The nnU-Net training augmentation of REHRSeg on the device (utils/seg_utils.py:511-728 MySpatialTransform /
get_training_transforms, applied at utils/train_set.py:145-158 for stage 2 and :366-380 for stage 1).

The reference runs the chain per item on the host with batchgenerators 0.25; here the patches are already in HBM, so
the chain runs there: the host draws every parameter per item from `np.random` in the reference's order (`draw`),
uploads them once per batch without waiting, and the kernels of csrc/augment.hip plus the tap tables of
`rehr_axis_resample_f32` do the arithmetic (`apply`).

Restated from the published behaviour of batchgenerators 0.25, scipy.ndimage and skimage (absent offline or not
vendored), PARITY UNPINNED as `resize` and `degrade` are: the intensity transforms, Convert3DTo2D / Convert2DTo3D,
the coordinate helpers and the deep-supervision label pyramid (DownsampleSegForDSTransform2).
What the fixtures of tools/gen_golden_augment.py pin: the spatial draw protocol and the warp against the reference's
own augment_spatial.  Deliberate differences:
  * batchgenerators draws the noise variance and the blur sigma from Python's `random`; here they come from
    `np.random`, so that Python's `random` stays the patch draw protocol of train_set.py alone.
  * the noise field comes from a counter-based generator in the kernel, seeded by one `np.random.randint` draw, not
    from `np.random.normal`: once noise fires for an item, the `np.random` stream no longer matches the reference's
    (it could not anyway: the reference consumes one normal per voxel).
"""
import math

import numpy as np
import torch

Z3 = math.sqrt(3.0) - 2.0          # pole of the cubic B-spline prefilter
_K = 24                            # prefilter taps each side: |Z3|^24 < 2e-14


# ----------------------------------------------------------------------------- host tap tables (fp64 -> fp32)
def _mirror(k, n):
    """scipy's whole-sample mirror (d c b | a b c d | c b a)."""
    if n == 1:
        return 0
    period = 2 * (n - 1)
    k = abs(k) % period
    return period - k if k >= n else k


def _reflect(k, n):
    """scipy's half-sample reflect (b a | a b c d | d c)."""
    period = 2 * n
    k %= period
    return period - 1 - k if k >= n else k


def dense_to_taps(m, tol=0.0):
    """Dense operator (n_out, n_in) -> (idx int32, w float32) tap tables of its nonzero columns (idx -1: no term)."""
    m = np.asarray(m, np.float64)
    rows = [np.nonzero(np.abs(r) > tol)[0] for r in m]
    taps = max(1, max(len(r) for r in rows))
    idx = np.full((m.shape[0], taps), -1, np.int32)
    w = np.zeros((m.shape[0], taps), np.float32)
    for j, r in enumerate(rows):
        idx[j, :len(r)] = r
        w[j, :len(r)] = m[j, r]
    return idx, w


def prefilter_matrix(n):
    """Cubic B-spline coefficients of a length-n signal, mirror boundary (scipy's spline_filter1d for map_coordinates
    with mode 'constant'): c = sqrt(3) * sum_k Z3^|k| x[mirror(j + k)]."""
    m = np.zeros((n, n))
    for j in range(n):
        for k in range(-_K, _K + 1):
            m[j, _mirror(j + k, n)] += math.sqrt(3.0) * Z3 ** abs(k)
    return m


def gaussian_matrix(n, sigma, truncate=4.0):
    """scipy.ndimage.gaussian_filter1d(order=0, mode='reflect', truncate=4) along one axis of length n."""
    r = int(truncate * float(sigma) + 0.5)
    x = np.arange(-r, r + 1)
    k = np.exp(-0.5 / (float(sigma) * float(sigma)) * x * x)
    k /= k.sum()
    m = np.zeros((n, n))
    for j in range(n):
        for t in range(-r, r + 1):
            m[j, _reflect(j + t, n)] += k[t + r]
    return m


def _bspline3(t):
    t = abs(t)
    if t < 1:
        return 2.0 / 3.0 - t * t + 0.5 * t ** 3
    if t < 2:
        return (2.0 - t) ** 3 / 6.0
    return 0.0


def zoom_nearest_matrix(n_in, n_out):
    """ndimage.zoom(order=0, mode='nearest', grid_mode=True) along one axis (skimage resize(order=0, mode='edge',
    anti_aliasing=False)): output j reads input floor(c + 0.5), c = (j + 0.5) n_in / n_out - 0.5, clamped."""
    m = np.zeros((n_out, n_in))
    z = n_in / n_out
    for j in range(n_out):
        c = (j + 0.5) * z - 0.5
        m[j, min(max(int(math.floor(c + 0.5)), 0), n_in - 1)] = 1.0
    return m


def zoom_cubic_matrix(n_in, n_out):
    """ndimage.zoom(order=3, mode='nearest', grid_mode=True) along one axis: the B-spline of the edge-extended signal
    (prefilter over the nearest extension) sampled at c = (j + 0.5) n_in / n_out - 0.5."""
    m = np.zeros((n_out, n_in))
    z = n_in / n_out
    clamp = lambda i: min(max(i, 0), n_in - 1)  # noqa: E731
    for j in range(n_out):
        c = (j + 0.5) * z - 0.5
        f = math.floor(c)
        for k in range(f - 1, f + 3):
            bw = _bspline3(c - k)
            if bw == 0.0:
                continue
            for t in range(-_K, _K + 1):
                m[j, clamp(k + t)] += bw * math.sqrt(3.0) * Z3 ** abs(t)
    return m


def lowres_shape(shape, zoom, ignore_axes=(0,)):
    """SimulateLowResolutionTransform's target shape: np.round(shape * zoom) (half to even), ignored axes kept."""
    tgt = np.round(np.asarray(shape) * zoom).astype(int)
    for a in ignore_axes or ():
        tgt[a] = shape[a]
    return [int(v) for v in tgt]


# ----------------------------------------------------------------------------- parameter draws (np.random, reference order)
def _either(lo, hi, rng):
    """`np.random.random() < 0.5 and lo < 1` picks [lo, 1), else [max(lo, 1), hi) (contrast, gamma, scale)."""
    if rng.random() < 0.5 and lo < 1:
        return rng.uniform(lo, 1)
    return rng.uniform(max(lo, 1), hi)


def draw_spatial(angle_x, rng=np.random, p_rot=0.2, p_scale=0.2, scale=(0.7, 1.4), p_rot_per_axis=1):
    """augment_spatial (utils/seg_utils.py:403-449) for one item, dim 2, no elastic deformation, random_crop=False,
    one scale for both axes; get_training_transforms passes p_rot = p_scale = 0.2, scale (0.7, 1.4).
    -> {"angle": float or None, "scale": float or None}."""
    angle = sc = None
    if rng.uniform() < p_rot:
        angle = rng.uniform(angle_x[0], angle_x[1]) if rng.uniform() <= p_rot_per_axis else 0.0
    if rng.uniform() < p_scale:
        sc = _either(scale[0], scale[1], rng)
    return {"angle": angle, "scale": sc}


def draw_intensity(rng=np.random):
    """The seven intensity transforms of get_training_transforms (:678-688) for one single-channel item."""
    p = {}
    if rng.uniform() < 0.1:                       # GaussianNoiseTransform(p_per_sample=0.1), variance (0, 0.1)
        std = rng.uniform(0.0, 0.1)
        rng.uniform()                             # p_per_channel = 1
        p["noise"] = (std, int(rng.randint(0, 2 ** 31 - 1)))
    if rng.uniform() < 0.2 and rng.uniform() <= 0.5:   # GaussianBlurTransform(p 0.2, p_per_channel 0.5)
        p["blur"] = rng.uniform(0.5, 1.0)
    if rng.uniform() < 0.15:                      # BrightnessMultiplicativeTransform: one draw unused, one per channel
        rng.uniform(0.75, 1.25)
        p["brightness"] = rng.uniform(0.75, 1.25)
    if rng.uniform() < 0.15 and rng.uniform() < 1:     # ContrastAugmentationTransform(preserve_range=True)
        p["contrast"] = _either(0.75, 1.25, rng)
    if rng.uniform() < 0.25 and rng.uniform() < 0.5:   # SimulateLowResolutionTransform(p 0.25, p_per_channel 0.5)
        p["lowres"] = rng.uniform(0.5, 1.0)
    if rng.uniform() < 0.1:                       # GammaTransform((0.7, 1.5), invert_image=True, retain_stats=True)
        p["gamma_inv"] = _either(0.7, 1.5, rng)
    if rng.uniform() < 0.3:                       # GammaTransform((0.7, 1.5), invert_image=False, retain_stats=True)
        p["gamma"] = _either(0.7, 1.5, rng)
    return p


def warp_params(draw, in_hw):
    """Per-item record of rehr_aug_warp2d_f32: rotation matrix, scale, centre shape / 2 - 0.5."""
    r = np.eye(2)
    if draw["angle"] is not None:
        a = draw["angle"]
        r = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    s = 1.0 if draw["scale"] is None else draw["scale"]
    return [r[0, 0], r[0, 1], r[1, 0], r[1, 1], s, in_hw[0] / 2.0 - 0.5, in_hw[1] / 2.0 - 0.5, 0.0]


# ----------------------------------------------------------------------------- the device chain
_table_cache = {}   # (builder, sizes, device) -> device tap tables: integer-keyed tables never change


def _upload(a, device):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.pin_memory().to(device, non_blocking=True)


def _taps_dev(m, device):
    idx, w = dense_to_taps(m)
    return _upload(idx, device), _upload(w, device)


def _cached_taps(builder, sizes, device):
    key = (builder.__name__, tuple(sizes), device)
    if key not in _table_cache:
        _table_cache[key] = _taps_dev(builder(*sizes), device)
    return _table_cache[key]


def _prefilter_taps(n, device):
    return _cached_taps(prefilter_matrix, (n,), device)


class TrainingTransforms:
    """get_training_transforms(...) for what REHRSeg passes: callable over keyword tensors (B, 1, z, y, x) float32 on
    the device; `data` is augmented, the extra keys follow the spatial step only.  Items draw one after another.
    With `deep_supervision_scales` the result's `seg` (and, with enable_uncertainty, the uncertainty) is a list with one
    tensor per scale; `data` and the other keys are untouched by that step, which draws no random numbers."""

    def __init__(self, patch_size_spatial, angle_x, enable_spatial, enable_uncertainty, extra_keys, rng=np.random,
                 deep_supervision_scales=None):
        self.patch_size_spatial = None if patch_size_spatial is None else [int(v) for v in patch_size_spatial]
        self.angle_x, self.enable_spatial = tuple(angle_x), bool(enable_spatial)
        self.enable_uncertainty, self.extra_keys = bool(enable_uncertainty), list(extra_keys)
        self.rng = rng
        # the last step of the chain (ref :723-725): 'seg' becomes the list of its deep-supervision levels, and with
        # enable_uncertainty the uncertainty map (the last extra key) follows through the same index maps
        self.pyramid = None
        if deep_supervision_scales is not None:
            also = (self.extra_keys[-1],) if self.enable_uncertainty and self.extra_keys and \
                self.extra_keys[-1] != "seg" else ()
            self.pyramid = DownsampleSegForDSTransform2(deep_supervision_scales, 0, input_key="seg", output_key="seg",
                                                        also=also)

    def draw(self, n):
        out = []
        for _ in range(n):
            d = {"spatial": draw_spatial(self.angle_x, self.rng)} if self.enable_spatial else {}
            d["intensity"] = draw_intensity(self.rng)
            out.append(d)
        return out

    def __call__(self, **data):
        x = data["data"]
        return self.apply(self.draw(x[..., 0, 0, 0, 0].numel() if x.dim() >= 5 else 0), **data)

    def apply(self, draws, **data):
        """`draws` (one per item, from `draw`) applied to keyword tensors (..., 1, z, y, x): every leading index is one
        item (the stage-2 feed hands out (B, 1, 1, z, y, x), the reference's per-item (1, 1, z, y, x) stacked)."""
        from .. import hip_backend as hb
        lead = tuple(data["data"].shape[:-4])
        B = len(draws)
        flat = {}
        for k, t in data.items():
            if t.dim() < 5 or tuple(t.shape[:-4]) != lead or t.shape[-4] != 1 or not t.is_cuda:
                raise hb.L.RehrsegHipError(f"augmentation: {k} must be a (..., 1, z, y, x) device tensor with the "
                                           "leading extents of `data`")
            flat[k] = t.reshape((B,) + tuple(t.shape[-4:]))
        out = dict(flat)
        if self.enable_spatial:
            out.update(self._spatial(draws, flat, hb))
        out["data"] = self._intensity(draws, out["data"].contiguous(), hb)
        out = {k: v.reshape(lead + tuple(v.shape[1:])) for k, v in out.items()}
        return out if self.pyramid is None else self.pyramid(**out)

    # Convert3DTo2D -> MySpatialTransform -> Convert2DTo3D: (B, 1, z, y, x) -> (B, z, y, x) -> warp -> back
    def _spatial(self, draws, data, hb):
        keys = [k for k in ["data"] + self.extra_keys if k in data]
        flat = {k: data[k].reshape(data[k].shape[0], data[k].shape[2], *data[k].shape[3:]) for k in keys}
        img = {"data"} | ({self.extra_keys[-1]} if self.enable_uncertainty and self.extra_keys else set())
        res = warp_keys([d["spatial"] for d in draws], flat, img, self.patch_size_spatial)
        return {k: v.unsqueeze(1) for k, v in res.items()}

    def _intensity(self, draws, x, hb):
        B, dev = x.shape[0], x.device
        shape = tuple(x.shape[2:])
        pw = {op: np.zeros((B, hb.AUG_PW_PARAMS)) for op in ("noise", "brightness", "contrast", "gamma_inv", "gamma")}
        for b, d in enumerate(draws):
            p = d["intensity"]
            if "noise" in p:
                pw["noise"][b] = (1.0, p["noise"][0], float(p["noise"][1]), 0.0)
            if "brightness" in p:
                pw["brightness"][b] = (1.0, p["brightness"], 0.0, 0.0)
            if "contrast" in p:
                pw["contrast"][b] = (1.0, p["contrast"], 0.0, 0.0)
            if "gamma_inv" in p:
                pw["gamma_inv"][b] = (1.0, p["gamma_inv"], -1.0, 0.0)
            if "gamma" in p:
                pw["gamma"][b] = (1.0, p["gamma"], 1.0, 0.0)
        fires = {k: bool(v[:, 0].any()) for k, v in pw.items()}
        names = [k for k in pw if fires[k]]
        if names:
            blob = _upload(np.stack([pw[k] for k in names]), dev)
            dp = {k: blob[i] for i, k in enumerate(names)}
        x = x.view(B, -1)
        if fires["noise"]:
            hb.aug_pointwise(x, hb.AUG_NOISE, dp["noise"])
        for b, d in enumerate(draws):
            if "blur" in d["intensity"]:
                s = d["intensity"]["blur"]
                v = x[b].view(shape)
                for axis in range(3):
                    v = hb.axis_resample(v.contiguous(), axis, *_taps_dev(gaussian_matrix(shape[axis], s), dev),
                                         validated=True)
                x[b].copy_(v.reshape(-1))
        if fires["brightness"]:
            hb.aug_pointwise(x, hb.AUG_SCALE, dp["brightness"])
        if fires["contrast"]:
            hb.aug_pointwise(x, hb.AUG_CONTRAST, dp["contrast"], hb.aug_stats(x))
        for b, d in enumerate(draws):
            if "lowres" in d["intensity"]:
                x[b].copy_(self._lowres(x[b].view(shape), d["intensity"]["lowres"], hb).reshape(-1))
        for key, op_sign in (("gamma_inv", -1.0), ("gamma", 1.0)):
            if fires[key]:
                st0 = hb.aug_stats(x)
                hb.aug_pointwise(x, hb.AUG_GAMMA, dp[key], st0)
                hb.aug_pointwise(x, hb.AUG_RETAIN, dp[key], st0, hb.aug_stats(x))
        return x.view(B, 1, *shape)

    @staticmethod
    def _lowres(v, zoom, hb):
        """augment_linear_downsampling_scipy with order_downsample 0, order_upsample 3, ignore_axes (0,): nearest
        down, cubic up (depth untouched), clipped to the range of the down-sampled image (skimage resize clip)."""
        dev, shape = v.device, tuple(v.shape)
        tgt = lowres_shape(shape, zoom)
        down = v.contiguous()
        for axis in (1, 2):
            down = hb.axis_resample(down, axis, *_cached_taps(zoom_nearest_matrix, (shape[axis], tgt[axis]), dev),
                                    validated=True)
        st = hb.aug_stats(down.view(1, -1))
        up = down
        for axis in (1, 2):
            up = hb.axis_resample(up, axis, *_cached_taps(zoom_cubic_matrix, (tgt[axis], shape[axis]), dev),
                                  validated=True)
        one = _upload(np.array([[1.0, 0.0, 0.0, 0.0]]), dev)
        return hb.aug_pointwise(up.view(1, -1), hb.AUG_CLIP, one, st)


def warp_keys(draws, tensors, image_keys, out_hw):
    """The in-plane affine of each item (`draws[b]` of draw_spatial) over every (B, C, y, x) tensor: order-3 B-spline,
    cval 0, for `image_keys`; the order-1 label vote (cval -1) for the others.  Same coordinates for all keys."""
    from .. import hip_backend as hb
    first = next(iter(tensors.values()))
    B, dev, in_hw = first.shape[0], first.device, tuple(first.shape[2:])
    params = _upload(np.array([warp_params(d, in_hw) for d in draws], np.float64), dev)
    res = {}
    for key, t in tensors.items():
        if tuple(t.shape[2:]) != in_hw or t.shape[0] != B or t.dim() != 4:
            raise hb.L.RehrsegHipError("augmentation: every key is (B, C, y, x) with the in-plane extent of `data`")
        t = t.to(torch.float32).contiguous()
        if key in image_keys:
            py, px = _prefilter_taps(in_hw[0], dev), _prefilter_taps(in_hw[1], dev)
            t = hb.axis_resample(hb.axis_resample(t, 3, *px, validated=True), 2, *py, validated=True)
            res[key] = hb.aug_warp2d(t, params, out_hw, hb.AUG_WARP_SPLINE3)
        else:
            res[key] = hb.aug_warp2d(t, params, out_hw, hb.AUG_WARP_LABEL)
    return res


class MySpatialTransform:
    """utils/seg_utils.py:511-630 for what get_training_transforms passes on the dummy-2D path: (B, C, y, x) device
    tensors, no elastic deformation, random_crop=False, one scale for both axes, constant borders, order 3 for data
    (and the uncertainty, last label key, with enable_uncertainty), order 1 label vote with cval -1 for the labels."""

    def __init__(self, patch_size, patch_center_dist_from_border=30, do_elastic_deform=True, alpha=(0., 1000.),
                 sigma=(10., 13.), do_rotation=True, angle_x=(0, 2 * np.pi), angle_y=(0, 2 * np.pi),
                 angle_z=(0, 2 * np.pi), do_scale=True, scale=(0.75, 1.25), border_mode_data='nearest',
                 border_cval_data=0, order_data=3, border_mode_seg='constant', border_cval_seg=0, order_seg=0,
                 random_crop=True, data_key="data", label_key=["seg", ], p_el_per_sample=1, p_scale_per_sample=1,
                 p_rot_per_sample=1, independent_scale_for_each_axis=False, p_rot_per_axis: float = 1,
                 p_independent_scale_per_axis: int = 1, enable_uncertainty: bool = False):
        def no(what):
            raise NotImplementedError(f"MySpatialTransform: {what} is not used by REHRSeg and not implemented")
        if patch_size is None or len(patch_size) != 2:
            no("a patch size other than 2-D (dim == 3)")
        if do_elastic_deform and p_el_per_sample > 0:
            no("elastic deformation")
        if random_crop:
            no("random_crop=True")
        if independent_scale_for_each_axis:
            no("independent_scale_for_each_axis")
        if (border_mode_data, border_cval_data, order_data) != ("constant", 0, 3) or \
                (border_mode_seg, border_cval_seg, order_seg) != ("constant", -1, 1):
            no("borders / orders other than constant 0 order 3 (data) and constant -1 order 1 (labels)")
        self.patch_size, self.data_key, self.label_key = [int(v) for v in patch_size], data_key, list(label_key)
        self.do_elastic_deform, self.p_el_per_sample = do_elastic_deform, p_el_per_sample
        self.angle_x = tuple(angle_x)
        self.p_rot = p_rot_per_sample if do_rotation else 0.0
        self.p_scale = p_scale_per_sample if do_scale else 0.0
        self.scale, self.p_rot_per_axis, self.enable_uncertainty = tuple(scale), p_rot_per_axis, enable_uncertainty

    def draw(self, n, rng=np.random):
        out = []
        for _ in range(n):
            if self.do_elastic_deform:
                rng.uniform()  # `do_elastic_deform and np.random.uniform() < p_el_per_sample` (p 0: never fires)
            out.append(draw_spatial(self.angle_x, rng, self.p_rot, self.p_scale, self.scale, self.p_rot_per_axis))
        return out

    def __call__(self, **data_dict):
        keys = [self.data_key] + [k for k in self.label_key if data_dict.get(k) is not None]
        img = {self.data_key} | ({self.label_key[-1]} if self.enable_uncertainty else set())
        draws = self.draw(data_dict[self.data_key].shape[0])
        data_dict.update(warp_keys(draws, {k: data_dict[k] for k in keys}, img, self.patch_size))
        return data_dict


# the reference's scale table of the six outputs of the 3d_fullres network, (z, y, x) per level (utils/seg_utils.py:364,
# utils/train_set.py:67)
DEEP_SUPERVISION_SCALES = [[1.0, 1.0, 1.0], [1.0, 0.5, 0.5], [1.0, 0.25, 0.25], [0.5, 0.125, 0.125],
                           [0.25, 0.0625, 0.0625], [0.25, 0.03125, 0.03125]]


def zoom_nearest_index(n_in, n_out):
    """zoom_nearest_matrix as an index table: int32 [n_out], entry j = the input sample output j reads."""
    if n_out < 1:
        raise ValueError(f"order-0 resize of {n_in} samples to {n_out}: the target extent must be at least 1")
    idx = np.argmax(zoom_nearest_matrix(n_in, n_out), axis=1).astype(np.int32)
    assert idx.min() >= 0 and idx.max() < n_in
    return idx


def pyramid_extents(shape, scales):
    """DownsampleSegForDSTransform2's target extents: np.round(extent * scale) per axis (half to even) for every level;
    `scales` holds one number or one (z, y, x) triple per level.  An extent of 0 raises."""
    out = []
    for s in scales:
        s = [float(s)] * len(shape) if np.isscalar(s) else [float(v) for v in s]
        if len(s) != len(shape):
            raise ValueError(f"deep supervision scale {s} for a {len(shape)}-axis label map")
        ext = [int(v) for v in np.round(np.asarray(shape, np.float64) * np.asarray(s))]
        if min(ext) < 1:
            raise ValueError(f"deep supervision scale {s} leaves no voxel of a {tuple(shape)} label map: {ext}")
        out.append(tuple(ext))
    return out


_index_cache = {}   # (n_in, n_out, device) -> device int32 index table of the order-0 resize


def _cached_index(n_in, n_out, device):
    key = (int(n_in), int(n_out), device)
    if key not in _index_cache:
        _index_cache[key] = _upload(zoom_nearest_index(n_in, n_out), device)
    return _index_cache[key]


class DownsampleSegForDSTransform2:
    """batchgenerators' DownsampleSegForDSTransform2 for what get_training_transforms passes (order 0), restated (skimage
    absent offline, PARITY UNPINNED): `input_key` (B, C, z, y, x) becomes under `output_key` a list with one tensor per
    scale.  A level whose scales are all 1 is the input itself; every other level is the order-0 resize of every axis
    (zoom_nearest_matrix: skimage resize(order=0, mode='edge', anti_aliasing=False)), all levels written by one launch
    of rehr_label_pyramid_f32.  `also` names further keys resampled with the same index maps (the uncertainty)."""

    def __init__(self, ds_scales=(1, 0.5, 0.25), order=0, input_key="seg", output_key="seg", axes=None, also=()):
        if order != 0:
            raise NotImplementedError("DownsampleSegForDSTransform2: order 0 only (what get_training_transforms passes)")
        if axes is not None:
            raise NotImplementedError("DownsampleSegForDSTransform2: axes other than the three spatial ones")
        self.ds_scales, self.input_key, self.output_key, self.also = list(ds_scales), input_key, output_key, tuple(also)

    def pyramid(self, t):
        from .. import hip_backend as hb
        if not t.is_cuda or t.dim() < 4:
            raise hb.L.RehrsegHipError("deep supervision: the label pyramid is built from a (..., z, y, x) device tensor")
        shape = tuple(t.shape[-3:])
        extents = pyramid_extents(shape, self.ds_scales)
        work = [l for l, s in enumerate(self.ds_scales) if not all(float(v) == 1 for v in np.atleast_1d(s))]
        out = [t] * len(extents)
        if work:
            src = t.to(torch.float32).contiguous()
            res = hb.label_pyramid(src, [extents[l] for l in work],
                                   [tuple(_cached_index(n, m, t.device) for n, m in zip(shape, extents[l])) for l in work])
            for l, r in zip(work, res):
                out[l] = r
        return out

    def __call__(self, **data_dict):
        for key_in, key_out in [(self.input_key, self.output_key)] + [(k, k) for k in self.also]:
            if data_dict.get(key_in) is not None:
                data_dict[key_out] = self.pyramid(data_dict[key_in])
        return data_dict


def get_training_transforms(patch_size, rotation_for_DA, deep_supervision_scales, mirror_axes, do_dummy_2d_data_aug,
                            order_resampling_data=3, order_resampling_seg=1, border_val_seg=-1, use_mask_for_norm=None,
                            is_cascaded=False, foreground_labels=None, regions=None, ignore_label=None,
                            enable_spatial=True, enable_uncertainty=False, extra_keys=['seg', 'seg_sr', 'uncertainty']):
    """utils/seg_utils.py:632-728 for the arguments REHRSeg passes (train_set.py:79-84, :270-276); anything else
    raises NotImplementedError.  Returns a TrainingTransforms over device tensors."""
    def no(what):
        raise NotImplementedError(f"get_training_transforms: {what} is not used by REHRSeg and not implemented")
    if deep_supervision_scales is not None:
        # REHRSeg passes None or its one hard-coded table (utils/train_set.py:65-69), whose level weights _build_loss
        # hard-codes next to it (utils/seg_utils.py:364-369); any other table has no weights to go with it
        try:
            table = [[float(v) for v in s] for s in deep_supervision_scales]
        except TypeError:
            table = None
        if table != DEEP_SUPERVISION_SCALES:
            no("deep_supervision_scales other than the reference's table (augment.DEEP_SUPERVISION_SCALES)")
    if mirror_axes is not None and len(mirror_axes) > 0:
        no("mirror_axes")
    if not do_dummy_2d_data_aug:
        no("do_dummy_2d_data_aug=False (3-D spatial augmentation)")
    if order_resampling_data != 3 or order_resampling_seg != 1 or border_val_seg != -1:
        no("resampling orders other than 3 / 1 or border_val_seg != -1")
    if use_mask_for_norm is not None and any(use_mask_for_norm):
        no("use_mask_for_norm")
    if is_cascaded:
        no("is_cascaded")
    if regions is not None:
        no("regions")
    if ignore_label is not None:
        no("ignore_label")
    angles = rotation_for_DA
    if tuple(angles.get("y", (0, 0))) != (0, 0) or tuple(angles.get("z", (0, 0))) != (0, 0):
        no("rotation about y / z (the dummy-2D path rotates in-plane only)")
    return TrainingTransforms(list(patch_size)[1:] if enable_spatial else None, angles["x"], enable_spatial,
                              enable_uncertainty, extra_keys, deep_supervision_scales=deep_supervision_scales)
