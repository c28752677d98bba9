"""Losses and normalisation used by the two training loops, under the reference's import
path (`utils.seg_utils`): same names, arguments and numerics as utils/seg_utils.py:74-156
(percentile_normalization, zeroone_normalization -- on the device for device tensors, csrc/intensity_norm.hip, DESIGN
section 3.17 -- and zscore_normalization), :289-372 (RobustCrossEntropyLoss, DC_and_weighted_CE_loss,
_build_loss, with nnunetv2's DeepSupervisionWrapper restated) and :786-885 (DiceLoss, BCEDiceLoss).

The stage-2 loss (`DC_and_weighted_CE_loss`) runs as one fused HIP pass over the logits each way when
given device tensors (`_FusedDCCE`); the torch composition below it is the same
arithmetic and is what the CPU-side tests and the oracle comparisons evaluate.  The tiled predictor
helpers at the end of the file mirror utils/seg_utils.py:176-287, and the validation
after them (:45-72, :158-174, :730-784: read_image, preprocess_image, calculate_dice, evaluate_case) runs a case on
the device through csrc/seg_eval.hip.
`TopKLoss` / `DC_and_topk_loss` (`_build_loss(topk=k)`; not the reference's: nnU-Net's top-k CE over the same loss map,
restated, parity unpinned) run on the device through csrc/seg_loss_topk.hip (`_FusedDCTopK`).
`MemoryEfficientSoftDiceLoss` lives in nnunetv2==2.3.1 (absent offline): its published
formula is restated in `SoftDiceLoss` below -- that term's parity is unpinned.
"""
import functools

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .augment import (DEEP_SUPERVISION_SCALES, DownsampleSegForDSTransform2, MySpatialTransform,  # noqa: F401
                      get_training_transforms)                                              # (utils/seg_utils.py:511-728)


def zscore_normalization(image):
    """Per-sample z-score of channel 0, IN PLACE on the caller's tensor (ref :137-149);
    returns the normalised channel as (B, 1, ...)."""
    if not isinstance(image, torch.Tensor):
        image = image.astype(np.float32, copy=False)
        image -= image.mean()
        image /= max(image.std(), 1e-8)
        return image
    outs = []
    for i in range(image.shape[0]):
        view = image[i:i + 1, 0, ...]
        mean, std = view.mean(), view.std()
        view -= mean
        view /= max(std, 1e-8)
        outs.append(view)
    return torch.stack(outs, dim=0)


# ----------------------------------------------------------------------------- percentile / zero-one
def _percentile_norm(input_tensor, reference_tensor=None, p_min=0.5, p_max=99.5, strictlyPositive=True):
    """ref :74-98 on the host: clip to the two percentiles (the lower one raised to 0 with strictlyPositive), scale to
    [0, 1].  Only reference_tensor=None is reachable from the public function."""
    if reference_tensor is None:
        reference_tensor = input_tensor
    v_min, v_max = np.percentile(reference_tensor, [p_min, p_max])
    if v_min < 0 and strictlyPositive:
        v_min = 0
    output_tensor = np.clip(input_tensor, v_min, v_max)
    return (output_tensor - v_min) / (v_max - v_min)


def _channel0_runs(image, what):
    """image[:, 0] of a (B, C, ...) device tensor, every item one dense run; ValueError for any other layout."""
    if image.dim() < 2:
        raise ValueError(f"{what}: expected a (B, C, ...) tensor, got {tuple(image.shape)}")
    ch = image[:, 0]
    if ch.numel() == 0 or not ch[0].is_contiguous():
        raise ValueError(f"{what}: channel 0 of every item must be one dense run (C == 1 or a contiguous NCDHW "
                         f"tensor); got shape {tuple(image.shape)} with strides {tuple(image.stride())} "
                         "(channels-last?): call .contiguous() first")
    return ch


def _percentile_normalization_device(image, p_min=0.5, p_max=99.5, strictlyPositive=True):
    """percentile_normalization of a device tensor: two order statistics per percentile by radix select, numpy's
    lerp and the clip / scale pass, all on the device and without a host sync (csrc/intensity_norm.hip)."""
    from .. import ops
    from ..hip_backend import INTENSITY_PERCENTILE, percentile_plan
    be = ops.get_backend()
    ch = _channel0_runs(image, "percentile_normalization")
    if ch.dtype != torch.float32:
        ch = ch.to(torch.float32)
    S = ch[0].numel()
    ranks, t = percentile_plan(S, (p_min, p_max))
    bounds = be.percentile_bounds(be.order_stats(ch, ranks), t, strictlyPositive)
    out = be.intensity_apply(ch, bounds, INTENSITY_PERCENTILE)
    return out.view((image.shape[0], 1) + tuple(image.shape[2:]))


def _zeroone_normalization_device(image):
    """zeroone_normalization of a float32 device tensor, channel 0 rewritten in place; returns that channel as a
    (B, 1, ...) view of `image`.  No host sync."""
    from .. import ops
    from ..hip_backend import INTENSITY_ZEROONE
    be = ops.get_backend()
    ch = _channel0_runs(image, "zeroone_normalization")
    if ch.dtype != torch.float32:
        raise ValueError(f"zeroone_normalization writes the caller's tensor in place: float32 on the device, got "
                         f"{ch.dtype}")
    if ch.is_contiguous():
        stats = be.aug_stats(ch)
    else:       # C > 1: the items are apart, one statistics call each
        stats = torch.empty((ch.shape[0], 4), dtype=torch.float64, device=ch.device)
        for b in range(ch.shape[0]):
            be.aug_stats(ch[b:b + 1], out=stats[b:b + 1])
    be.intensity_apply(ch, stats[:, 2:], INTENSITY_ZEROONE, out=ch)
    return image[:, 0:1]


def percentile_normalization(image, p_min=0.5, p_max=99.5, strictlyPositive=True):
    """ref :100-114: clip channel 0 of every item at its p_min / p_max percentiles and scale to [0, 1]; returns
    (B, 1, ...), or the normalised array for a numpy array (taken as one item).

    numpy arrays and CPU tensors run on the host as the reference's lines do.  A device tensor stays on the device
    (DESIGN section 3.17): the result is a float32 device tensor (B, 1, ...), the input is not written and the call
    makes no host sync.  Deviation: the reference moves a device tensor to the CPU and, under numpy 2, returns
    float64; here the bounds are numpy's float64 percentiles rounded to float32 and the clip, the subtraction and the
    division are float32.  Channel 0 of every item must be one dense run (C == 1 or contiguous NCDHW), ValueError
    otherwise.  An item with a NaN, or with v_max == v_min, comes back all NaN, as from the reference."""
    if isinstance(image, torch.Tensor):
        if image.is_cuda:
            return _percentile_normalization_device(image, p_min, p_max, strictlyPositive)
        out_imgs = []
        for i in range(image.shape[0]):
            img = image[i:i + 1, 0, ...].cpu().numpy()
            img = _percentile_norm(img, p_min=p_min, p_max=p_max, strictlyPositive=strictlyPositive)
            out_imgs.append(torch.from_numpy(img))
        return torch.stack(out_imgs, dim=0)
    image = image.astype(np.float32, copy=False)
    return _percentile_norm(image, p_min=p_min, p_max=p_max, strictlyPositive=strictlyPositive)


def zeroone_normalization(image):
    """ref :116-135: (x - min) / (max - min) of channel 0 of every item, IN PLACE on the caller's tensor (or float32
    array); returns the normalised channel as (B, 1, ...).  A device tensor (float32, channel 0 of every item one
    dense run) is rewritten by the kernels without a host sync; min and max come from rehr_aug_stats_f32, which skips
    NaNs where torch's min / max would return NaN.  A constant item gives 0 / 0 = NaN, as the reference."""
    if isinstance(image, torch.Tensor):
        if image.is_cuda:
            return _zeroone_normalization_device(image).clone()     # the reference's torch.stack copies as well
        out_imgs = []
        for i in range(image.shape[0]):
            img = image[i:i + 1, 0, ...]
            lo, hi = img.min(), img.max()
            img -= lo
            img /= (hi - lo)
            out_imgs.append(img)
        return torch.stack(out_imgs, dim=0)
    image = image.astype(np.float32, copy=False)
    lo, hi = image.min(), image.max()
    image -= lo
    image /= (hi - lo)
    return image


def intensity_percentiles(image, q, *, device=None):
    """numpy.percentile(image[b].astype(float64), q) for every item b of `image` (B, ...), as a (B, len(q)) float64
    tensor on the device, without a host sync: exact order statistics by radix select and numpy's 'linear' lerp in
    fp64.  `image`: a numpy array or a tensor, host or device, converted to float32; `q`: up to 4
    percentiles in [0, 100].  An item with a NaN gives NaN.  `device` defaults to a device tensor's, else the current
    device."""
    from .. import ops
    from ..hip_backend import PERCENTILE_MAX_Q, percentile_plan
    be = ops.get_backend()
    q = [float(v) for v in np.atleast_1d(np.asarray(q, dtype=np.float64))]
    if not 1 <= len(q) <= PERCENTILE_MAX_Q:
        raise ValueError(f"intensity_percentiles: 1 to {PERCENTILE_MAX_Q} percentiles per call, got {len(q)}")
    dev = _map_device(device, image)
    if isinstance(image, torch.Tensor):
        t = image.detach().to(torch.float32)
        if t.device != dev:
            t = t.to(dev) if t.is_cuda else _upload(t.contiguous(), dev)
    else:
        t = _upload(torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32)), dev)
    if t.dim() < 1 or t.numel() == 0:
        raise ValueError(f"intensity_percentiles: expected a non-empty (B, ...) volume, got {tuple(t.shape)}")
    t = t.contiguous()
    ranks, frac = percentile_plan(t[0].numel(), q)
    return be.percentile_bounds(be.order_stats(t, ranks), frac, False)


def _norm_spec(norm, also=()):
    """The device normalisations by name: 'percentile' -> ('percentile', 0.5, 99.5), ('percentile', lo, hi),
    'zeroone' -> ('zeroone',); a value in `also` is returned as it is; anything else raises ValueError."""
    if any(norm is a or (isinstance(a, str) and isinstance(norm, str) and norm == a) for a in also):
        return norm
    if isinstance(norm, str) and norm == "percentile":
        return ("percentile", 0.5, 99.5)
    if isinstance(norm, str) and norm == "zeroone":
        return ("zeroone",)
    if isinstance(norm, (tuple, list)) and len(norm) == 3 and norm[0] == "percentile":
        lo, hi = float(norm[1]), float(norm[2])
        if not 0.0 <= lo < hi <= 100.0:
            raise ValueError(f"norm: percentiles 0 <= p_min < p_max <= 100, got {norm!r}")
        return ("percentile", lo, hi)
    names = [repr(a) for a in also] + ["'percentile'", "('percentile', p_min, p_max)", "'zeroone'"]
    raise ValueError(f"norm: one of {', '.join(names)}; got {norm!r}")


def _normalize_on_device(vol, spec):
    """One float32 volume of any shape on the device, normalised as _norm_spec's `spec` says: a new tensor of the
    same shape, no host sync."""
    x = vol.to(torch.float32).contiguous().view((1, 1) + tuple(vol.shape))
    if spec[0] == "percentile":
        return _percentile_normalization_device(x, spec[1], spec[2], True).view(tuple(vol.shape))
    if x.data_ptr() == vol.data_ptr():      # the caller's volume is not written
        x = x.clone()
    return _zeroone_normalization_device(x).view(tuple(vol.shape))


class RobustCrossEntropyLoss(nn.CrossEntropyLoss):
    """CE on float targets with an optional uncertainty weight (ref :289-304).  The weight has a
    channel axis the loss map lacks, so (B,D,H,W) * (B,1,D,H,W) broadcasts to (B,B,D,H,W)
    before the mean -- reproduced as is."""

    def loss_map(self, input, target, uncertainty=None):
        if target.ndim == input.ndim:
            assert target.shape[1] == 1
            target = target[:, 0]
        loss = nn.CrossEntropyLoss.forward(self, input, target.long())
        if uncertainty is not None:
            loss = loss * uncertainty
        return loss

    def forward(self, input, target, uncertainty=None):
        return self.loss_map(input, target, uncertainty).mean()


class SoftDiceLoss(nn.Module):
    """nnunetv2 MemoryEfficientSoftDiceLoss, restated (unpinned): -mean over (b, c) of
    (2*intersect + smooth) / clip(sum_gt + sum_pred + smooth, 1e-8)."""

    def __init__(self, apply_nonlin=None, batch_dice=False, do_bg=True, smooth=1.0, ddp=False):
        super().__init__()
        if ddp and batch_dice:
            raise NotImplementedError("REHRSeg passes batch_dice=False, ddp=False (utils/seg_utils.py:356-357)")
        self.apply_nonlin, self.batch_dice, self.do_bg, self.smooth = apply_nonlin, batch_dice, do_bg, smooth

    def forward(self, x, y, loss_mask=None):
        if self.apply_nonlin is not None:
            x = self.apply_nonlin(x)
        axes = tuple(range(2, x.ndim))
        with torch.no_grad():
            if x.ndim != y.ndim:
                y = y.view((y.shape[0], 1, *y.shape[1:]))
            if x.shape == y.shape:
                y_onehot = y
            else:
                y_onehot = torch.zeros(x.shape, device=x.device, dtype=torch.bool)
                y_onehot.scatter_(1, y.long(), 1)
            if not self.do_bg:
                y_onehot = y_onehot[:, 1:]
            sum_gt = y_onehot.sum(axes) if loss_mask is None else (y_onehot * loss_mask).sum(axes)
        if not self.do_bg:
            x = x[:, 1:]
        if loss_mask is None:
            intersect, sum_pred = (x * y_onehot).sum(axes), x.sum(axes)
        else:
            intersect, sum_pred = (x * y_onehot * loss_mask).sum(axes), (x * loss_mask).sum(axes)
        if self.batch_dice:
            intersect, sum_pred, sum_gt = intersect.sum(0), sum_pred.sum(0), sum_gt.sum(0)
        dc = (2 * intersect + self.smooth) / torch.clip(sum_gt + sum_pred + self.smooth, 1e-8)
        return -dc.mean()


def softmax_helper_dim1(x):
    return torch.softmax(x, 1)


class _FusedDCCE(torch.autograd.Function):
    """softmax + (uncertainty-weighted) CE + soft Dice as one HIP pass over the logits each way
    (include/rehrseg_hip.h: rehr_seg_loss_{fwd,bwd}_f32)."""

    @staticmethod
    def forward(ctx, logits, target, unc, w_ce, w_dice, smooth, do_bg):
        from .. import hip_backend as hb, ops
        logits = ops.to_cl(logits)
        N, C = logits.shape[:2]
        S = logits.shape[2] * logits.shape[3] * logits.shape[4]
        target = target.reshape(N, S).to(torch.float32).contiguous()
        unc = None if unc is None else unc.reshape(N, S).to(torch.float32).contiguous()
        stats = hb.seg_loss_fwd(logits, target, unc)
        ipg = stats[:-1].view(N, C, 3)
        dc = (2 * ipg[..., 0] + smooth) / torch.clip(ipg[..., 2] + ipg[..., 1] + smooth, 1e-8)
        if not do_bg:
            dc = dc[:, 1:]
        loss = w_ce * stats[-1] / (N * N * S if unc is not None else N * S) - w_dice * dc.mean()
        ctx.save_for_backward(logits, target, unc, stats)
        ctx.cfg = (w_ce, w_dice, smooth, do_bg)
        return loss.to(torch.float32)

    @staticmethod
    def backward(ctx, grad_out):
        from .. import hip_backend as hb
        logits, target, unc, stats = ctx.saved_tensors
        w_ce, w_dice, smooth, do_bg = ctx.cfg
        go = grad_out.to(torch.float32).reshape(1).contiguous()
        return hb.seg_loss_bwd(logits, target, unc, stats, w_ce, w_dice, smooth, do_bg, go), None, None, None, \
            None, None, None


class DC_and_weighted_CE_loss(nn.Module):
    """ref :306-351: weight_ce * CE(uncertainty-weighted) + weight_dice * soft Dice."""
    _warned = False

    def __init__(self, soft_dice_kwargs, ce_kwargs, weight_ce=1, weight_dice=1, ignore_label=None,
                 dice_class=SoftDiceLoss):
        super().__init__()
        if ignore_label is not None:
            ce_kwargs["ignore_index"] = ignore_label
        self.weight_dice, self.weight_ce, self.ignore_label = weight_dice, weight_ce, ignore_label
        self.ce = RobustCrossEntropyLoss(**ce_kwargs)
        self.dc = dice_class(apply_nonlin=softmax_helper_dim1, **soft_dice_kwargs)

    def _fusable(self, net_output, target, uncertainty):
        """The fused kernel covers what the reference's stage-2 loop passes (train_all.py:538-548): 5-D logits with
        2..4 classes, a (N,1,D,H,W) label map with values in [0, C) (precondition, unchecked: torch's CE would raise),
        no ignore label, and an uncertainty map of exactly (N,1,D,H,W) -- the shape whose product with the (N,D,H,W)
        loss map broadcasts across samples; any other uncertainty shape multiplies differently
        in the reference and takes the composition below."""
        return net_output.is_cuda and self._fusable_config(net_output, target, uncertainty)

    def _fusable_config(self, net_output, target, uncertainty):
        dc = self.dc
        N = net_output.shape[0]
        return (net_output.dim() == 5 and self.ignore_label is None and
                type(dc) is SoftDiceLoss and not dc.batch_dice and dc.apply_nonlin is softmax_helper_dim1 and
                2 <= net_output.shape[1] <= 4 and target.dim() == 5 and target.shape[1] == 1 and
                target.numel() == net_output.numel() // net_output.shape[1] and
                (uncertainty is None or tuple(uncertainty.shape) == (N, 1) + tuple(net_output.shape[2:])) and
                self.ce.weight is None and self.ce.label_smoothing == 0.0)

    def forward(self, net_output, target, uncertainty=None):
        if self._fusable(net_output, target, uncertainty):  # device tensors: one HIP pass each way
            return _FusedDCCE.apply(net_output, target, uncertainty, float(self.weight_ce), float(self.weight_dice),
                                    float(self.dc.smooth), bool(self.dc.do_bg))
        if net_output.is_cuda and not DC_and_weighted_CE_loss._warned:
            DC_and_weighted_CE_loss._warned = True
            import warnings
            warnings.warn("DC_and_weighted_CE_loss: configuration outside the fused HIP kernel (classes > 4, ignore label, "
                          "class weights or an unusual target / uncertainty shape): composed from torch ops on the device")
        return self._composition(net_output, target, uncertainty)

    def _composition(self, net_output, target, uncertainty):
        if self.ignore_label is not None:
            assert target.shape[1] == 1
            mask = target != self.ignore_label
            target_dice = torch.where(mask, target, 0)
            num_fg = mask.sum()
        else:
            target_dice, mask = target, None
        dc_loss = self.dc(net_output, target_dice, loss_mask=mask) if self.weight_dice != 0 else 0
        ce_loss = self.ce(net_output, target[:, 0], uncertainty) \
            if self.weight_ce != 0 and (self.ignore_label is None or num_fg > 0) else 0
        return self.weight_ce * ce_loss + self.weight_dice * dc_loss


def _topk_count(M, k):
    """K = int(M * k / 100), as TopKLoss computes it; raises before anything is launched."""
    if not 0 < k <= 100:
        raise ValueError(f"top-k percentage k = {k} is outside (0, 100]")
    K = int(M * k / 100)
    if K < 1:
        raise ValueError(f"top-k: k = {k} % of the {M} elements of the loss map leaves none (K = {K}); "
                         "the patch is too small for this k")
    return K


class TopKLoss(RobustCrossEntropyLoss):
    """nnunetv2's TopKLoss, restated (absent offline -> parity unpinned), with RobustCrossEntropyLoss's uncertainty
    weight: the mean of the k percent largest elements of the loss map the parent forms before its mean -- (B,D,H,W),
    or (B,B,D,H,W) with a (B,1,D,H,W) uncertainty.  K = int(numel * k / 100)."""

    def __init__(self, weight=None, ignore_index=-100, k=10, label_smoothing=0.0, **kwargs):
        if not 0 < k <= 100:
            raise ValueError(f"top-k percentage k = {k} is outside (0, 100]")
        kwargs.pop("reduction", None)
        super().__init__(weight=weight, ignore_index=ignore_index, reduction="none", label_smoothing=label_smoothing,
                         **kwargs)
        self.k = k

    def forward(self, input, target, uncertainty=None):
        loss = self.loss_map(input, target, uncertainty)
        K = _topk_count(loss.numel(), self.k)
        return loss.reshape(-1).topk(K, sorted=False)[0].mean()


class _FusedDCTopK(torch.autograd.Function):
    """softmax + top-k (uncertainty-weighted) CE + soft Dice on the device: the loss map, an exact select of its K-th
    largest element and the counts around it forward, one pass backward (include/rehrseg_hip.h:
    rehr_seg_topk_{fwd,bwd}_f32).  Elements equal to the threshold share the gradient that is
    left: (K - n_gt) / n_eq each."""

    @staticmethod
    def forward(ctx, logits, target, unc, K, w_ce, w_dice, smooth, do_bg):
        from .. import ops
        be = ops.get_backend()
        logits = ops.to_cl(logits)
        N, C = logits.shape[:2]
        S = logits.shape[2] * logits.shape[3] * logits.shape[4]
        target = target.reshape(N, S).to(torch.float32).contiguous()
        unc = None if unc is None else unc.reshape(N, S).to(torch.float32).contiguous()
        stats, workspace = be.seg_topk_fwd(logits, target, unc, K)
        ipg = stats[:N * C * 3].view(N, C, 3)
        dc = (2 * ipg[..., 0] + smooth) / torch.clip(ipg[..., 2] + ipg[..., 1] + smooth, 1e-8)
        if not do_bg:
            dc = dc[:, 1:]
        n_gt, _, above, thr = stats[N * C * 3 + 1:].unbind()
        rest = K - n_gt                 # what the elements on the threshold supply; 0 * inf must not make a NaN
        topk = (above + torch.where(rest > 0, rest * thr, torch.zeros_like(thr))) / K
        loss = w_ce * topk - w_dice * dc.mean()
        ctx.save_for_backward(logits, target, unc, stats, workspace)
        ctx.cfg = (K, w_ce, w_dice, smooth, do_bg)
        return loss.to(torch.float32)

    @staticmethod
    def backward(ctx, grad_out):
        from .. import ops
        logits, target, unc, stats, workspace = ctx.saved_tensors
        K, w_ce, w_dice, smooth, do_bg = ctx.cfg
        go = grad_out.to(torch.float32).reshape(1).contiguous()
        dl = ops.get_backend().seg_topk_bwd(logits, target, unc, K, stats, workspace, w_ce, w_dice, smooth, do_bg, go)
        return dl, None, None, None, None, None, None, None


class DC_and_topk_loss(nn.Module):
    """nnunetv2's DC_and_topk_loss, restated (absent offline -> parity unpinned) over this file's losses:
    weight_ce * TopKLoss(k) + weight_dice * soft Dice, the Dice exactly as in DC_and_weighted_CE_loss, the CE with
    RobustCrossEntropyLoss's optional uncertainty.  Not a DC_and_weighted_CE_loss: DeepSupervisionWrapper's one-launch
    node must not take it, it sums this loss level by level."""
    _warned = False
    _fusable_config = DC_and_weighted_CE_loss._fusable_config
    _composition = DC_and_weighted_CE_loss._composition

    def __init__(self, soft_dice_kwargs, ce_kwargs, weight_ce=1, weight_dice=1, ignore_label=None, k=10,
                 dice_class=SoftDiceLoss):
        super().__init__()
        if ignore_label is not None:
            ce_kwargs["ignore_index"] = ignore_label
        self.weight_dice, self.weight_ce, self.ignore_label = weight_dice, weight_ce, ignore_label
        self.ce = TopKLoss(k=k, **ce_kwargs)
        self.dc = dice_class(apply_nonlin=softmax_helper_dim1, **soft_dice_kwargs)

    def _map_elements(self, net_output, uncertainty):
        N = net_output.shape[0]
        return (net_output.numel() // net_output.shape[1]) * (N if uncertainty is not None else 1)

    def _fusable(self, net_output, target, uncertainty):
        """DC_and_weighted_CE_loss's conditions, at most 4 samples and a loss map the select can take."""
        from .. import ops
        from ..hip_backend import SEG_TOPK_MAX_ELEMENTS, SEG_TOPK_MAX_SAMPLES
        on_device = net_output.is_cuda or getattr(ops.get_backend(), "seg_topk_on_host", False)   # the latter: tests
        return (on_device and self._fusable_config(net_output, target, uncertainty) and
                net_output.shape[0] <= SEG_TOPK_MAX_SAMPLES and
                self._map_elements(net_output, uncertainty) <= SEG_TOPK_MAX_ELEMENTS)

    def forward(self, net_output, target, uncertainty=None):
        if self._fusable(net_output, target, uncertainty):
            K = _topk_count(self._map_elements(net_output, uncertainty), self.ce.k)
            return _FusedDCTopK.apply(net_output, target, uncertainty, K, float(self.weight_ce),
                                      float(self.weight_dice), float(self.dc.smooth), bool(self.dc.do_bg))
        if net_output.is_cuda and not DC_and_topk_loss._warned:
            DC_and_topk_loss._warned = True
            import warnings
            warnings.warn("DC_and_topk_loss: configuration outside the fused HIP kernel (classes > 4, batch > 4, more "
                          "than 2**30 loss-map elements, ignore label, class weights or an unusual target / uncertainty "
                          "shape): composed from torch ops on the device")
        return self._composition(net_output, target, uncertainty)


@functools.lru_cache(maxsize=16)
def _ds_coefficients(weights, sizes, N, with_unc, w_ce, w_dice, device):
    """(levels, 2) double on the device: per level the factors of its CE statistic and of its mean Dice in the weighted
    sum.  Uploaded once per configuration, so that the sum over levels is formed without a host sync."""
    rows = [(w * w_ce / ((N * N * S) if with_unc else (N * S)) if w != 0 else 0.0, w * w_dice)
            for w, S in zip(weights, sizes)]
    return _upload(torch.tensor(rows, dtype=torch.float64), torch.device(device))


class _FusedDSDCCE(torch.autograd.Function):
    """DeepSupervisionWrapper(DC_and_weighted_CE_loss) over device tensors: all levels in one HIP launch each way
    (include/rehrseg_hip.h: rehr_seg_loss_ds_{fwd,bwd}_f32).  The logits are the trailing arguments.  The wrapper hands
    in the weighted levels only: a level with weight 0 stays outside the graph, so its logits get no gradient at all
    (a None returned here would be filled with zeros by the node that made those logits)."""

    @staticmethod
    def forward(ctx, cfg, weights, targets, uncs, *logits):
        from .. import hip_backend as hb, ops
        w_ce, w_dice, smooth, do_bg = cfg
        n = len(logits)
        N, C = logits[0].shape[:2]
        sizes = [x.shape[2] * x.shape[3] * x.shape[4] for x in logits]
        xs = [ops.to_cl(x.float()) for x in logits]
        ts = [t.reshape(N, S).to(torch.float32).contiguous() for t, S in zip(targets, sizes)]
        us = None if uncs is None else [u.reshape(N, S).to(torch.float32).contiguous() for u, S in zip(uncs, sizes)]
        stats = hb.seg_loss_ds_fwd(xs, ts, us, weights)
        ipg = stats[:, :-1].view(n, N, C, 3)
        dc = (2 * ipg[..., 0] + smooth) / torch.clip(ipg[..., 2] + ipg[..., 1] + smooth, 1e-8)
        if not do_bg:
            dc = dc[:, :, 1:]
        k = _ds_coefficients(tuple(weights), tuple(sizes), N, uncs is not None, w_ce, w_dice, str(stats.device))
        loss = (k[:, 0] * stats[:, -1]).sum() - (k[:, 1] * dc.mean((1, 2))).sum()
        ctx.save_for_backward(stats, *xs, *ts, *([] if us is None else us))
        ctx.cfg, ctx.weights = cfg, weights
        ctx.dtypes = [x.dtype for x in logits]
        return loss.to(torch.float32)

    @staticmethod
    def backward(ctx, grad_out):
        from .. import hip_backend as hb
        stats, *saved = ctx.saved_tensors
        n = len(ctx.weights)
        xs, ts, us = saved[:n], saved[n:2 * n], (saved[2 * n:] or None)
        w_ce, w_dice, smooth, do_bg = ctx.cfg
        go = grad_out.to(torch.float32).reshape(1).contiguous()
        dl = hb.seg_loss_ds_bwd(xs, ts, us, ctx.weights, stats, w_ce, w_dice, smooth, do_bg, go)
        return (None, None, None, None, *[g if g.dtype == dt else g.to(dt) for g, dt in zip(dl, ctx.dtypes)])


class DeepSupervisionWrapper(nn.Module):
    """nnunetv2's DeepSupervisionWrapper, restated (absent offline -> parity unpinned): every positional argument is a
    list or tuple with one entry per output level, and the result is
        sum(weight_factors[i] * loss(*args_i) for i, args_i in enumerate(zip(*args)) if weight_factors[i] != 0).
    zip truncates to the shortest list; a level with weight 0 is not evaluated, so its logits receive no gradient.
    Trailing arguments that are None (the step's `uncertainty=None`) are dropped.

    Over device tensors that DC_and_weighted_CE_loss would take through its fused kernel at every weighted level,
    the whole sum is one autograd node with one HIP launch each way (`_FusedDSDCCE`); otherwise it is the Python sum
    above over the inner loss."""

    def __init__(self, loss, weight_factors=None):
        super().__init__()
        if weight_factors is not None and not any(x != 0 for x in weight_factors):
            raise ValueError("At least one weight factor should be != 0.0")
        self.weight_factors = None if weight_factors is None else tuple(float(x) for x in weight_factors)
        self.loss = loss

    def forward(self, *args):
        while args and args[-1] is None:
            args = args[:-1]
        if not all(isinstance(a, (tuple, list)) for a in args):
            raise TypeError("DeepSupervisionWrapper: every argument is a list or tuple with one entry per output level "
                            f"(the uncertainty as well: one map per level), got {[type(a).__name__ for a in args]}")
        levels = list(zip(*args))
        weights = (1.0,) * len(levels) if self.weight_factors is None else self.weight_factors
        if len(weights) < len(levels):
            raise ValueError(f"{len(levels)} output levels but only {len(weights)} weight factors")
        weights = weights[:len(levels)]
        live = [i for i, w in enumerate(weights) if w != 0]
        if not live:
            raise ValueError("every level present carries weight 0")
        for i in live:
            x, y = levels[i][0], levels[i][1]
            if tuple(x.shape[2:]) != tuple(y.shape[-(x.dim() - 2):]) or x.shape[0] != y.shape[0]:
                raise ValueError(f"level {i}: logits {tuple(x.shape)} do not match the label level {tuple(y.shape)}")
        if self._fusable(levels, live):
            inner = self.loss
            cfg = (float(inner.weight_ce), float(inner.weight_dice), float(inner.dc.smooth), bool(inner.dc.do_bg))
            # only the weighted levels enter the node: a gradient of None returned for an input would be turned into
            # zeros by the node that produced those logits, and the optimizer would then decay that head
            used = [levels[i] for i in live]
            uncs = [lv[2] for lv in used] if len(args) == 3 else None
            return _FusedDSDCCE.apply(cfg, tuple(weights[i] for i in live), [lv[1] for lv in used], uncs,
                                      *[lv[0] for lv in used])
        return sum(weights[i] * self.loss(*levels[i]) for i in live)

    def _fusable(self, levels, live):
        from ..lib import DS_MAX_LEVELS
        if not isinstance(self.loss, DC_and_weighted_CE_loss) or not 2 <= len(levels[0]) <= 3 or \
                len(levels) > DS_MAX_LEVELS:
            return False
        first = levels[live[0]][0]
        return all(self.loss._fusable(*levels[i], *([None] * (3 - len(levels[i])))) and
                   tuple(levels[i][0].shape[:2]) == tuple(first.shape[:2]) and levels[i][0].device == first.device
                   for i in live)


def _build_loss(enable_deep_supervision=False, weight_dice=1, topk=None):
    """ref :353-372.  With enable_deep_supervision the loss is wrapped for the network's per-stage outputs: weights
    1 / 2**i over the reference's six scales, the last set to 0, normalised to sum 1 (:363-369).
    topk (not the reference's: nnU-Net's DC_and_topk_loss): None is the reference's loss; a
    percentage k builds DC_and_topk_loss(k=k), whose CE term averages the hardest k % of the voxels only."""
    dice_kwargs = {"batch_dice": False, "smooth": 1e-5, "do_bg": False, "ddp": False}
    if topk is None:
        loss = DC_and_weighted_CE_loss(dice_kwargs, {"reduction": "none"}, weight_ce=1, weight_dice=weight_dice,
                                       ignore_label=None, dice_class=SoftDiceLoss)
    else:
        loss = DC_and_topk_loss(dice_kwargs, {}, weight_ce=1, weight_dice=weight_dice, ignore_label=None, k=topk,
                                dice_class=SoftDiceLoss)
    if enable_deep_supervision:
        weights = np.array([1 / (2 ** i) for i in range(len(DEEP_SUPERVISION_SCALES))])
        weights[-1] = 0
        weights = weights / weights.sum()
        loss = DeepSupervisionWrapper(loss, weights)
    return loss


def compute_per_channel_dice(input, target, epsilon=1e-6, weight=None):
    """ref :829-857: 2*sum(p*t) / clamp(sum(p^2) + sum(t^2), eps) per channel."""
    assert input.size() == target.size()
    c = input.size(1)
    p = input.transpose(0, 1).reshape(c, -1)
    t = target.transpose(0, 1).reshape(c, -1).float()
    inter = (p * t).sum(-1)
    if weight is not None:
        inter = weight * inter
    return 2 * (inter / ((p * p).sum(-1) + (t * t).sum(-1)).clamp(min=epsilon))


class DiceLoss(nn.Module):
    def __init__(self, weight=None, normalization="sigmoid"):
        super().__init__()
        self.register_buffer("weight", weight)
        assert normalization in ("sigmoid", "softmax", "none")
        self.normalization = {"sigmoid": torch.sigmoid, "softmax": lambda x: torch.softmax(x, 1),
                              "none": lambda x: x}[normalization]

    def forward(self, input, target):
        return 1.0 - torch.mean(compute_per_channel_dice(self.normalization(input), target, weight=self.weight))


class _FusedBCEDice(torch.autograd.Function):
    """BCE-with-logits + sigmoid Dice as one HIP pass over the logits each way (rehr_bce_dice_{fwd,bwd}_f32)."""

    @staticmethod
    def forward(ctx, logits, target, alpha, beta):
        from .. import hip_backend as hb
        N, C = logits.shape[:2]
        x = logits.reshape(N, C, -1).to(torch.float32).contiguous()
        t = target.reshape(N, C, -1).to(torch.float32).contiguous()
        stats = hb.bce_dice_fwd(x, t)
        dice = 2 * stats[:, 1] / (stats[:, 2] + stats[:, 3]).clamp(min=1e-6)
        loss = alpha * stats[:, 0].sum() / x.numel() + beta * (1.0 - dice.mean())
        ctx.save_for_backward(x, t, stats)
        ctx.cfg = (alpha, beta, tuple(logits.shape))
        return loss.to(torch.float32)

    @staticmethod
    def backward(ctx, grad_out):
        from .. import hip_backend as hb
        x, t, stats = ctx.saved_tensors
        alpha, beta, shape = ctx.cfg
        go = grad_out.to(torch.float32).reshape(1).contiguous()
        return hb.bce_dice_bwd(x, t, stats, alpha, beta, go).reshape(shape), None, None, None


class BCEDiceLoss(nn.Module):
    """alpha * BCEWithLogits + beta * Dice (ref :872-885).  Device tensors take one fused HIP pass each way."""

    def __init__(self, alpha, beta):
        super().__init__()
        self.alpha, self.beta = alpha, beta
        self.bce = nn.BCEWithLogitsLoss()
        self.dice = DiceLoss()

    def forward(self, input, target):
        if input.is_cuda and input.dim() >= 3 and input.shape == target.shape and self.dice.weight is None:
            return _FusedBCEDice.apply(input, target, float(self.alpha), float(self.beta))
        return self.alpha * self.bce(input, target) + self.beta * self.dice(input, target)


# ----------------------------------------------------------------------------- whole-volume inference
# (ref utils/seg_utils.py:176-287: nnU-Net style tiled predictor with mirror TTA)
def compute_steps_for_sliding_window(image_size, tile_size, tile_step_size):
    """ref :176-199."""
    assert [i >= j for i, j in zip(image_size, tile_size)], "image size must be as large or larger than patch_size"
    assert 0 < tile_step_size <= 1, "step_size must be larger than 0 and smaller or equal to 1"
    target = [i * tile_step_size for i in tile_size]
    num_steps = [int(np.ceil((i - k) / j)) + 1 for i, j, k in zip(image_size, target, tile_size)]
    steps = []
    for dim in range(len(tile_size)):
        max_step = image_size[dim] - tile_size[dim]
        actual = max_step / (num_steps[dim] - 1) if num_steps[dim] > 1 else 99999999999
        steps.append([int(np.round(actual * i)) for i in range(num_steps[dim])])
    return steps


def _internal_get_sliding_window_slicers(image_size, patch_size=[14, 320, 384], tile_step_size=0.5):
    """ref :229-238."""
    steps = compute_steps_for_sliding_window(image_size, patch_size, tile_step_size)
    return [tuple([slice(None), *[slice(si, si + ti) for si, ti in zip((sx, sy, sz), patch_size)]])
            for sx in steps[0] for sy in steps[1] for sz in steps[2]]


def _internal_maybe_mirror_and_predict(model, x, out_idx=None, deep_supervision=True, save=False):
    """ref :201-227: mean over the identity and the 7 mirrorings of (D,H,W).  The 8 variants are independent
    (InstanceNorm is per sample), so they go through the network as ONE batch instead of 8 calls; the
    un-mirrored predictions are summed in the reference's order."""
    import itertools
    mirror_axes = (0, 1, 2)
    assert max(mirror_axes) <= x.ndim - 3, "mirror_axes does not match the dimension of the input!"
    combos = [c for i in range(len(mirror_axes)) for c in itertools.combinations([m + 2 for m in mirror_axes], i + 1)]
    B = x.shape[0]
    pred = model(torch.cat([x] + [torch.flip(x, axes) for axes in combos], 0))
    if out_idx is not None:
        pred = pred[out_idx]
        if out_idx == 0 and deep_supervision:
            pred = pred[0]
    prediction = pred[:B].clone()
    for k, axes in enumerate(combos):
        prediction += torch.flip(pred[(k + 1) * B:(k + 2) * B], axes)
    prediction /= (len(combos) + 1)
    return prediction


@functools.lru_cache(maxsize=2)
def compute_gaussian(tile_size, sigma_scale=1. / 8, value_scaling_factor=1, dtype=torch.float16, device="cpu"):
    """nnunetv2 compute_gaussian, restated (absent offline -> unpinned): Gaussian importance map of a tile."""
    from scipy.ndimage import gaussian_filter
    tmp = np.zeros(tile_size)
    tmp[tuple(i // 2 for i in tile_size)] = 1
    g = gaussian_filter(tmp, [i * sigma_scale for i in tile_size], 0, mode="constant", cval=0)
    g = torch.from_numpy(g)
    g = g / (torch.max(g) / value_scaling_factor)
    g = g.to(device=device, dtype=dtype)
    mask = g == 0
    g[mask] = torch.min(g[~mask])
    return g


def _internal_predict_sliding_window_return_logits(data, slicers, network, do_on_device=True, out_idx=None,
                                                   slice_seperation=1, patch_size=[14, 320, 384],
                                                   use_gaussian=False, deep_supervision=True):
    """ref :240-287 (fp16 accumulators as there; (sic) `slice_seperation`)."""
    results_device = data.device if do_on_device else torch.device("cpu")
    if do_on_device and not data.is_cuda and torch.cuda.is_available():
        results_device = torch.device("cuda")
    data = data.to(results_device)
    predicted_logits = torch.zeros((2, data.shape[1] * slice_seperation, data.shape[2], data.shape[3]),
                                   dtype=torch.half, device=results_device)
    n_predictions = torch.zeros((data.shape[1] * slice_seperation, data.shape[2], data.shape[3]), dtype=torch.half,
                                device=results_device)
    gaussian = compute_gaussian(tuple(patch_size), sigma_scale=1. / 8, value_scaling_factor=10,
                                device=str(results_device)) if use_gaussian else 1
    for i, sl in enumerate(slicers):
        workon = data[sl][None].to(results_device)
        prediction = _internal_maybe_mirror_and_predict(network, workon, out_idx, deep_supervision, i == len(slicers) - 1)
        prediction = prediction[0].to(results_device)
        msl = tuple([slice(None)] + [slice(sl[k].start * slice_seperation, sl[k].stop * slice_seperation) if k == 1
                                     else slice(sl[k].start, sl[k].stop) for k in range(1, len(sl))])
        predicted_logits[msl] += prediction * gaussian
        n_predictions[msl[1:]] += gaussian
    predicted_logits /= n_predictions
    if torch.any(torch.isinf(predicted_logits)):
        raise RuntimeError("Encountered inf in predicted array. Aborting... If this problem persists, reduce "
                           "value_scaling_factor in compute_gaussian or increase the dtype of predicted_logits to fp32")
    if use_gaussian:
        compute_gaussian.cache_clear()
    return predicted_logits


# ----------------------------------------------------------------------------- stage-2 validation
# (ref utils/seg_utils.py:45-72 read_image, :158-174 preprocess_image, :730-784 calculate_dice / evaluate_case)
def calculate_dice(prediction, ground_truth, smooth=1e-5):
    """ref :730-734."""
    prediction = prediction.flatten()
    ground_truth = ground_truth.flatten()
    intersection = np.sum(prediction * ground_truth)
    return (2. * intersection + smooth) / (np.sum(prediction) + np.sum(ground_truth) + smooth)


def _dice_from_counts(intersection, sum_pred, sum_gt, smooth=1e-5):
    """calculate_dice of two uint8 maps from their exact integer sums (numpy's uint64 accumulators)."""
    intersection, sum_pred, sum_gt = np.uint64(intersection), np.uint64(sum_pred), np.uint64(sum_gt)
    return (2. * intersection + smooth) / (sum_pred + sum_gt + smooth)


def _sitk():
    try:
        import SimpleITK as sitk
    except ImportError as e:
        raise ImportError("reading or writing image files needs SimpleITK, which is not installed; pass the volume as "
                          "an array or tensor of shape (1, D, H, W) instead") from e
    return sitk


def read_image(image_fname):
    """ref :45-72: (float32 (1, D, H, W) array, {'sitk_stuff': ..., 'spacing': (z, y, x)})."""
    sitk = _sitk()
    itk_image = sitk.ReadImage(image_fname)
    spacing, origin, direction = itk_image.GetSpacing(), itk_image.GetOrigin(), itk_image.GetDirection()
    npy_image = sitk.GetArrayFromImage(itk_image)
    if npy_image.ndim != 3:
        raise RuntimeError(f"Unexpected number of dimensions: {npy_image.ndim} in file {image_fname}")
    props = {"sitk_stuff": {"spacing": spacing, "origin": origin, "direction": direction},
             "spacing": list(np.abs(list(spacing)[::-1]))}
    return npy_image[None].astype(np.float32), props


def preprocess_image(image_file, apply_norm=True):
    """ref :158-174: a file name (SimpleITK) or an array / tensor of shape (1, D, H, W) -> (float32 CPU tensor
    (1, D, H, W), properties).  The z-score runs on the host in numpy, as the reference's."""
    if isinstance(image_file, (np.ndarray, torch.Tensor)):
        data = image_file.detach().cpu().numpy() if isinstance(image_file, torch.Tensor) else image_file
        if data.ndim != 4 or data.shape[0] != 1:
            raise ValueError(f"expected a (1, D, H, W) volume, got {tuple(data.shape)}")
        data, properties = np.asarray(data).astype(np.float32), {}
    else:
        data, properties = read_image(image_file)
    data = np.copy(data)
    if apply_norm:
        data = zscore_normalization(data)
    return torch.from_numpy(data).contiguous().float(), properties


def _pad_geometry(shape, new_shape):
    """acvl_utils pad_nd_image's geometry: (padded shape, pad below, pad above) of `shape` grown to at least
    `new_shape` (leading axes not named keep their size)."""
    shape = [int(s) for s in shape]
    new_shape = list(shape[:len(shape) - len(new_shape)]) + [int(s) for s in new_shape]
    padded = [max(n, o) for n, o in zip(new_shape, shape)]
    below = [(p - o) // 2 for p, o in zip(padded, shape)]
    above = [p - o - b for p, o, b in zip(padded, shape, below)]
    return padded, below, above


def pad_nd_image(image, new_shape=None, mode="constant", kwargs=None, return_slicer=False,
                 shape_must_be_divisible_by=None):
    """acvl_utils pad_nd_image, restated (absent offline -> parity unpinned) for what REHRSeg passes: pad to at least
    `new_shape` with pad_below = diff // 2, pad_above = diff - pad_below; with return_slicer, also the slicer that
    reverts the padding."""
    if new_shape is None or shape_must_be_divisible_by is not None:
        raise NotImplementedError("pad_nd_image: REHRSeg passes a new_shape and no divisibility constraint")
    padded, below, above = _pad_geometry(image.shape, new_shape)
    pad_list = list(zip(below, above))
    if any(below) or any(above):
        if isinstance(image, np.ndarray):
            res = np.pad(image, pad_list, mode, **(kwargs or {}))
        else:
            res = F.pad(image, [v for p in pad_list[::-1] for v in p], mode, **(kwargs or {}))
    else:
        res = image
    if not return_slicer:
        return res
    return res, tuple(slice(b, p - a) for b, a, p in zip(below, above, padded))


def _integral_separation(slice_separation):
    sep = float(slice_separation)
    if not sep.is_integer() or sep < 1:
        raise ValueError(f"slice_separation must be a positive integer, got {slice_separation!r}")
    return int(sep)


@functools.lru_cache(maxsize=4)
def _device_gaussian(tile, device):
    """compute_gaussian's fp16 importance map (the predictor's arguments) built on the host and uploaded without a
    host sync; kept for the next case."""
    g = compute_gaussian(tuple(tile), sigma_scale=1. / 8, value_scaling_factor=10, device="cpu")
    return _upload(g, torch.device(device))


def _upload(t, dev):
    if dev.type != "cuda":
        return t.to(dev)
    return t.pin_memory().to(dev, non_blocking=True)


def _to_host(t):
    if not t.is_cuda:
        return t
    out = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    out.copy_(t, non_blocking=True)
    return out


def _fused_tiles(vol, pad, slicers, network, out_idx, deep_supervision, sep, gaussian):
    """The tile loop of the tiled predictor on the device: per tile one gather of the 8-variant batch, one forward,
    one blend into the fp16 accumulators.  Returns (logits, counts) before the normalisation; no host sync."""
    from .. import ops
    be = ops.get_backend()
    D, H, W = (int(n) for n in _slicers_extent(slicers))
    logits = torch.zeros((2, D * sep, H, W), dtype=torch.half, device=vol.device)
    counts = torch.zeros((D * sep, H, W), dtype=torch.half, device=vol.device)
    batch = None
    for sl in slicers:
        start = [s.start for s in sl[1:]]
        tile = [s.stop - s.start for s in sl[1:]]
        reuse = batch is not None and tuple(batch.shape[2:]) == tuple(tile)   # stream order keeps this safe
        batch = be.tta_gather(vol, pad, start, tile, out=batch if reuse else None)
        pred = network(batch)
        if out_idx is not None:
            pred = pred[out_idx]
            if out_idx == 0 and deep_supervision:
                pred = pred[0]
        if pred.shape[1] != 2:
            raise NotImplementedError("the fused predictor accumulates 2 classes, as the reference's predictor does")
        if tuple(pred.shape[2:]) != (tile[0] * sep, tile[1], tile[2]):
            raise ValueError(f"network output {tuple(pred.shape)} does not cover the tile {tile} x {sep} in depth")
        if pred.dtype != torch.float32:  # bf16 under ops.mixed_precision(): blended in fp32
            pred = pred.float()
        be.tta_blend(pred, logits, counts, (start[0] * sep, start[1], start[2]), gaussian)
    return logits, counts


def _slicers_extent(slicers):
    """The spatial extent (D, H, W) the sliding-window slicers cover (the padded volume)."""
    return [max(sl[k].stop for sl in slicers) for k in range(1, 4)]


def _check_inf(flag):
    if flag:
        raise RuntimeError("Encountered inf in predicted array. Aborting... If this problem persists, reduce "
                           "value_scaling_factor in compute_gaussian or increase the dtype of predicted_logits to fp32")


def _fused_predict_sliding_window_return_logits(data, slicers, network, out_idx=None, slice_seperation=1,
                                                patch_size=[14, 320, 384], use_gaussian=False, deep_supervision=True,
                                                pad=(0, 0, 0)):
    """_internal_predict_sliding_window_return_logits with the per-tile and the final work in HIP kernels: the same
    normalised fp16 logits, bit for bit.  `data` (1, D, H, W) on the device is the volume before the constant padding
    of `pad` voxels below (the slicers address the padded volume); the padded copy is never built."""
    from .. import ops
    vol = data[0].to(torch.float32).contiguous()
    gaussian = _device_gaussian(tuple(int(p) for p in patch_size), str(vol.device)) if use_gaussian else None
    logits, counts = _fused_tiles(vol, pad, slicers, network, out_idx, deep_supervision, int(slice_seperation),
                                  gaussian)
    stats = torch.zeros(4, dtype=torch.int64, device=vol.device)
    ops.get_backend().seg_eval_finalize(logits, counts, stats)
    _check_inf(int(stats[0]))
    return logits


def _model_device(model):
    for t in list(model.parameters()) + list(model.buffers()):
        return t.device
    return torch.device("cuda", torch.cuda.current_device())


# ----------------------------------------------------------------------------- boundary metrics
def _spacing_f32(spacing):
    """(sd, sh, sw) in the array's axis order, rounded once to fp32: the values the kernels use, as Python floats."""
    sp = np.asarray(spacing, dtype=np.float64).reshape(-1)
    if sp.shape != (3,):
        raise ValueError(f"spacing must have 3 entries (sd, sh, sw), got {spacing!r}")
    sp = sp.astype(np.float32)
    if not (np.isfinite(sp).all() and (sp > 0).all()):
        raise ValueError(f"spacing must be finite and positive, got {spacing!r}")
    return tuple(float(v) for v in sp)


def _surface_launch(be, pred, gt, spacing, out):
    """The surface kernels on two uint8 maps on the device; out (int64 [5], zeroed) receives the bits of the fp64
    hd, hd95, assd and the two surface sizes.  No host sync; the sort between the two calls is torch's."""
    counts = out[3:5]
    dist, workspace = be.seg_surface_distances(pred, gt, spacing, counts)
    be.seg_surface_reduce(dist, torch.sort(dist.view(-1)).values, counts, out[0:3], workspace)


def _surface_result(vals):
    """The host form of _surface_launch's five int64."""
    vals = np.ascontiguousarray(np.asarray(vals, dtype=np.int64))
    hd, hd95, assd = (float(v) for v in vals[:3].view(np.float64))
    return {"hd": hd, "hd95": hd95, "assd": assd, "n_pred": int(vals[3]), "n_gt": int(vals[4])}


def _map_shape(a):
    shape = tuple(int(n) for n in a.shape)
    if len(shape) == 4 and shape[0] == 1:
        shape = shape[1:]
    if len(shape) != 3:
        raise ValueError(f"expected a (D, H, W) or (1, D, H, W) label map, got {tuple(a.shape)}")
    return shape


def _binary_u8(a, dev):
    """A (D, H, W) or (1, D, H, W) array or tensor of any dtype -> its non-zero mask as uint8 (D, H, W) on dev."""
    if isinstance(a, torch.Tensor):
        t = a.detach()
        if t.device != dev:
            t = t.to(dev) if t.is_cuda else _upload(t.contiguous(), dev)
        t = (t != 0).to(torch.uint8)
    else:
        t = _upload(torch.from_numpy((np.asarray(a) != 0).astype(np.uint8)), dev)
    return t.reshape(_map_shape(a)).contiguous()


def surface_distance_metrics(prediction, ground_truth, spacing=(1., 1., 1.), *, device=None):
    """Boundary metrics of two label maps in the units of `spacing`: {'hd', 'hd95', 'assd'} as floats and
    {'n_pred', 'n_gt'}, the sizes of the two surfaces, as ints.

    `prediction` / `ground_truth`: (D, H, W) or (1, D, H, W) numpy arrays or tensors of any integer, bool or float
    dtype, on the host or on the device; non-zero is foreground.  `spacing` = (sd, sh, sw) in the array's axis order
    (read_image's properties['spacing'] has it), converted to fp32 once.  A surface voxel is a foreground voxel with a
    background face neighbour (outside the volume is background); hd is the largest distance of a surface voxel of one
    map to the surface of the other, hd95 numpy.percentile(., 95) of all those distances, assd the mean of the two
    directed means.  All three are NaN when either map has no foreground (the counts say which).  Everything runs on
    the device (csrc/seg_surface.hip); the call makes one host sync, the read of the five numbers.  Raises
    RehrsegHipError for an axis above 2048 or more than 2**30 voxels.  `device` defaults to a device tensor's, else
    the current device."""
    from .. import ops
    from ..hip_backend import seg_surface_check_extent
    be = ops.get_backend()
    sp = _spacing_f32(spacing)
    shape = _map_shape(prediction)
    if _map_shape(ground_truth) != shape:
        raise ValueError(f"prediction {shape} and ground truth {_map_shape(ground_truth)} differ in shape")
    seg_surface_check_extent(shape)     # before any upload or launch
    if device is not None:
        dev = torch.device(device)
    else:
        on_dev = [a.device for a in (prediction, ground_truth) if isinstance(a, torch.Tensor) and a.is_cuda]
        dev = on_dev[0] if on_dev else torch.device("cuda", torch.cuda.current_device())
    pred, gt = _binary_u8(prediction, dev), _binary_u8(ground_truth, dev)
    out = torch.zeros(5, dtype=torch.int64, device=dev)
    _surface_launch(be, pred, gt, sp, out)
    return _surface_result(out.cpu().numpy())   # the one host sync


# ----------------------------------------------------------------------------- components
def _map_device(device, *maps):
    if device is not None:
        return torch.device(device)
    on_dev = [a.device for a in maps if isinstance(a, torch.Tensor) and a.is_cuda]
    return on_dev[0] if on_dev else torch.device("cuda", torch.cuda.current_device())


def _lesion_launch(be, pred, gt, connectivity, out):
    """The component kernels on two uint8 maps on the device; out (int64 [8], zeroed) receives the eight integers of
    rehr_seg_cc_lesion_i64.  No host sync; one workspace serves the three calls."""
    roots_pred, workspace = be.seg_cc_roots(pred, connectivity)
    roots_gt, _ = be.seg_cc_roots(gt, connectivity, workspace)
    be.seg_cc_lesion(roots_pred, roots_gt, out, workspace)


def _ratio(num, den):
    return num / den if den else float("nan")


def _lesion_result(vals):
    """The host form of _lesion_launch's eight int64."""
    n_pred, n_gt, tp_pred, tp_gt, largest_pred, largest_gt, inter, sum_gt = (int(v) for v in vals)
    precision, recall = _ratio(tp_pred, n_pred), _ratio(tp_gt, n_gt)
    if np.isnan(precision) or np.isnan(recall):
        f1 = float("nan")
    else:
        f1 = 2 * precision * recall / (precision + recall) if precision + recall else 0.0
    terms = (inter, largest_pred, sum_gt)
    return {"n_pred": n_pred, "n_gt": n_gt, "tp_pred": tp_pred, "tp_gt": tp_gt, "fp": n_pred - tp_pred,
            "fn": n_gt - tp_gt, "largest_pred": largest_pred, "largest_gt": largest_gt, "precision": precision,
            "recall": recall, "f1": f1, "dice_largest": float(_dice_from_counts(*terms)), "dice_largest_terms": terms}


def connected_components(mask, connectivity=26, *, device=None):
    """(labels, n): the connected components of a mask, int32 labels (D, H, W) on the device and their number.

    `mask`: a (D, H, W) or (1, D, H, W) numpy array or tensor of any dtype, host or device; non-zero is foreground.
    `connectivity` 6, 18 or 26: scipy.ndimage.generate_binary_structure(3, 1 | 2 | 3); outside the volume is
    background.  Component k (1..n) is the one whose first voxel in raster order is the k-th such voxel; background is
    0.  Everything runs on the device (csrc/seg_components.hip); reading n is the call's one host sync.  Raises
    RehrsegHipError for more than 2**30 voxels or another connectivity."""
    from .. import ops
    from ..hip_backend import seg_cc_check_extent
    be = ops.get_backend()
    seg_cc_check_extent(_map_shape(mask))     # before any upload or launch
    dev = _map_device(device, mask)
    roots, _ = be.seg_cc_roots(_binary_u8(mask, dev), connectivity)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    labels = be.seg_cc_compact(roots, count)
    return labels, int(count.cpu().numpy()[0])   # the one host sync


def keep_largest_component(mask, connectivity=26, *, device=None):
    """The mask reduced to its largest component: a uint8 device tensor of the mask's shape, 1 on that component and
    0 elsewhere; among components of equal size the one whose first voxel comes first in raster order; all zero for an
    empty mask.  Arguments as connected_components'.  No host sync."""
    from .. import ops
    from ..hip_backend import seg_cc_check_extent
    be = ops.get_backend()
    seg_cc_check_extent(_map_shape(mask))
    dev = _map_device(device, mask)
    roots, workspace = be.seg_cc_roots(_binary_u8(mask, dev), connectivity)
    out = torch.zeros(8, dtype=torch.int64, device=dev)
    key = be.seg_cc_lesion(roots, roots, out, workspace)[0]     # (size << 32) | (0xffffffff - root); 0 if empty
    root = torch.where(key != 0, 0xffffffff - (key & 0xffffffff), -2)
    return (roots == root).to(torch.uint8).reshape(tuple(mask.shape))


def lesion_metrics(prediction, ground_truth, connectivity=26, *, device=None):
    """Lesion-wise detection scores of two label maps: a dict of the ints `n_pred`, `n_gt` (the
    numbers of components), `tp_pred` (predicted components holding a foreground voxel of the ground truth), `tp_gt`
    (the reverse), `fp` = n_pred - tp_pred, `fn` = n_gt - tp_gt, `largest_pred`, `largest_gt` (voxels of the largest
    component); the floats `precision` = tp_pred / n_pred, `recall` = tp_gt / n_gt (NaN for a zero denominator), `f1`
    (NaN if either is NaN, 0.0 if both are 0); `dice_largest`, the Dice the case would have if only the largest
    predicted component were kept, and its integer terms `dice_largest_terms` (intersection, prediction, label).

    Arguments as connected_components'; both maps have one shape.  One host sync, the read of the eight integers."""
    from .. import ops
    from ..hip_backend import seg_cc_check_extent
    be = ops.get_backend()
    shape = _map_shape(prediction)
    if _map_shape(ground_truth) != shape:
        raise ValueError(f"prediction {shape} and ground truth {_map_shape(ground_truth)} differ in shape")
    seg_cc_check_extent(shape)
    dev = _map_device(device, prediction, ground_truth)
    out = torch.zeros(8, dtype=torch.int64, device=dev)
    _lesion_launch(be, _binary_u8(prediction, dev), _binary_u8(ground_truth, dev), connectivity, out)
    return _lesion_result(out.cpu().numpy())   # the one host sync


def _evaluate_case(model, case_img, case_label, slice_separation, patch_size, get_HR_results=False, device=None,
                   surface=False, spacing=None, components=False, connectivity=26, norm="zscore"):
    """evaluate_case, plus the exact Dice terms (intersection, sum of the prediction, sum of the label) and, with
    `surface`, the boundary metrics of the LR maps as a sixth element; with `components`, lesion_metrics' dict of the
    LR maps as the last element."""
    from .. import ops
    be = ops.get_backend()
    spec = _norm_spec(norm, also=("zscore", None))
    model.eval()
    sep = _integral_separation(slice_separation)
    dev = torch.device(device) if device is not None else _model_device(model)
    lr_data, properties = preprocess_image(case_img, apply_norm=spec == "zscore")
    lr_label, _ = preprocess_image(case_label, apply_norm=False)
    if surface:
        sp = _spacing_f32(spacing if spacing is not None else properties.get("spacing", (1., 1., 1.)))
    patch = [int(p) for p in patch_size]
    padded, pad, _ = _pad_geometry(lr_data.shape[1:], patch)
    revert = tuple(slice(b, b + n) for b, n in zip(pad, lr_data.shape[1:]))
    vol = _upload(lr_data[0], dev)
    if isinstance(spec, tuple):     # the raw volume, normalised on the device in front of the tiles: no host sync
        vol = _normalize_on_device(vol, spec)
    gt = _upload(torch.from_numpy(lr_label.squeeze(0).numpy().astype("uint8")), dev)
    slicers = _internal_get_sliding_window_slicers(padded, patch_size=patch)
    # with `surface`, the five numbers of the boundary metrics ride behind the eight stats in the same tensor
    # and with `components` the eight lesion integers behind those
    n_surf = 5 if surface else 0
    buf = torch.zeros(8 + n_surf + (8 if components else 0), dtype=torch.int64, device=dev)
    stats = buf[:8].view(2, 4)
    with torch.no_grad():
        logits, counts = _fused_tiles(vol, pad, slicers, model, 0, False, 1, _device_gaussian(tuple(patch), str(dev)))
        labels_lr = torch.empty(tuple(gt.shape), dtype=torch.uint8, device=dev)
        be.seg_eval_finalize(logits, counts, stats[0], revert, labels_lr, gt)
        del logits, counts
        lr_host = _to_host(labels_lr)
        if surface:
            _surface_launch(be, labels_lr, gt, sp, buf[8:13])
        if components:
            _lesion_launch(be, labels_lr, gt, connectivity, buf[8 + n_surf:])
        if get_HR_results:
            # the reference's HR branch: no Gaussian, no softmax, and the padding is not reverted
            logits, counts = _fused_tiles(vol, pad, slicers, model, 1, True, sep, None)
            labels_hr = torch.empty(tuple(counts.shape), dtype=torch.uint8, device=dev)
            be.seg_eval_finalize(logits, counts, stats[1], None, labels_hr)
            del logits, counts
            hr_host = _to_host(labels_hr)
    host = buf.cpu().numpy()  # the one host sync of the case: after it the label maps are on the host as well
    st = host[:8].reshape(2, 4)
    _check_inf(st[0, 0] or st[1, 0])
    prediction_lr = lr_host.numpy()
    prediction_hr = hr_host.numpy() if get_HR_results else prediction_lr
    terms = tuple(int(v) for v in st[0, 1:])
    out = (prediction_lr, prediction_hr, lr_label, _dice_from_counts(*terms), terms)
    if surface:
        out += (_surface_result(host[8:13]),)
    if components:
        out += (_lesion_result(host[8 + n_surf:]),)
    return out


def evaluate_case(model, case_img, case_label, slice_separation, patch_size, get_HR_results=False, *, device=None,
                  surface=False, spacing=None, components=False, connectivity=26, norm="zscore"):
    """ref :736-784 on the device: (prediction_lr uint8 (D, H, W), prediction_hr, lr_label float (1, D, H, W) CPU
    tensor, dice_lr float64).

    `case_img` / `case_label` are file names (SimpleITK) or (1, D, H, W) arrays / tensors.  The z-score runs on the host
    as the reference's; then every tile is one gather of the 8 mirrorings, one forward of that batch and one blend into
    the fp16 accumulators, and one finalize normalises, checks for inf, takes the argmax inside the un-padding crop and
    counts the Dice terms.  The case makes one host sync, which reads the inf flag and the counts.

    Deviations: the network runs in the caller's mode (fp32, or bf16 inside ops.mixed_precision()); the reference's
    torch.autocast fp16 region has no effect on the HIP kernels and is not opened.  The argmax is taken on the fp16
    logits instead of their fp32 softmax: the same class except for two logits within one fp16 ulp of each other,
    where exp rounding can make the softmax tie.  `slice_separation` must be integral (ValueError otherwise).
    `device` defaults to the model's.

    With `surface=True` a fifth element follows: surface_distance_metrics' dict for the LR prediction against the LR
    label, in the units of `spacing` = (sd, sh, sw), else of the image file's properties['spacing'], else (1, 1, 1).
    The surface kernels run on the two maps while they are on the device and their results travel with the same
    read: still one host sync.  With `surface=False` nothing changes.

    With `components=True` the last element is lesion_metrics' dict for the LR prediction against the LR label at
    `connectivity` (after the surface dict if both are asked for); its eight integers travel with the same read as
    well.  With `components=False` nothing changes.

    `norm`: "zscore" (default) is the host z-score above; None feeds the volume as it is; "percentile",
    ("percentile", p_min, p_max) and "zeroone" upload the raw volume and normalise it on the device in front of the
    tiles (percentile_normalization / zeroone_normalization's kernels): still one host sync.
    Anything else raises ValueError."""
    out = _evaluate_case(model, case_img, case_label, slice_separation, patch_size, get_HR_results, device, surface,
                         spacing, components, connectivity, norm)
    return out[:4] + out[5:]


# ----------------------------------------------------------------------------- class locations
def _label_u8(a, dev):
    """A label volume as a contiguous uint8 tensor on dev: a host array is uploaded, a tensor on dev stays there."""
    if isinstance(a, torch.Tensor):
        t = a.detach()
        if t.device != dev:
            t = t.to(dev) if t.is_cuda else _upload(t.contiguous(), dev)
        return t.to(torch.uint8).contiguous()
    return _upload(torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.uint8, copy=False))), dev)


def sample_class_locations(label, classes=(1,), n=10000, seed=0, *, device=None):
    """Voxel locations of classes of a label volume, the table a foreground-oversampling patch feed draws its crop
    centres from: {class: int64 numpy array (m, 3)} of coordinates into `label`'s own shape, m = n for a class that
    occurs and 0 for one that does not.

    `label`: a 3-D numpy array (uploaded) or tensor (one on the device stays there; other dtypes are cast to uint8).
    `classes`: label values 0..255, or -1 for "any non-zero label".  Row j of a class's table is the voxel of rank
    (u[j] * count) >> 32 among the class's `count` voxels in linear (C) order, with
    u = np.random.default_rng(seed).integers(0, 2**32, n, dtype=np.uint32), the same stream for every class; count and
    the ranks are formed on the device (csrc/class_locations.hip), so all classes are queued before the one download
    that is the call's only host sync.  The same label, classes, n and seed give the same table on every run.

    A list (or tuple) of volumes gives a list of such dicts, volume i drawn with seed + i, still with one host sync:
    the outputs of all volumes and classes lie in one device buffer.

    Deviation from nnU-Net: its class_locations hold up to 10 000 voxels per class drawn WITHOUT replacement; this
    table is n draws WITH replacement, uniform over the class's voxels.  A patch centre drawn uniformly from either
    table is uniform over the class's voxels, and the with-replacement form needs no count on the host before the
    ranks are formed."""
    from .. import ops
    from ..hip_backend import CLASS_LOCATIONS_MAX_RANKS, CLASS_LOCATIONS_MAX_VOXELS
    be = ops.get_backend()
    many = isinstance(label, (list, tuple))
    volumes = list(label) if many else [label]
    classes = [int(c) for c in classes]
    n = int(n)
    if not 1 <= n <= CLASS_LOCATIONS_MAX_RANKS:
        raise ValueError(f"n must lie in [1, 2**20], got {n}")
    if not classes or len(set(classes)) != len(classes) or not all(-1 <= c <= 255 for c in classes):
        raise ValueError(f"classes: distinct label values in [0, 255], or -1 for any non-zero label; got {classes}")
    shapes = [tuple(int(s) for s in v.shape) for v in volumes]
    for s in shapes:
        if len(s) != 3 or not 1 <= int(np.prod(s, dtype=np.int64)) <= CLASS_LOCATIONS_MAX_VOXELS:
            raise ValueError(f"expected 3-D label volumes of 1 to 2**31 - 1 voxels, got {s}")
    if not volumes:
        return []
    dev = _map_device(device, *volumes)
    nv, nc = len(volumes), len(classes)
    u = np.stack([np.random.default_rng(int(seed) + i).integers(0, 2**32, n, dtype=np.uint32) for i in range(nv)])
    u = _upload(torch.from_numpy(u.view(np.int32)), dev)       # uint32 bits in int32 storage (hip_backend.class_locations)
    # one buffer for everything that is read back: nv * nc counts (int64, as int32 pairs), then as many rows of n indices
    out = torch.empty(nv * nc * (2 + n), dtype=torch.int32, device=dev)
    counts = out[:2 * nv * nc].view(torch.int64)
    index = out[2 * nv * nc:].view(nv * nc, n)
    for i, v in enumerate(volumes):
        lab = _label_u8(v, dev)
        workspace = be.class_locations_workspace(lab.numel(), lab.device)     # one for the volume's classes
        for k, c in enumerate(classes):
            r = i * nc + k
            be.class_locations(lab, c, u[i], counts[r:r + 1], index[r], workspace)
    host = out.cpu().numpy()                                    # the one host sync
    h_counts = host[:2 * nv * nc].view(np.int64)
    h_index = host[2 * nv * nc:].reshape(nv * nc, n)
    tables = []
    for i, s in enumerate(shapes):
        t = {}
        for k, c in enumerate(classes):
            r = i * nc + k
            if h_counts[r] == 0:
                t[c] = np.zeros((0, 3), np.int64)
            else:
                t[c] = np.stack(np.unravel_index(h_index[r].astype(np.int64), s), axis=1).astype(np.int64)
        tables.append(t)
    return tables if many else tables[0]
