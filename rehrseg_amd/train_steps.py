"""The two hot training loops of the reference as per-step functions, plus the teacher
pass, on the MI355X modules.

  get_intermediate_features   train_all.py:85-112   (teacher features for distillation)
  train_sr_step               train_all.py:118-139  (stage 1b/1c: FLAVR self-SR step)
  validate_sr                 (no counterpart)      (stage-1 validation on held-out LR / HR pairs, on the device)
  train_segsr_step            train_all.py:521-556  (stage 2: SegModel + distillation step)
  evaluate / evaluate_cases   train_all.py:154-193  (stage-2 validation, evaluate_case on the device)

Results are those of the reference loops; two things are restructured for the GPU:
  * the teacher's D-1 four-slice windows are ONE batched encoder call instead of D-1
    calls (windows are independent samples: no BatchNorm, per-sample SE pooling), and
  * `levels` lets the caller stop the teacher after the level it consumes (the stage-2
    loop only reads level 1).
"""
import numpy as np
import torch
import torch.nn.functional as F

from .utils.seg_utils import zscore_normalization


def get_intermediate_features(model_sr, img_lr, label_lr, device=None, levels=None, _normalized=None):
    """dict level -> (B, C_level, D, h, w).  Like the reference it z-scores `img_lr` IN PLACE
    (the student is fed the normalised image afterwards, train_all.py:533-534).
    _normalized: the result of zscore_normalization(img_lr) when the caller has already applied it (train_segsr_step
    normalises on the main stream and runs the rest of the teacher pass on a second one)."""
    img_lr = zscore_normalization(img_lr) if _normalized is None else _normalized
    x = torch.cat((img_lr, label_lr), dim=1)                     # (B, 2, D, H, W)
    B, C, D, H, W = x.shape
    if D < 2:
        raise ValueError("need at least two slices")
    padded = F.pad(x, (0, 0, 0, 0, 1, 2))                       # [0, x_0 .. x_{D-1}, 0, 0] along depth
    upto = 4 if levels is None else max(levels)
    enc = getattr(model_sr, "encoder", None)
    truncated = upto < 4 and enc is not None and "upto" in enc.forward.__code__.co_varnames
    if truncated and not torch.is_grad_enabled() and H % 2 == 0 and W % 2 == 0:
        # frozen teacher: the stem's per-slice work is shared between the overlapping windows
        from .models.FLAVR.resnet_3D import encoder_on_windows
        feats = encoder_on_windows(enc, padded[:, :, :D + 2], D - 1, upto)  # (the windows never reach the last slice)
    else:
        # window st = padded[st : st+4], st = 0 .. D-2 (zero slice in front of the first, behind the last)
        win = padded.unfold(2, 4, 1)[:, :, :D - 1]              # (B, 2, D-1, H, W, 4)
        win = win.permute(0, 2, 1, 5, 3, 4).reshape(B * (D - 1), C, 4, H, W).contiguous()
        if truncated:
            mean_ = win[:, 0:1].mean(2, keepdim=True).mean(3, keepdim=True).mean(4, keepdim=True)
            win[:, 0:1] = win[:, 0:1] - mean_                   # UNet_3D_3D.forward's mean subtraction
            feats = enc(win, upto=upto)
        else:
            feats = model_sr(win, return_inetermediate_feature=True)
    out = {}
    for i, f in enumerate(feats):
        if levels is not None and i not in levels:
            continue
        f = f.reshape(B, D - 1, f.shape[1], 4, f.shape[3], f.shape[4])
        mid = f[:, :, :, 1].permute(0, 2, 1, 3, 4)              # slice 1 of every window
        last = f[:, -1, :, 2].unsqueeze(2)                      # slice 2 of the last window
        out[i] = torch.cat([mid, last], dim=2)
    return out


def _zero_grad(opt, grad_sync, zero_grad):
    """`opt.zero_grad()` of the reference loops.  With patch-parallel training (grad_sync =
    PatchParallel.reduce_gradients) the wrapper's own zero_grad is used: it keeps the conv weights' `.grad`
    views into the flat exchange buffer, so their gradients are written in place instead of re-allocated.
    (A plain optimizer.zero_grad() stays correct -- PatchParallel reconciles at the exchange -- just slower.)"""
    if zero_grad is not None:
        return zero_grad()
    owner = getattr(grad_sync, "__self__", None)
    if owner is not None and callable(getattr(owner, "zero_grad", None)) and hasattr(owner, "reduce_gradients"):
        return owner.zero_grad()
    return opt.zero_grad()


def train_sr_step(model, opt, scheduler, patches_lr, patches_hr, loss_obj, loss_seg, slice_separation, num_slices,
                  enable_uncertainty, grad_sync=None, zero_grad=None):
    """One iteration of train_sr's inner loop (train_all.py:118-139); returns the loss tensor.
    grad_sync: called between backward and the optimizer step (PatchParallel.reduce_gradients);
    zero_grad: overrides how gradients are cleared (default: see _zero_grad)."""
    if num_slices > 1:
        s = int(slice_separation)
        patches_hr = patches_hr[:, :, s * (num_slices // 2 - 1):s * (num_slices // 2), ...]
    if enable_uncertainty:
        hat, unc = model(patches_lr)
        loss = loss_obj(hat[:, 0:1], patches_hr[:, 0:1])
        loss = loss + torch.mean(torch.div(torch.abs(hat[:, 0:1] - patches_hr[:, 0:1]), unc) + torch.log(unc))
        loss = loss + loss_obj(unc, torch.abs(hat[:, 0:1].detach() - patches_hr[:, 0:1]))
    else:
        hat = model(patches_lr)
        loss = loss_obj(hat[:, 0:1], patches_hr[:, 0:1])
    loss = loss + loss_seg(hat[:, 1:], patches_hr[:, 1:]) * 1.0
    _zero_grad(opt, grad_sync, zero_grad)
    loss.backward()
    if grad_sync is not None:
        grad_sync()
    opt.step()
    if scheduler is not None:
        scheduler.step()
    return loss


def validate_sr(model, data_set, n_batches, batch_size, slice_separation, num_slices, enable_uncertainty=False,
                data_range=1.0, seed=0):
    """Stage-1 validation (the reference has none): the (patches_lr, patches_hr) pairs TrainSetMultiple builds from
    held-out subjects have known truth, so the network's channel 0 is scored against the HR image (L1, MSE, PSNR, SSIM
    per slice) and its channel 1 against the HR label (Dice), on the device (ops backend sr_metrics).  Returns
    utils.sr_utils.sr_quality's dict over the n_batches * batch_size samples.

    Batch b holds the items (b * batch_size + j) % len(data_set), j = 0 .. batch_size - 1, drawn from Python's `random`
    seeded with `seed`; the generator's state is saved first and restored on exit (also on an exception), so a training
    loop's draws are untouched.  patches_hr is cut to the middle slice_separation slices as train_sr_step does.  The
    model runs in eval() under no_grad in the caller's precision mode (its previous mode is restored) and its output is
    read where it lies, in the dtype it comes in.  The stats stay on the device until the one host read at the end."""
    import random

    from . import ops
    from .utils.sr_utils import sr_quality
    if getattr(data_set, "train_transform", None) is not None:
        raise ValueError("validate_sr: a data set with train_transform set yields augmented patches (and draws from "
                         "other generators); build the validation set without it")
    n_batches, batch_size = int(n_batches), int(batch_size)
    if n_batches < 1 or batch_size < 1 or len(data_set) < 1:
        raise ValueError("validate_sr needs at least one batch of at least one item of a non-empty data set")
    be = ops.get_backend()
    state = random.getstate()
    was_training = model.training
    stats, voxels = [], None
    try:
        random.seed(seed)
        model.eval()
        with torch.no_grad():
            for b in range(n_batches):
                patches_lr, patches_hr = data_set.batch([(b * batch_size + j) % len(data_set)
                                                         for j in range(batch_size)])
                if num_slices > 1:
                    s = int(slice_separation)
                    patches_hr = patches_hr[:, :, s * (num_slices // 2 - 1):s * (num_slices // 2), ...]
                hat = model(patches_lr)
                if enable_uncertainty:
                    hat = hat[0]
                stats.append(be.sr_metrics(hat[:, 0], patches_hr[:, 0], hat[:, 1], patches_hr[:, 1], data_range))
                voxels = hat[0, 0].numel()
    finally:
        model.train(was_training)
        random.setstate(state)
    return sr_quality(torch.cat(stats, 0), voxels, data_range)


_TEACHER_STREAMS = {}


def _teacher_stream(t):
    """One extra HIP stream per device for the teacher pass of train_segsr_step (None for CPU tensors: host-logic tests)."""
    if not t.is_cuda:
        return None
    key = t.device.index
    if key not in _TEACHER_STREAMS:
        _TEACHER_STREAMS[key] = torch.cuda.Stream(device=t.device)
    return _TEACHER_STREAMS[key]


def train_segsr_step(model_seg, model_sr, distiller, opt, img, label_lr, label_hr, uncertainty_lr, loss_lr_seg,
                     loss_hr_seg, enable_uncertainty=True, teacher_levels=(1,), grad_sync=None, zero_grad=None,
                     teacher_stream=True):
    """One iteration of the stage-2 loop (train_all.py:521-556); returns the loss tensor.
    teacher_stream: run the frozen teacher's pass on a second HIP stream next to the student's forward.
    With deep supervision (model_seg.decoder.deep_supervision, a _build_loss(True) loss_lr_seg) label_lr and
    uncertainty_lr are the per-level lists of the data set; the teacher reads level 0."""
    model_seg.train()
    label_levels = list(label_lr) if isinstance(label_lr, (list, tuple)) else [label_lr]
    unc_levels = list(uncertainty_lr) if isinstance(uncertainty_lr, (list, tuple)) else []
    label_full = label_levels[0]
    if distiller is not None:
        side = _teacher_stream(img) if teacher_stream else None
        if side is None:
            with torch.no_grad():
                features_sr = get_intermediate_features(model_sr, img, label_full, img.device, levels=teacher_levels)
            seg_lr, seg_sr, features_seg = model_seg(img, return_inetermediate_feature=True)
        else:
            # The frozen teacher's pass and the student's forward are independent once the image is z-scored (in place,
            # as the reference does: the student reads the normalised image): the teacher runs on a second HIP stream,
            # the student on the current one, joined before the distillation loss.  Same kernels, same results.
            main = torch.cuda.current_stream(img.device)
            with torch.no_grad():
                normalized = zscore_normalization(img)
            side.wait_stream(main)
            with torch.cuda.stream(side), torch.no_grad():
                features_sr = get_intermediate_features(model_sr, img, label_full, img.device, levels=teacher_levels,
                                                        _normalized=normalized)
            seg_lr, seg_sr, features_seg = model_seg(img, return_inetermediate_feature=True)
            main.wait_stream(side)
            for t in features_sr.values():
                t.record_stream(main)          # allocated on the side stream, consumed (and later freed) on the main one
            for t in (img, normalized, *label_levels, *unc_levels):
                t.record_stream(side)
    else:
        seg_lr, seg_sr = model_seg(img)
    if enable_uncertainty:
        loss = loss_lr_seg(seg_lr, label_lr, uncertainty_lr) + loss_hr_seg(seg_sr, label_hr, None)
    else:
        loss = loss_lr_seg(seg_lr, label_lr) + loss_hr_seg(seg_sr, label_hr)
    if distiller is not None:
        loss = loss + distiller(features_seg[1], features_sr[1])
    _zero_grad(opt, grad_sync, zero_grad)
    loss.backward()
    if grad_sync is not None:
        grad_sync()
    opt.step()
    return loss


def _report(dice, terms):
    """train_all.py:188-193's summary; the global Dice from the summed exact per-case terms."""
    from .utils.seg_utils import _dice_from_counts
    tot = [sum(t[k] for t in terms) for k in range(3)]
    print(f"Global dice: {_dice_from_counts(*tot)}")
    print(f"Average dice: {sum(dice) / len(dice)}")
    print(f"Std dice: {np.std(dice)}")
    print(f"Max dice: {max(dice)}")
    print(f"Min dice: {min(dice)}")
    return sum(dice) / len(dice)


def _subject_line(name, dice, surf=None, les=None):
    line = f"Subject {name}: {dice}"
    if surf is not None:
        line += f" | HD95: {surf['hd95']} | ASSD: {surf['assd']}"
    if les is not None:
        line += f" | Lesions: {les['tp_gt']}/{les['n_gt']} found, {les['fp']} false"
    return line


def _report_surface(surf):
    """Mean, std, max and min of HD95 and ASSD over the cases where they are finite, and the number of cases with an
    empty surface (no foreground in the prediction or in the label: NaN)."""
    for key, label in (("hd95", "HD95"), ("assd", "ASSD")):
        vals = [s[key] for s in surf if np.isfinite(s[key])]
        if vals:
            print(f"Average {label}: {sum(vals) / len(vals)}")
            print(f"Std {label}: {np.std(vals)}")
            print(f"Max {label}: {max(vals)}")
            print(f"Min {label}: {min(vals)}")
        else:
            print(f"Average {label}: nan (no case with both surfaces)")
    print(f"Empty-surface cases: {sum(1 for s in surf if s['n_pred'] == 0 or s['n_gt'] == 0)} of {len(surf)}")


def _report_lesions(les, dice):
    """Lesion-wise totals over all cases with the micro-averaged precision, recall and F1, and nnU-Net's
    post-processing decision: whether keeping only the largest predicted component raises the mean Dice."""
    from .utils.seg_utils import _lesion_result
    tot = {k: sum(c[k] for c in les) for k in ("n_pred", "n_gt", "tp_pred", "tp_gt", "fp", "fn")}
    micro = _lesion_result([tot["n_pred"], tot["n_gt"], tot["tp_pred"], tot["tp_gt"], 0, 0, 0, 0])
    print(f"Lesions: {tot['tp_gt']}/{tot['n_gt']} found, {tot['fn']} missed; "
          f"{tot['n_pred']} predicted, {tot['fp']} false")
    print(f"Lesion precision: {micro['precision']}")
    print(f"Lesion recall: {micro['recall']}")
    print(f"Lesion F1: {micro['f1']}")
    mean, largest = sum(dice) / len(dice), sum(c["dice_largest"] for c in les) / len(les)
    print(f"Average dice: {mean} | largest component only: {largest}")
    print(f"Keep largest component: {'yes' if largest > mean else 'no'} "
          f"({'raises' if largest > mean else 'does not raise'} the mean Dice)")


def evaluate_cases(model_seg, cases, patch_size_ori, eval_HR=False, seperation=1, *, device=None, surface=False,
                   spacing=None, components=False, connectivity=26, norm="zscore"):
    """train_all.py:154-193 over in-memory cases: `cases` yields (name, image, label), each a (1, D, H, W) array or
    tensor (or a file name).  Prints the reference's summary and returns the mean Dice.

    The global Dice is calculate_dice over the concatenated LR maps, formed from the summed per-case integer terms, so
    no map is kept.  (The reference concatenates float32 label tensors, so its float32 sums can differ from these
    exact ones in the last bits once the counts pass 2**24.)  `device`: as evaluate_case's.

    With `surface=True` every subject's line gains HD95 and ASSD (evaluate_case's `surface` / `spacing`) and the
    summary their mean, std, max and min over the cases with finite values and the number of cases with an empty
    surface; the return value stays the mean Dice.

    With `components=True` every subject's line gains `| Lesions: <tp_gt>/<n_gt> found, <fp> false` (evaluate_case's
    `components` / `connectivity`) and the summary the totals over all cases, the micro-averaged lesion precision,
    recall and F1, the mean Dice next to the mean Dice of the largest predicted component alone, and a last line
    saying whether keeping only that component raises the mean Dice; the return value stays the mean Dice.

    `norm`: evaluate_case's ("zscore" on the host by default, None, or "percentile" / ("percentile", p_min, p_max) /
    "zeroone" on the device)."""
    from .utils.seg_utils import _evaluate_case
    dice, terms, surf, les = [], [], [], []
    for name, img, label in cases:
        out = _evaluate_case(model_seg, img, label, seperation, patch_size_ori[::-1], eval_HR, device, surface, spacing,
                             components, connectivity, norm)
        print(_subject_line(name, out[3], out[5] if surface else None, out[-1] if components else None))
        dice.append(out[3])
        terms.append(out[4])
        if surface:
            surf.append(out[5])
        if components:
            les.append(out[-1])
    mean = _report(dice, terms)
    if surface:
        _report_surface(surf)
    if components:
        _report_lesions(les, dice)
    return mean


def evaluate(model_seg, patch_size_ori, val_img_path, val_label_path, split_path, fold, save_path=None, eval_HR=False,
             seperation=1, surface=False, components=False, connectivity=26, norm="zscore"):
    """train_all.py:154-193: every validation subject of the split's fold, read with SimpleITK; with `save_path`, the
    predictions are written next to it as NIfTI via SimpleITK as the reference does.  `surface`: as evaluate_cases',
    in the units of each image file's spacing.  `components`, `connectivity`, `norm`: as evaluate_cases'."""
    import json
    import os
    from .utils.seg_utils import _evaluate_case, _sitk
    sitk = _sitk()
    with open(split_path, "r") as f:
        split_data = json.load(f)[fold]["val"]
    dice, terms, surf, les = [], [], [], []
    for subject in split_data:
        test_img = os.path.join(val_img_path, subject + "_0000.nii.gz")
        test_label = os.path.join(val_label_path, subject + ".nii.gz")
        pred_lr, pred_hr, _, dice_lr, t, *s = _evaluate_case(model_seg, test_img, test_label, seperation,
                                                              patch_size_ori[::-1], eval_HR, None, surface, None,
                                                              components, connectivity, norm)
        if surface:
            surf.append(s[0])
        if components:
            les.append(s[-1])
        if save_path is not None:
            os.makedirs(os.path.join(save_path, "val"), exist_ok=True)
            ori = sitk.ReadImage(test_img)
            img = sitk.GetImageFromArray(pred_lr)
            img.SetSpacing(ori.GetSpacing())
            img.SetOrigin(ori.GetOrigin())
            img.SetDirection(ori.GetDirection())
            sitk.WriteImage(img, os.path.join(save_path, "val", f"{subject}_pred_lr.nii.gz"))
            if eval_HR:
                img = sitk.GetImageFromArray(pred_hr)
                sp = ori.GetSpacing()
                img.SetSpacing([sp[0], sp[1], sp[2] / seperation])
                img.SetOrigin(ori.GetOrigin())
                img.SetDirection(ori.GetDirection())
                sitk.WriteImage(img, os.path.join(save_path, "val", f"{subject}_pred_hr.nii.gz"))
        print(_subject_line(subject, dice_lr, s[0] if surface else None, s[-1] if components else None))
        dice.append(dice_lr)
        terms.append(t)
    mean = _report(dice, terms)
    if surface:
        _report_surface(surf)
    if components:
        _report_lesions(les, dice)
    return mean
