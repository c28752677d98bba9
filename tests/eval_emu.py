"""CPU emulation of the stage-2 validation kernels of csrc/seg_eval.hip (test only): the contract of
rehr_tta_gather_f32, rehr_tta_blend_f16acc and rehr_seg_eval_finalize_f16 in torch on the CPU, with the same
operations and roundings (fp32 arithmetic, one fp16 rounding per store).  Install it with ops.set_backend()."""
import itertools

import torch

name = "eval_emu"
COMBOS = [c for i in range(3) for c in itertools.combinations([1, 2, 3], i + 1)]  # axes of a (1, d, h, w) variant


def tta_gather(vol, pad, start, tile, out=None):
    D, H, W = vol.shape
    src = [s - p for s, p in zip(start, pad)]
    t = torch.zeros(tuple(tile), dtype=torch.float32)
    lo = [max(0, -s) for s in src]
    hi = [min(n, s + n_t) - s for s, n, n_t in zip(src, (D, H, W), tile)]
    if all(h > l for l, h in zip(lo, hi)):
        t[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = vol[src[0] + lo[0]:src[0] + hi[0], src[1] + lo[1]:src[1] + hi[1],
                                                       src[2] + lo[2]:src[2] + hi[2]]
    x = t[None]
    res = torch.stack([x] + [torch.flip(x, axes) for axes in COMBOS])
    if out is not None:
        out.copy_(res)
        return out
    return res


def tta_blend(pred, logits, counts, start, gaussian=None):
    p = pred[0].clone()
    for k, axes in enumerate(COMBOS):
        p += torch.flip(pred[k + 1], axes)
    p /= 8
    g = gaussian.float() if gaussian is not None else torch.ones(p.shape[1:])
    sl = tuple(slice(s, s + n) for s, n in zip(start, p.shape[1:]))
    logits[(slice(None),) + sl] = (logits[(slice(None),) + sl].float() + p * g).half()
    counts[sl] = (counts[sl].float() + g).half()


def seg_eval_finalize(logits, counts, stats, crop=None, labels=None, gt=None):
    q = (logits.float() / counts.float()).half()
    logits.copy_(q)
    if bool(torch.isinf(q).any()):
        stats[0] = 1
    if labels is None:
        return
    crop = crop or tuple(slice(None) for _ in counts.shape)
    c = q[(slice(None),) + tuple(crop)].float()
    lab = (c[1] > c[0]).to(torch.uint8)
    labels.copy_(lab)
    if gt is not None:
        g = gt.to(torch.int64)
        stats[1] += int((lab.to(torch.int64) * g).sum())
        stats[2] += int(lab.sum())
        stats[3] += int(g.sum())
