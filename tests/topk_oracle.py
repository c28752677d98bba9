"""The contract of the top-k cross-entropy + soft Dice loss in fp64 torch on the CPU (test only).

    m       the loss map RobustCrossEntropyLoss forms before its mean: ce (N,D,H,W), or with a (N,1,D,H,W) uncertainty
            the broadcast product m[j,i] = ce[i] * unc[j] of shape (N,N,D,H,W)
    K       int(m.numel() * k / 100)
    t       the K-th largest value of m, n_gt = #(m > t), n_eq = #(m == t)  (-0.0 == +0.0: values, not bit patterns)
    weight  1 above t, (K - n_gt) / n_eq on t, 0 below
    value   (sum_{m > t} m + (K - n_gt) t) / K  == m.view(-1).topk(K)[0].mean() for any tie-break
    d/dm    weight / K

The full loss is weight_ce * value + weight_dice * SoftDiceLoss (restated here as well: -mean over (n, c >= !do_bg) of
(2 I + smooth) / clip(G + P + smooth, 1e-8))."""
import torch
import torch.nn.functional as F


def loss_map(logits, target, unc=None):
    """logits (N,C,D,H,W), target (N,1,D,H,W) class ids, unc None or (N,1,D,H,W) -> fp64 (N,D,H,W) or (N,N,D,H,W)."""
    ce = F.cross_entropy(logits.double(), target[:, 0].long(), reduction="none")
    return ce if unc is None else ce * unc.double()


def topk_count(M, k):
    if not 0 < k <= 100:
        raise ValueError(f"k = {k} outside (0, 100]")
    K = int(M * k / 100)
    if K < 1:
        raise ValueError(f"K = {K} < 1")
    return K


def select(m, K):
    """(t, n_gt, n_eq) of the map: t a Python float, the counts Python ints."""
    flat = m.detach().reshape(-1)
    t = torch.sort(flat).values[flat.numel() - K]
    return float(t), int((flat > t).sum()), int((flat == t).sum())


def tie_weights(m, K):
    """The weight of every element of m, in m's shape (detached)."""
    t, n_gt, n_eq = select(m, K)
    md = m.detach()
    w = torch.zeros_like(md)
    w[md > t] = 1.0
    w[md == t] = (K - n_gt) / n_eq
    return w


def topk_value(m, K):
    t, n_gt, _ = select(m, K)
    flat = m.reshape(-1)
    rest = K - n_gt
    return (flat[flat.detach() > t].sum() + (rest * t if rest > 0 else 0.0)) / K


def soft_dice(logits, target, smooth=1e-5, do_bg=False):
    p = torch.softmax(logits.double(), 1)
    y = torch.zeros_like(p).scatter_(1, target.long(), 1.0)
    axes = (2, 3, 4)
    inter, sp, sg = (p * y).sum(axes), p.sum(axes), y.sum(axes)
    dc = (2 * inter + smooth) / torch.clip(sg + sp + smooth, 1e-8)
    if not do_bg:
        dc = dc[:, 1:]
    return -dc.mean()


def dc_and_topk(logits, target, unc=None, k=10, weight_ce=1.0, weight_dice=1.0, smooth=1e-5, do_bg=False):
    """-> dict: value (fp64 scalar tensor), grad (d value / d logits, fp64), m, K, t, n_gt, n_eq, weights."""
    x = logits.detach().double().requires_grad_(True)
    m = loss_map(x, target, unc)
    K = topk_count(m.numel(), k)
    t, n_gt, n_eq = select(m, K)
    w = tie_weights(m, K)
    value = weight_ce * topk_value(m, K) + weight_dice * soft_dice(x, target, smooth, do_bg)
    # the gradient rule: d value / d m = weight / K (a subgradient where elements tie)
    surrogate = weight_ce * (w * m).sum() / K + weight_dice * soft_dice(x, target, smooth, do_bg)
    surrogate.backward()
    return dict(value=value.detach(), grad=x.grad, m=m.detach(), K=K, t=t, n_gt=n_gt, n_eq=n_eq, weights=w)


def ambiguous(m, K, rel=1e-5):
    """Boolean mask over m: elements whose value lies within rel * max(|t|, 1e-6) of t.  A device that selects on an
    fp32 map may put them on either side."""
    t, _, _ = select(m, K)
    return (m.detach() - t).abs() <= rel * max(abs(t), 1e-6)


def tie_case():
    """Logits 40 / 0 on a (1, 2, 1, 4, 8) patch, 5 voxels labelled against the logits, k = 50: K = 16, t = 0, n_gt = 5,
    n_eq = 27 (the right voxels' fp64 CE is -0.0), value 12.5 + Dice, every tied voxel weight 11 / 27."""
    logits = torch.zeros(1, 2, 1, 4, 8)
    logits[:, 0] = 40.0
    target = torch.zeros(1, 1, 1, 4, 8)
    target.view(-1)[[1, 6, 13, 20, 31]] = 1.0
    return logits, target
