"""Stage-1 structure losses (the reference's models/losses.py names l1_sobel_loss / l2_sobel_loss over kornia; this is
the repository's own text over csrc/sr_losses.hip).

    loss = l1 mean|p - t| + l2 mean (p - t)^2 + ssim (1 - mean SSIM(p, t)) + sobel mean|G(p) - G(t)|

over (N, C, D, H, W) or (N, C, H, W) fp32 device tensors, every (H, W) slice an image.  SSIM is the index
train_steps.validate_sr reports (11x11 Gaussian window, sigma 1.5, valid positions, C1 = (0.01 R)^2, C2 = (0.03 R)^2);
G is kornia's Sobel() default restated from its published behaviour -- sqrt(gx^2 + gy^2 + 1e-6), 3x3 kernels / 8,
replicate padding.  Parity with kornia is unpinned: kornia is not available to the tests.

One fused HIP pass each way; the operands are read through their strides (the channels-last network output's
hat[:, 0:1] is not copied), the value stays on the device and the gradient goes to the first operand only."""
import torch
from torch import nn


class _FusedStructureLoss(torch.autograd.Function):
    """rehr_structure_loss_{fwd,bwd}_f32 through the ops backend."""

    @staticmethod
    def forward(ctx, input, target, weights, data_range):
        from .. import ops
        need = ctx.needs_input_grad[0]
        loss, _, fields = ops.get_backend().structure_loss_fwd(input, target, weights, data_range, need_grad=need)
        if need:
            ctx.save_for_backward(input, target, fields)
            ctx.weights = weights
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        from .. import ops
        input, target, fields = ctx.saved_tensors
        go = grad_out.to(torch.float32).reshape(1).contiguous()
        return ops.get_backend().structure_loss_bwd(input, target, ctx.weights, fields, go), None, None, None


class StructureLoss(nn.Module):
    """forward(input, target) -> 0-dim device tensor; differentiable in `input` only."""

    def __init__(self, l1=1.0, l2=0.0, ssim=0.0, sobel=0.0, data_range=1.0):
        super().__init__()
        self.weights = (float(l1), float(l2), float(ssim), float(sobel))
        self.data_range = float(data_range)

    def forward(self, input, target):
        if target.requires_grad:
            raise ValueError("StructureLoss: the target takes no gradient (detach it)")
        return _FusedStructureLoss.apply(input, target, self.weights, self.data_range)

    def extra_repr(self):
        return "l1={}, l2={}, ssim={}, sobel={}".format(*self.weights) + f", data_range={self.data_range}"


def l1_sobel_loss(y_true, y_pred):
    """L1 + Sobel edge term, in the reference's argument order; the gradient goes to y_pred."""
    return StructureLoss(l1=1.0, sobel=1.0)(y_pred, y_true)


def l2_sobel_loss(y_true, y_pred):
    """L2 + Sobel edge term, in the reference's argument order; the gradient goes to y_pred."""
    return StructureLoss(l1=0.0, l2=1.0, sobel=1.0)(y_pred, y_true)
