"""Seconds per validation case (GPU box): evaluate_case's fused path against the composed one, at the reference's
case size -- a 1 x 20 x 455 x 633 volume, 12 tiles x 8 mirrorings, the cfg-4 anisotropic 6-stage student plan of
bench.py, random init, fp32.  That plan halves the depth twice, so it returns 16 slices for the reference's 14-slice
tile; the tile here is [16, 320, 384], which gives the same 2 x 2 x 3 tiles.

  fused     su.evaluate_case: gather / forward / blend per tile, one finalize, one host sync
  composed  the unchanged torch predictor (_internal_predict_sliding_window_return_logits on the padded volume), then
            the reference's host tail: fp16 logits to the host, crop, fp32 softmax, argmax and calculate_dice in numpy

The network's share is the sum of HIP-event times around the forward calls of the fused path.

    python tools/bench_eval.py [--reps 5]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from rehrseg_amd.models.seg_model import SegModel  # noqa: E402
from rehrseg_amd.utils import seg_utils as su  # noqa: E402


def student(dev):
    torch.manual_seed(0)
    return SegModel(input_channels=1, num_classes=2, n_stages=6, upscale=4,
                    features_per_stage=[32, 64, 128, 256, 320, 320], conv_op=nn.Conv3d,
                    kernel_sizes=[[1, 3, 3], [1, 3, 3], [3, 3, 3], [3, 3, 3], [3, 3, 3], [3, 3, 3]],
                    strides=[[1, 1, 1], [1, 2, 2], [1, 2, 2], [2, 2, 2], [2, 2, 2], [1, 2, 2]],
                    n_conv_per_stage=[2] * 6, n_conv_per_stage_decoder=[2] * 5, conv_bias=True,
                    norm_op=nn.InstanceNorm3d, norm_op_kwargs={"eps": 1e-5, "affine": True}, dropout_op=None,
                    dropout_op_kwargs=None, nonlin=nn.LeakyReLU, nonlin_kwargs={"inplace": True},
                    deep_supervision=False).to(dev).eval()


class Timed(nn.Module):
    """The network with HIP events around every forward."""

    def __init__(self, net):
        super().__init__()
        self.net, self.events = net, []

    def forward(self, x):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = self.net(x)
        b.record()
        self.events.append((a, b))
        return out


def composed(model, img, label, patch):
    """what evaluate_case costs when built from the existing predictor and the reference's host tail"""
    model.eval()
    lr_data, _ = su.preprocess_image(img)
    lr_label, _ = su.preprocess_image(label, apply_norm=False)
    lr_data, rev = su.pad_nd_image(lr_data, patch, "constant", {"value": 0}, True, None)
    with torch.no_grad():
        slicers = su._internal_get_sliding_window_slicers(lr_data.shape[1:], patch_size=patch)
        logits = su._internal_predict_sliding_window_return_logits(lr_data, slicers, model, True, 0, 1, patch,
                                                                   use_gaussian=True, deep_supervision=False)
    pred = logits.to("cpu")[tuple([slice(None), *rev[1:]])]
    with torch.no_grad():
        prob = torch.softmax(pred.float(), dim=0).numpy()
    pred_lr = prob.argmax(0).astype("uint8")
    return pred_lr, su.calculate_dice(pred_lr, lr_label.squeeze(0).numpy().astype("uint8"))


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    img = rng.randint(0, 1000, size=(1, 20, 455, 633)).astype(np.float32)
    label = (rng.rand(1, 20, 455, 633) < 0.3).astype(np.float32)
    patch = [16, 320, 384]
    net = Timed(student(dev))
    t_fused, out_f = timed(lambda: su.evaluate_case(net, img, label, 4.0, patch), args.reps)
    n_fwd = len(net.events) // (args.reps + 1)
    fwd = [a.elapsed_time(b) for a, b in net.events[-n_fwd * args.reps:]]
    net_s = sum(fwd) / 1e3 / args.reps
    net.events.clear()
    t_comp, out_c = timed(lambda: composed(net, img, label, patch), args.reps)
    same = bool(np.array_equal(out_f[0], out_c[0]))
    print(f"case 1x20x455x633, tile {patch}, {n_fwd} tiles x 8 mirrorings, fp32, median of {args.reps}:")
    print(f"  fused    {t_fused:.3f} s/case  (network {net_s:.3f} s = {100 * net_s / t_fused:.1f} %, "
          f"rest {t_fused - net_s:.3f} s)")
    print(f"  composed {t_comp:.3f} s/case  (rest {t_comp - net_s:.3f} s)")
    print(f"  same LR map: {same}, dice fused {out_f[3]!r} composed {out_c[1]!r}", flush=True)


if __name__ == "__main__":
    main()
