"""The bar of a bf16-stored result of the matrix-core kernels (bf16 operands, fp32 accumulation, ONE rounding at the
store) against an fp64 reference on the same bf16-rounded operands -- a plain helper module, shared by
test_bf16_bar_cpu.py, test_bf16_conv_edges_gpu.py and test_bf16_kernels_gpu.py.

Per element (bf16_bar / assert_bf16_bar):

    |got - ref| <= 2^-8 * |ref| + acc * max|ref|

  * 2^-8 * |ref|: the store rounds an fp32 value to the nearest bf16.  bf16 keeps 8 significant bits, so a value in
    [2^e, 2^(e+1)) has the ulp 2^(e-7) and round-to-nearest moves it by at most half of that, 2^(e-8) <= 2^-8 * |value|
    (equality at the power of two).  A store that truncates loses up to a whole ulp, 2^-7.
  * acc * max|ref|: the fp32 accumulation of the products in another order than the reference's.  acc = 1e-4 is the bar
    this project sets for fp32-STORED outputs of the same accumulators (the docstrings of test_kernels_gpu.py and
    test_bf16_kernels_gpu.py: 1e-4 of the tensor's largest value).
  * The two terms add, so an element whose fp32 sum lies within the accumulation error of a rounding boundary and rounds
    the other way than the reference would stays inside: it is off by at most half an ulp plus that error.

The bound is a condition on EVERY element: nothing is masked and no element is left out.  The epilogues tested with
it are continuous (bias, LeakyReLU: a kink, no jump in value) and the input gradients take dz as given, so no element
sits at a discontinuity that an accumulation error could push across.  A NaN counts as a violation.

Per (sample, channel) reduction (stats_bar / assert_stats_bar), the project's reduction bar (test_stream_kernels_gpu.py):

    |got - sum(summands)| <= factor * sum|summands|          factor = 5e-6

with the summands taken from the fp64 reference (the sum statistic: ref; the sum of squares: ref^2).

Both checkers return (violations, worst ratio of |error| to the bound); the assert_ forms print that figure before they
assert, so a run with `pytest -s` shows how far from the bar every case sits."""
import torch

HALF_ULP = 2.0 ** -8      # round-to-nearest bf16 store, relative
ACC = 1e-4                # fp32 accumulation, relative to the largest reference value
ACC_STREAM = 1e-5         # the streaming kernels' term (test_stream_kernels_gpu.py): printed next to the asserted figure
RED_FACTOR = 5e-6         # reductions: of the fp64 sum of |summand|


def _f64(t):
    return t.detach().double().cpu()


def _ratio(err, bound):
    """err / bound per element with 0 / 0 = 0; a NaN in err stays NaN (and is a violation)."""
    return torch.where(err == 0, torch.zeros_like(err), err / bound)


def _tally(err, bound):
    violations = int((~(err <= bound)).sum())
    ratio = _ratio(err, bound)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if bool(torch.isnan(ratio).any()):
        worst = float("nan")
    return violations, worst


def bf16_bar(got, ref64, acc=ACC):
    """(violations, worst ratio) of |got - ref| <= 2^-8 |ref| + acc max|ref| over every element."""
    got, ref = _f64(got), _f64(ref64)
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    bound = HALF_ULP * ref.abs() + acc * float(ref.abs().max())
    return _tally((got - ref).abs(), bound)


def assert_bf16_bar(name, got, ref64, acc=ACC):
    violations, worst = bf16_bar(got, ref64, acc)
    _, worst_stream = bf16_bar(got, ref64, ACC_STREAM)
    print(f"{name} {worst:.3f}/1 {violations} violations (acc {acc:g}; with acc {ACC_STREAM:g}: {worst_stream:.3f}/1)")
    assert violations == 0, (name, violations, worst)
    return worst, worst_stream


def stats_bar(got, summands64, factor=RED_FACTOR):
    """(violations, worst ratio) of |got[n, c] - sum summands[n, c]| <= factor * sum |summands[n, c]|;
    got: (N, C), summands64: (N, C, ...) fp64 values of the reference."""
    got, s = _f64(got), _f64(summands64)
    assert s.dim() > 2 and tuple(got.shape) == tuple(s.shape[:2]), (tuple(got.shape), tuple(s.shape))
    s = s.flatten(2)
    return _tally((got - s.sum(2)).abs(), factor * s.abs().sum(2))


def assert_stats_bar(name, got, summands64, factor=RED_FACTOR):
    violations, worst = stats_bar(got, summands64, factor)
    print(f"{name} {worst:.3f}/1 {violations} violations (reduction bar {factor:g} of sum |summand|)")
    assert violations == 0, (name, violations, worst)
    return worst


def assert_conv_stats(name, stats, ref64, factor=RED_FACTOR):
    """The (N, C, 2) statistics of a conv epilogue (stats_mode 2): sum and sum of squares of the fp64 reference."""
    return (assert_stats_bar(name + " sum", stats[..., 0], ref64, factor),
            assert_stats_bar(name + " sumsq", stats[..., 1], ref64 * ref64, factor))
