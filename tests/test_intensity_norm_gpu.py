"""Intensity normalisation on the MI355X (csrc/intensity_norm.hip) against the numpy statement of its contract
(tests/intensity_oracle.py).  Every comparison is exact equality: order statistics as uint32 bit patterns (-0 and +0
alike), percentile bounds as fp64 bits, normalised volumes as fp32 bits (every NaN alike).  No tolerance anywhere.

The cases are the smallest shapes at which each step of the radix select can go wrong (intensity_oracle.order_cases):
sizes around one wave, one block and a 16-byte vector, items that start misaligned, keys that differ in the last or
in the first digit only, one bin, a step at the rank, ties at the rank, negative keys, a NaN in one item of three and
ranks whose prefixes collide.  In the two prefix cases the eight ranks point at keys built from the digit fields for
8/8/8/8 and for 11/11/10 digits: ranks (0, 1) share digit 0 and differ in digit 1, (2, 3) share digits 0 and 1 and
differ in digit 2, (4, 5) differ in the last digit only, (6, 7) differ in digit 0 already."""
import functools

import numpy as np
import pytest
import torch

import intensity_oracle as io
from rehrseg_amd import hip_backend as hb
from rehrseg_amd.utils import seg_utils as su
from test_components_gpu import _count_syncs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CASES = io.order_cases()
NORM_CASES = ("size_1", "size_2", "size_3", "size_65", "size_65537", "three_items_4099", "constant", "step_q0.5_0",
              "step_q0.5_1", "step_q99.5_0", "step_q99.5_1", "ties", "all_negative", "mixed_sign", "nan_item")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("name", sorted(CASES))
def test_order_statistics_meet_the_sort(name):
    x, ranks = CASES[name]
    want = io.order_stats(x, ranks)
    got = hb.order_stats(_dev(x), ranks).cpu().numpy()
    print(f"{name}: ranks {ranks}\n  device {got.view(np.uint32)}\n  sort   {want.view(np.uint32)}")
    assert got.dtype == np.float32 and io.same_order_stats(got, want)
    if name == "nan_item":
        assert np.isnan(got[1]).all() and not np.isnan(got[[0, 2]]).any()
    if name == "last_digit":
        keys = x.view(np.uint32) ^ np.uint32(0x80000000)
        assert len(set((keys >> 10).ravel().tolist())) == 1 and len(set(got.ravel().tolist())) > 4   # 1024 floats: ties
    if name.startswith("prefix"):
        assert len(set(got.ravel().tolist())) == 8


@pytest.mark.parametrize("name", NORM_CASES)
def test_bounds_and_volumes_meet_the_oracle(name):
    x = CASES[name][0]
    t = _dev(x)
    for q in io.Q_SETS:
        ranks, frac = hb.percentile_plan(x.shape[1], q)
        assert (ranks, frac) == io.plan(x.shape[1], q)
        for sp in (False, True):
            got = hb.percentile_bounds(hb.order_stats(t, ranks), frac, sp).cpu().numpy()
            want = io.percentiles(x, q, sp)
            print(f"{name} q = {q} strictly_positive = {sp}: device {got.tolist()} oracle {want.tolist()}")
            assert io.same_values(got, want)
        got = su.intensity_percentiles(t, q)
        assert got.device == DEV and io.same_values(got.cpu().numpy(), io.percentiles(x, q))
    img = t.view(x.shape[0], 1, 1, 1, x.shape[1])
    for p_min, p_max, sp in ((0.5, 99.5, True), (0.5, 99.5, False), (5.0, 95.0, True), (5.0, 95.0, False)):
        out = su.percentile_normalization(img, p_min, p_max, sp)
        want = io.percentile_norm(x, p_min, p_max, sp)
        assert out.dtype == torch.float32 and out.device == DEV and tuple(out.shape) == tuple(img.shape)
        assert io.same_values(out.cpu().numpy().reshape(x.shape), want), (name, p_min, p_max, sp)
    assert np.array_equal(t.cpu().numpy().view(np.uint32), x.view(np.uint32))          # the input is not written
    if name == "nan_item":
        out = su.percentile_normalization(img).cpu().numpy().reshape(x.shape)
        assert np.isnan(out[1]).all() and not np.isnan(out[[0, 2]]).any()
    if name in ("all_negative", "mixed_sign"):
        on, off = io.percentiles(x, [0.5, 99.5], True), io.percentiles(x, [0.5, 99.5], False)
        assert off[0, 0] < 0 and on[0, 0] == 0
        assert (off[0, 1] < 0) == (name == "all_negative")
    if not name.startswith(("nan", "constant", "size_1")):
        z = t.clone().view(x.shape[0], 1, 1, 1, x.shape[1])
        out = su.zeroone_normalization(z)
        want = io.zeroone(x)
        assert io.same_values(out.cpu().numpy().reshape(x.shape), want)
        assert io.same_values(z.cpu().numpy().reshape(x.shape), want)                   # in place


@functools.lru_cache(maxsize=1)
def _volume():
    x = io.volume_case()
    return x, io.percentile_norm(x.reshape(1, -1)).reshape(x.shape)


def test_volume_shaped_case_meets_the_oracle_on_every_run():
    x, want = _volume()
    assert 0.59 < float((x == 0).mean()) < 0.61
    t = _dev(x)
    first = su.percentile_normalization(t)
    second = su.percentile_normalization(t)
    a, b = first.cpu().numpy(), second.cpu().numpy()
    assert tuple(first.shape) == (1, 1, 20, 455, 633) and io.same_values(a, want)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))                         # run to run
    q = [0.5, 99.5]
    p1, p2 = su.intensity_percentiles(t[0], q).cpu().numpy(), su.intensity_percentiles(t[0], q).cpu().numpy()
    assert io.same_values(p1, io.percentiles(x.reshape(1, -1), q)) and np.array_equal(p1.view(np.uint64), p2.view(np.uint64))


def test_public_functions_on_device_tensors():
    x = np.stack([io.zero_heavy(5 * 9 * 11, 30), io.gaussian(5 * 9 * 11, 31) * np.float32(40.0),
                  io.integers(5 * 9 * 11, 32)]).reshape(3, 1, 5, 9, 11)
    x2 = np.ascontiguousarray(np.concatenate([x, x[::-1] + np.float32(1.0)], axis=1))
    for src in (x, x2):                      # C == 1, and C == 2 contiguous: item starts 1980 bytes apart, misaligned
        t = _dev(src)
        out = su.percentile_normalization(t)
        assert tuple(out.shape) == (3, 1, 5, 9, 11) and out.dtype == torch.float32 and out.device == DEV
        assert io.same_values(out.cpu().numpy()[:, 0], io.percentile_norm(src[:, 0]))
        assert np.array_equal(t.cpu().numpy(), src)
        out = su.zeroone_normalization(t)
        want = io.zeroone(src[:, 0])
        assert tuple(out.shape) == (3, 1, 5, 9, 11) and io.same_values(out.cpu().numpy()[:, 0], want)
        after = t.cpu().numpy()
        assert io.same_values(after[:, 0], want)                                        # the caller's tensor is written
        if src.shape[1] == 2:
            assert np.array_equal(after[:, 1], src[:, 1])                               # channel 1 is untouched
    cl = _dev(x2).to(memory_format=torch.channels_last_3d)
    with pytest.raises(ValueError, match="dense run"):
        su.percentile_normalization(cl)
    with pytest.raises(ValueError, match="dense run"):
        su.zeroone_normalization(cl)
    with pytest.raises(ValueError, match="float32"):
        su.zeroone_normalization(_dev(x).double())


def _stage2_volumes(raw):
    return [{"img": _dev(raw), "seg": _dev((raw > 100).astype(np.uint8))}]


def test_device_paths_make_no_host_sync():
    from rehrseg_amd.utils.train_set import TrainSetMultipleSegSREfficient
    x = io.zero_heavy(2 * 6 * 40 * 37, 40).reshape(2, 1, 6, 40, 37)
    raw = io.zero_heavy(24 * 20 * 9, 41).reshape(24, 20, 9)
    mk = lambda vols: TrainSetMultipleSegSREfficient(None, [0], 4.0, 1.0, (8, 8, 2), (8, 8), norm="percentile",  # noqa: E731
                                                     device=DEV, volumes=vols)
    t, z, vols = _dev(x), _dev(x), _stage2_volumes(raw)
    su.percentile_normalization(t)                                                      # warm-up: library load
    su.zeroone_normalization(z.clone())
    mk(_stage2_volumes(raw))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = su.percentile_normalization(t)
        zo = su.zeroone_normalization(z)
        pct = su.intensity_percentiles(t[:, 0], [5, 95])
        ds = mk(vols)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert io.same_values(out.cpu().numpy()[:, 0], io.percentile_norm(x[:, 0]))
    assert io.same_values(zo.cpu().numpy()[:, 0], io.zeroone(x[:, 0]))
    assert io.same_values(pct.cpu().numpy(), io.percentiles(x[:, 0], [5, 95]))
    assert io.same_values(ds.imgs[0].cpu().numpy(), io.percentile_norm(raw[None])[0])
    assert np.array_equal(vols[0]["img"].cpu().numpy(), raw)
    # host arrays are uploaded raw and normalised by the same kernels
    host = TrainSetMultipleSegSREfficient(None, [0], 4.0, 1.0, (8, 8, 2), (8, 8), norm=("percentile", 2.0, 98.0),
                                          device=DEV, volumes=[{"img": raw, "seg": (raw > 100).astype(np.uint8)}])
    assert io.same_values(host.imgs[0].cpu().numpy(), io.percentile_norm(raw[None], 2.0, 98.0)[0])


class ThresholdToy(torch.nn.Module):
    """Class 1 where the normalised voxel stands above a shifted neighbour; device ops only (no syncs)."""

    def __init__(self, sep):
        super().__init__()
        self.sep = sep

    def forward(self, x):
        sh = torch.roll(x, shifts=(1, 2), dims=(3, 4))
        lr = torch.cat([sh * 0.5 + 0.02, x - 0.01], 1)
        return lr, torch.repeat_interleave(lr, self.sep, dim=2) * 1.5


@pytest.mark.parametrize("norm", ("percentile", "zeroone"))
def test_evaluate_case_normalises_on_the_device_with_one_host_sync(norm):
    model = ThresholdToy(sep=4)
    g = np.random.RandomState(3)
    img = io.zero_heavy(10 * 70 * 80, 50).reshape(1, 10, 70, 80)
    lab = (g.rand(1, 10, 70, 80) < 0.4).astype(np.float32)
    args = (model, img, lab, 4, [8, 32, 32], True, DEV)
    run = lambda: su._evaluate_case(*args, norm=norm)  # noqa: E731
    run()                                                                               # warm-up: cached Gaussian
    torch.cuda.synchronize()
    out, syncs = _count_syncs(run)
    assert len(syncs) == 1, [str(w.message) for w in syncs]
    pre = io.percentile_norm(img) if norm == "percentile" else io.zeroone(img)
    want = su._evaluate_case(model, pre, lab, 4, [8, 32, 32], True, DEV, norm=None)
    assert np.array_equal(out[0], want[0]) and np.array_equal(out[1], want[1]) and torch.equal(out[2], want[2])
    assert out[3] == want[3] and out[4] == want[4]
    assert 0 < out[0].sum() < out[0].size
    public = su.evaluate_case(model, img, lab, 4, [8, 32, 32], get_HR_results=True, device=DEV, norm=norm)
    assert np.array_equal(public[0], out[0]) and public[3] == out[3]
