"""Intensity normalisation without a GPU: the host paths of percentile_normalization / zeroone_normalization against
the reference's own outputs (tests/golden/intensity_norm.npz, written by tools/gen_golden_intensity.py), the numpy
statement of the device contract (tests/intensity_oracle.py) against numpy.percentile, the device paths, the data set
and evaluate_case over the CPU emulation of the kernels (tests/intensity_emu.py), and the four new C-ABI symbols."""
import os

import numpy as np
import pytest
import torch

import intensity_oracle as io
from rehrseg_amd import lib as L
from rehrseg_amd import ops
from rehrseg_amd.utils import seg_utils as su
from test_eval_cpu import G as EVAL
from toy_models import ToySegNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "intensity_norm.npz"))
SAME_NUMPY = str(G["numpy_version"]).split(".")[0] == np.__version__.split(".")[0]
NEW_SYMBOLS = ("rehr_order_stats_workspace_bytes", "rehr_order_stats_f32", "rehr_percentile_f64",
               "rehr_intensity_apply_f32")
EINVAL, ENOSUP = -1, -2


@pytest.fixture
def intensity_emu():
    import intensity_emu as E
    old = ops.set_backend(E)
    yield E
    ops.set_backend(old)


def _meets_fixture(got, want, src, p=(0.5, 99.5), strictly_positive=True):
    """Bit-equal under the recording numpy's major version; else within 8 * 2^-24 * (|v_max| + |v_min|) / (v_max -
    v_min): the most that rounding the two bounds to fp32 and three fp32 operations can move a value in [0, 1]."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    if SAME_NUMPY:
        assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True)
        return
    v_min, v_max = np.percentile(src, list(p))
    if strictly_positive and v_min < 0:
        v_min = 0.0
    bound = 8 * 2.0 ** -24 * (abs(v_max) + abs(v_min)) / (v_max - v_min)
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    print(f"max |difference| {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_host_percentile_paths_reproduce_the_reference():
    _meets_fixture(su.percentile_normalization(G["arr3"].copy()), G["perc_arr3"], G["arr3"])
    _meets_fixture(su.percentile_normalization(G["vol5"].copy()), G["perc_vol5_array"], G["vol5"])
    t = torch.from_numpy(G["vol5"].copy())
    out = su.percentile_normalization(t)
    assert isinstance(out, torch.Tensor) and tuple(out.shape) == (2, 1, 5, 9, 11)
    assert np.array_equal(t.numpy(), G["vol5"])                       # not written in place
    for b in range(2):
        _meets_fixture(out[b].numpy(), G["perc_vol5_tensor"][b], G["vol5"][b])
    sh = G["shifted"]
    _meets_fixture(su.percentile_normalization(sh.copy(), 5, 95, False), G["perc_shifted_5_95"], sh, (5, 95), False)
    _meets_fixture(su.percentile_normalization(sh.copy(), 5, 95, True), G["perc_shifted_pos"], sh, (5, 95), True)


def test_host_zeroone_paths_reproduce_the_reference():
    for key in ("arr3", "vol5"):
        a = G[key].copy()
        out = su.zeroone_normalization(a)
        want = G["zeroone_arr3" if key == "arr3" else "zeroone_vol5_array"]
        assert out.dtype == np.float32 and np.array_equal(out, want) and np.array_equal(a, want)     # in place
    t = torch.from_numpy(G["vol5"].copy())
    out = su.zeroone_normalization(t)
    assert tuple(out.shape) == (2, 1, 5, 9, 11) and out.dtype == torch.float32
    assert np.array_equal(out.numpy(), G["zeroone_vol5_tensor"])
    assert np.array_equal(t.numpy(), G["zeroone_vol5_tensor_after"])


def _np_cases():
    for name, (x, _) in io.order_cases().items():
        if not name.startswith("nan"):
            yield name, x
    yield "gauss_1e6", io.gaussian(1 << 20, 21)[None]
    yield "zeros_1e6", io.zero_heavy((1 << 20) + 3, 22)[None]


@pytest.mark.parametrize("q", io.Q_SETS)
def test_oracle_meets_numpy_percentile(q):
    """The oracle's virtual index and lerp against numpy's own on x.astype(float64): at most 16 * 2^-53 * S *
    (max - min) apart.  The two virtual indices differ by at most a few fp64 roundings of a number <= S and the lerp is
    continuous across an index step."""
    worst = 0.0
    for name, x in _np_cases():
        fin = x[np.isfinite(x)]
        if fin.size != x.size:
            continue                                   # +-inf: numpy's lerp forms inf - inf
        got = io.percentiles(x, q)
        for b in range(x.shape[0]):
            want = np.percentile(x[b].astype(np.float64), q)
            bound = 16 * 2.0 ** -53 * x.shape[1] * (float(x[b].max()) - float(x[b].min()))
            err = float(np.abs(got[b] - want).max())
            worst = max(worst, err)
            assert err <= bound, (name, b, q, got[b], want)
    print(f"q = {q}: largest difference {worst:.3e}")


def test_emulated_select_meets_the_sort(intensity_emu):
    for name, (x, ranks) in io.order_cases().items():
        got = intensity_emu.order_stats(torch.from_numpy(x.copy()), ranks).numpy()
        assert io.same_order_stats(got, io.order_stats(x, ranks)), name


def test_device_paths_meet_the_oracle_under_the_emulation(intensity_emu):
    x = np.stack([io.zero_heavy(5 * 9 * 11, 30), io.gaussian(5 * 9 * 11, 31) * np.float32(40.0)]).reshape(2, 1, 5, 9, 11)
    t = torch.from_numpy(x.copy())
    out = su._percentile_normalization_device(t)
    assert out.dtype == torch.float32 and tuple(out.shape) == (2, 1, 5, 9, 11) and np.array_equal(t.numpy(), x)
    assert np.array_equal(io.bits(out.numpy()), io.bits(io.percentile_norm(x)))
    out = su._percentile_normalization_device(t, 5, 95, False)
    assert np.array_equal(io.bits(out.numpy()), io.bits(io.percentile_norm(x, 5, 95, False)))
    # two channels, contiguous: channel 0 of every item is a dense run, channel 1 is left alone
    x2 = np.concatenate([x, x[::-1] + np.float32(1.0)], axis=1)
    t2 = torch.from_numpy(x2.copy())
    out = su._zeroone_normalization_device(t2)
    want = io.zeroone(x2[:, 0])
    assert np.array_equal(io.bits(out.numpy()[:, 0]), io.bits(want))
    assert np.array_equal(io.bits(t2.numpy()[:, 0]), io.bits(want)) and np.array_equal(t2.numpy()[:, 1], x2[:, 1])
    with pytest.raises(ValueError, match="dense run"):
        su._percentile_normalization_device(torch.from_numpy(x2.copy()).to(memory_format=torch.channels_last_3d))
    with pytest.raises(ValueError, match="dense run"):
        su._zeroone_normalization_device(torch.from_numpy(x2.copy()).to(memory_format=torch.channels_last_3d))
    for q in io.Q_SETS:
        got = su.intensity_percentiles(x[:, 0], q, device="cpu")
        assert got.dtype == torch.float64 and tuple(got.shape) == (2, 2)
        assert np.array_equal(got.numpy().view(np.uint64), io.percentiles(x[:, 0], q).view(np.uint64))
    with pytest.raises(ValueError):
        su.intensity_percentiles(x, [1, 2, 3, 4, 5], device="cpu")
    with pytest.raises(ValueError):
        su.intensity_percentiles(x, [101.0], device="cpu")


def _volumes(rng):
    img = (np.abs(rng.randn(12, 10, 8)) * 100).astype(np.float32)
    img[rng.rand(12, 10, 8) < 0.5] = 0
    return [{"img": img, "seg": (rng.rand(12, 10, 8) > 0.5).astype(np.uint8)}]


@pytest.mark.parametrize("norm", ("percentile", ("percentile", 2.0, 98.0), "zeroone"))
def test_data_set_holds_the_oracle_volume(intensity_emu, monkeypatch, norm):
    from rehrseg_amd.utils import train_set as ts
    monkeypatch.setattr(ts._DeviceSet, "_check_device", lambda self, device: torch.device("cpu"))
    vols = _volumes(np.random.RandomState(0))
    raw = vols[0]["img"].copy()
    ds = ts.TrainSetMultipleSegSREfficient(None, [0], 4.0, 1.0, (8, 8, 2), (8, 8), norm=norm, device="cpu",
                                           volumes=vols)
    if norm == "zeroone":
        want = io.zeroone(raw[None])[0]
    else:
        p = (0.5, 99.5) if norm == "percentile" else norm[1:]
        want = io.percentile_norm(raw[None], *p)[0]
    assert np.array_equal(io.bits(ds.imgs[0].numpy()), io.bits(want)) and np.array_equal(vols[0]["img"], raw)
    # a volume that is a tensor on the data set's device is taken as it is and not written
    dev_vols = [{"img": torch.from_numpy(raw.copy()), "seg": torch.from_numpy(vols[0]["seg"])}]
    ds = ts.TrainSetMultipleSegSREfficient(None, [0], 4.0, 1.0, (8, 8, 2), (8, 8), norm=norm, device="cpu",
                                           volumes=dev_vols)
    assert np.array_equal(io.bits(ds.imgs[0].numpy()), io.bits(want)) and np.array_equal(dev_vols[0]["img"].numpy(), raw)


@pytest.mark.parametrize("norm", ("minmax", 2.5, ("percentile", 99.0, 1.0), ("percentile", 1.0)))
def test_bad_norm_raises(monkeypatch, norm):
    from rehrseg_amd.utils import train_set as ts
    monkeypatch.setattr(ts._DeviceSet, "_check_device", lambda self, device: torch.device("cpu"))
    with pytest.raises(ValueError, match="norm"):
        ts.TrainSetMultipleSegSREfficient(None, [0], 4.0, 1.0, (8, 8, 2), (8, 8), norm=norm, device="cpu",
                                          volumes=_volumes(np.random.RandomState(0)))
    img, label = EVAL["multi_img"].astype(np.float32), EVAL["multi_label"].astype(np.float32)
    with pytest.raises(ValueError, match="norm"):
        su.evaluate_case(ToySegNet(sep=2), img, label, 2, list(EVAL["multi_patch"]), device="cpu", norm=norm)


@pytest.mark.parametrize("norm", ("percentile", ("percentile", 5.0, 95.0), "zeroone"))
def test_evaluate_case_normalises_in_front_of_the_tiles(intensity_emu, norm):
    sep = int(EVAL["sep"])
    img, label = EVAL["multi_img"].astype(np.float32), EVAL["multi_label"].astype(np.float32)
    patch = list(EVAL["multi_patch"])
    if norm == "zeroone":
        pre = io.zeroone(img)
    else:
        pre = io.percentile_norm(img, *((0.5, 99.5) if norm == "percentile" else norm[1:]))
    got = su.evaluate_case(ToySegNet(sep=sep), img, label, sep, patch, get_HR_results=True, device="cpu", norm=norm)
    want = su.evaluate_case(ToySegNet(sep=sep), pre, label, sep, patch, get_HR_results=True, device="cpu", norm=None)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and torch.equal(got[2], want[2])
    assert got[3] == want[3]
    zs = su.evaluate_case(ToySegNet(sep=sep), img, label, sep, patch, get_HR_results=True, device="cpu")
    same = su.evaluate_case(ToySegNet(sep=sep), img, label, sep, patch, get_HR_results=True, device="cpu", norm="zscore")
    assert np.array_equal(zs[0], EVAL["multi_pred_lr"]) and np.array_equal(same[0], zs[0]) and same[3] == zs[3]


def test_reference_import_line_and_abi():
    from rehrseg_amd.utils.seg_utils import get_training_transforms, zeroone_normalization, zscore_normalization  # noqa: F401
    from rehrseg_amd.utils.train_set import zeroone_normalization as z2
    assert z2 is zeroone_normalization and callable(su.percentile_normalization) and callable(su.intensity_percentiles)
    assert L.ABI_VERSION == 6
    declared = L.declared_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared and s in L.PROTOTYPES


def test_c_abi_argument_checks():
    """The argument checks run before any launch, so they run without a GPU."""
    import ctypes as C
    lib = L.load()
    assert lib.rehr_abi_version() == 6
    buf = (C.c_char * 4096)()
    p = (C.addressof(buf) + 15) & ~15
    ranks = (C.c_int64 * 8)(0, 1, 2, 3, 4, 5, 6, 7)
    t = (C.c_double * 4)(0.5, 0.5, 0.5, 0.5)
    big = 1 << 40
    assert lib.rehr_order_stats_workspace_bytes(1, 2) == 32 + 16 + 2048
    assert lib.rehr_order_stats_workspace_bytes(0, 2) == EINVAL and lib.rehr_order_stats_workspace_bytes(1, 0) == EINVAL
    assert lib.rehr_order_stats_workspace_bytes(65536, 2) == ENOSUP and lib.rehr_order_stats_workspace_bytes(1, 9) == ENOSUP
    assert lib.rehr_order_stats_f32(None, 1, 8, 8, ranks, 8, p, p, big, None) == EINVAL
    assert lib.rehr_order_stats_f32(p, 1, 8, 8, ranks, 8, p, None, big, None) == EINVAL
    assert lib.rehr_order_stats_f32(p, 1, 0, 0, ranks, 1, p, p, big, None) == EINVAL
    assert lib.rehr_order_stats_f32(p, 1, 7, 7, ranks, 8, p, p, big, None) == EINVAL          # rank 7 of 7 elements
    assert lib.rehr_order_stats_f32(p, 1, 8, 8, ranks, 8, p, p, 64, None) == EINVAL           # workspace too small
    assert lib.rehr_order_stats_f32(p, 1, 8, 8, ranks, 8, p, p + 4, big, None) == EINVAL      # misaligned workspace
    assert lib.rehr_order_stats_f32(p, 1, (1 << 30) + 1, 0, ranks, 8, p, p, big, None) == ENOSUP
    assert lib.rehr_order_stats_f32(p, 65536, 8, 8, ranks, 8, p, p, big, None) == ENOSUP
    assert lib.rehr_order_stats_f32(p, 1, 8, 8, ranks, 9, p, p, big, None) == ENOSUP
    assert lib.rehr_percentile_f64(p, 1, 5, t, 0, p, None) == ENOSUP
    assert lib.rehr_percentile_f64(p, 0, 2, t, 0, p, None) == EINVAL and lib.rehr_percentile_f64(None, 1, 2, t, 0, p, None) == EINVAL
    assert lib.rehr_percentile_f64(p, 1, 2, (C.c_double * 2)(0.5, 1.0), 0, p, None) == EINVAL
    assert lib.rehr_intensity_apply_f32(p, p, 1, 8, 8, 8, 2, p, 2, None) == EINVAL             # no such mode
    assert lib.rehr_intensity_apply_f32(p, None, 1, 8, 8, 8, 0, p, 2, None) == EINVAL
    assert lib.rehr_intensity_apply_f32(p, p, 1, 0, 8, 8, 0, p, 2, None) == EINVAL
    assert lib.rehr_intensity_apply_f32(p, p, 2, 8, 7, 8, 0, p, 2, None) == EINVAL             # items overlap
    assert lib.rehr_intensity_apply_f32(p, p, 1, (1 << 30) + 1, 0, 0, 0, p, 2, None) == ENOSUP


def test_percentile_plan_is_numpys_virtual_index():
    from rehrseg_amd.hip_backend import percentile_plan
    for S in (1, 2, 3, 201, 4099, 5760300, 1 << 30):
        for q in io.Q_SETS:
            assert percentile_plan(S, q) == io.plan(S, q)
    with pytest.raises(ValueError):
        percentile_plan(10, [-1.0])
