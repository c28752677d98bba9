"""Stage-1 volume preparation without a GPU: the three new C-ABI symbols, the zoom tables, and the host logic of
postprocess_smore_volume / stage1_volumes / postprocess_smore / TrainSetMultiple(volumes=device dicts) over the CPU
statement of their kernels (tests/stage1_emu.py) against the reference's own outputs (tests/golden/stage1_smore.npz,
written by tools/gen_golden_stage1.py from the reference's postprocess_smore with real scipy)."""
import os

import numpy as np
import pytest
import torch

from rehrseg_amd import lib as L
from rehrseg_amd import ops
from rehrseg_amd.utils import sr_utils as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "stage1_smore.npz"))
CASES = ("odd", "wide_x", "wide_y", "tie", "single")
NEW_SYMBOLS = ("rehr_zoom_depth_f32", "rehr_bspline_prefilter_axis_f64acc_f32", "rehr_blur_to_slices_f32")
ULP = 2.0 ** -23


def case(name):
    return {k: G[f"{name}_{k}"] for k in ("vol", "sep", "kernel", "img_hr", "label_hr", "image_x_rgb", "image_y_rgb")}


def check_against_fixture(name, res):
    """res: postprocess_smore_volume's dict.  The bounds: one fp32 ulp at the volume's largest magnitude for the zoomed
    image (the fp64 line differs from scipy's in its last bits, which can flip the one fp32 rounding and nothing more),
    L more fp32 roundings of a non-negative unit-sum profile for the blurred copies; the label exact."""
    c = case(name)
    got = {k: res[k].cpu().numpy() for k in ("img_hr", "label_hr", "image_x_rgb", "image_y_rgb")}
    for k, v in got.items():
        assert v.shape == c[k].shape and v.dtype == c[k].dtype, (k, v.shape, v.dtype)
    assert np.array_equal(got["label_hr"], c["label_hr"])
    top = float(np.abs(c["img_hr"]).max())
    err = float(np.abs(got["img_hr"] - c["img_hr"]).max())
    print(f"{name} img_hr: max abs error {err:.3e}, bound {ULP * top:.3e}, "
          f"{int((got['img_hr'] != c['img_hr']).sum())} of {c['img_hr'].size} voxels not bit-equal")
    assert err <= ULP * top
    L_ = c["kernel"].size
    for k in ("image_x_rgb", "image_y_rgb"):
        err = float(np.abs(got[k] - c[k]).max())
        print(f"{name} {k}: max abs error {err:.3e}, bound {(L_ + 1) * ULP * top:.3e}")
        assert err <= (L_ + 1) * ULP * top


@pytest.fixture
def semu():
    import stage1_emu as E
    old = ops.set_backend(E)
    yield E
    ops.set_backend(old)


def test_new_symbols_are_declared_and_exported():
    lib = L.load()
    declared = L.declared_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared and s in L.PROTOTYPES and hasattr(lib, s), s
    assert L.ABI_VERSION == 6 and lib.rehr_abi_version() == 6


def test_new_entry_points_reject_null_arguments_without_launching():
    lib = L.load()
    assert lib.rehr_zoom_depth_f32(None, 4, 3, 2, None, None, None, 12, None, None, None) == -1
    assert lib.rehr_bspline_prefilter_axis_f64acc_f32(None, None, 4, 3, 1, None) == -1
    assert lib.rehr_blur_to_slices_f32(None, None, 3, None, 4, 4, 4, 0, None) == -1


def test_malformed_arguments_are_rejected_before_any_launch():
    """Non-null but inconsistent arguments (host addresses that are never dereferenced: every call returns first)."""
    import ctypes
    lib = L.load()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    q = ctypes.c_void_p(p.value + 64)
    assert lib.rehr_zoom_depth_f32(p, 4, 3, 3, p, p, p, 12, q, q, None) == -1        # C = 3
    assert lib.rehr_zoom_depth_f32(p, 4, 3, 2, p, p, None, 12, q, q, None) == -1     # C = 2 without the label table
    assert lib.rehr_zoom_depth_f32(p, 4, 3, 2, p, p, p, 12, q, None, None) == -1     # C = 2 without the label output
    assert lib.rehr_zoom_depth_f32(p, 0, 3, 2, p, p, p, 12, q, q, None) == -1        # no line
    assert lib.rehr_zoom_depth_f32(p, 4, 0, 2, p, p, p, 12, q, q, None) == -1        # no sample
    assert lib.rehr_zoom_depth_f32(p, 4, 3, 2, p, p, p, 0, q, q, None) == -1         # no output slice
    assert lib.rehr_zoom_depth_f32(p, 4, 284, 2, p, p, p, 12, q, q, None) == -2      # beyond the LDS bound on n
    assert lib.rehr_zoom_depth_f32(p, 4, 3, 2, p, ctypes.c_void_p(p.value + 4), p, 12, q, q, None) == -1   # w misaligned
    assert lib.rehr_bspline_prefilter_axis_f64acc_f32(p, p, 4, 3, 1, None) == -1     # in place
    assert lib.rehr_bspline_prefilter_axis_f64acc_f32(p, q, 4, 0, 1, None) == -1
    assert lib.rehr_bspline_prefilter_axis_f64acc_f32(p, q, 4, 3, 0, None) == -1
    assert lib.rehr_bspline_prefilter_axis_f64acc_f32(p, q, 4, 284, 2, None) == -2
    assert lib.rehr_blur_to_slices_f32(p, p, 3, p, 4, 4, 4, 0, None) == -1           # in place
    assert lib.rehr_blur_to_slices_f32(p, p, 3, q, 4, 4, 4, 2, None) == -1           # axis 2
    assert lib.rehr_blur_to_slices_f32(p, p, 0, q, 4, 4, 4, 0, None) == -1           # no tap
    assert lib.rehr_blur_to_slices_f32(p, p, 3, q, 4, 0, 4, 1, None) == -1
    assert lib.rehr_blur_to_slices_f32(p, p, 33, q, 4, 4, 4, 0, None) == -2          # L > 32


def test_launch_layer_refuses_host_tensors_and_wrong_dtypes():
    from rehrseg_amd import hip_backend as hb
    idx, w, nn = (torch.from_numpy(t) for t in sr.zoom_taps(3, 4))
    with pytest.raises(L.RehrsegHipError):
        hb.zoom_depth(torch.zeros(4, 4, 3, 2), idx, w, nn)
    with pytest.raises(L.RehrsegHipError):
        hb.bspline_prefilter(torch.zeros(4, 4, 3), 2)
    with pytest.raises(L.RehrsegHipError):
        hb.blur_to_slices(torch.zeros(4, 4, 3), torch.ones(3), 0)


@pytest.mark.parametrize("name", CASES)
def test_zoom_taps_geometry_matches_the_fixture(name):
    c = case(name)
    n = c["vol"].shape[2]
    idx, w, nn = sr.zoom_taps(n, float(c["sep"]))
    Z = c["img_hr"].shape[2]
    assert idx.shape == (Z, 4) and idx.dtype == np.int32 and w.shape == (Z, 4) and w.dtype == np.float64
    assert nn.shape == (Z,) and nn.dtype == np.int32
    assert idx.min() >= 0 and idx.max() < n and nn.min() >= 0 and nn.max() < n
    assert np.abs(w.sum(1) - 1.0).max() < 1e-15 and w.min() > -1e-15
    # the order-0 gather is the whole label path
    assert np.array_equal(c["vol"][..., 1][..., nn].astype(np.uint8), c["label_hr"][..., 0])
    # the end samples sit on input samples: weights (1/6, 2/3, 1/6, 0) over the mirrored neighbours
    assert nn[0] == 0 and nn[-1] == n - 1
    assert np.allclose(w[0], [1 / 6, 2 / 3, 1 / 6, 0], atol=1e-15)
    assert idx[0].tolist() == {1: [0, 0, 0, 0], 2: [1, 0, 1, 0]}.get(n, [1, 0, 1, 2])


def test_zoom_taps_tie_single_sample_and_odd_separations():
    _, _, nn = sr.zoom_taps(7, 3)
    assert nn[15] == 5                                    # position 4.5: half up, where half-to-even gives 4
    idx, w, nn = sr.zoom_taps(1, 4)
    assert not idx.any() and not nn.any() and idx.shape == (4, 4) and np.abs(w.sum(1) - 1.0).max() < 1e-15
    idx, w, nn = sr.zoom_taps(6, 2.5)                     # no integrality constraint on this path
    assert idx.shape == (15, 4) and nn[-1] == 5
    idx, w, nn = sr.zoom_taps(2, 0.5)                     # one output sample sits at position 0
    assert idx.shape == (1, 4) and nn.tolist() == [0] and idx[0].tolist() == [1, 0, 1, 0]
    with pytest.raises(ValueError):
        sr.zoom_taps(1, 0.25)
    # 86 * (28 / 86) rounds to a position beyond the last sample: ndimage writes cval = 0 there
    idx, w, nn = sr.zoom_taps(29, 3)
    assert nn[-1] == -1 and not w[-1].any() and (nn[:-1] >= 0).all()
    a, b = sr.zoom_taps(7, 3, "cpu"), sr.zoom_taps(7, 3, "cpu")
    assert all(x is y for x, y in zip(a, b)) and a[1].dtype == torch.float64


@pytest.mark.parametrize("name", CASES)
def test_postprocess_smore_volume_reproduces_the_reference_fixture(semu, name):
    c = case(name)
    res = sr.postprocess_smore_volume(c["vol"], float(c["sep"]), torch.from_numpy(c["kernel"]).view(1, 1, -1, 1), "cpu")
    check_against_fixture(name, res)
    # the unit axes are views of the kernels' outputs
    assert res["img_hr"].is_contiguous() and res["image_x_rgb"].is_contiguous() and res["image_y_rgb"].is_contiguous()
    again = sr.stage1_volumes([torch.from_numpy(c["vol"])], float(c["sep"]), c["kernel"])[0]
    assert all(torch.equal(again[k], res[k]) for k in res)
    if name == "single":
        assert torch.equal(res["img_hr"], torch.from_numpy(c["vol"][..., :1]).expand(-1, -1, -1, 4).reshape(5, 4, 4, 1))


def test_prefilter_statement_reproduces_spline_filter1d(semu):
    x = torch.from_numpy(G["prefilter_x"])
    for axis in range(3):
        want = G[f"prefilter_axis{axis}"]
        err = float(np.abs(semu.bspline_prefilter(x, axis).numpy() - want).max())
        assert err <= ULP * float(np.abs(want).max()), (axis, err)


@pytest.mark.parametrize("name", ["odd", "tie"])
def test_reference_named_wrapper(semu, monkeypatch, name):
    """postprocess_smore derives its Gaussian from the separation: the profile of the fixture."""
    c = case(name)
    monkeypatch.setattr(sr, "_as_device_volume",
                        lambda v, d: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)))
    sep = int(c["sep"])
    out = sr.postprocess_smore(name, sep, {name: c["vol"]})
    assert isinstance(out, tuple) and len(out) == 4
    check_against_fixture(name, dict(zip(("img_hr", "label_hr", "image_x_rgb", "image_y_rgb"), out)))
    direct = sr.postprocess_smore(name, sep, c["vol"])
    assert all(torch.equal(a, b) for a, b in zip(out, direct))
    with pytest.raises(NotImplementedError, match="WDSR"):
        sr.postprocess_smore(name, sep, c["vol"], "sr_out")
    with pytest.raises(ImportError, match="nibabel"):
        sr.postprocess_smore(name, sep, "merge_dir")
    with pytest.raises(ImportError, match="nibabel"):
        sr.postprocess_smore(name, sep)


def test_train_set_keeps_resident_tensors_where_they_lie(semu, monkeypatch):
    """TrainSetMultiple(volumes=stage1_volumes(...)): no copy of the four tensors, and the same patches as the data set
    built from the same arrays as numpy dicts."""
    import random
    from feed_cases import emu_axis_resample, emu_patch_gather
    from rehrseg_amd import hip_backend as hb
    from rehrseg_amd.utils import train_set as ts
    monkeypatch.setattr(hb, "patch_gather", emu_patch_gather)
    monkeypatch.setattr(hb, "axis_resample", emu_axis_resample)
    monkeypatch.setattr(ts._DeviceSet, "_check_device", lambda self, device: torch.device("cpu"))
    vols = sr.stage1_volumes([G["odd_vol"], G["tie_vol"]], 4, G["odd_kernel"], "cpu")
    args = (None, ["a", "b"], 4.0, 1.0, None, None, (16, 16, 1), True, "cpu")
    ds = ts.TrainSetMultiple(*args, volumes=vols)
    for i, v in enumerate(vols):
        assert ds.imgs_hr[i].data_ptr() == v["img_hr"].data_ptr()
        assert ds.labels_hr[i].data_ptr() == v["label_hr"].data_ptr() and ds.labels_hr[i].dtype == torch.uint8
        assert ds.imgs_filtered_x[i].data_ptr() == v["image_x_rgb"].data_ptr()
        assert ds.imgs_filtered_y[i].data_ptr() == v["image_y_rgb"].data_ptr()
    ref = ts.TrainSetMultiple(*args, volumes=[{k: t.numpy() for k, t in v.items()} for v in vols])
    random.seed(3)
    a = ds.batch([0, 1])
    random.seed(3)
    b = ref.batch([0, 1])
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    plain = ts.TrainSetMultiple(*args, blur=False, volumes=vols)
    assert plain.imgs_filtered_x == [None, None] and plain.imgs_hr[1].data_ptr() == vols[1]["img_hr"].data_ptr()
