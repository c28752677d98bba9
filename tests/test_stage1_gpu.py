"""Stage-1 volume preparation on the MI355X: the kernels of csrc/stage1_volume.hip against the reference's fixture
(tests/golden/stage1_smore.npz: the reference's postprocess_smore with real scipy), against the data set's own blur
route, and against their CPU statement (tests/stage1_emu.py) where the fixture's shapes do not reach a code path; the
data set fed from device tensors, and the absence of host synchronisation."""
import random

import numpy as np
import pytest
import torch

import stage1_emu
from rehrseg_amd import hip_backend as hb
from rehrseg_amd import lib as L
from rehrseg_amd.utils import sr_utils as sr
from rehrseg_amd.utils.train_set import TrainSetMultiple, _resample, blur_taps
from test_stage1_cpu import CASES, G, ULP, case, check_against_fixture

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _kernel(name):
    return torch.from_numpy(G[f"{name}_kernel"]).view(1, 1, -1, 1)


@pytest.mark.parametrize("name", CASES)
def test_postprocess_smore_volume_reproduces_the_reference_fixture_on_device(name):
    """label_hr bit-exact, img_hr within one fp32 ulp of the volume's largest magnitude, the blurred copies within
    L + 1 of them (the bounds and the printed figures: test_stage1_cpu.check_against_fixture)."""
    c = case(name)
    res = sr.postprocess_smore_volume(c["vol"], float(c["sep"]), _kernel(name), DEV)
    assert all(t.is_cuda and t.is_contiguous() for t in res.values())
    check_against_fixture(name, res)
    again = sr.postprocess_smore_volume(torch.from_numpy(c["vol"]).to(DEV), float(c["sep"]), _kernel(name))
    assert all(torch.equal(again[k], res[k]) for k in res)


@pytest.mark.parametrize("name", CASES)
def test_one_channel_zoom_equals_the_image_of_the_two_channel_zoom(name):
    c = case(name)
    vol = torch.from_numpy(c["vol"]).to(DEV)
    tabs = sr.zoom_taps(vol.shape[2], float(c["sep"]), vol.device)
    img2, lab2 = hb.zoom_depth(vol, *tabs)
    img1, lab1 = hb.zoom_depth(vol[..., :1].contiguous(), *tabs)
    assert lab1 is None and lab2.dtype == torch.uint8
    assert torch.equal(img1.view(torch.int32), img2.view(torch.int32))


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("taps", ["fixture", 19])
def test_blur_to_slices_is_bit_identical_to_the_tap_table_route(name, taps):
    """Both add one fused multiply-add per tap in tap order.  The fixture's profiles have 5 to 9 taps (the 8- and
    16-tap register windows); 19 taps, of both signs and an even count's off-centre split with 18, take the 32-tap one."""
    img = torch.from_numpy(np.ascontiguousarray(G[f"{name}_img_hr"][..., 0])).to(DEV)
    if taps == "fixture":
        ks = [G[f"{name}_kernel"]]
    else:
        rng = np.random.RandomState(taps)
        ks = [(rng.rand(taps) - 0.3).astype(np.float32), (rng.rand(taps - 1) - 0.3).astype(np.float32)]
    for k in ks:
        kd = torch.from_numpy(k).to(DEV)
        fx = _resample(img, 0, blur_taps(img.shape[0], k)).permute(2, 0, 1).contiguous()
        fy = _resample(img, 1, blur_taps(img.shape[1], k)).permute(2, 1, 0).contiguous()
        gx, gy = hb.blur_to_slices(img, kd, 0), hb.blur_to_slices(img, kd, 1)
        assert tuple(gx.shape) == tuple(fx.shape) and tuple(gy.shape) == tuple(fy.shape)
        assert torch.equal(gx.view(torch.int32), fx.view(torch.int32))
        assert torch.equal(gy.view(torch.int32), fy.view(torch.int32))


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_bspline_prefilter_reproduces_spline_filter1d(axis):
    """(9, 70, 6): 9 samples at 256 lines per block, 70 at 64 (the strided kernel's LDS rule), 6 along the contiguous
    axis (the zoom kernel's layout)."""
    x = torch.from_numpy(G["prefilter_x"]).to(DEV)
    want = G[f"prefilter_axis{axis}"]
    got = hb.bspline_prefilter(x, axis).cpu().numpy()
    err = float(np.abs(got - want).max())
    print(f"axis {axis}: max abs error {err:.3e}, bound {ULP * float(np.abs(want).max()):.3e}, "
          f"{int((got != want).sum())} of {want.size} coefficients not bit-equal")
    assert err <= ULP * float(np.abs(want).max())
    assert np.array_equal(hb.bspline_prefilter(x, axis - 3).cpu().numpy(), got)


def test_longest_supported_lines_against_the_cpu_statement():
    """283 samples per line: 64 lines fill the LDS of one workgroup (two blocks here, the second partial); 284 are
    refused.  The CPU statement performs the same fp64 operations in the same order."""
    g = torch.Generator().manual_seed(283)
    vol = torch.cat([torch.rand((3, 30, 283, 1), generator=g) * 1000, (torch.rand((3, 30, 283, 1), generator=g) > 0.5).float()], 3)
    tabs = tuple(torch.from_numpy(t) for t in sr.zoom_taps(283, 2))
    want_img, want_lab = stage1_emu.zoom_depth(vol, *tabs)
    img, lab = hb.zoom_depth(vol.to(DEV), *(t.to(DEV) for t in tabs))
    assert torch.equal(lab.cpu(), want_lab)
    err = float((img.cpu() - want_img).abs().max())
    print(f"n = 283: max abs error {err:.3e}, {int((img.cpu() != want_img).sum())} of {want_img.numel()} not bit-equal")
    assert err <= ULP * float(want_img.abs().max())
    x = vol[..., 0].contiguous()
    for axis in (1, 2):
        xa = x.transpose(axis, 2).contiguous()
        got = hb.bspline_prefilter(xa.to(DEV), axis).cpu()
        want = stage1_emu.bspline_prefilter(xa, axis)
        assert float((got - want).abs().max()) <= ULP * float(want.abs().max())
    with pytest.raises(L.RehrsegHipError, match="ENOSUP"):
        hb.zoom_depth(torch.zeros((2, 2, 284, 1), device=DEV), *(t.to(DEV) for t in sr.zoom_taps(284, 2, "cpu")))


def test_out_of_axis_position_reads_zero_as_ndimage_does():
    """29 slices at separation 3: the last position rounds beyond the axis (utils/sr_utils.py zoom_taps)."""
    g = torch.Generator().manual_seed(29)
    vol = torch.cat([torch.rand((4, 5, 29, 1), generator=g) + 1.0, torch.ones((4, 5, 29, 1))], 3)
    tabs = tuple(torch.from_numpy(t) for t in sr.zoom_taps(29, 3))
    want_img, want_lab = stage1_emu.zoom_depth(vol, *tabs)
    img, lab = hb.zoom_depth(vol.to(DEV), *(t.to(DEV) for t in tabs))
    assert not img[..., -1].any() and not lab[..., -1].any() and lab[..., :-1].all()
    assert torch.equal(lab.cpu(), want_lab) and float((img.cpu() - want_img).abs().max()) <= ULP * float(want_img.abs().max())


def test_data_set_takes_stage1_volumes_without_a_host_round_trip():
    """stage1_volumes -> TrainSetMultiple(volumes=...) under sync debug mode 'error'; the same batch as the data set
    built from the same four arrays as numpy dicts."""
    subjects = [torch.from_numpy(G[f"{n}_vol"]).to(DEV) for n in ("odd", "tie")]
    kernel = _kernel("odd")
    sr.stage1_volumes(subjects, 4, kernel)                               # warm-up: the tables' and the taps' caches
    probe = torch.ones(3, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        raised = False
        try:
            probe.sum().item()
        except RuntimeError:
            raised = True
        assert raised, "this torch build does not raise on a synchronising call in sync debug mode 'error'"
        vols = sr.stage1_volumes(subjects, 4, kernel)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    args = (None, ["a", "b"], 4.0, 1.0, None, None, (16, 16, 1), True, DEV)
    a = TrainSetMultiple(*args, volumes=vols)
    for i, v in enumerate(vols):
        assert a.imgs_hr[i].data_ptr() == v["img_hr"].data_ptr() and a.labels_hr[i].data_ptr() == v["label_hr"].data_ptr()
        assert a.imgs_filtered_x[i].data_ptr() == v["image_x_rgb"].data_ptr()
        assert a.imgs_filtered_y[i].data_ptr() == v["image_y_rgb"].data_ptr()
    b = TrainSetMultiple(*args, volumes=[{k: t.cpu().numpy() for k, t in v.items()} for v in vols])
    random.seed(21)
    pa = a.batch([0, 1])
    random.seed(21)
    pb = b.batch([0, 1])
    assert len(pa) == len(pb) == 2
    for x, y in zip(pa, pb):
        assert x.is_cuda and torch.equal(x.view(torch.int32), y.view(torch.int32))
