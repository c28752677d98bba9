"""Stage-1 -> stage-2 handoff without a GPU: the five new C-ABI symbols, and the host logic of sr_volume_flavr /
postprocess_flavr_volume / the reference-named wrappers over the CPU statement of their kernels (tests/handoff_emu.py,
the network through tests/emu_backend.py) against the reference's own outputs (tests/golden/handoff_flavr.npz, written
by tools/gen_golden_handoff.py)."""
import os

import numpy as np
import pytest
import torch

from rehrseg_amd import lib as L
from rehrseg_amd import ops
from rehrseg_amd.utils import sr_utils as sr
from test_inference_cpu import _flavr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "handoff_flavr.npz"))
NEW_SYMBOLS = ("rehr_minmax_f32", "rehr_sr_window_gather_f32", "rehr_sr_volume_scatter_f32", "rehr_stage2_prep_f32",
               "rehr_stage2_unc_u8_f32")
REL_BAR = 1e-4   # tests/test_inference_gpu.py's bar on the network output, relative to its largest magnitude


def image_bar():
    """The network-output bar carried through inv_normalize: x (orig_max - orig_min)."""
    return REL_BAR * float(G["net_absmax"]) * float(G["vol"].max() - G["vol"].min())


def check_against_fixture(res, post, post_absent):
    """res: sr_volume_flavr's dict; post / post_absent: postprocess_flavr_volume with / without the uncertainty map."""
    bar = image_bar()
    img, seg, unc = (res[k].cpu().numpy() for k in ("img", "seg", "uncertainty"))
    assert img.shape == G["img"].shape and img.dtype == np.float32 and seg.dtype == np.uint8
    err = float(np.abs(img - G["img"]).max())
    print(f"image: max abs error {err:.3e}, bar {bar:.3e}")
    assert err <= bar
    sure = np.abs(G["seg_pre"]) > bar
    print(f"labels: {float((~sure).mean()):.4%} of the voxels within the bar of 0, "
          f"{int((seg != G['seg'])[sure].sum())} of the others differ")
    assert float((~sure).mean()) <= 0.01
    assert np.array_equal(seg[sure], G["seg"][sure])
    uerr = float(np.abs(unc - G["uncertainty"]).max())
    print(f"uncertainty: max abs error {uerr:.3e}")
    assert uerr <= bar
    image, label, u8 = (t.cpu().numpy() for t in post)
    assert image.shape == G["post_img"].shape and label.dtype == np.uint8 and u8.dtype == np.uint8
    # the prepared image is 255 (v - min) / (max - min) blurred by a unit-sum profile: the image bar x 255 / (max - min)
    # would be the propagated error; the issue sets the looser "same bar x 255" and that is what is asserted
    perr = float(np.abs(image - G["post_img"]).max())
    print(f"prepared image: max abs error {perr:.3e}, bar {bar * 255:.3e}")
    assert perr <= bar * 255
    sure_xyz = sure.transpose(2, 1, 0)
    assert np.array_equal(label[sure_xyz], G["post_seg"][sure_xyz])
    assert not post_absent[2].cpu().numpy().any() and post_absent[2].dtype == torch.uint8
    assert torch.equal(post_absent[0], post[0]) and torch.equal(post_absent[1], post[1])
    return u8


@pytest.fixture
def hemu():
    import handoff_emu as E
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
    import ctypes
    lib = L.load()
    strides = (ctypes.c_int64 * 5)(1, 1, 1, 1, 1)
    assert lib.rehr_minmax_f32(None, 4, None, None) == -1
    assert lib.rehr_sr_window_gather_f32(None, None, 16, 16, 4, 2, 0, 1, 16, 16, None) == -1
    assert lib.rehr_sr_volume_scatter_f32(None, strides, 1, 2, 4, 16, 16, 0, 3, None, None, None, None, None) == -1
    assert lib.rehr_stage2_prep_f32(None, None, None, 3, None, 4, 4, None) == -1
    assert lib.rehr_stage2_unc_u8_f32(None, None, None, 4, None) == -1


def test_malformed_arguments_are_rejected_before_any_launch():
    """Non-null but inconsistent arguments (host addresses that are never dereferenced: every call returns first)."""
    import ctypes
    lib = L.load()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    strides = (ctypes.c_int64 * 5)(1, 1, 1, 1, 1)
    assert lib.rehr_sr_window_gather_f32(p, p, 16, 16, 4, 3, 0, 1, 16, 16, None) == -1     # C = 3
    assert lib.rehr_sr_window_gather_f32(p, p, 16, 16, 4, 2, 2, 2, 16, 16, None) == -1     # windows [2, 4) of 3
    assert lib.rehr_sr_window_gather_f32(p, p, 17, 16, 4, 2, 0, 1, 16, 16, None) == -1     # Xp < X
    assert lib.rehr_sr_window_gather_f32(p, p, 16, 16, 4, 2, 0, 1, 16, 24, None) == -1     # Yp % 16
    assert lib.rehr_sr_volume_scatter_f32(p, strides, 2, 2, 4, 16, 16, 2, 3, p, p, p, p, None) == -1   # beyond n_windows
    assert lib.rehr_sr_volume_scatter_f32(p, strides, 1, 1, 4, 16, 16, 0, 3, p, p, p, p, None) == -1   # seg with C = 1
    assert lib.rehr_stage2_prep_f32(p, p, p, 3, p, 4, 4, None) == -1                        # in place
    assert lib.rehr_stage2_prep_f32(p, p, p, 33, ctypes.c_void_p(p.value + 64), 4, 4, None) == -2   # L > 32
    assert lib.rehr_minmax_f32(p, 0, p, None) == -1


def test_minmax_codes_order_like_floats(hemu):
    vals = torch.tensor([-3.5, -0.0, 0.0, 1e-30, 2.0, 7.25])
    codes = hemu._encode(vals).to(torch.int64) & 0xFFFFFFFF
    assert torch.equal(torch.argsort(codes, stable=True), torch.arange(6))
    from rehrseg_amd import hip_backend as hb
    assert torch.equal(hb.minmax_decode(hemu._encode(vals)), vals)
    mm = hemu.minmax(torch.tensor([[3.0, -2.0], [5.0, 4.0]]))
    hemu.minmax(torch.tensor([9.0, 0.5]), out=mm)
    assert hb.minmax_decode(mm).tolist() == [-2.0, 9.0]


def test_window_gather_statement_equals_apply_to_vol_construction(hemu):
    """handoff_emu's gather == the torch chain of apply_to_vol_flavr on the reference's orientation of the volume."""
    for shape in ((20, 18, 6, 2), (5, 33, 2, 2), (17, 16, 3, 2)):
        vol = torch.rand(shape)
        image = vol.permute(2, 0, 1, 3).permute(0, 3, 2, 1)              # lr_axis_to_z(., 0), then (:164)
        image = torch.nn.functional.pad(image, (0, (-shape[0]) % 16, 0, (-shape[1]) % 16))
        S = shape[2]
        src = torch.cat([image, torch.zeros_like(image[:1])], 0)
        idx = torch.tensor(sr._window_indices(S)) % (S + 1)
        want = src[idx].permute(0, 2, 1, 4, 3)
        got = hemu.sr_window_gather(vol, 0, S - 1)
        assert torch.equal(got, want)
        if S > 3:
            assert torch.equal(hemu.sr_window_gather(vol, 2, 2), want[2:4])


def test_handoff_reproduces_the_reference_fixture(hemu):
    model = _flavr()
    res = sr.sr_volume_flavr(model, G["vol"], float(G["sep"]), enable_uncertainty=True, window_batch=2)
    from rehrseg_amd import hip_backend as hb
    mm = hb.minmax_decode(res["minmax"])
    assert mm.tolist() == [float(res["img"].min()), float(res["img"].max()), float(res["uncertainty"].min()),
                           float(res["uncertainty"].max())]
    post = sr.postprocess_flavr_volume(res["img"], res["seg"], torch.from_numpy(G["kernel"]).view(1, 1, -1, 1),
                                       res["uncertainty"], res["minmax"])
    absent = sr.postprocess_flavr_volume(res["img"], res["seg"], G["kernel"])
    u8 = check_against_fixture(res, post, absent)
    # uint8 uncertainty: exact wherever the float map agrees with the reference's bit for bit; on this fixture's input
    # written by the reference itself, exact everywhere
    same = (res["uncertainty"].numpy() == G["uncertainty"]).transpose(2, 1, 0)
    lo, hi = res["uncertainty"].numpy().min(), res["uncertainty"].numpy().max()
    if lo == G["uncertainty"].min() and hi == G["uncertainty"].max():
        assert np.array_equal(u8[same], G["post_unc"][same])
    own = hemu.stage2_unc_u8(torch.from_numpy(G["uncertainty"].transpose(2, 1, 0).copy()),
                             hemu.minmax(torch.from_numpy(G["uncertainty"])))
    assert np.array_equal(own.numpy(), G["post_unc"])


def test_prep_statement_reproduces_postprocess_on_the_reference_image(hemu):
    """The fixture's own written image through the prep contract: only the blur's summation order separates the two."""
    img = torch.from_numpy(G["img"])
    image, label, unc = sr.postprocess_flavr_volume(img, torch.from_numpy(G["seg"]), G["kernel"])
    L_ = G["kernel"].size
    # L products of values <= 255 with taps summing to 1, accumulated in fp32 in either order: <= L ulp(255) each way
    assert float((image - torch.from_numpy(G["post_img"])).abs().max()) <= 2 * L_ * 255 * 2.0 ** -23
    assert np.array_equal(label.numpy(), G["post_seg"]) and not unc.any()


def test_non_integral_separation_raises(hemu):
    with pytest.raises(ValueError):
        sr.sr_volume_flavr(_flavr(), G["vol"], 2.5)
    with pytest.raises(ValueError):
        sr.inference_flavr(_flavr(), "img+seg", G["vol"], None, {}, 5.0, 2.0, "cpu", False)


def test_reference_named_wrappers_round_trip_through_a_dict(hemu):
    model, store = _flavr(), {}
    sr.inference_flavr(model, "img+seg", G["vol"], "ref.nii.gz", store, 4.0, 1.0, "cpu", False)
    assert sorted(store) == ["_img", "_seg"]
    image0, label0, unc0 = sr.postprocess_flavr("case.nii.gz", 4, store)
    assert not unc0.any()
    sr.inference_flavr(model, "uncertainty", G["vol"], "ref.nii.gz", store, 4.0, 1.0, "cpu", True)
    assert sorted(store) == ["_img", "_seg", "_uncertainty"]
    image, label, unc = sr.postprocess_flavr("case.nii.gz", 4, store)
    assert torch.equal(image, image0) and torch.equal(label, label0)
    res = {"img": store["_img"], "seg": store["_seg"], "uncertainty": store["_uncertainty"]}
    check_against_fixture(res, (image, label, unc), (image0, label0, unc0))
    with pytest.raises(ImportError, match="SimpleITK"):
        sr.inference_flavr(model, "img+seg", "case.nii.gz", "ref.nii.gz", store, 4.0, 1.0, "cpu", False)
    with pytest.raises(ImportError, match="nibabel"):
        sr.postprocess_flavr("case.nii.gz", 4, "out_dir")
