"""Stage-1 -> stage-2 handoff on the MI355X: the kernels of csrc/sr_volume.hip one by one against torch / numpy
statements of the reference's code, the whole path against the reference's fixture (tests/golden/handoff_flavr.npz),
the data set fed from device tensors, and the absence of host synchronisation."""
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from rehrseg_amd import hip_backend as hb
from rehrseg_amd.utils import sr_utils as sr
from rehrseg_amd.utils.train_set import TrainSetMultipleSegSREfficient
from test_handoff_cpu import G, check_against_fixture
from test_inference_cpu import _flavr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ----------------------------------------------------------------------------- kernels, exact
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("shape", [(20, 18, 6), (5, 33, 2), (17, 16, 3), (64, 48, 9)])
def test_window_gather_is_bit_equal_to_the_torch_construction(shape, C):
    """Odd in-plane sizes (padding), S = 2 and S = 3 (both end windows), C = 1 and 2, whole and partial ranges."""
    g = torch.Generator().manual_seed(sum(shape) + C)
    vol = (torch.rand(shape + (C,), generator=g) - 0.3).to(DEV)
    image = vol.permute(2, 0, 1, 3).permute(0, 3, 2, 1)                  # lr_axis_to_z(., 0), then (:164): (S, C, y, x)
    image = F.pad(image, (0, (-shape[0]) % 16, 0, (-shape[1]) % 16))
    S = shape[2]
    src = torch.cat([image, torch.zeros_like(image[:1])], 0)            # apply_to_vol_flavr's chain from here on
    idx = torch.tensor(sr._window_indices(S), device=DEV) % (S + 1)
    want = src[idx].permute(0, 2, 1, 4, 3).contiguous()
    got = hb.sr_window_gather(vol, 0, S - 1)
    assert tuple(got.shape) == tuple(want.shape)
    assert got.permute(0, 2, 3, 4, 1).is_contiguous()                   # the network's NDHWC layout: to_cl is a no-op
    assert torch.equal(got.contiguous().view(torch.int32), want.view(torch.int32))
    if S > 4:
        part = hb.sr_window_gather(vol, 3, S - 1 - 3)
        assert torch.equal(part.contiguous().view(torch.int32), want[3:].view(torch.int32))


def _reference_tail(net, vol_min, vol_max):
    """inference_flavr :169-193 in numpy on the network output (n_windows, C, 4, X, Y) -> (img, seg) as written."""
    n, C = net.shape[:2]
    rot = net.transpose(0, 2, 1, 3, 4).reshape(-1, C, net.shape[3], net.shape[4])   # apply_to_vol_flavr's result
    final = rot.transpose(0, 3, 1, 2).astype(np.float32)                             # (:169) + the mean of one angle
    tmp = final - 0                                                                  # inv_normalize(a=0, b=1)
    tmp = tmp * (vol_max - vol_min)
    tmp = tmp / (1 - 0)
    tmp += vol_min
    final = tmp.transpose(2, 0, 1, 3)                                                # z_axis_to_lr_axis(., 0)
    img = final[0].copy()
    s = final[1].copy() if C > 1 else None
    if s is not None:
        s[s > 0] = 1
        s[s < 0] = 0
        s = s.astype("uint8")
    return img, s


@pytest.mark.parametrize("layout", ["channels_last", "contiguous"])
@pytest.mark.parametrize("X,Y", [(20, 18), (64, 48), (70, 129), (7, 5)])
def test_volume_scatter_is_exact_and_tracks_min_max(X, Y, layout):
    g = torch.Generator().manual_seed(X * Y)
    n_windows, b = 5, 2
    Xp, Yp = X + (-X) % 16, Y + (-Y) % 16
    net = (torch.randn(n_windows, 2, 4, Xp, Yp, generator=g) * 0.7)
    net[0, 1, 0, 0, :3] = torch.tensor([0.0, -0.0, 1e-30])               # the sign test at and next to zero
    vol_min, vol_max = np.float32(0.0 if layout == "contiguous" else -3.0), np.float32(1234.5)
    in_mm = hb.minmax(torch.tensor([float(vol_min), 7.0, float(vol_max)], device=DEV))
    dnet = net.to(DEV)
    if layout == "channels_last":
        dnet = dnet.contiguous(memory_format=torch.channels_last_3d)
    img = torch.full((n_windows * 4, Y, X), float("nan"), device=DEV)
    seg = torch.full((n_windows * 4, Y, X), 9, device=DEV, dtype=torch.uint8)
    mm = hb.minmax_new(DEV)
    for w0 in range(0, n_windows, b):
        hb.sr_volume_scatter(dnet[w0:w0 + b], in_mm, w0, img, seg, mm)
    want_img, want_seg = _reference_tail(net.numpy()[:, :, :, :X, :Y], vol_min, vol_max)
    assert np.array_equal(img.cpu().numpy().view(np.int32), want_img.view(np.int32))
    assert np.array_equal(seg.cpu().numpy(), want_seg)
    lo, hi = torch.aminmax(img)
    assert hb.minmax_decode(mm).tolist() == [float(lo), float(hi)]
    # the uncertainty mode: one channel, no label map, its own min / max pair
    unc = torch.empty_like(img)
    mm2 = hb.minmax_new(DEV, 2)
    hb.sr_volume_scatter(dnet[:, 1:2], in_mm, 0, unc, None, mm2[2:4])
    want_unc, _ = _reference_tail(net.numpy()[:, 1:2, :, :X, :Y], vol_min, vol_max)
    assert np.array_equal(unc.cpu().numpy().view(np.int32), want_unc.view(np.int32))
    assert hb.minmax_decode(mm2[2:4]).tolist() == [float(unc.min()), float(unc.max())]
    assert mm2[0:2].tolist() == [-1, 0]                                   # the image's pair was not touched


@pytest.mark.parametrize("n", [1, 3, 4, 1000, 262147])
def test_minmax_equals_aminmax(n):
    g = torch.Generator().manual_seed(n)
    x = (torch.randn(n + 1, generator=g) * 50).to(DEV)
    for t in (x[:n], x[1:]):                                             # 16-byte aligned and not
        lo, hi = torch.aminmax(t)
        assert hb.minmax_decode(hb.minmax(t)).tolist() == [float(lo), float(hi)]


@pytest.mark.parametrize("L", [1, 4, 9, 12, 21])
@pytest.mark.parametrize("shape", [(20, 18, 20), (150, 6, 10), (9, 5, 3)])
def test_stage2_prep_matches_the_conv2d_statement(shape, L):
    """Bound: both sides sum L products k[t] n[t] with 0 <= n <= 255 and positive taps of unit sum in fp32.  A product
    carries a relative error <= 2^-24, every partial sum is <= 255 and each of the L - 1 additions rounds it by
    <= 2^-24 x 255, so either side is within L x 255 x 2^-24 of the exact sum and the two within L x 255 x 2^-23 of each
    other, whatever the order and whether or not conv2d fuses its multiply-adds.  The normalised values n themselves are
    the same three correctly rounded operations on both sides."""
    rng = np.random.RandomState(L + shape[0])
    img = (rng.rand(*shape) * 900 + 17).astype(np.float32)
    k = rng.rand(L).astype(np.float64) + 0.1
    k = (k / k.sum()).astype(np.float32)
    data = (img - np.min(img)) / (np.max(img) - np.min(img))             # zeroonenorm (:279-282)
    data = data * 255.0
    assert data.dtype == np.float32
    it = torch.from_numpy(data.transpose(2, 0, 1)).unsqueeze(1)          # postprocess_flavr (:301-303)
    want = F.conv2d(it, torch.from_numpy(k).view(1, 1, L, 1), padding="same").squeeze(1).numpy().transpose(1, 2, 0)
    dimg = torch.from_numpy(img).to(DEV)
    got = hb.stage2_prep(dimg, hb.minmax(dimg), torch.from_numpy(k).to(DEV)).cpu().numpy()
    err, bound = float(np.abs(got - want).max()), L * 255 * 2.0 ** -23
    print(f"prep {shape} L={L}: max abs error {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    if L == 1:
        assert np.array_equal(got, data * k[0])


def test_uncertainty_cast_wraps_exactly():
    rng = np.random.RandomState(5)
    u = (rng.rand(37, 11, 13) * 41 + 100).astype(np.float32)
    q = (u - np.min(u)) / (np.max(u) - np.min(u))
    q = (q * 255.0) * 255.0                                               # (zeroonenorm(u) * 255.0), up to 65025
    want = (q.astype(np.int32) & 0xFF).astype(np.uint8)                   # .astype('uint8'): truncate, keep 8 bits
    du = torch.from_numpy(u).to(DEV)
    got = hb.stage2_unc_u8(du, hb.minmax(du)).cpu().numpy()
    assert len(np.unique(want)) == 256 and np.array_equal(got, want)
    fu = torch.from_numpy(G["uncertainty"].transpose(2, 1, 0).copy()).to(DEV)   # the reference's own map and cast
    assert np.array_equal(hb.stage2_unc_u8(fu, hb.minmax(fu)).cpu().numpy(), G["post_unc"])


# ----------------------------------------------------------------------------- end to end
def _kernel():
    return torch.from_numpy(G["kernel"]).view(1, 1, -1, 1)


@pytest.mark.parametrize("window_batch", [2, 32])
def test_handoff_reproduces_the_reference_fixture_on_device(window_batch):
    model = _flavr(DEV)
    res = sr.sr_volume_flavr(model, G["vol"], float(G["sep"]), enable_uncertainty=True, window_batch=window_batch)
    assert all(res[k].is_cuda for k in ("img", "seg", "uncertainty", "minmax"))
    assert hb.minmax_decode(res["minmax"]).tolist() == [float(res["img"].min()), float(res["img"].max()),
                                                        float(res["uncertainty"].min()),
                                                        float(res["uncertainty"].max())]
    post = sr.postprocess_flavr_volume(res["img"], res["seg"], _kernel(), res["uncertainty"], res["minmax"])
    absent = sr.postprocess_flavr_volume(res["img"], res["seg"], _kernel())
    assert all(t.is_cuda and t.is_contiguous() for t in post + absent)
    check_against_fixture(res, post, absent)
    # the same batching on both sides: the network's output depends on it in the last bits (test_inference_gpu.py's
    # test_apply_to_vol_flavr_batching_is_invisible allows 1e-5), everything behind it is exact
    vols = sr.stage2_volumes(model, [torch.from_numpy(G["vol"]).to(DEV)], 4, _kernel(), enable_uncertainty=True,
                             window_batch=window_batch)
    assert torch.equal(vols[0]["img"], post[0]) and torch.equal(vols[0]["seg"], post[1])
    assert torch.equal(vols[0]["uncertainty"], post[2])


def test_data_set_takes_device_volumes_without_a_host_round_trip():
    vols_np = [{"img": G["post_img"], "seg": G["post_seg"], "uncertainty": G["post_unc"]},
               {"img": G["post_img"][::-1, :, 2:].copy(), "seg": G["post_seg"][::-1, :, 2:].copy(),
                "uncertainty": G["post_unc"][::-1, :, 2:].copy()}]
    vols_dev = [{k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in d.items()} for d in vols_np]
    args = (None, ["a", "b"], 4.0, 1.0, [8, 8, 2], [8, 8, 2])
    a = TrainSetMultipleSegSREfficient(*args, random_flip=True, uncertainty=True, device=DEV, volumes=vols_np)
    b = TrainSetMultipleSegSREfficient(*args, random_flip=True, uncertainty=True, device=DEV, volumes=vols_dev)
    for i in range(2):
        assert b.labels[i].data_ptr() == vols_dev[i]["seg"].data_ptr()   # used where it lies
    random.seed(12)
    pa = a.batch([0, 1, 1, 0, 0, 1])
    random.seed(12)
    pb = b.batch([0, 1, 1, 0, 0, 1])
    for k in (1, 2, 3):                                                   # from the uint8 volumes: bit-equal
        assert torch.equal(pa[k], pb[k])
    # z = (v - mean) / std with mean and std reduced in fp32 on either side: each reduction of n = 8640 values is good
    # to about log2(n) x 2^-24 relative, so |dz| <= (|d mean| + |z| |d std|) / std + ulp(z) <= 4e-6 (|mean| / std + |z|)
    z = pa[0].abs().max().item()
    img = G["post_img"]
    bound = 4e-6 * (abs(float(img.mean())) / float(img.std()) + z) + 2.0 ** -23 * z
    err = float((pa[0] - pb[0]).abs().max())
    print(f"z-scored patches: max abs difference {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    c = TrainSetMultipleSegSREfficient(*args, uncertainty=True, norm=False, device=DEV, volumes=vols_dev)
    assert c.imgs[0].data_ptr() == vols_dev[0]["img"].data_ptr()


def test_stage2_volumes_makes_no_host_synchronisation():
    model = _flavr(DEV)
    g = torch.Generator().manual_seed(8)
    subjects = [torch.cat([torch.rand(s + (1,), generator=g) * 300, (torch.rand(s + (1,), generator=g) > 0.5).float()],
                          3).to(DEV) for s in ((20, 18, 6), (33, 16, 4))]
    kernel = _kernel()
    sr.stage2_volumes(model, subjects, 4, kernel, enable_uncertainty=True)          # warm-up: caches, workspaces
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
        vols = sr.stage2_volumes(model, subjects, 4, kernel, enable_uncertainty=True)
        ds = TrainSetMultipleSegSREfficient(None, ["a", "b"], 4.0, 1.0, [8, 8, 2], [8, 8, 2], uncertainty=True,
                                            device=DEV, volumes=vols)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(ds) == 2 and tuple(vols[1]["img"].shape) == (33, 16, 12)
    assert torch.isfinite(vols[0]["img"]).all()
