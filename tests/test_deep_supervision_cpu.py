"""Deep supervision on the host: the order-0 index tables of the label pyramid against scipy.ndimage.zoom, the level
weights of `_build_loss(True)`, and DeepSupervisionWrapper's semantics on CPU tensors (the plain Python sum over the
inner loss; the fused device path is tests/test_deep_supervision_gpu.py).

nnunetv2 (DeepSupervisionWrapper) and skimage / batchgenerators (DownsampleSegForDSTransform2) are absent offline:
both are restated from their published behaviour, parity unpinned.  What IS pinned here is the resize rule itself,
against the scipy call skimage's resize(order=0, mode='edge', anti_aliasing=False) makes."""
import numpy as np
import pytest
import torch
from scipy import ndimage

from rehrseg_amd.utils import augment as A
from rehrseg_amd.utils import seg_utils as su

SCALES = sorted({s for lvl in A.DEEP_SUPERVISION_SCALES for s in lvl})   # 1, 0.5, 0.25, 0.125, 0.0625, 0.03125


def _n_out(n_in, scale):
    return int(np.round(n_in * scale))


def test_scale_table_is_the_references():
    assert A.DEEP_SUPERVISION_SCALES == [[1.0, 1.0, 1.0], [1.0, 0.5, 0.5], [1.0, 0.25, 0.25], [0.5, 0.125, 0.125],
                                         [0.25, 0.0625, 0.0625], [0.25, 0.03125, 0.03125]]
    assert len(SCALES) == 6


@pytest.mark.parametrize("scale", SCALES)
def test_index_tables_equal_scipy_zoom(scale):
    checked = 0
    for n_in in range(1, 66):
        n_out = _n_out(n_in, scale)
        if n_out == 0:
            with pytest.raises(ValueError):
                A.zoom_nearest_index(n_in, n_out)
            continue
        ref = ndimage.zoom(np.arange(n_in, dtype=float), n_out / n_in, order=0, mode="nearest", grid_mode=True)
        got = A.zoom_nearest_index(n_in, n_out)
        assert got.dtype == np.int32 and got.shape == (n_out,) == ref.shape
        assert np.array_equal(got.astype(float), ref), (n_in, n_out, got, ref)
        checked += 1
    assert checked >= 34     # the smallest scale, 1/32, leaves a voxel from n_in = 17 on


def test_extents_round_half_to_even():
    assert A.pyramid_extents((5, 14, 6), [[0.5, 0.25, 0.25]]) == [(2, 4, 2)]      # 2.5 -> 2, 3.5 -> 4, 1.5 -> 2
    assert A.pyramid_extents((14, 320, 384), A.DEEP_SUPERVISION_SCALES) == [
        (14, 320, 384), (14, 160, 192), (14, 80, 96), (7, 40, 48), (4, 20, 24), (4, 10, 12)]
    assert A.pyramid_extents((8, 8, 8), [0.5]) == [(4, 4, 4)]
    with pytest.raises(ValueError):
        A.pyramid_extents((1, 32, 32), [[0.25, 1, 1]])        # 0.25 -> 0 voxels
    with pytest.raises(ValueError):
        A.zoom_nearest_index(8, 0)
    assert _n_out(5, 0.5) == 2 and _n_out(14, 0.25) == 4


def test_get_training_transforms_accepts_the_scales():
    rot = {"x": (-np.pi, np.pi), "y": (0, 0), "z": (0, 0)}
    tr = A.get_training_transforms([3, 24, 32], rot, [list(s) for s in A.DEEP_SUPERVISION_SCALES], None, True,
                                   use_mask_for_norm=[False], enable_uncertainty=True,
                                   extra_keys=["seg", "seg_sr", "uncertainty"])
    assert tr.pyramid.ds_scales == A.DEEP_SUPERVISION_SCALES and tr.pyramid.also == ("uncertainty",)
    # like every other argument of this function: what REHRSeg passes (None or its one table, whose level weights
    # _build_loss hard-codes), nothing else
    for other in (A.DEEP_SUPERVISION_SCALES[:3], [[1, 1, 1]], [1, 0.5], A.DEEP_SUPERVISION_SCALES + [[0.5, 0.5, 0.5]]):
        with pytest.raises(NotImplementedError, match="reference's table"):
            A.get_training_transforms([3, 24, 32], rot, other, None, True, use_mask_for_norm=[False])
    plain = A.get_training_transforms([3, 24, 32], rot, None, None, True, use_mask_for_norm=[False])
    assert plain.pyramid is None
    # the pyramid step draws nothing: the parameter draws of an item are the same with and without it
    np.random.seed(11)
    a = tr.draw(3)
    np.random.seed(11)
    b = A.get_training_transforms([3, 24, 32], rot, None, None, True, use_mask_for_norm=[False], enable_uncertainty=True,
                                  extra_keys=["seg", "seg_sr", "uncertainty"]).draw(3)
    assert repr(a) == repr(b)


def test_build_loss_weights():
    loss = su._build_loss(True)
    assert isinstance(loss, su.DeepSupervisionWrapper) and isinstance(loss.loss, su.DC_and_weighted_CE_loss)
    deep_supervision_scales = [[1.0, 1.0, 1.0], [1.0, 0.5, 0.5], [1.0, 0.25, 0.25], [0.5, 0.125, 0.125],
                               [0.25, 0.0625, 0.0625], [0.25, 0.03125, 0.03125]]
    weights = np.array([1 / (2 ** i) for i in range(len(deep_supervision_scales))])
    weights[-1] = 0
    weights = weights / weights.sum()
    assert loss.weight_factors == tuple(float(w) for w in weights)
    assert loss.weight_factors[-1] == 0.0 and abs(sum(loss.weight_factors) - 1.0) < 1e-15
    assert su._build_loss(True, weight_dice=0).loss.weight_dice == 0
    assert isinstance(su._build_loss(False), su.DC_and_weighted_CE_loss)


DIMS = [(4, 16, 16), (4, 8, 8), (2, 4, 4)]


def _levels(n_logits=3, n_labels=3, N=2, C=2, seed=5):
    g = torch.Generator().manual_seed(seed)
    logits = [torch.randn((N, C) + d, generator=g, dtype=torch.float64).requires_grad_(True) for d in DIMS[:n_logits]]
    labels = [torch.randint(0, C, (N, 1) + d, generator=g).double() for d in DIMS[:n_labels]]
    uncs = [1 - torch.rand((N, 1) + d, generator=g, dtype=torch.float64) * 0.99 for d in DIMS[:n_labels]]
    return logits, labels, uncs


@pytest.mark.parametrize("with_unc", [False, True])
def test_wrapper_equals_the_weighted_sum(with_unc):
    w = (0.5, 0.3, 0.2)
    inner = su._build_loss(False)
    wrap = su.DeepSupervisionWrapper(inner, w)
    logits, labels, uncs = _levels()
    got = wrap(logits, labels, uncs) if with_unc else wrap(logits, labels)
    ref = sum(w[i] * inner(logits[i].detach(), labels[i], uncs[i] if with_unc else None) for i in range(3))
    assert got.dtype == torch.float64 and abs(got.item() - ref.item()) <= 1e-14 * abs(ref.item())
    got.backward()
    for i in range(3):
        x = logits[i].detach().clone().requires_grad_(True)
        (w[i] * inner(x, labels[i], uncs[i] if with_unc else None)).backward()
        assert torch.allclose(logits[i].grad, x.grad, rtol=1e-13, atol=0)
    # the step's `loss(seg, label, None)` form: a trailing None is no argument
    assert wrap(logits, labels, None).item() == wrap(logits, labels).item()


def test_wrapper_truncates_like_zip():
    """The reference's six weights meet fewer outputs and a longer label list: the shortest list decides."""
    wrap = su._build_loss(True)
    logits, labels, _ = _levels(n_logits=2, n_labels=3)
    got = wrap(logits, labels)
    w = wrap.weight_factors
    ref = sum(w[i] * wrap.loss(logits[i].detach(), labels[i]) for i in range(2))
    assert abs(got.item() - ref.item()) <= 1e-14 * abs(ref.item())
    with pytest.raises(ValueError):
        su.DeepSupervisionWrapper(wrap.loss, (1.0,))(logits, labels)        # more levels than weight factors


def test_wrapper_skips_zero_weights():
    wrap = su.DeepSupervisionWrapper(su._build_loss(False), (1.0, 0.0, 0.25))
    logits, labels, _ = _levels()
    wrap(logits, labels).backward()
    assert logits[1].grad is None                      # not evaluated: None, not zeros
    assert logits[0].grad is not None and logits[2].grad is not None and float(logits[2].grad.abs().max()) > 0
    with pytest.raises(ValueError):
        su.DeepSupervisionWrapper(su._build_loss(False), (0.0, 0.0))


def test_wrapper_refuses_a_bare_uncertainty_tensor():
    wrap = su._build_loss(True)
    logits, labels, uncs = _levels()
    with pytest.raises(TypeError, match="list or tuple"):
        wrap(logits, labels, uncs[0])
    with pytest.raises(TypeError, match="list or tuple"):
        wrap(logits[0], labels[0])


def test_wrapper_names_both_shapes_on_an_extent_mismatch():
    wrap = su._build_loss(True)
    logits, labels, _ = _levels()
    labels[1] = labels[2]
    with pytest.raises(ValueError, match=r"\(2, 2, 4, 8, 8\).*\(2, 1, 2, 4, 4\)"):
        wrap(logits, labels)


def test_entry_points_reject_malformed_levels_without_launching():
    """REHR_EINVAL (-1) / REHR_ENOSUP (-2) are returned before any launch (dummy pointers nothing dereferences): every
    call below is malformed for the entry point it reaches, so none of them can launch where there is a device."""
    import ctypes as C
    from rehrseg_amd import lib as L
    lib = L.load()

    def level(**over):
        lv = L.SegDsLevel()
        lv.logits, lv.target, lv.dlogits = 0x1000, 0x2000, 0x3000
        lv.S, lv.d, lv.h, lv.w, lv.ld, lv.ldd, lv.weight = 24, 2, 3, 4, 2, 2, 1.0
        for k, v in over.items():
            setattr(lv, k, v)
        return lv

    def both(levels, n, N=2, Cc=2, stats=0x4000, go=0x5000):
        arr = (L.SegDsLevel * len(levels))(*levels)
        return (lib.rehr_seg_loss_ds_fwd_f32(arr, n, N, Cc, stats, None),
                lib.rehr_seg_loss_ds_bwd_f32(arr, n, N, Cc, stats, 1.0, 1.0, 1e-5, 0, go, None))

    assert both([level()] * 9, 9) == (-1, -1)                       # more than 8 levels
    assert both([level()], 0) == (-1, -1)
    assert both([level(S=23)], 1) == (-1, -1)                       # S is not d * h * w
    assert both([level(logits=None)], 1) == (-1, -1)
    assert both([level(target=None)], 1) == (-1, -1)
    assert both([level(ld=1)], 1) == (-1, -1)
    assert both([level(weight=0.0)], 1) == (-1, -1)                 # nothing carries a weight
    assert both([level()], 1, Cc=5) == (-2, -2) and both([level()], 1, Cc=1) == (-2, -2)
    assert both([level()], 1, stats=None) == (-1, -1)
    one = (L.SegDsLevel * 1)(level())
    assert lib.rehr_seg_loss_ds_bwd_f32(one, 1, 2, 2, 0x4000, 1.0, 1.0, 1e-5, 0, None, None) == -1     # null grad_out
    one = (L.SegDsLevel * 1)(level(dlogits=None))
    assert lib.rehr_seg_loss_ds_bwd_f32(one, 1, 2, 2, 0x4000, 1.0, 1.0, 1e-5, 0, 0x5000, None) == -1   # bwd only
    one = (L.SegDsLevel * 1)(level(ldd=1))
    assert lib.rehr_seg_loss_ds_bwd_f32(one, 1, 2, 2, 0x4000, 1.0, 1.0, 1e-5, 0, 0x5000, None) == -1
    # a skipped level is not looked at: its nonsense does not make the list malformed (the weighted one still does)
    assert both([level(weight=0.0, S=-5, logits=None), level(S=23)], 2) == (-1, -1)
    p = L.PyramidLevel()
    p.dst, p.iz, p.iy, p.ix, p.d, p.h, p.w = 0x1000, 0x2000, 0x3000, 0x4000, 1, 2, 3
    arr = (L.PyramidLevel * 9)(*[p] * 9)
    assert lib.rehr_label_pyramid_f32(None, 1, 2, 3, 4, arr, 1, None) == -1
    assert lib.rehr_label_pyramid_f32(0x9000, 1, 2, 3, 4, arr, 9, None) == -1
    assert lib.rehr_label_pyramid_f32(0x9000, 1, 2, 3, 4, arr, 0, None) == -1
    assert lib.rehr_label_pyramid_f32(0x9000, 0, 2, 3, 4, arr, 1, None) == -1
    q = L.PyramidLevel()
    q.dst, q.iz, q.iy, q.d, q.h, q.w = 0x1000, 0x2000, 0x3000, 1, 2, 3      # ix missing
    assert lib.rehr_label_pyramid_f32(0x9000, 1, 2, 3, 4, (L.PyramidLevel * 1)(q), 1, None) == -1
    assert C.sizeof(L.SegDsLevel) == 64 and C.sizeof(L.PyramidLevel) == 48
