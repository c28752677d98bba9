"""tests/guarded_alloc.py proven on host tensors (devices=("cpu",)): the overruns, the unwritten element and the
out-of-range read that test_conv_guard_gpu.py relies on it to report are each staged here with plain tensor writes, so
nobody needs a broken kernel on a device to trust the helper."""
import struct

import pytest
import torch

import guarded_alloc
from guarded_alloc import FILL, GUARD, Guarded
from rehrseg_amd import hip_backend

CPU = ("cpu",)


def _past(t, k=0):
    """The element k places past the end of dense 1-D tensor t (k < 0: -k places before its start), as a view."""
    return t.as_strided((1,), (1,), t.storage_offset() + (t.numel() + k if k >= 0 else k))


def test_fill_word_reads_as_nan_in_fp32_and_in_both_bf16_halves():
    w = torch.tensor([FILL], dtype=torch.int32)
    assert bool(torch.isnan(w.view(torch.float32)).all())
    assert bool(torch.isnan(w.view(torch.bfloat16)).all()) and w.view(torch.bfloat16).numel() == 2
    # (an fp64 has 11 exponent bits: two fill words read as 3.0e307 there -- finite, and no sum survives it unnoticed)
    assert float(torch.tensor([FILL, FILL], dtype=torch.int32).view(torch.float64)) > 1e307
    assert struct.unpack("<f", struct.pack("<I", FILL))[0] != struct.unpack("<f", struct.pack("<I", FILL))[0]
    assert GUARD == 128 * 128 * 4


def test_untouched_allocations_pass_and_are_poisoned():
    with Guarded(devices=CPU) as ga:
        a = torch.empty(5, 3, dtype=torch.float32, device="cpu")
        b = torch.empty(7, dtype=torch.bfloat16, device="cpu")
        c = torch.empty_like(a)
        d = torch.empty(0, dtype=torch.uint8, device="cpu")
        e = torch.empty(13, dtype=torch.uint8, device="cpu")      # the back guard starts at an odd byte
        assert ga.check() == 5
    for t in (a, b, c):
        assert bool(torch.isnan(t).all())
    assert d.numel() == 0 and bool((e.view(torch.uint8) == torch.tensor([0xC5, 0x7F] * 7)[:13]).all())
    assert all(t.data_ptr() % 16 == 0 for t in (a, b, c, e))


def test_a_write_one_element_past_the_payload_is_reported():
    with Guarded(devices=CPU) as ga:
        y = torch.empty(6, dtype=torch.float32, device="cpu")
        y.fill_(1.0)
        ga.check()
        _past(y)[0] = 1.0
        with pytest.raises(AssertionError, match=r"guard after the torch.float32 allocation of shape \(6,\) changed 0 bytes past"):
            ga.check()


def test_a_write_one_element_before_the_payload_is_reported():
    with Guarded(devices=CPU) as ga:
        torch.empty(4, dtype=torch.float32, device="cpu")
        y = torch.empty((2, 3), dtype=torch.bfloat16, device="cpu")
        y.fill_(1.0)
        _past(y.view(-1), -1)[0] = 0.5
        msg = r"guard before the torch.bfloat16 allocation of shape \(2, 3\) changed 2 bytes before"
        with pytest.raises(AssertionError, match=msg):
            ga.check()


def test_one_flipped_bit_at_the_far_end_of_the_guard_is_seen():
    """The last byte of the back guard, changed in one bit: the guards are compared byte by byte, to their end."""
    with Guarded(devices=CPU) as ga:
        y = torch.empty(3, dtype=torch.uint8, device="cpu")
        far = y.as_strided((1,), (1,), y.storage_offset() + 3 + GUARD + 12)       # the last byte of the buffer
        far[0] = int(far[0]) ^ 1
        with pytest.raises(AssertionError, match=rf"changed {GUARD + 12} bytes past its end"):
            ga.check()


def test_an_unwritten_element_shows_as_nan():
    with Guarded(devices=CPU) as ga:
        y = torch.empty(9, dtype=torch.float32, device="cpu")
        y[:8] = torch.arange(8.0)                      # a ragged last tile that leaves a row out
        ga.check()
    assert int(torch.isnan(y).sum()) == 1 and bool(torch.isnan(y[8]))


def test_a_read_past_the_end_poisons_a_sum():
    with Guarded(devices=CPU) as ga:
        x = ga.guarded(torch.arange(6.0), device="cpu")
        assert torch.equal(x, torch.arange(6.0)) and float(x.sum()) == 15.0
        wide = x.as_strided((7,), (1,))                # one element too many
        assert bool(torch.isnan(wide.sum()))
        before = x.as_strided((7,), (1,), x.storage_offset() - 1)
        assert bool(torch.isnan((before * 0.0).sum()))   # 0 x NaN stays NaN
        ga.check()                                     # reading changes nothing


def test_zeros_payloads_are_zero_between_nan_guards():
    with Guarded(devices=CPU) as ga:
        z = torch.zeros((3, 5, 2), dtype=torch.float64, device="cpu")
        assert bool((z == 0).all()) and z.dtype == torch.float64 and z.is_contiguous()
        assert float(_past(z.view(-1))) > 1e307 and float(_past(z.view(-1), -1)) > 1e307      # fp64: the fill is 3.0e307
        f = torch.zeros(5, dtype=torch.float32, device="cpu")
        assert bool((f == 0).all()) and bool(torch.isnan(_past(f)).all()) and bool(torch.isnan(_past(f, -1)).all())
        ga.check()


@pytest.mark.parametrize("skew", [0, 16])
def test_shapes_strides_and_alignment_equal_the_real_calls(skew):
    real_empty, real_like = torch.empty, torch.empty_like
    shape = (2, 6, 3, 4, 5)
    src = real_empty(shape).permute(0, 2, 1, 3, 4)       # a non-contiguous source for empty_like
    with Guarded(skew=skew, devices=CPU) as ga:
        for kw in (dict(memory_format=torch.channels_last_3d), dict(memory_format=torch.contiguous_format), {}):
            got = torch.empty(shape, dtype=torch.float32, device="cpu", **kw)
            want = real_empty(shape, dtype=torch.float32, device="cpu", **kw)
            assert got.shape == want.shape and got.stride() == want.stride() and got.dtype == want.dtype, kw
            assert got.is_contiguous(**kw) if kw else got.is_contiguous()
        got = torch.empty(*shape[:3], dtype=torch.bfloat16, device=torch.device("cpu"))     # sizes as varargs
        assert tuple(got.shape) == shape[:3] and got.dtype == torch.bfloat16
        for kw in (dict(memory_format=torch.contiguous_format), dict(memory_format=torch.preserve_format), {},
                   dict(dtype=torch.float64)):
            got, want = torch.empty_like(src, **kw), real_like(src, **kw)
            assert got.shape == want.shape and got.stride() == want.stride() and got.dtype == want.dtype, kw
        cl = torch.empty_like(real_empty(shape, memory_format=torch.channels_last_3d))
        assert cl.is_contiguous(memory_format=torch.channels_last_3d) and cl.permute(0, 2, 3, 4, 1).is_contiguous()
        for flat, lo, hi, _, _ in ga.allocs:
            assert lo == GUARD + skew and (flat.data_ptr() + lo) % 16 == 0
            assert flat.numel() - hi >= GUARD
        part = torch.empty((4, 8), dtype=torch.float32, device="cpu")[1:3]      # a slice (the split-K slabs) stays inside
        part.fill_(2.0)
        assert ga.check() == len(ga.allocs)
    assert torch.empty(3).device.type == "cpu"


def test_other_devices_and_default_device_calls_are_left_alone():
    with Guarded() as ga:                                # wraps "cuda" only
        t = torch.empty(4, device="cpu")
        u = torch.zeros(4)
        v = torch.empty_like(u)
        assert not ga.allocs and bool((u == 0).all()) and t.shape == v.shape


def test_torch_and_the_backend_globals_are_restored_also_when_the_body_raises():
    saved = (torch.empty, torch.empty_like, torch.zeros, hip_backend._ZERO_CHUNK, hip_backend._zero_pool)
    marker = object()
    hip_backend._zero_pool["marker"] = marker
    hip_backend._forms["stale"] = marker
    try:
        with Guarded(devices=CPU):
            assert torch.empty is not saved[0] and torch.zeros is not saved[2] and torch.empty_like is not saved[1]
            assert hip_backend._ZERO_CHUNK == 0 and hip_backend._zero_pool == {} and not hip_backend._forms
            hip_backend._forms["inside"] = marker
        assert (torch.empty, torch.empty_like, torch.zeros, hip_backend._ZERO_CHUNK, hip_backend._zero_pool) == saved
        assert hip_backend._zero_pool["marker"] is marker and not hip_backend._forms
        with pytest.raises(KeyError):
            with Guarded(devices=CPU):
                raise KeyError("body")
        assert (torch.empty, torch.empty_like, torch.zeros, hip_backend._ZERO_CHUNK, hip_backend._zero_pool) == saved
        assert hip_backend._zero_pool["marker"] is marker
    finally:
        hip_backend._zero_pool.pop("marker", None)
        hip_backend._forms.clear()


def test_the_pooled_accumulators_come_through_the_wrapper():
    with Guarded(devices=CPU) as ga:
        s = hip_backend.zeros_f64((2, 3, 2), torch.device("cpu"))
        assert len(ga.allocs) == 1 and ga.allocs[0][3] == (2, 3, 2) and ga.allocs[0][4] == torch.float64
        assert bool((s == 0).all()) and hip_backend._zero_pool == {}
        ga.check()


def test_guarded_keeps_values_layout_and_guards():
    src = torch.randn(2, 4, 3, 5, 6).contiguous(memory_format=torch.channels_last_3d)
    with Guarded(skew=16, devices=CPU) as ga:
        x = ga.guarded(src, device="cpu")
        assert torch.equal(x, src) and x.stride() == src.stride() and x.data_ptr() % 16 == 0
        assert bool(torch.isnan(_past(x.permute(0, 2, 3, 4, 1).reshape(-1))).all())
        ga.check()
    with pytest.raises(RuntimeError):
        ga.guarded(src, device="cpu")                    # outside the context nothing would be checked
    assert guarded_alloc.FILL == 0x7FC57FC5
