"""Stage-1 validation without a GPU: the three new C-ABI symbols and their argument checks, the launch layer's
refusals, the CPU statement of the kernel (tests/sr_metrics_emu.py) against the fp64 oracle (tests/sr_metrics_cases.py,
where the tolerances are derived), sr_quality's arithmetic and validate_sr's host logic over the CPU statement."""
import ctypes
import math
import random

import numpy as np
import pytest
import torch

import sr_metrics_cases as sc
from rehrseg_amd import lib as L
from rehrseg_amd import ops
from rehrseg_amd.utils import sr_utils as sr

NEW_SYMBOLS = ("rehr_sr_metrics_workspace_bytes", "rehr_sr_metrics_f32", "rehr_sr_metrics_bf16")


@pytest.fixture
def memu():
    import sr_metrics_emu as E
    old = ops.set_backend(E)
    yield E
    ops.set_backend(old)


def test_new_symbols_are_declared_and_exported():
    lib = L.load()
    declared = L.declared_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared and s in L.PROTOTYPES and hasattr(lib, s), s
    assert L.ABI_VERSION == 6 and lib.rehr_abi_version() == 6


def test_workspace_query():
    lib = L.load()
    q = lib.rehr_sr_metrics_workspace_bytes
    assert q(1, 1, 11, 11) > 0 and q(2, 4, 128, 128) == 2 * q(1, 4, 128, 128) == 8 * q(1, 1, 128, 128)
    assert q(1, 1, 33, 32) == 2 * q(1, 1, 32, 32) == q(1, 1, 32, 33)      # a ragged row / column of tiles counts
    for bad in ((0, 1, 11, 11), (1, 0, 11, 11), (1, 1, 0, 11), (1, 1, 11, -1)):
        assert q(*bad) == -1, bad
    assert q(1, 1, 10, 11) == -2 and q(1, 1, 11, 10) == -2


@pytest.mark.parametrize("fn", ["rehr_sr_metrics_f32", "rehr_sr_metrics_bf16"])
def test_malformed_arguments_are_rejected_before_any_launch(fn):
    """Host addresses that are never dereferenced by a kernel: every call returns before a launch (the library loads
    and answers without a GPU)."""
    lib = L.load()
    f = getattr(lib, fn)
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    st = (ctypes.c_int64 * 4)(121, 121, 11, 1)
    neg = (ctypes.c_int64 * 4)(121, 121, -11, 1)
    need = lib.rehr_sr_metrics_workspace_bytes(1, 1, 11, 11)

    def call(pred=p, ps=st, tgt=p, ts=st, sl=None, ls=None, sg=None, gs=None, dims=(1, 1, 11, 11), rng=1.0, out=p, ws=p,
             nbytes=need):
        return f(pred, ps, tgt, ts, sl, ls, sg, gs, *dims, rng, out, ws, nbytes, None)

    assert call(pred=None) == -1 and call(ps=None) == -1 and call(tgt=None) == -1 and call(ts=None) == -1
    assert call(out=None) == -1 and call(ws=None) == -1
    assert call(sl=p, ls=st) == -1 and call(sg=p, gs=st) == -1            # half a segmentation pair
    assert call(sl=p, ls=None, sg=p, gs=st) == -1 and call(sl=p, ls=st, sg=p, gs=None) == -1
    for dims in ((0, 1, 11, 11), (1, 0, 11, 11), (1, 1, 0, 11), (1, 1, 11, 0), (-1, 1, 11, 11)):
        assert call(dims=dims) == -1, dims
    assert call(rng=0.0) == -1 and call(rng=-1.0) == -1 and call(rng=float("nan")) == -1
    assert call(nbytes=need - 1) == -1 and call(nbytes=0) == -1
    assert call(dims=(2, 1, 11, 11)) == -1                                 # the workspace of one sample for two
    assert call(ps=neg) == -1 and call(ts=neg) == -1 and call(sl=p, ls=neg, sg=p, gs=st) == -1
    assert call(ws=ctypes.c_void_p(p.value + 4)) == -1                     # misaligned doubles
    assert call(dims=(1, 1, 10, 11)) == -2 and call(dims=(1, 1, 11, 10)) == -2
    if fn.endswith("bf16"):
        assert call(pred=ctypes.c_void_p(p.value + 1)) == -1


def test_launch_layer_refuses_host_tensors_wrong_dtypes_and_shapes():
    from rehrseg_amd import hip_backend as hb
    x = torch.zeros(1, 1, 11, 11)
    with pytest.raises(L.RehrsegHipError):
        hb.sr_metrics(x, x)
    meta = torch.zeros(1, 1, 11, 11, device="meta")

    class Dev(torch.Tensor):
        """A meta tensor that claims to live on the device: reaches the checks behind `is_cuda`, never a launch."""
        is_cuda = True

    def dev(t):
        return t.as_subclass(Dev)

    with pytest.raises(L.RehrsegHipError, match="float32 or bfloat16"):
        hb.sr_metrics(dev(meta.half()), dev(meta))
    with pytest.raises(L.RehrsegHipError, match="float32 or bfloat16"):
        hb.sr_metrics(dev(meta.double()), dev(meta))
    with pytest.raises(L.RehrsegHipError, match="targets are float32"):
        hb.sr_metrics(dev(meta), dev(meta.bfloat16()))
    with pytest.raises(L.RehrsegHipError, match="shape"):
        hb.sr_metrics(dev(meta), dev(torch.zeros(1, 1, 11, 12, device="meta")))
    with pytest.raises(L.RehrsegHipError, match="shape"):
        hb.sr_metrics(dev(meta[0]), dev(meta[0]))
    with pytest.raises(L.RehrsegHipError, match="come together"):
        hb.sr_metrics(dev(meta), dev(meta), seg_logits=dev(meta))
    with pytest.raises(L.RehrsegHipError, match="prediction's dtype"):
        hb.sr_metrics(dev(meta), dev(meta), dev(meta.bfloat16()), dev(meta))


@pytest.mark.parametrize("shape", sc.SMALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", sc.KINDS)
def test_cpu_statement_against_the_oracle(memu, kind, shape):
    p, t, lg, sg, rng = sc.make_case(kind, shape)
    got = memu.sr_metrics(*(torch.from_numpy(a) for a in (p, t, lg, sg)), data_range=rng)
    assert got.dtype == torch.float64 and tuple(got.shape) == (shape[0], 7)
    sc.check_stats(f"emu {kind} {shape}", got.numpy(), p, t, lg, sg, rng)
    plain = memu.sr_metrics(torch.from_numpy(p), torch.from_numpy(t), data_range=rng)
    assert torch.equal(plain[:, :4], got[:, :4]) and not plain[:, 4:].any()
    pb = torch.from_numpy(p).bfloat16()
    lb = torch.from_numpy(lg).bfloat16()
    assert torch.equal(memu.sr_metrics(pb, torch.from_numpy(t), lb, torch.from_numpy(sg), rng),
                       memu.sr_metrics(pb.float(), torch.from_numpy(t), lb.float(), torch.from_numpy(sg), rng))


@pytest.mark.parametrize("kind", sc.KINDS)
def test_cpu_statement_identical_images(memu, kind):
    _, t, _, _, rng = sc.make_case(kind, (2, 3, 45, 37))
    t = torch.from_numpy(t)
    got = memu.sr_metrics(t, t.clone(), data_range=rng)
    assert not got[:, :2].any()
    assert float((got[:, 2] / got[:, 3] - 1).abs().max()) <= 1e-6
    q = sr.sr_quality(got, t[0].numel(), rng)
    assert q["psnr"] == math.inf and q["l1"] == 0.0 and q["mse"] == 0.0 and abs(q["ssim"] - 1) <= 1e-6


def test_sr_quality_arithmetic():
    stats = torch.tensor([[10.0, 4.0, 30.0, 40.0, 5, 8, 9], [30.0, 0.0, 40.0, 40.0, 1, 2, 3],
                          [20.0, 1.0, 10.0, 40.0, 0, 0, 0]], dtype=torch.float64)
    q = sr.sr_quality(stats, 100, data_range=2.0)
    assert q["n"] == 3 and q["psnr"] == math.inf
    assert q["l1"] == pytest.approx(0.2, rel=1e-15) and q["mse"] == pytest.approx(5.0 / 300, rel=1e-15)
    assert q["ssim"] == pytest.approx((0.75 + 1.0 + 0.25) / 3, rel=1e-15)
    assert q["dice"] == pytest.approx((2 * 6 + 1e-5) / (10 + 12 + 1e-5), rel=1e-15)   # from the SUMMED counts
    q = sr.sr_quality(stats[[0, 2]], 100, data_range=2.0)
    want = (10 * math.log10(4 / 0.04) + 10 * math.log10(4 / 0.01)) / 2
    assert q["psnr"] == pytest.approx(want, rel=1e-14) and q["n"] == 2
    assert all(type(v) in (float, int) for v in q.values())
    empty = sr.sr_quality(torch.tensor([[1.0, 1.0, 1.0, 1.0, 0, 0, 0]], dtype=torch.float64), 1)
    assert empty["dice"] == 1.0                                               # smooth / smooth, as calculate_dice
    with pytest.raises(ValueError):
        sr.sr_quality(torch.zeros((0, 7), dtype=torch.float64), 1)


class _Stub(torch.nn.Module):
    """Stands where the network stands: (B, 2, 4, h, w) -> the same shape (or a pair), and remembers its inputs."""

    def __init__(self, pair=False):
        super().__init__()
        self.k = torch.nn.Parameter(torch.tensor(0.9))
        self.pair, self.seen, self.modes = pair, [], []

    def forward(self, x):
        assert not torch.is_grad_enabled()
        self.seen.append(x.clone())
        self.modes.append(self.training)
        out = torch.cat((x[:, 0:1] * self.k + 0.02, x[:, 1:2] - 0.5), 1)
        return (out, torch.ones_like(out[:, :1])) if self.pair else out


@pytest.fixture
def held_out(memu, monkeypatch):
    from feed_cases import KERNEL, emu_axis_resample, emu_patch_gather, volumes_multi
    from rehrseg_amd import hip_backend as hb
    from rehrseg_amd.utils import train_set as ts
    monkeypatch.setattr(hb, "patch_gather", emu_patch_gather)
    monkeypatch.setattr(hb, "axis_resample", emu_axis_resample)
    monkeypatch.setattr(ts._DeviceSet, "_check_device", lambda self, device: torch.device("cpu"))
    vols = volumes_multi(5, [(20, 18, 17), (18, 19, 16), (17, 17, 18)])
    return ts.TrainSetMultiple(None, [0, 1, 2], 4.0, 1.0, None, None, (16, 16, 16), True, "cpu", volumes=vols,
                               blur_kernel=KERNEL)


@pytest.mark.parametrize("pair", [False, True])
def test_validate_sr_host_logic(held_out, monkeypatch, pair):
    from rehrseg_amd.train_steps import validate_sr
    ds = held_out
    drawn, batches = [], []
    plain_batch = ds.batch

    def batch(indices):
        drawn.append(list(indices))
        out = plain_batch(indices)
        batches.append(out)
        return out

    monkeypatch.setattr(ds, "batch", batch)
    model = _Stub(pair).train()
    random.seed(123)
    before = random.getstate()
    q = validate_sr(model, ds, 3, 2, 4.0, 4, enable_uncertainty=pair, seed=7)
    assert random.getstate() == before
    assert model.training and model.modes == [False] * 3
    assert drawn == [[0, 1], [2, 0], [1, 2]]                                # (b * batch_size + j) % len
    assert q["n"] == 6 and set(q) == {"l1", "mse", "psnr", "ssim", "dice", "n"}
    # the same draws again under the same seed, by hand: the LR batches the model saw, and the numbers from the oracle
    # on the stub's outputs against the middle slice_separation slices of the HR batch
    state = random.getstate()
    random.seed(7)
    rows = []
    for b, idx in enumerate(drawn):
        lr, hr = plain_batch(idx)
        assert torch.equal(lr, model.seen[b]) and torch.equal(hr, batches[b][1])
        assert tuple(hr.shape) == (2, 2, 16, 16, 16) and tuple(lr.shape) == (2, 2, 4, 16, 16)
        cut = hr[:, :, 4:8]
        with torch.no_grad():
            hat = model(lr)
        hat = hat[0] if pair else hat
        rows.append(sc.oracle(hat[:, 0].numpy(), cut[:, 0].numpy(), hat[:, 1].numpy(), cut[:, 1].numpy(), 1.0))
    random.setstate(state)
    want = sr.sr_quality(torch.from_numpy(np.concatenate(rows)), 4 * 16 * 16, 1.0)
    assert q["dice"] == want["dice"] and q["n"] == want["n"]
    for k in ("l1", "mse", "psnr"):
        assert q[k] == pytest.approx(want[k], rel=5e-7), k
    assert abs(q["ssim"] - want["ssim"]) <= 1e-5
    # a second call with the same seed: identical numbers; another seed: other patches
    model.eval()
    again = validate_sr(model, ds, 3, 2, 4.0, 4, enable_uncertainty=pair, seed=7)
    assert again == q and not model.training
    assert validate_sr(model, ds, 3, 2, 4.0, 4, enable_uncertainty=pair, seed=8) != q


def test_validate_sr_refusals_leave_no_trace(held_out, monkeypatch):
    from rehrseg_amd.train_steps import validate_sr
    ds = held_out
    model = _Stub().train()
    random.seed(5)
    before = random.getstate()
    monkeypatch.setattr(ds, "train_transform", lambda **kw: kw)
    with pytest.raises(ValueError, match="train_transform"):
        validate_sr(model, ds, 1, 2, 4.0, 4)
    monkeypatch.setattr(ds, "train_transform", None)

    def boom(indices):
        random.random()
        raise RuntimeError("feed failed")

    monkeypatch.setattr(ds, "batch", boom)
    with pytest.raises(RuntimeError, match="feed failed"):
        validate_sr(model, ds, 1, 2, 4.0, 4)
    assert random.getstate() == before and model.training
