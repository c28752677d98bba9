"""Top-k cross-entropy + soft Dice without a device: the C-ABI's symbols and argument checks
(every refusal comes back before any launch, so it comes back here), TopKLoss / DC_and_topk_loss on CPU tensors against
the plain F.cross_entropy -> topk -> mean composition and against tests/topk_oracle.py, the tie rule on the oracle's
tie case, `_build_loss`'s unchanged defaults, and the fused autograd node's host logic over tests/topk_emu.py."""
import pytest
import torch
import torch.nn.functional as F

import topk_emu
import topk_oracle as to
from rehrseg_amd import lib as L
from rehrseg_amd import ops
from rehrseg_amd.train_steps import train_segsr_step
from rehrseg_amd.utils import seg_utils as su
from test_segmodel_cpu import SMALL, build

SHAPES = [(2, 2, 3, 5, 7), (1, 3, 2, 9, 13), (3, 4, 1, 4, 33), (2, 2, 6, 10, 12)]
KS = [1, 10, 37.5, 100]
NEW = ("rehr_seg_topk_workspace_bytes", "rehr_seg_topk_fwd_f32", "rehr_seg_topk_bwd_f32")


def _inputs(shape, seed, dtype=torch.float64):
    N, Cc, D, H, W = shape
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(shape, generator=g, dtype=dtype) * 2
    target = torch.randint(0, Cc, (N, 1, D, H, W), generator=g).to(dtype)
    unc = 1 - torch.rand((N, 1, D, H, W), generator=g, dtype=dtype) * 0.99
    return logits, target, unc


@pytest.fixture
def emu_topk():
    old = ops.set_backend(topk_emu)
    del topk_emu.calls[:]
    yield topk_emu
    ops.set_backend(old)


# ----------------------------------------------------------------------------- 1. the C-ABI
def test_symbols_declared_exported_and_abi_version():
    lib = L.load()
    declared = set(L.declared_symbols())
    for name in NEW:
        assert name in L.PROTOTYPES and name in declared and hasattr(lib, name), name
    assert lib.rehr_abi_version() == 6 == L.ABI_VERSION


def test_workspace_query():
    lib = L.load()
    sel = lib.rehr_order_stats_workspace_bytes(1, 1)
    assert sel > 0
    # [map: M floats, padded to 16 bytes][threshold: 16][the select's own workspace]
    assert lib.rehr_seg_topk_workspace_bytes(2, 2, 105, 0) == 848 + 16 + sel          # 840 bytes of map: padding
    assert lib.rehr_seg_topk_workspace_bytes(2, 2, 480, 0) == 3840 + 16 + sel         # none
    assert lib.rehr_seg_topk_workspace_bytes(3, 4, 132, 1) == 9 * 132 * 4 + 16 + sel
    assert lib.rehr_seg_topk_workspace_bytes(0, 2, 105, 0) == -1
    assert lib.rehr_seg_topk_workspace_bytes(2, 2, 0, 0) == -1
    assert lib.rehr_seg_topk_workspace_bytes(2, 5, 105, 0) == -2
    assert lib.rehr_seg_topk_workspace_bytes(2, 1, 105, 0) == -2
    assert lib.rehr_seg_topk_workspace_bytes(5, 2, 105, 0) == -2
    assert lib.rehr_seg_topk_workspace_bytes(1, 2, (1 << 30) + 1, 0) == -2
    assert lib.rehr_seg_topk_workspace_bytes(2, 2, 1 << 28, 1) == (1 << 32) + 16 + sel   # M = 2^30 exactly
    assert lib.rehr_seg_topk_workspace_bytes(2, 2, (1 << 28) + 1, 1) == -2
    assert lib.rehr_seg_topk_workspace_bytes(2, 2, (1 << 28) + 1, 0) > 0


def test_entry_points_refuse_before_any_launch():
    """Dummy pointers nothing dereferences: every call is malformed for its entry point, so none can launch."""
    lib = L.load()
    N, Cc, S = 2, 2, 105
    need = lib.rehr_seg_topk_workspace_bytes(N, Cc, S, 0)
    need_u = lib.rehr_seg_topk_workspace_bytes(N, Cc, S, 1)
    base = dict(logits=0x10000, ld=Cc, target=0x20000, unc=None, N=N, C=Cc, S=S, K=21, stats=0x30000, ws=0x40000,
                ws_bytes=need, go=0x50000, dl=0x60000, ldd=Cc)

    def both(**over):
        a = dict(base, **over)
        fwd = lib.rehr_seg_topk_fwd_f32(a["logits"], a["ld"], a["target"], a["unc"], a["N"], a["C"], a["S"], a["K"],
                                        a["stats"], a["ws"], a["ws_bytes"], None)
        bwd = lib.rehr_seg_topk_bwd_f32(a["logits"], a["ld"], a["target"], a["unc"], a["N"], a["C"], a["S"], a["K"],
                                        a["stats"], a["ws"], a["ws_bytes"], 1.0, 1.0, 1e-5, 0, a["go"], a["dl"],
                                        a["ldd"], None)
        return fwd, bwd

    for null in ("logits", "target", "stats", "ws"):
        assert both(**{null: None}) == (-1, -1), null
    assert both(N=0) == (-1, -1) and both(S=0) == (-1, -1)
    assert both(K=0) == (-1, -1) and both(K=N * S + 1) == (-1, -1) and both(K=-3) == (-1, -1)
    assert both(ld=1) == (-1, -1)
    assert both(ws=0x40008) == (-1, -1)                              # misaligned workspace
    assert both(ws_bytes=need - 1) == (-1, -1)                       # too small
    assert both(unc=0x70000, ws_bytes=need) == (-1, -1)              # the (N, N, S) map needs the larger workspace
    assert need_u > need
    assert both(unc=0x70000, ws_bytes=need_u, K=N * N * S + 1) == (-1, -1)
    assert both(C=5) == (-2, -2) and both(C=1) == (-2, -2) and both(N=5) == (-2, -2)
    assert both(S=(1 << 30) + 1, K=1, ws_bytes=1 << 40) == (-2, -2)
    # backward only
    assert both(go=None)[1] == -1 and both(dl=None)[1] == -1 and both(ldd=1)[1] == -1


# ----------------------------------------------------------------------------- 2. the losses on CPU tensors
def _plain(logits, target, unc, k):
    m = F.cross_entropy(logits, target[:, 0].long(), reduction="none")
    if unc is not None:
        m = m * unc
    return m.view(-1).topk(int(m.numel() * k / 100), sorted=False)[0].mean(), m


@pytest.mark.parametrize("with_unc", [False, True])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_cpu_losses_equal_the_plain_composition(i, k, with_unc):
    shape = SHAPES[i]
    logits, target, unc = _inputs(shape, 100 + i)
    unc = unc if with_unc else None
    ref, m = _plain(logits, target, unc, k)
    N = shape[0]
    assert tuple(m.shape) == ((N, N) if with_unc else (N,)) + shape[2:]
    got = su.TopKLoss(k=k)(logits, target, unc)
    assert got.dtype == torch.float64 and abs(float(got) - float(ref)) <= 1e-12
    dc = su.SoftDiceLoss(apply_nonlin=su.softmax_helper_dim1, batch_dice=False, smooth=1e-5, do_bg=False)(logits, target)
    full = su._build_loss(topk=k)(logits, target, unc)
    assert abs(float(full) - float(ref + dc)) <= 1e-12
    # the tie-weight form of the contract against torch.topk
    o = to.dc_and_topk(logits, target, unc, k=k)
    assert o["K"] == int(m.numel() * k / 100) and tuple(o["m"].shape) == tuple(m.shape)
    assert abs(float(o["value"]) - float(ref + dc)) <= 2e-15 * max(1.0, abs(float(ref + dc)))
    assert o["n_gt"] + o["n_eq"] >= o["K"] > o["n_gt"]
    # without ties the subgradient is the gradient of the composition
    if o["n_eq"] == 1:
        x = logits.clone().requires_grad_(True)
        su._build_loss(topk=k)(x, target, unc).backward()
        assert float((x.grad - o["grad"]).abs().max()) <= 1e-13 * float(o["grad"].abs().max())


def test_oracle_tie_case():
    logits, target = to.tie_case()
    o = to.dc_and_topk(logits, target, None, k=50, weight_dice=0.0)
    assert (o["K"], o["t"], o["n_gt"], o["n_eq"]) == (16, 0.0, 5, 27)
    tied = o["m"] == 0
    assert int(tied.sum()) == 27 and bool(torch.signbit(o["m"][tied]).all())      # -0.0: the -0 / +0 case
    assert float(o["value"]) == 12.5
    assert torch.equal(o["weights"][tied], torch.full((27,), 11 / 27, dtype=torch.float64))
    assert torch.equal(o["weights"][~tied], torch.ones(5, dtype=torch.float64))
    assert abs(float(su.TopKLoss(k=50)(logits.double(), target.double())) - 12.5) <= 1e-12
    # the tied voxels share one gradient, the wrong ones carry the full 1 / K
    g = o["grad"][0, 0].reshape(-1)
    tied_g = g[tied.reshape(-1)]
    assert float(tied_g.max() - tied_g.min()) == 0.0


def test_build_loss_defaults_are_unchanged():
    logits, target, unc = _inputs((2, 2, 3, 5, 7), 3)
    plain, deep = su._build_loss(), su._build_loss(True)
    assert type(plain) is su.DC_and_weighted_CE_loss and type(plain.ce) is su.RobustCrossEntropyLoss
    assert type(deep) is su.DeepSupervisionWrapper and type(deep.loss) is su.DC_and_weighted_CE_loss
    assert type(su._build_loss(topk=None)) is su.DC_and_weighted_CE_loss
    # the value on a fixed input: weight_ce * mean CE (with the (N, N, ...) broadcast) + the soft Dice
    ce = F.cross_entropy(logits, target[:, 0].long(), reduction="none")
    dc = to.soft_dice(logits, target)
    assert abs(float(plain(logits, target)) - float(ce.mean() + dc)) <= 1e-14
    assert abs(float(plain(logits, target, unc)) - float((ce * unc).mean() + dc)) <= 1e-14
    assert abs(float(deep([logits], [target])) - float(deep.weight_factors[0] * (ce.mean() + dc))) <= 1e-14
    top = su._build_loss(topk=10)
    assert type(top) is su.DC_and_topk_loss and type(top.ce) is su.TopKLoss and top.ce.k == 10
    assert issubclass(su.TopKLoss, su.RobustCrossEntropyLoss) and su.TopKLoss().k == 10
    wrapped = su._build_loss(True, weight_dice=0.5, topk=10)
    assert type(wrapped) is su.DeepSupervisionWrapper and type(wrapped.loss) is su.DC_and_topk_loss
    assert wrapped.loss.weight_dice == 0.5 and wrapped.weight_factors == deep.weight_factors
    # not the one-launch deep-supervision node: that one is the plain loss's
    assert not isinstance(top, su.DC_and_weighted_CE_loss)


def test_value_errors_before_anything_runs():
    logits, target, _ = _inputs((1, 2, 1, 1, 5), 1)
    for mod in (su._build_loss(topk=10), su.TopKLoss(k=10)):
        with pytest.raises(ValueError, match="K = 0"):
            mod(logits, target)
    for bad in (0, -1, 100.5):
        with pytest.raises(ValueError, match=r"\(0, 100\]"):
            su._build_loss(topk=bad)
        with pytest.raises(ValueError, match=r"\(0, 100\]"):
            su.TopKLoss(k=bad)
    assert su._build_loss(topk=100)(logits, target) is not None


def test_fused_path_raises_value_error_before_the_backend(emu_topk):
    logits, target, _ = _inputs((1, 2, 1, 1, 5), 1)
    mod = su._build_loss(topk=10)
    assert mod._fusable(logits, target, None)
    with pytest.raises(ValueError, match="K = 0"):
        mod(logits, target)
    assert emu_topk.calls == []


# ----------------------------------------------------------------------------- 3. the autograd node over the emulation
def _node(t):
    assert t.grad_fn is not None and type(t.grad_fn).__name__ == "_FusedDCTopKBackward", type(t.grad_fn).__name__


@pytest.mark.parametrize("with_unc", [False, True])
@pytest.mark.parametrize("k", [10, 100])
def test_autograd_node_over_the_emulation(emu_topk, k, with_unc):
    shape = (2, 3, 2, 5, 7)
    logits, target, unc = _inputs(shape, 41)
    unc = unc if with_unc else None
    o = to.dc_and_topk(logits, target, unc, k=k, weight_dice=0.5)
    x = logits.clone().requires_grad_(True)
    val = su._build_loss(weight_dice=0.5, topk=k)(x, target, unc)
    _node(val)
    (val * 3.0).backward()                     # a non-unit upstream gradient
    assert val.dtype == torch.float32
    assert abs(float(val.detach()) - float(o["value"])) <= 1e-6 * abs(float(o["value"]))        # an fp32 scalar
    # the node hands the uncertainty over in fp32 (2^-24 relative), everything else here is fp64
    assert float((x.grad / 3.0 - o["grad"]).abs().max()) <= (1e-6 if with_unc else 1e-12) * float(o["grad"].abs().max())
    N, Cc = shape[:2]
    M = (N * N if with_unc else N) * 70
    assert emu_topk.calls == [("fwd", N, Cc, 70, int(M * k / 100), with_unc), ("bwd", N, Cc, 70, int(M * k / 100), with_unc)]


def test_node_on_the_tie_case(emu_topk):
    logits, target = to.tie_case()
    o = to.dc_and_topk(logits, target, None, k=50)
    x = logits.double().requires_grad_(True)
    val = su._build_loss(topk=50)(x, target.double())
    _node(val)
    val.backward()
    assert abs(float(val.detach()) - float(o["value"])) <= 1e-6
    assert float((x.grad - o["grad"]).abs().max()) <= 1e-12


def test_not_fusable_configurations_take_the_composition(emu_topk):
    logits, target, unc = _inputs((2, 2, 3, 5, 7), 8)
    mod = su._build_loss(topk=10)
    assert mod._fusable(logits, target, unc) and mod._fusable(logits, target, None)
    assert not mod._fusable(logits, target, unc[:, 0])                      # another broadcast in the reference
    assert not mod._fusable(torch.randn(5, 2, 1, 2, 2), torch.zeros(5, 1, 1, 2, 2), None)     # more than 4 samples
    assert not mod._fusable(torch.randn(2, 5, 1, 2, 2), torch.zeros(2, 1, 1, 2, 2), None)     # more than 4 classes
    assert not su.DC_and_topk_loss({}, {}, ignore_label=1)._fusable(logits, target, None)
    val = mod(logits.requires_grad_(True), target, unc[:, 0])
    assert type(val.grad_fn).__name__ != "_FusedDCTopKBackward" and emu_topk.calls == []


def test_deep_supervision_sums_the_levels(emu_topk):
    dims = [(4, 16, 16), (4, 8, 8), (2, 4, 4)]
    g = torch.Generator().manual_seed(5)
    logits = [torch.randn((2, 2) + d, generator=g, dtype=torch.float64).requires_grad_(True) for d in dims]
    labels = [torch.randint(0, 2, (2, 1) + d, generator=g).double() for d in dims]
    uncs = [1 - torch.rand((2, 1) + d, generator=g, dtype=torch.float64) * 0.99 for d in dims]
    w = (0.5, 0.0, 0.25)
    wrap = su.DeepSupervisionWrapper(su._build_loss(topk=10), w)
    assert not wrap._fusable(list(zip(logits, labels, uncs)), [0, 2])       # the Python sum, one node per level
    val = wrap(logits, labels, uncs)
    val.backward()
    ref = [to.dc_and_topk(logits[i], labels[i], uncs[i], k=10) for i in (0, 2)]
    want = 0.5 * float(ref[0]["value"]) + 0.25 * float(ref[1]["value"])
    assert abs(float(val.detach()) - want) <= 1e-6 * abs(want)
    assert logits[1].grad is None                                          # a zero-weight level: None, not zeros
    for i, r, wi in ((0, ref[0], 0.5), (2, ref[1], 0.25)):
        assert float((logits[i].grad - wi * r["grad"]).abs().max()) <= 1e-6 * float(r["grad"].abs().max())
    assert [c[0] for c in emu_topk.calls].count("fwd") == 2 and [c[0] for c in emu_topk.calls].count("bwd") == 2
    # without an uncertainty list
    for x in logits:
        x.grad = None
    wrap(logits, labels).backward()
    assert logits[1].grad is None and logits[0].grad is not None


@pytest.mark.parametrize("deep", [False, True])
@pytest.mark.parametrize("with_unc", [False, True])
def test_train_segsr_step_on_the_toy_model(emu_topk, deep, with_unc):
    from oracle.detinit import det_input
    model, sd = build(SMALL, deep_supervision=deep)
    img = det_input("tk.img", (2, 1, 4, 16, 16), "rand") * 2 + 0.5
    lab = det_input("tk.lr", (2, 1, 4, 16, 16), "randint2")
    lab_hr = det_input("tk.hr", (2, 1, 16, 16, 16), "randint2")
    unc = 1 - det_input("tk.u", (2, 1, 4, 16, 16), "rand") * 0.99
    if deep:
        labs, uncs = [lab, lab[..., ::2, ::2].contiguous()], [unc, unc[..., ::2, ::2].contiguous()]
    else:
        labs, uncs = lab, unc
    opt = torch.optim.SGD(model.parameters(), lr=1e-2)
    loss = train_segsr_step(model, None, None, opt, img, labs, lab_hr, uncs if with_unc else None,
                            su._build_loss(deep, topk=10), su._build_loss(False, topk=10), enable_uncertainty=with_unc)
    assert torch.isfinite(loss)
    fwd = [c for c in emu_topk.calls if c[0] == "fwd"]
    assert len(fwd) == (3 if deep else 2) and len(emu_topk.calls) == 2 * len(fwd)
    assert [c[5] for c in fwd] == [with_unc] * (len(fwd) - 1) + [False]          # the HR loss has no uncertainty
    moved = [k for k, p in model.named_parameters() if not torch.equal(p.detach(), sd[k])]
    assert any("seg_layers" in k for k in moved) and any(k.startswith("encoder.stages.0") for k in moved)
