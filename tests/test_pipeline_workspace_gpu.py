"""The five workspace-taking families of the pipeline kernels stay inside the size their query reports.  Every call
runs twice on the same inputs: with the wrapper's own workspace, and with a buffer of exactly the queried size that is
followed by 4096 guard bytes of a pattern inside the same tensor (workspace_bytes = the queried size).  The guard must
come back untouched -- a carve that disagrees with the query shows as a changed byte, not as a fault -- and every
output of the tight run must equal the first run bit for bit.  The shapes are the smallest whose segments need padding
to 16 bytes (voxel counts that are no multiple of 4) next to ones that need none."""
import ctypes as C

import pytest
import torch

from rehrseg_amd import hip_backend as hb
from rehrseg_amd import lib as L

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD, PATTERN = 4096, 0xA5


class Tight:
    """A workspace of exactly query(*args) bytes with the guard behind it."""

    def __init__(self, query, *args):
        n = int(query(*args))
        assert n > 0, n
        self.buf = torch.full((n + GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
        self.ws = self.buf[:n]
        assert self.ws.data_ptr() % 16 == 0 and self.ws.numel() == n

    def check(self):
        torch.cuda.synchronize()
        guard = self.buf[self.ws.numel():]
        assert guard.numel() == GUARD and bool((guard == PATTERN).all()), "the kernels wrote past the queried size"


def _same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    assert torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def _masks(dims, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(dims, generator=g) < 0.4).to(torch.uint8).to(DEV) for _ in range(2)]


@pytest.mark.parametrize("dims", [(3, 5, 7), (2, 16, 16)])
def test_surface_workspace(dims):
    pred, gt = _masks(dims, 3)

    def run(workspace):
        counts = torch.zeros(2, dtype=torch.int64, device=DEV)
        dist, workspace = hb.seg_surface_distances(pred, gt, (2.0, 0.5, 0.75), counts, workspace)
        out = torch.zeros(3, dtype=torch.int64, device=DEV)
        hb.seg_surface_reduce(dist, torch.sort(dist.view(-1)).values, counts, out, workspace)
        return dist, counts, out

    roomy = run(None)
    tight = Tight(L.load().rehr_seg_surface_workspace_bytes, *dims)
    got = run(tight.ws)
    tight.check()
    for a, b in zip(got, roomy):
        _same(a, b)
    assert int(roomy[1].min()) > 0     # both surfaces exist: the three metrics are numbers


@pytest.mark.parametrize("dims", [(3, 5, 7), (2, 16, 16)])
def test_components_workspace(dims):
    pred, gt = _masks(dims, 5)

    def run(workspace):
        rp, _ = hb.seg_cc_roots(pred, 26, workspace)
        rg, _ = hb.seg_cc_roots(gt, 6, workspace)
        out = torch.zeros(8, dtype=torch.int64, device=DEV)
        keys = hb.seg_cc_lesion(rp, rg, out, workspace).clone()
        return rp, rg, out, keys

    roomy = run(None)
    tight = Tight(L.load().rehr_seg_cc_workspace_bytes, *dims)
    got = run(tight.ws)
    tight.check()
    for a, b in zip(got, roomy):
        _same(a, b)
    assert int(roomy[2][0]) > 0 and int(roomy[2][1]) > 0     # components on both sides


def test_order_stats_workspace():
    B, S, ranks = 3, 105, (0, 52, 104)
    x = torch.randn((B, S), generator=torch.Generator().manual_seed(7)).to(DEV)
    roomy = hb.order_stats(x, ranks)
    tight = Tight(L.load().rehr_order_stats_workspace_bytes, B, len(ranks))
    got = hb.order_stats(x, ranks, workspace=tight.ws)
    tight.check()
    _same(got, roomy)
    _same(roomy, torch.sort(x, dim=1).values[:, list(ranks)])


@pytest.mark.parametrize("shape", [(1, 1, 11, 11), (2, 3, 12, 13)])
def test_sr_metrics_workspace(shape):
    g = torch.Generator().manual_seed(9)
    pred, tgt, slog, stgt = (torch.rand(shape, generator=g).to(DEV) for _ in range(4))
    slog = slog - 0.5
    roomy = hb.sr_metrics(pred, tgt, slog, stgt)
    lib = L.load()
    tight = Tight(lib.rehr_sr_metrics_workspace_bytes, *shape)
    stats = torch.empty((shape[0], 7), dtype=torch.float64, device=DEV)
    strides = [(C.c_int64 * 4)(*t.stride()) for t in (pred, tgt, slog, stgt)]
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    L.check(lib.rehr_sr_metrics_f32(ptr(pred), strides[0], ptr(tgt), strides[1], ptr(slog), strides[2], ptr(stgt),
                                    strides[3], *shape, 1.0, ptr(stats), ptr(tight.ws), tight.ws.numel(),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)), "rehr_sr_metrics_f32")
    tight.check()
    _same(stats, roomy)


@pytest.mark.parametrize("shape", [(1, 1, 1, 11, 11), (2, 2, 3, 12, 13)])
def test_structure_loss_workspace(shape):
    g = torch.Generator().manual_seed(11)
    x, t = (torch.rand(shape, generator=g).to(DEV) for _ in range(2))
    w = (1.0, 0.5, 0.25, 2.0)
    roomy = hb.structure_loss_fwd(x, t, w)
    lib = L.load()
    tight = Tight(lib.rehr_structure_loss_workspace_bytes, *shape)
    stats = torch.empty((shape[0], 4), dtype=torch.float64, device=DEV)
    loss = torch.empty((), dtype=torch.float32, device=DEV)
    fields = torch.empty(shape[:3] + (3,) + shape[3:], dtype=torch.float32, device=DEV)
    strides = [(C.c_int64 * 5)(*v.stride()) for v in (x, t)]
    ptr = lambda v: C.c_void_p(v.data_ptr())  # noqa: E731
    L.check(lib.rehr_structure_loss_fwd_f32(ptr(x), strides[0], ptr(t), strides[1], *shape, *w, 1.0, ptr(stats),
                                            ptr(loss), ptr(fields), ptr(tight.ws), tight.ws.numel(),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)),
            "rehr_structure_loss_fwd_f32")
    tight.check()
    _same(loss, roomy[0])
    _same(stats, roomy[1])
    _same(fields[..., 5:-5, 5:-5], roomy[2][..., 5:-5, 5:-5])     # written where an 11x11 window fits, read only there
