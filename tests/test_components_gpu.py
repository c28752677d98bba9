"""Connected components and lesion-wise scores on the MI355X (csrc/seg_components.hip) against the scipy oracle
(tests/components_oracle.py).  Every comparison is exact equality of integers: the root map element by element, the
labels and their number, the largest component, the eight integers and the public dict.  No tolerance anywhere.

The small cases are the smallest shapes at which each part of the labelling can go wrong: a W that is odd and crosses
a 64-lane step (67) or two of them (130), runs that continue over a step, neighbours that exist at one connectivity
only, voxels at the ends of adjacent rows and slices (no wrap-around), a path about N/4 long, components that join
only in the last or the first row, and single rows, columns and slices."""
import warnings

import numpy as np
import pytest
import torch

import components_oracle as co
from rehrseg_amd import hip_backend as hb
from rehrseg_amd import lib as L
from rehrseg_amd.utils import seg_utils as su

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(mask):
    return torch.from_numpy(np.asarray(mask).astype(np.uint8)).to(DEV)


def _run(name, connectivity):
    """The backend calls on a case and its partner map: (roots, labels, n, the eight integers), on the host."""
    pred, gt = _dev(co.case(name)), _dev(co.partner(name))
    out = torch.zeros(9, dtype=torch.int64, device=DEV)
    roots_p, ws = hb.seg_cc_roots(pred, connectivity)
    roots_g, _ = hb.seg_cc_roots(gt, connectivity, ws)
    hb.seg_cc_lesion(roots_p, roots_g, out[:8], ws)
    labels = hb.seg_cc_compact(roots_p, out[8:])
    host = out.cpu()
    return roots_p.cpu().numpy(), labels.cpu().numpy(), int(host[8]), [int(v) for v in host[:8]]


def _check_case(name, connectivity):
    want = co.expected(name, connectivity)
    roots, labels, n, vals = _run(name, connectivity)
    print(f"{name} / {connectivity}: n = {n} (oracle {want['n']}), eight = {vals} (oracle {want['eight']})")
    assert roots.dtype == np.int32 and np.array_equal(roots, want["roots"])
    assert n == want["n"] and labels.dtype == np.int32 and np.array_equal(labels, want["labels"])
    assert vals == want["eight"]
    return want


@pytest.mark.parametrize("connectivity", co.CONNECTIVITIES)
@pytest.mark.parametrize("name", co.SMALL)
def test_small_cases_meet_the_oracle(name, connectivity):
    want = _check_case(name, connectivity)
    m, g = co.case(name), co.partner(name)
    labels, n = su.connected_components(m, connectivity, device=DEV)
    assert type(n) is int and n == want["n"] and labels.dtype == torch.int32 and labels.device == DEV
    assert np.array_equal(labels.cpu().numpy(), want["labels"])
    keep = su.keep_largest_component(m, connectivity, device=DEV)
    assert keep.dtype == torch.uint8 and keep.device == DEV and np.array_equal(keep.cpu().numpy(), want["keep"])
    got = su.lesion_metrics(m, g, connectivity, device=DEV)
    assert co.same_dict(got, want["dict"]), (got, want["dict"])
    counts = {name: [co.expected(name, c)["n"] for c in co.CONNECTIVITIES]}
    if name == "checkerboard":
        assert counts[name] == [120, 1, 1]
    if name == "corners":
        assert counts[name] == [2, 2, 1]
    if name == "edges":
        assert counts[name] == [2, 1, 1]
    if name == "no_wrap":
        assert counts[name] == [4, 4, 4]
    if name == "snake":
        assert counts[name][0] == 1 and m.sum() > m.size // 4
    if name in ("late_join", "late_join_mirror", "full"):
        assert counts[name] == [1, 1, 1]
    if name == "empty":
        assert counts[name] == [0, 0, 0] and not keep.any()
    if name == "noise_0.1" and connectivity == 6:
        # three components tie for the largest size; the one with the smallest root is kept
        assert want["n"] == 571 and co.n_largest_ties(m, 6) == 3 and want["eight"][4] == 7
        r = want["roots"]
        sizes = np.bincount(r[r >= 0])
        first = int(np.flatnonzero(sizes == 7)[0])
        assert np.array_equal(keep.cpu().numpy(), (r == first).astype(np.uint8)) and int(keep.sum()) == 7
    if name == "lesions_pred":
        d = want["dict"]
        assert d["n_gt"] >= 5 and 0 < d["tp_gt"] < d["n_gt"] and d["fp"] >= 1 and d["tp_pred"] != d["tp_gt"]
        overlap = [int(((want["labels"] == k) & g).sum()) for k in range(1, want["n"] + 1)]
        assert d["dice_largest_terms"][0] < max(overlap)     # the largest blob is not the best-overlapping one


@pytest.mark.parametrize("connectivity,count", ((26, 336), (6, 121212)))
def test_stage2_lattice_meets_the_oracle(connectivity, count):
    want = _check_case("lattice", connectivity)
    assert want["n"] == count


@pytest.mark.parametrize("name,connectivity", (("noise_0.3", 6), ("noise_0.3", 26), ("lattice", 6), ("lattice", 26)))
def test_two_runs_give_the_same_bits(name, connectivity):
    a, b = _run(name, connectivity), _run(name, connectivity)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_unsupported_extent_raises_without_a_launch():
    big = torch.zeros((1, 8, 8), dtype=torch.uint8, device=DEV).expand(1 << 26, 8, 8)   # no memory behind it
    tiny = torch.zeros((2, 3, 4), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for fn in (su.connected_components, su.keep_largest_component, lambda m, device: su.lesion_metrics(m, m)):
            with pytest.raises(L.RehrsegHipError, match="unsupported extent"):
                fn(big, device=DEV)
        with pytest.raises(L.RehrsegHipError, match="unsupported extent"):
            hb.seg_cc_check_extent(big.shape)
        with pytest.raises(L.RehrsegHipError, match="connectivity"):
            hb.seg_cc_roots(tiny, 7)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    lib = L.load()
    p = tiny.data_ptr()
    assert lib.rehr_seg_cc_workspace_bytes(1 << 26, 8, 8) == -2 and lib.rehr_seg_cc_workspace_bytes(2, 0, 4) == -2
    assert lib.rehr_seg_cc_roots_i32(p, 1 << 26, 8, 8, 26, p, p, 1 << 40, None) == -2
    assert lib.rehr_seg_cc_lesion_i64(p, p, (1 << 30) + 1, p, p, 1 << 40, None) == -2
    assert lib.rehr_seg_cc_compact_i32(p, (1 << 30) + 1, p, p, p, None) == -2
    assert lib.rehr_seg_cc_roots_i32(p, 2, 3, 4, 7, p, p, 1 << 40, None) == -1


class DevToy(torch.nn.Module):
    """A position- and orientation-sensitive toy network built from device ops only (no host tensors, no syncs)."""

    def __init__(self, sep=2, scale=1.0):
        super().__init__()
        self.sep, self.scale = sep, scale

    def forward(self, x):
        sh = torch.roll(x, shifts=(1, 2), dims=(3, 4))
        lr = torch.cat([x * 0.5 + sh * 0.25, -x * 0.75 + sh * sh * 0.125 - 0.1], 1) * self.scale
        return lr, torch.repeat_interleave(lr, self.sep, dim=2) * 1.5


def _count_syncs(fn):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            out = fn()
        finally:
            torch.cuda.set_sync_debug_mode(0)
    return out, [w for w in rec if "called a synchronizing" in str(w.message)]


def test_evaluate_case_with_surface_and_components_makes_one_host_sync():
    model = DevToy(sep=4)
    g = np.random.RandomState(3)
    img = g.randint(0, 256, size=(1, 10, 70, 80)).astype(np.float32)
    lab = (g.rand(1, 10, 70, 80) < 0.4).astype(np.float32)
    sp = (4.0, 0.75, 0.5)
    args = (model, img, lab, 4, [8, 32, 32], True, DEV)
    run = lambda: su._evaluate_case(*args, surface=True, spacing=sp, components=True, connectivity=18)  # noqa: E731
    first = run()                                                      # warm-up: cached Gaussian, sort's workspace
    torch.cuda.synchronize()
    out, syncs = _count_syncs(run)
    assert len(syncs) == 1, [str(w.message) for w in syncs]
    plain = su._evaluate_case(*args)
    surf = su._evaluate_case(*args, surface=True, spacing=sp)
    assert len(plain) == 5 and len(surf) == 6 and len(out) == 7
    assert np.array_equal(out[0], plain[0]) and np.array_equal(out[1], plain[1]) and torch.equal(out[2], plain[2])
    assert out[3] == plain[3] and out[4] == plain[4] and out[5] == surf[5] and out[6] == first[6]
    want = co.lesion_dict(co.eight(out[0], lab[0], 18))
    assert co.same_dict(out[6], want), (out[6], want)
    assert want["n_pred"] > 1 and want["n_gt"] > 1
    only, syncs = _count_syncs(lambda: su._evaluate_case(*args, components=True, connectivity=18))
    assert len(syncs) == 1 and len(only) == 6 and only[5] == out[6]
    public = su.evaluate_case(model, img, lab, 4, [8, 32, 32], device=DEV, surface=True, spacing=sp, components=True,
                              connectivity=18)
    assert len(public) == 6 and public[4] == out[5] and public[5] == out[6]


def test_sync_counts_of_the_public_functions():
    pred, gt = _dev(co.case("lesions_pred")), _dev(co.case("lesions_gt"))
    want = co.expected("lesions_pred", 26)
    su.lesion_metrics(pred, gt)                                         # warm-up
    su.keep_largest_component(pred)
    su.connected_components(pred)
    torch.cuda.synchronize()
    out, syncs = _count_syncs(lambda: su.lesion_metrics(pred, gt))
    assert len(syncs) == 1, [str(w.message) for w in syncs]
    assert co.same_dict(out, want["dict"])
    keep, syncs = _count_syncs(lambda: su.keep_largest_component(pred))
    assert len(syncs) == 0, [str(w.message) for w in syncs]
    assert np.array_equal(keep.cpu().numpy(), want["keep"])
    (labels, n), syncs = _count_syncs(lambda: su.connected_components(pred))
    assert len(syncs) == 1, [str(w.message) for w in syncs]
    assert n == want["n"] and np.array_equal(labels.cpu().numpy(), want["labels"])
